// plba_track_dev.h — the arithmetic of plba_track_pose (include/plba.h), shared by the kernel (plba_track.hip, 64 lanes), the host check
// (plba_track_hostcheck.cpp, 64 emulated lanes) and the plain-C++ drop-in (include/plba_g2o/track_pose.h, one lane).
//
// StereoFrameHandler::optimizePose (stvo-pl/src/stereoFrameHandler.cpp:334-419) for ONE frame pair, mode 0 of :356: the first stage
// (gaussNewtonOptimization, :421-458) on a copy of the start pose, isGoodSolution (:319-332), the MAD cut (removeOutliers, :1015-1094;
// vector_mean_stdv_mad, auxiliar.cpp:387-430) and the refinement FROM THE START POSE, or the robust fallback
// (gaussNewtonOptimizationRobust, :460-507, over optimizeFunctionsRobust, :723-989).  The structure is plba_relpose_dev.h's, whose SE(3)
// helpers, jac6, pivoted QR, Jacobi eigenvalues and balanced tree are used from there: functions of (lane, lane count), a Wave that runs a
// lane function on every lane and adds the lanes' results in the tree (sum) or as integers (sum_i), one lane for the serial part.
//
// New here is the order statistic (select): element k of the ascending list of a problem's residuals, which the lanes hold strided.  The
// residuals are non-negative doubles, so their bit patterns order like unsigned integers; the pattern of the answer is found from bit 62
// down: with the bits above fixed, the lanes count their values that match them and have the next bit clear, the counts are added over
// the wave, and k falls in the clear or in the set half.  63 rounds, integers only: the result is THE k-th smallest value, whatever
// the lane count, which is what makes the 64-lane and the 1-lane run take the same median, MAD, cut and Cauchy scale.
#pragma once
#include <cstring>

#include "plba_relpose_dev.h"

namespace plba {
namespace track {

namespace rp = relpose;
using rp::Acc;
using rp::Pose;

constexpr int OK = 0, NONFINITE = 2, RANK = 3;      // PLBA_TRACK_* of include/plba.h: the values of the relpose codes
constexpr int REFINED = 0, ROBUST = 1, FEW_BEFORE = 2, FEW_AFTER = 3;      // path

struct Opt {
    int max_iters, max_iters_ref, min_features;
    double min_error, min_error_change, inlier_k;
    rp::Opt ro;      // homog_th and the intrinsics, for the feature bodies shared with relpose
};
struct Prob {        // one problem's matched features; the masks are read and, by the cut, written
    rp::Cand rc;     // np, nl, P3, uv2, pq6 (sP | eP), l3 (le_obs), pt_in, ln_in
    const double *pt_s2, *se4, *ln_s2;      // sigma2 per point; spl | epl and sigma2 per line
    double *res_p, *dev_p, *res_l, *dev_l;  // workspace: np, np, nl, nl doubles; a lane reads back only what it wrote
};
struct State {
    Pose T0, T;      // the start pose; DT as the optimiser left it
    double H[21], g[6], e, err_prev, err;      // err: err_ of the stage calls (-1 by :435 / :503)
    double cov_eig[6], stat[4];                // stat: pt_mean, pt_stdv, ln_mean, ln_stdv of the cut
    int iters[3], status, path, good, negdet, n_pt, n_ln;
};

RP_HD uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
RP_HD double double_of(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }

// ---- StereoFrame::lineSegmentOverlap, stvo-pl/src/stereoFrame.cpp:521-627 -------------------------------------------------------------
RP_HD double overlap_of(double ls, double le) {      // :541-553 (= :571-583, :609-621)
    const double lmin = ls < le ? ls : le, lmax = ls < le ? le : ls;      // std::min / std::max
    if (lmin < 0.0 && lmax > 1.0) return 1.0;
    if (lmax < 0.0 || lmin > 1.0) return 0.0;
    if (lmin < 0.0) return lmax;
    if (lmax > 1.0) return 1.0 - lmin;
    return lmax - lmin;
}
RP_HD double line_overlap(const double* so, const double* eo, const double* sp, const double* ep) {
    const double lx = eo[0] - so[0], ly = eo[1] - so[1];
    if (fabs(so[0] - eo[0]) < 1.0) return overlap_of((sp[1] - so[1]) / ly, (ep[1] - so[1]) / ly);      // vertical
    if (fabs(so[1] - eo[1]) < 1.0) return overlap_of((sp[0] - so[0]) / lx, (ep[0] - so[0]) / lx);      // horizontal
    const double a = so[1] - eo[1], b = eo[0] - so[0], c = so[0] * eo[1] - eo[0] * so[1];
    const double lxy = 1.0 / (a * a + b * b);
    const double sx = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy, ex = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy;
    return overlap_of((sx - so[0]) / lx, (ex - so[0]) / lx);
}

// ---- one feature (:594-615 points, :641-695 lines): the error norm and, with J, J_aux and the overlap -----------------------------------
RP_HD double line_feature(const Prob& c, const rp::Opt& o, const Pose& T, int i, double* J, double* ov) {
    double gs[3], ge[3];
    rp::to_cam(T, c.rc.pq6 + 6 * (size_t)i, gs);
    rp::to_cam(T, c.rc.pq6 + 6 * (size_t)i + 3, ge);
    const double lx = c.rc.l3[3 * (size_t)i], ly = c.rc.l3[3 * (size_t)i + 1], lz = c.rc.l3[3 * (size_t)i + 2];
    const double sp[2] = {o.cx + o.fx * gs[0] / gs[2], o.cy + o.fy * gs[1] / gs[2]}, ep[2] = {o.cx + o.fx * ge[0] / ge[2], o.cy + o.fy * ge[1] / ge[2]};
    const double ds = lx * sp[0] + ly * sp[1] + lz, de = lx * ep[0] + ly * ep[1] + lz;
    const double n = sqrt(ds * ds + de * de);
    if (J) {
        double Js[6], Je[6];
        rp::jac6(gs, lx, ly, o.fx, o.homog_th, Js);
        rp::jac6(ge, lx, ly, o.fx, o.homog_th, Je);
        const double dn = rp::max_th(o.homog_th, n);
        for (int q = 0; q < 6; ++q) J[q] = (Js[q] * ds + Je[q] * de) / dn;
        *ov = line_overlap(c.se4 + 4 * (size_t)i, c.se4 + 4 * (size_t)i + 2, sp, ep);
    }
    return n;
}
RP_HD void acc_add(Acc& a, const double* J, double r, double w) {      // :628-631
    int q = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) a.v[q++] += J[i] * J[j] * w;
    for (int i = 0; i < 6; ++i) a.v[21 + i] += J[i] * r * w;
    a.v[27] += r * r * w;
    ++a.n;
}
// a lane's share of one pass over the inliers.  optimizeFunctions: r = |err| sqrt(sigma2), w = cauchy(r); optimizeFunctionsRobust:
// r = |err|, w = cauchy(r / s); lines: w *= overlap in both
RP_HD void lane_pass(const Prob& c, const Opt& o, const Pose& T, bool robust, double s_p, double s_l, int lane, int nl, Acc& a) {
    double J[6];
    for (int i = lane; i < c.rc.np; i += nl)
        if (c.rc.pt_in[i]) {
            const double n = rp::point_feature(c.rc, o.ro, T, i, J);
            const double r = robust ? n : n * sqrt(c.pt_s2[i]);
            const double x = robust ? r / s_p : r;
            acc_add(a, J, r, 1.0 / (1.0 + x * x));
        }
    for (int i = lane; i < c.rc.nl; i += nl)
        if (c.rc.ln_in[i]) {
            double ov;
            const double n = line_feature(c, o.ro, T, i, J, &ov);
            const double r = robust ? n : n * sqrt(c.ln_s2[i]);
            const double x = robust ? r / s_l : r;
            double w = 1.0 / (1.0 + x * x);
            w *= ov;
            acc_add(a, J, r, w);
        }
}
// a lane's residuals into the workspace.  The cut (:1030, :1068): |err| sqrt(sigma2) of EVERY feature; the robust pass (:745, :763):
// |err| of the inliers
RP_HD int lane_residuals(const Prob& c, const Opt& o, const Pose& T, bool robust, int lane, int nl) {
    for (int i = lane; i < c.rc.np; i += nl)
        if (!robust || c.rc.pt_in[i]) { const double n = rp::point_feature(c.rc, o.ro, T, i, nullptr); c.res_p[i] = robust ? n : n * sqrt(c.pt_s2[i]); }
    for (int i = lane; i < c.rc.nl; i += nl)
        if (!robust || c.rc.ln_in[i]) { const double n = line_feature(c, o.ro, T, i, nullptr, nullptr); c.res_l[i] = robust ? n : n * sqrt(c.ln_s2[i]); }
    return 0;
}
RP_HD int lane_count(const uint8_t* m, int n, int lane, int nl) {
    int k = 0;
    for (int i = lane; i < n; i += nl) k += m[i] ? 1 : 0;
    return k;
}
// a lane's values (m null: all; else the flagged) whose known bits equal `prefix` and whose bit `bit` is clear
RP_HD int lane_count0(const double* v, const uint8_t* m, int n, int lane, int nl, uint64_t prefix, uint64_t known, uint64_t bit) {
    int k = 0;
    for (int i = lane; i < n; i += nl)
        if (!m || m[i]) { const uint64_t u = bits_of(v[i]); k += ((u & known) == prefix && !(u & bit)) ? 1 : 0; }
    return k;
}
RP_HD int lane_deviations(const double* v, double* d, const uint8_t* m, int n, double median, int lane, int nl) {
    for (int i = lane; i < n; i += nl)
        if (!m || m[i]) d[i] = (double)fabsf((float)(v[i] - median));      // fabsf of auxiliar.cpp:401 / :453: the deviation rounded to float
    return 0;
}
RP_HD void lane_mean(const double* v, int n, double thr, int lane, int nl, Acc& a) {      // auxiliar.cpp:406-426: v[0] the best samples, v[1] all
    for (int i = lane; i < n; i += nl) {
        if (v[i] < thr) { a.v[0] += v[i]; ++a.n; }
        a.v[1] += v[i];
    }
}
RP_HD int lane_cut(const double* v, uint8_t* m, int n, double mean, double th, int lane, int nl) {      // :1043, :1083; returns the remaining inliers
    int kept = 0;
    for (int i = lane; i < n; i += nl)
        if (m[i]) { if (fabs(v[i] - mean) > th) m[i] = 0; else ++kept; }
    return kept;
}

// element k of the ascending list of the n (m null) or the flagged values of v, all non-negative; the same in every lane
template <class Wave>
RP_HD double select(Wave& w, const double* v, const uint8_t* m, int n, int k) {
    uint64_t prefix = 0, known = 0;
    for (int b = 62; b >= 0; --b) {
        const uint64_t bit = (uint64_t)1 << b;
        const int c0 = w.sum_i([&](int lane, int nl) { return lane_count0(v, m, n, lane, nl, prefix, known, bit); });
        if (k >= c0) { k -= c0; prefix |= bit; }
        known |= bit;
    }
    return double_of(prefix);
}
// 1.4826 MAD of vector_stdv_mad (auxiliar.cpp:444-460) over the cnt values of v (m null: cnt = n); the median in *med
template <class Wave>
RP_HD double stdv_mad(Wave& w, const double* v, double* dev, const uint8_t* m, int n, int cnt, double* med) {
    if (cnt == 0) { *med = 0.0; return 0.0; }
    const double median = select(w, v, m, n, cnt / 2);
    w.sum_i([&](int lane, int nl) { return lane_deviations(v, dev, m, n, median, lane, nl); });
    *med = median;
    return 1.4826 * select(w, dev, m, n, cnt / 2);
}
// removeOutliers for one kind: statistics over ALL n residuals, removal among the flagged; returns the remaining inliers
template <class Wave>
RP_HD int cut_kind(Wave& w, const double* res, double* dev, uint8_t* m, int n, double inlier_k, double* mean_out, double* stdv_out) {
    double med;
    const double stdv = stdv_mad(w, res, dev, nullptr, n, n, &med);
    Acc a;
    w.sum([&](int lane, int nl, Acc& la) { lane_mean(res, n, 2.0 * stdv, lane, nl, la); }, a, 2);
    const double mean = a.n >= (int)(0.2 * (double)n) ? a.v[0] / (double)a.n : a.v[1] / (double)n;
    *mean_out = mean; *stdv_out = stdv;
    return w.sum_i([&](int lane, int nl) { return lane_cut(res, m, n, mean, inlier_k * stdv, lane, nl); });
}

// ---- the serial part --------------------------------------------------------------------------------------------------------------------
RP_HD bool pose_finite(const Pose& T) {
    bool f = true;
    for (int i = 0; i < 9; ++i) f = f && std::isfinite(T.R[i]);
    for (int i = 0; i < 3; ++i) f = f && std::isfinite(T.t[i]);
    return f;
}
RP_HD bool pose_is_identity(const Pose& T) {
    bool f = true;
    for (int i = 0; i < 9; ++i) f = f && T.R[i] == ((i % 4 == 0) ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) f = f && T.t[i] == 0.0;
    return f;
}
// isGoodSolution (:319-332) on DT_cov = H^-1: its eigenvalues are the reciprocals of H's (deviation: the reference decomposes the
// inverse).  0 = not good, 1 = good, -1 = H rank deficient by the QR's rule (no covariance)
RP_HD int is_good(const double* H21, double err, const Pose& T, double* cov_eig) {
    for (int i = 0; i < 6; ++i) cov_eig[i] = 0.0;
    if (rp::qr_solve6(H21, nullptr, nullptr) < 6) return -1;
    double ev[6];
    rp::sym_eig6(H21, ev);
    for (int i = 0; i < 6; ++i) cov_eig[i] = 1.0 / ev[5 - i];
    if (cov_eig[0] < 0.0 || cov_eig[5] > 1.0 || err < 0.0 || err > 1.0 || !pose_finite(T)) return 0;
    return 1;
}
RP_HD void take_sums(State& s, const Acc& a, int stage) {
    for (int q = 0; q < 21; ++q) s.H[q] = a.v[q];
    for (int q = 0; q < 6; ++q) s.g[q] = a.v[21 + q];
    s.e = a.v[27] / (double)a.n;
    ++s.iters[stage];
}
RP_HD void apply_step(State& s, const double* x) {      // DT = DT inverse_se3(expmap_se3(DT_inc))
    Pose E, Ei, Tn;
    rp::se3_exp(x, E); rp::se3_inv(E, Ei); rp::se3_mul(s.T, Ei, Tn);
    s.T = Tn;
}
// after the pass `it` of gaussNewtonOptimization (:431-453): 1 = go on, 0 = the stage ends, -1 = non-finite e, -2 = the return of :435
RP_HD int gn_step(State& s, const Acc& a, const Opt& o, int it, int stage) {
    take_sums(s, a, stage);
    if (!std::isfinite(s.e)) return -1;
    if (s.e > s.err_prev) return it > 0 ? 0 : -2;
    if (s.e < o.min_error || fabs(s.e - s.err_prev) < o.min_error_change) return 0;
    double x[6];
    rp::qr_solve6(s.H, s.g, x);
    apply_step(s, x);
    if (sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) < o.min_error_change && sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < o.min_error_change) return 0;
    s.err_prev = s.e;
    return 1;
}
// after a pass of gaussNewtonOptimizationRobust (:475-492): as above, -3 = logAbsDeterminant() < 0
RP_HD int gnr_step(State& s, const Acc& a, const Opt& o) {
    take_sums(s, a, 2);
    if (!std::isfinite(s.e)) return -1;
    if (fabs(s.e - s.err_prev) < o.min_error_change || s.e < o.min_error) return 0;
    double x[6], piv[6];
    rp::qr_solve6(s.H, s.g, x, piv);
    double lad = 0.0;
    for (int k = 0; k < 6; ++k) lad += log(piv[k]);      // sum log |R_kk|
    if (lad < 0.0) return -3;
    apply_step(s, x);
    double xx = 0.0;
    for (int q = 0; q < 6; ++q) xx += x[q] * x[q];
    if (sqrt(xx) < o.min_error_change) return 0;
    s.err_prev = s.e;
    return 1;
}
RP_HD double clamp_s(double s) {      // :798-806
    const double th_min = 0.0001, th_max = sqrt(7.815);
    if (s < th_min) s = th_min;
    if (s > th_max) s = th_max;
    return s;
}

// a stage's passes from s.T; returns the last verdict (0, -1, -2, -3; 0 also when the limit ran out or was 0)
template <class Wave>
RP_HD int run_stage(Wave& w, const Prob& c, const Opt& o, State& s, int stage, int lim) {
    s.err_prev = 999999999.9;
    for (int q = 0; q < 21; ++q) s.H[q] = 0.0;      // a stage without a pass reports zeros (the reference: uninitialised)
    for (int q = 0; q < 6; ++q) s.g[q] = 0.0;
    s.e = 0.0;
    int go = 1;
    for (int it = 0; it < lim && go == 1; ++it) {
        double s_p = 1.0, s_l = 1.0;
        if (stage == 2) {
            w.sum_i([&](int lane, int nl) { return lane_residuals(c, o, s.T, true, lane, nl); });
            double med;
            s_p = clamp_s(stdv_mad(w, c.res_p, c.dev_p, c.rc.pt_in, c.rc.np, s.n_pt, &med));
            s_l = clamp_s(stdv_mad(w, c.res_l, c.dev_l, c.rc.ln_in, c.rc.nl, s.n_ln, &med));
        }
        Acc a;
        w.sum([&](int lane, int nl, Acc& la) { lane_pass(c, o, s.T, stage == 2, s_p, s_l, lane, nl, la); }, a, rp::NACC);
        go = 0;
        if (w.leader()) go = stage == 2 ? gnr_step(s, a, o) : gn_step(s, a, o, it, stage);
        w.share(go, s.T);
    }
    return go == 1 ? 0 : go;
}

RP_HD void state_init(State& s, const double* T0_12) {
    if (T0_12) {
        for (int i = 0; i < 9; ++i) s.T0.R[i] = T0_12[i];
        for (int i = 0; i < 3; ++i) s.T0.t[i] = T0_12[9 + i];
    } else rp::se3_identity(s.T0);
    s.T = s.T0;
    for (int q = 0; q < 21; ++q) s.H[q] = 0.0;
    for (int q = 0; q < 6; ++q) s.g[q] = s.cov_eig[q] = 0.0;
    for (int q = 0; q < 4; ++q) s.stat[q] = 0.0;
    s.e = 0.0; s.err = -1.0; s.err_prev = 999999999.9;
    s.iters[0] = s.iters[1] = s.iters[2] = 0;
    s.status = OK; s.path = REFINED; s.good = 0; s.negdet = 0; s.n_pt = s.n_ln = 0;
}

// One problem (:359-418).  In the leader's State afterwards: T (DT as the optimiser left it), H and e of the last pass evaluated, err,
// cov_eig (zeros unless good), the cut's statistics, counts, path, status, good.  A non-finite e ends the run where it arose.
template <class Wave>
RP_HD void run(Wave& w, const Prob& c, const Opt& o, const double* T0_12, State& s) {
    state_init(s, T0_12);
    s.n_pt = w.sum_i([&](int lane, int nl) { return lane_count(c.rc.pt_in, c.rc.np, lane, nl); });
    s.n_ln = w.sum_i([&](int lane, int nl) { return lane_count(c.rc.ln_in, c.rc.nl, lane, nl); });
    int verdict = 0;      // of the last stage: 0, -1 non-finite, -2 the return of :435, -3 negative determinant
    if (s.n_pt + s.n_ln < o.min_features) {
        s.path = FEW_BEFORE;
        rp::se3_identity(s.T);
    } else {
        verdict = run_stage(w, c, o, s, 0, o.max_iters);      // DT_ = DT (:362): s.T0 keeps the start pose
        int good1 = 0;
        if (w.leader()) {
            if (verdict == 0) s.err = s.e;
            good1 = verdict == -1 ? -1 : (verdict == 0 && is_good(s.H, s.err, s.T, s.cov_eig) == 1 ? 1 : 0);
        }
        w.share(good1, s.T);
        if (good1 < 0) s.status = NONFINITE;
        else if (good1 == 1) {
            w.sum_i([&](int lane, int nl) { return lane_residuals(c, o, s.T, false, lane, nl); });      // at DT_, the first stage's pose
            if (c.rc.np > 0) s.n_pt = cut_kind(w, c.res_p, c.dev_p, c.rc.pt_in, c.rc.np, o.inlier_k, &s.stat[0], &s.stat[1]);
            if (c.rc.nl > 0) s.n_ln = cut_kind(w, c.res_l, c.dev_l, c.rc.ln_in, c.rc.nl, o.inlier_k, &s.stat[2], &s.stat[3]);
            if (s.n_pt + s.n_ln >= o.min_features) {
                s.T = s.T0;      // :374 passes DT, not DT_
                verdict = run_stage(w, c, o, s, 1, o.max_iters_ref);
                if (verdict == 0) s.err = s.e;
                else if (verdict == -2) s.err = -1.0;      // DT_cov stays the first stage's; err < 0 fails the test before it is looked at
                else if (verdict == -1) s.status = NONFINITE;
            } else {
                s.path = FEW_AFTER;
                rp::se3_identity(s.T);
            }
        } else {
            s.path = ROBUST;
            s.T = s.T0;
            verdict = run_stage(w, c, o, s, 2, o.max_iters_ref);
            if (verdict == 0) s.err = s.e;
            else if (verdict == -3) { s.T = s.T0; s.err = -1.0; s.negdet = 1; }      // :502-504
            else if (verdict == -1) s.status = NONFINITE;
        }
    }
    // :399-418, by the leader
    if (w.leader()) {
        for (int i = 0; i < 6; ++i) s.cov_eig[i] = 0.0;
        s.good = 0;
        if (s.status == OK && s.path != FEW_BEFORE && !s.negdet) {
            double ce[6];
            const int g = is_good(s.H, s.err, s.T, ce);
            if (g < 0) s.status = RANK;
            else if (g == 1 && !pose_is_identity(s.T)) {
                s.good = 1;
                for (int i = 0; i < 6; ++i) s.cov_eig[i] = ce[i];
            }
        }
        if (!s.good) s.err = -1.0;
    }
}

// curr_frame->DT (:401 / :412) from the State
RP_HD void frame_dt(const State& s, Pose& DT) {
    rp::se3_identity(DT);
    if (!s.good) return;
    Pose Ti;
    double x[6];
    rp::se3_inv(s.T, Ti); rp::se3_log(Ti, x); rp::se3_exp(x, DT);
}

// the lanes of the host: nl emulated lanes, one after the other (nl = 1: the plain serial loop of the reference)
struct HostWave {
    int nl;
    Acc* lanes;      // nl of them
    bool leader() const { return true; }
    void share(int&, Pose&) const {}
    template <class F> void sum(F f, Acc& a, int) {
        for (int l = 0; l < nl; ++l) { rp::acc_zero(lanes[l]); f(l, nl, lanes[l]); }
        rp::tree_sum(lanes, nl);
        a = lanes[0];
    }
    template <class F> int sum_i(F f) { int n = 0; for (int l = 0; l < nl; ++l) n += f(l, nl); return n; }
};

// ---- host only: DT_cov as the optimiser left it, row-major 6 x 6 -------------------------------------------------------------------------
// H^-1 column by column through the pivoted QR; the identity after the restore of :502-504; zeros where there is none
inline void covariance36(const State& s, double* cov36) {
    for (int i = 0; i < 36; ++i) cov36[i] = 0.0;
    if (s.negdet) { for (int i = 0; i < 6; ++i) cov36[i * 6 + i] = 1.0; return; }
    if (s.status != OK || s.path == FEW_BEFORE || rp::qr_solve6(s.H, nullptr, nullptr) < 6) return;
    for (int j = 0; j < 6; ++j) {
        double e[6] = {0, 0, 0, 0, 0, 0}, x[6];
        e[j] = 1.0;
        rp::qr_solve6(s.H, e, x);
        for (int i = 0; i < 6; ++i) cov36[i * 6 + j] = x[i];
    }
}

}  // namespace track
}  // namespace plba
