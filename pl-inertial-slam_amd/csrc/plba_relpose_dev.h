// plba_relpose_dev.h — the arithmetic of plba_relative_pose (include/plba.h), shared by the kernel (plba_relpose.hip, 64 lanes), the host
// check (plba_relpose_hostcheck.cpp, 64 emulated lanes) and the plain-C++ drop-in (include/plba_g2o/relative_pose.h, one lane).
//
// MapHandler::computeRelativePoseRobustGN / computeRelativePoseGN (src/mapHandler.cpp:3411-4066) for ONE candidate: a Gauss-Newton on one
// SE(3) increment over matched stereo points and line segments with scalar residuals (the norm of the reprojection error), Cauchy weights,
// the sqrt(chi2_th) cut and, for the robust variant, a refinement.  Everything here is a function of (lane, lane count): a lane adds its
// own features (lane, lane + nl, ...; points, then lines) in ascending order, the lanes' partial sums are added in a balanced tree over the
// lane index (run() of a Wave: the DPP / cross-row butterflies on the device, tree_sum() on the host: the same pairs, so the same bits up to
// the compiler's contraction of a * b + c), and one lane does the serial part: exit tests, the pivoted QR, expmap and the composition.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RP_HD __host__ __device__ inline
#else
#define RP_HD inline
#endif

namespace plba {
namespace relpose {

constexpr int OK = 0, EMPTY = 1, NONFINITE = 2, RANK = 3;      // PLBA_RELPOSE_* of include/plba.h
constexpr double EPS = 2.220446049250313e-16;                  // numeric_limits<double>::epsilon()
constexpr int NACC = 28;                                       // doubles of an Acc

struct Opt {
    int max_iters, max_iters_ref, protocol;
    double homog_th, cut;      // cut = sqrt(chi2_th)
    double fx, fy, cx, cy;
};
struct Cand {      // one candidate's matched features; the masks are read and, by the cut, written
    int np, nl;
    const double *P3, *uv2, *pq6, *l3;
    uint8_t *pt_in, *ln_in;
};
struct Pose { double R[9], t[3]; };
struct Acc { double v[NACC]; int n; };      // v: the 21 upper entries of H row by row, g[6], e
struct State {
    Pose T;
    double H[21], g[6], e, err_prev;
    int iters[2], status, n_inl;
};

// ---- stvo-pl/src/auxiliar.cpp:29-173 (the helpers of plba_lba.hip, copied: that file keeps its own) -----------------------------------
RP_HD void hat9(const double* w, double* s) { s[0] = 0; s[1] = -w[2]; s[2] = w[1]; s[3] = w[2]; s[4] = 0; s[5] = -w[0]; s[6] = -w[1]; s[7] = w[0]; s[8] = 0; }
RP_HD void mm3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
RP_HD void se3_identity(Pose& T) {
    for (int i = 0; i < 9; ++i) T.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    T.t[0] = T.t[1] = T.t[2] = 0.0;
}
RP_HD void se3_exp(const double* x, Pose& T) {      // expmap_se3, x = (t, w)
    const double w0 = x[3], w1 = x[4], w2 = x[5];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    se3_identity(T);
    T.t[0] = x[0]; T.t[1] = x[1]; T.t[2] = x[2];
    if (!(th < 0.000001)) {
        const double wn[3] = {w0 / th, w1 / th, w2 / th};
        double s[9], ss[9], V[9];
        hat9(wn, s); mm3(s, s, ss);
        const double sn = sin(th), cs = cos(th);
        for (int i = 0; i < 9; ++i) {
            const double I = (i % 4 == 0) ? 1.0 : 0.0;
            T.R[i] = I + s[i] * sn + ss[i] * (1.0 - cs);
            V[i] = I + s[i] * (1.0 - cs) / th + ss[i] * (th - sn) / th;
        }
        for (int i = 0; i < 3; ++i) T.t[i] = V[i * 3] * x[0] + V[i * 3 + 1] * x[1] + V[i * 3 + 2] * x[2];
    }
}
RP_HD void se3_inv(const Pose& T, Pose& Ti) {      // inverse_se3
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ti.R[i * 3 + j] = T.R[j * 3 + i];
    for (int i = 0; i < 3; ++i) Ti.t[i] = -(Ti.R[i * 3] * T.t[0] + Ti.R[i * 3 + 1] * T.t[1] + Ti.R[i * 3 + 2] * T.t[2]);
}
RP_HD void se3_mul(const Pose& A, const Pose& B, Pose& C) {
    mm3(A.R, B.R, C.R);
    for (int i = 0; i < 3; ++i) C.t[i] = A.R[i * 3] * B.t[0] + A.R[i * 3 + 1] * B.t[1] + A.R[i * 3 + 2] * B.t[2] + A.t[i];
}
RP_HD void inv3(const double* A, double* Ai) {      // Eigen's fixed-size inverse: cofactors over the determinant
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    Ai[0] = c00 / det; Ai[1] = (A[2] * A[7] - A[1] * A[8]) / det; Ai[2] = (A[1] * A[5] - A[2] * A[4]) / det;
    Ai[3] = c01 / det; Ai[4] = (A[0] * A[8] - A[2] * A[6]) / det; Ai[5] = (A[2] * A[3] - A[0] * A[5]) / det;
    Ai[6] = c02 / det; Ai[7] = (A[1] * A[6] - A[0] * A[7]) / det; Ai[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
RP_HD void se3_log(const Pose& T, double* x) {      // logmap_se3
    const double* R = T.R;
    double cosine = (R[0] + R[4] + R[8] - 1.0) / 2.0;
    cosine = cosine > 1.0 ? 1.0 : (cosine < -1.0 ? -1.0 : cosine);
    double sine = sqrt(1.0 - cosine * cosine);
    if (sine > 1.0) sine = 1.0;
    const double theta = acos(cosine);
    double w[3] = {0, 0, 0}, V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (theta > 0.000001) {
        const double f = theta / (2.0 * sine);
        w[0] = f * (R[7] - R[5]); w[1] = f * (R[2] - R[6]); w[2] = f * (R[3] - R[1]);
        const double wn[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
        double s[9], ss[9];
        hat9(wn, s); mm3(s, s, ss);
        for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + s[i] * (1.0 - cosine) / theta + ss[i] * (theta - sine) / theta;
    }
    double Vi[9];
    inv3(V, Vi);
    for (int i = 0; i < 3; ++i) x[i] = Vi[i * 3] * T.t[0] + Vi[i * 3 + 1] * T.t[1] + Vi[i * 3 + 2] * T.t[2];
    x[3] = w[0]; x[4] = w[1]; x[5] = w[2];
}

// ---- one feature (:3444-3475 points, :3484-3533 lines) -----------------------------------------------------------------------------
RP_HD double max_th(double th, double v) { return th < v ? v : th; }      // std::max(homogTh, v)
RP_HD void to_cam(const Pose& T, const double* X, double* g) {
    for (int i = 0; i < 3; ++i) g[i] = T.R[i * 3] * X[0] + T.R[i * 3 + 1] * X[1] + T.R[i * 3 + 2] * X[2] + T.t[i];
}
RP_HD void jac6(const double* g, double a, double b, double fx, double th, double* J) {
    const double gx = g[0], gy = g[1], gz = g[2];
    const double f = fx / max_th(th, gz * gz);
    J[0] = f * a * gz;
    J[1] = f * b * gz;
    J[2] = -f * (gx * a + gy * b);
    J[3] = -f * (gx * gy * a + gy * gy * b + gz * gz * b);
    J[4] = f * (gx * gx * a + gz * gz * a + gx * gy * b);
    J[5] = f * (gx * gz * b - gy * gz * a);
}
// the error norm of point i and, with J, its J_aux
RP_HD double point_feature(const Cand& c, const Opt& o, const Pose& T, int i, double* J) {
    double g[3];
    to_cam(T, c.P3 + 3 * (size_t)i, g);
    const double dx = o.cx + o.fx * g[0] / g[2] - c.uv2[2 * (size_t)i], dy = o.cy + o.fy * g[1] / g[2] - c.uv2[2 * (size_t)i + 1];
    const double n = sqrt(dx * dx + dy * dy);
    if (J) {
        jac6(g, dx, dy, o.fx, o.homog_th, J);
        const double dn = max_th(o.homog_th, n);
        for (int q = 0; q < 6; ++q) J[q] = J[q] / dn;
    }
    return n;
}
RP_HD double line_feature(const Cand& c, const Opt& o, const Pose& T, int i, double* J) {
    double gs[3], ge[3];
    to_cam(T, c.pq6 + 6 * (size_t)i, gs);
    to_cam(T, c.pq6 + 6 * (size_t)i + 3, ge);
    const double lx = c.l3[3 * (size_t)i], ly = c.l3[3 * (size_t)i + 1], lz = c.l3[3 * (size_t)i + 2];
    const double ds = lx * (o.cx + o.fx * gs[0] / gs[2]) + ly * (o.cy + o.fy * gs[1] / gs[2]) + lz;
    const double de = lx * (o.cx + o.fx * ge[0] / ge[2]) + ly * (o.cy + o.fy * ge[1] / ge[2]) + lz;
    const double n = sqrt(ds * ds + de * de);
    if (J) {
        double Js[6], Je[6];
        jac6(gs, lx, ly, o.fx, o.homog_th, Js);
        jac6(ge, lx, ly, o.fx, o.homog_th, Je);
        const double dn = max_th(o.homog_th, n);
        for (int q = 0; q < 6; ++q) J[q] = (Js[q] * ds + Je[q] * de) / dn;
    }
    return n;
}
RP_HD void acc_zero(Acc& a) {
    for (int q = 0; q < NACC; ++q) a.v[q] = 0.0;
    a.n = 0;
}
RP_HD void acc_add(Acc& a, const double* J, double n) {
    const double w = 1.0 / (1.0 + n * n);      // robustWeightCauchy, auxiliar.cpp:556-559
    int q = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) a.v[q++] += J[i] * J[j] * w;
    for (int i = 0; i < 6; ++i) a.v[21 + i] += J[i] * n * w;
    a.v[27] += n * n * w;
    ++a.n;
}
// a lane's share of one pass: its inlier points, then its inlier lines
RP_HD void lane_pass(const Cand& c, const Opt& o, const Pose& T, int lane, int nl, Acc& a) {
    acc_zero(a);
    double J[6];
    for (int i = lane; i < c.np; i += nl)
        if (c.pt_in[i]) { const double n = point_feature(c, o, T, i, J); acc_add(a, J, n); }
    for (int i = lane; i < c.nl; i += nl)
        if (c.ln_in[i]) { const double n = line_feature(c, o, T, i, J); acc_add(a, J, n); }
}
// a lane's share of the outlier cut (:3560-3591, :3827-3858): the unweighted norm against sqrt(chi2_th); returns its remaining inliers
RP_HD int lane_cut(const Cand& c, const Opt& o, const Pose& T, int lane, int nl) {
    int kept = 0;
    for (int i = lane; i < c.np; i += nl)
        if (c.pt_in[i]) { if (point_feature(c, o, T, i, nullptr) > o.cut) c.pt_in[i] = 0; else ++kept; }
    for (int i = lane; i < c.nl; i += nl)
        if (c.ln_in[i]) { if (line_feature(c, o, T, i, nullptr) > o.cut) c.ln_in[i] = 0; else ++kept; }
    return kept;
}
RP_HD int lane_count(const Cand& c, int lane, int nl) {
    int n = 0;
    for (int i = lane; i < c.np; i += nl) n += c.pt_in[i] ? 1 : 0;
    for (int i = lane; i < c.nl; i += nl) n += c.ln_in[i] ? 1 : 0;
    return n;
}
// the lanes' partial sums, added in a balanced tree over the lane index (what the butterflies of the kernel compute); nl a power of two
RP_HD void tree_sum(Acc* lanes, int nl) {
    for (int s = 1; s < nl; s <<= 1)
        for (int i = 0; i + s < nl; i += 2 * s) {
            for (int q = 0; q < NACC; ++q) lanes[i].v[q] += lanes[i + s].v[q];
            lanes[i].n += lanes[i + s].n;
        }
}

// ---- the 6 x 6 solve: Eigen's ColPivHouseholderQR by its documented algorithm ------------------------------------
// Householder QR with column pivoting by the largest remaining column norm (the first of equals), rank = the pivots above
// eps 6 |largest pivot|, the deficient part of the solution zero.  H21: upper entries row by row.  Returns the rank; x may be null.
// piv_out (optional): the six |R_kk| in pivot order, for logAbsDeterminant (plba_track_dev.h).
RP_HD int qr_solve6(const double* H21, const double* g, double* x, double* piv_out = nullptr) {
    double A[6][6], c[6], piv[6];
    int perm[6];
    {
        int q = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) { A[i][j] = H21[q]; A[j][i] = H21[q]; ++q; }
    }
    for (int i = 0; i < 6; ++i) { c[i] = g ? g[i] : 0.0; perm[i] = i; }
    for (int k = 0; k < 6; ++k) {
        int best = k;
        double nbest = -1.0;
        for (int j = k; j < 6; ++j) {
            double s = 0.0;
            for (int i = k; i < 6; ++i) s += A[i][j] * A[i][j];
            if (s > nbest) { nbest = s; best = j; }
        }
        if (best != k) {
            for (int i = 0; i < 6; ++i) { const double t = A[i][k]; A[i][k] = A[i][best]; A[i][best] = t; }
            const int t = perm[k]; perm[k] = perm[best]; perm[best] = t;
        }
        double s = 0.0;
        for (int i = k; i < 6; ++i) s += A[i][k] * A[i][k];
        const double nx = sqrt(s);
        if (!(nx > 0.0)) { piv[k] = 0.0; continue; }
        const double alpha = A[k][k] >= 0.0 ? -nx : nx;
        double v[6], vv = 0.0;
        for (int i = k; i < 6; ++i) v[i] = A[i][k];
        v[k] = v[k] - alpha;
        for (int i = k; i < 6; ++i) vv += v[i] * v[i];
        const double beta = 2.0 / vv;
        for (int j = k; j < 6; ++j) {
            double d = 0.0;
            for (int i = k; i < 6; ++i) d += v[i] * A[i][j];
            d = beta * d;
            for (int i = k; i < 6; ++i) A[i][j] = A[i][j] - v[i] * d;
        }
        double d = 0.0;
        for (int i = k; i < 6; ++i) d += v[i] * c[i];
        d = beta * d;
        for (int i = k; i < 6; ++i) c[i] = c[i] - v[i] * d;
        piv[k] = fabs(alpha);
    }
    double big = 0.0;
    for (int k = 0; k < 6; ++k) big = piv[k] > big ? piv[k] : big;
    if (piv_out) for (int k = 0; k < 6; ++k) piv_out[k] = piv[k];
    const double thr = EPS * 6.0 * big;
    int rank = 0;
    for (int k = 0; k < 6; ++k) rank += piv[k] > thr ? 1 : 0;
    if (x) {
        double y[6];
        for (int i = rank - 1; i >= 0; --i) {
            double s = 0.0;
            for (int j = i + 1; j < rank; ++j) s += A[i][j] * y[j];
            y[i] = (c[i] - s) / A[i][i];
        }
        for (int i = 0; i < 6; ++i) x[i] = 0.0;
        for (int i = 0; i < rank; ++i) x[perm[i]] = y[i];
    }
    return rank;
}

// ---- the pass control ------------------------------------------------------------------------------------------------------------------
RP_HD void state_init(State& s, const double* T0_12) {
    if (T0_12) {
        for (int i = 0; i < 9; ++i) s.T.R[i] = T0_12[i];
        for (int i = 0; i < 3; ++i) s.T.t[i] = T0_12[9 + i];
    } else se3_identity(s.T);
    for (int q = 0; q < 21; ++q) s.H[q] = 0.0;
    for (int q = 0; q < 6; ++q) s.g[q] = 0.0;
    s.e = 0.0; s.err_prev = 999999999.9;
    s.iters[0] = s.iters[1] = 0; s.status = OK; s.n_inl = 0;
}
// the serial part of one iteration, after the pass whose sums are `a` (:3537-3554): 1 = go on, 0 = the stage ends, -1 = the run ends
RP_HD int serial_step(State& s, const Acc& a, int stage) {
    for (int q = 0; q < 21; ++q) s.H[q] = a.v[q];
    for (int q = 0; q < 6; ++q) s.g[q] = a.v[21 + q];
    s.e = a.v[27] / (double)a.n;
    ++s.iters[stage];
    if (!std::isfinite(s.e)) { s.status = NONFINITE; return -1; }
    if (fabs(s.e - s.err_prev) < EPS || s.e < EPS) return 0;
    double x[6];
    qr_solve6(s.H, s.g, x);
    Pose E, Ei, Tn;
    se3_exp(x, E); se3_inv(E, Ei); se3_mul(s.T, Ei, Tn);
    s.T = Tn;
    double xx = 0.0;
    for (int q = 0; q < 6; ++q) xx += x[q] * x[q];
    if (sqrt(xx) < EPS) return 0;
    s.err_prev = s.e;
    return 1;
}
// what the run reports beside the State: logmap(T_inc) and the pose_inc of the protocol (:4060 / :3667)
RP_HD void finish(const State& s, int protocol, double* xlog6, double* pose_inc6) {
    se3_log(s.T, xlog6);
    Pose A, Ai;
    if (protocol == 0) se3_exp(xlog6, A);
    else A = s.T;
    se3_inv(A, Ai);
    se3_log(Ai, pose_inc6);
}

// One candidate.  A Wave supplies the lanes: pass(c, o, T, a) leaves the sums of all lanes in `a`, count(c) / cut(c, o, T) the inlier
// counts over all lanes, leader() names the lane of the serial part and share(go, T) gives every lane the leader's verdict and pose.
template <class Wave>
RP_HD void run(Wave& w, const Cand& c, const Opt& o, const double* T0_12, State& s) {
    state_init(s, T0_12);
    const int stages = o.protocol == 0 ? 2 : 1;
    s.n_inl = w.count(c);
    for (int st = 0; st < stages; ++st) {
        if (s.n_inl == 0) { s.status = EMPTY; break; }
        const int lim = st == 0 ? o.max_iters : o.max_iters_ref;
        int go = 1;
        for (int it = 0; it < lim && go == 1; ++it) {
            Acc a;
            w.pass(c, o, s.T, a);
            go = 0;
            if (w.leader()) go = serial_step(s, a, st);
            go = w.share(go, s.T);
        }
        if (go < 0) { s.status = NONFINITE; break; }
        if (st == 0) s.n_inl = w.cut(c, o, s.T);
    }
}

// the lanes of the host: nl emulated lanes, one after the other (nl = 1: the plain serial loop of the reference)
struct HostWave {
    int nl;
    Acc* lanes;      // nl of them
    bool leader() const { return true; }
    int share(int go, Pose&) const { return go; }
    void pass(const Cand& c, const Opt& o, const Pose& T, Acc& a) {
        for (int l = 0; l < nl; ++l) lane_pass(c, o, T, l, nl, lanes[l]);
        tree_sum(lanes, nl);
        a = lanes[0];
    }
    int count(const Cand& c) const { int n = 0; for (int l = 0; l < nl; ++l) n += lane_count(c, l, nl); return n; }
    int cut(const Cand& c, const Opt& o, const Pose& T) const { int n = 0; for (int l = 0; l < nl; ++l) n += lane_cut(c, o, T, l, nl); return n; }
};

// ---- host only: the uncertainty and the decision (:3593-3628, :3985-4021) --------------------------------------------------------------
struct Thresholds { double lc_res, lc_unc, lc_inl, lc_trs, lc_rot; };
struct Decision { double cov_eig[6], t, r; int status, lc_res, lc_unc, lc_inl, lc_trs, lc_rot, accepted; };

// eigenvalues of a symmetric 6 x 6 (upper entries row by row) by cyclic Jacobi, a fixed number of sweeps; ascending
RP_HD void sym_eig6(const double* H21, double* ev) {
    double A[6][6];
    int q = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = H21[q]; A[j][i] = H21[q]; ++q; }
    for (int sweep = 0; sweep < 12; ++sweep)
        for (int p = 0; p < 5; ++p)
            for (int r = p + 1; r < 6; ++r) {
                if (!(fabs(A[p][r]) > 0.0)) continue;
                const double th = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) { const double a = A[k][p], b = A[k][r]; A[k][p] = c * a - s * b; A[k][r] = s * a + c * b; }
                for (int k = 0; k < 6; ++k) { const double a = A[p][k], b = A[r][k]; A[p][k] = c * a - s * b; A[r][k] = s * a + c * b; }
            }
    for (int i = 0; i < 6; ++i) ev[i] = A[i][i];
    for (int i = 1; i < 6; ++i) { const double v = ev[i]; int j = i; while (j > 0 && ev[j - 1] > v) { ev[j] = ev[j - 1]; --j; } ev[j] = v; }
}
inline void decide(const State& s, const double* xlog6, int protocol, int n_features, const Thresholds& th, Decision& d) {
    const double inf = INFINITY;
    for (int i = 0; i < 6; ++i) d.cov_eig[i] = inf;
    d.t = d.r = 0.0;
    d.status = s.status;
    d.lc_res = d.lc_unc = d.lc_inl = d.lc_trs = d.lc_rot = d.accepted = 0;
    if (s.status != OK) return;
    d.lc_res = s.e < th.lc_res;
    if (qr_solve6(s.H, nullptr, nullptr) < 6) d.status = RANK;
    else {
        double ev[6];
        sym_eig6(s.H, ev);
        for (int i = 0; i < 6; ++i) d.cov_eig[i] = 1.0 / ev[5 - i];      // DT_cov = H^-1: its eigenvalues, ascending
        d.lc_unc = d.cov_eig[5] < th.lc_unc;
    }
    d.lc_inl = protocol == 0 ? 1 : ((double)s.n_inl / (double)(n_features > 0 ? n_features : 1) > th.lc_inl);
    d.t = sqrt(xlog6[0] * xlog6[0] + xlog6[1] * xlog6[1] + xlog6[2] * xlog6[2]);
    d.r = sqrt(xlog6[3] * xlog6[3] + xlog6[4] * xlog6[4] + xlog6[5] * xlog6[5]) * 180.0 / 3.14159265358979323846;
    d.lc_trs = d.t < th.lc_trs;
    d.lc_rot = d.r < th.lc_rot;
    d.accepted = d.status == OK && d.lc_res && d.lc_unc && d.lc_inl && d.lc_trs && d.lc_rot;
}

}  // namespace relpose
}  // namespace plba
