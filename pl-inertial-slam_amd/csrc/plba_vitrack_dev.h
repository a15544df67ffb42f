// plba_vitrack_dev.h — the arithmetic of plba_track_inertial (include/plba.h), shared by the kernel (plba_vitrack.hip, 64 lanes), the host
// check (plba_vitrack_hostcheck.cpp, 64 emulated lanes) and the plain-C++ drop-in (include/plba_g2o/track_inertial.h, one lane).
//
// ONE motion-only visual-inertial problem: two VertexNavState (i the anchor, j the new frame), one EdgeNavState between them, an
// EdgeNavStatePrior on i when i is free, pose-only point and line edges on j (IMU/g2otypes.h:411-695); g2o's Levenberg loop as
// SparseOptimizer::optimizeHost states it (include/plba_g2o/g2o_compat.h), in rounds with a chi2 gate after each, then one linearisation
// at the result and the Schur complement onto j, carried into the basis of an EdgeNavStatePrior on j.  Every formula is plba_math.h's.
//
// The protocol is written against a Wave: sum() adds the lanes' partial sums of the visual edges (21 + 6 + 1 doubles) in the balanced tree
// of plba_relpose_dev.h; par() runs one phase of lane functions on the shared block sh() (LDS on the device) and ends in a barrier; what
// stands between two phases is uniform: every lane computes it from the shared block and gets the same bits, so every branch is uniform.
// A phase never reads what another lane writes in the same phase, so the lanes of the host may run one after the other.  The system, the
// factor, the IMU edge's 15 x 30 Jacobian and the states live in the shared block and are indexed at run time there, never in registers.
// The order of every sum is fixed and does not depend on the lane count: the host check with 64 lanes and the drop-in with one lane differ
// only in the tree of the visual sums.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // __forceinline__ of plba_math.h's PLBA_HD
#endif

#include "plba_math.h"
#include "plba_relpose_dev.h"

namespace plba {
namespace vitrack {

namespace rp = relpose;
using rp::Acc;

constexpr int OK = 0, NONFINITE = 2, SINGULAR = 3;      // PLBA_VITRACK_* of include/plba.h
constexpr int STOP_ITERS = 0, STOP_TRIALS = 1, STOP_RHO0 = 2, STOP_LAMBDA = 3, STOP_NONFINITE = 4;
constexpr int N = 30, ND = 15, MAX_ROUNDS = 8, SREC = 24;      // SREC: a state record in the shared block (22 doubles in use)
constexpr int OUT_D = 22 + 22 + 900 + 225 + 3, OUT_I = 8 + 8 + 6;      // plba_vitrack_result as doubles and int32

// the shared block, in doubles
constexpr int SH_H = 0, SH_L = SH_H + 900, SH_J = SH_L + 900, SH_OJ = SH_J + 450, SH_JP = SH_OJ + 450, SH_OJP = SH_JP + 225, SH_B = SH_OJP + 225,
              SH_X = SH_B + 30, SH_R = SH_X + 30, SH_E = SH_R + 30, SH_WE = SH_E + 15, SH_EP = SH_WE + 15, SH_WEP = SH_EP + 15, SH_ACC = SH_WEP + 15,
              SH_S = SH_ACC + 28, SH_TOTAL = SH_S + 4 * SREC;

struct Opt {
    int rounds, iters, max_trials, robust_rounds;
    double tau, user_lambda_init, huber_pt, huber_ln, huber_imu, chi2_pt, chi2_ln;
    double gw[3];
    Cam cam;
};
struct Prob {      // one problem; the masks are read and, by the gate, written
    int np, nl, anchor_free;
    const double *Pw3, *uv2, *pt_w, *pq6, *l3, *ln_w;
    uint8_t *pt_in, *ln_in;
    const double *si0, *sj0, *pre, *ipvr, *ibias, *pst, *pinfo;      // pst, pinfo: read when anchor_free
    double* od;        // OUT_D doubles
    int32_t* oi;       // OUT_I int32
};

// ---- one lane's share of the visual edges ---------------------------------------------------------------------------------------------
// a.v[0]: the (robustified) chi2; a.v[1 .. 21]: the upper entries of sum J^T w J over the columns (dP, dPhi), row by row; a.v[22 .. 27]:
// sum J^T w e
PLBA_HD void acc_edge(Acc& a, const double* Jp12, const double* e2, double wgt) {
    int q = 1;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { a.v[q] += (Jp12[i] * Jp12[j] + Jp12[6 + i] * Jp12[6 + j]) * wgt; ++q; }
#pragma unroll
    for (int i = 0; i < 6; ++i) a.v[22 + i] += (Jp12[i] * e2[0] + Jp12[6 + i] * e2[1]) * wgt;
}
PLBA_HD void kc_load(const Opt& o, const double* sj, double* kc) { kfcam_make(o.cam, sj, kc); }
PLBA_HD void lane_pass(const Prob& c, const Opt& o, const double* kc, bool jac, bool robust, int lane, int nl, Acc& a) {
    double e2[2], Jp[12], Jl[6];
    bool dpos;
    for (int i = lane; i < c.np; i += nl)
        if (c.pt_in[i]) {
            const double* P = c.Pw3 + 3 * (size_t)i;
            point_edge(o.cam, kc, v3(P[0], P[1], P[2]), c.uv2[2 * (size_t)i], c.uv2[2 * (size_t)i + 1], e2, Jp, Jl, dpos, jac);
            const double chi = c.pt_w[i] * (e2[0] * e2[0] + e2[1] * e2[1]);
            double rho0 = chi, rho1 = 1.0;
            if (robust) huber(chi, o.huber_pt, rho0, rho1);
            a.v[0] += rho0;
            if (jac) acc_edge(a, Jp, e2, rho1 * c.pt_w[i]);
        }
    for (int i = lane; i < c.nl; i += nl)
        if (c.ln_in[i]) {
            const double* Q = c.pq6 + 6 * (size_t)i;
            const double* l = c.l3 + 3 * (size_t)i;
            line_edge(o.cam, kc, v3(Q[0], Q[1], Q[2]), v3(Q[3], Q[4], Q[5]), l[0], l[1], l[2], true, e2, Jp, Jl, dpos, jac);
            const double chi = c.ln_w[i] * (e2[0] * e2[0] + e2[1] * e2[1]);
            double rho0 = chi, rho1 = 1.0;
            if (robust) huber(chi, o.huber_ln, rho0, rho1);
            a.v[0] += rho0;
            if (jac) acc_edge(a, Jp, e2, rho1 * c.ln_w[i]);
        }
}
// the gate: every visual edge, active or not, at the estimate behind kc
PLBA_HD int lane_gate(const Prob& c, const Opt& o, const double* kc, int lane, int nl) {
    double e2[2], Jp[12], Jl[6];
    bool dpos;
    for (int i = lane; i < c.np; i += nl) {
        const double* P = c.Pw3 + 3 * (size_t)i;
        point_edge(o.cam, kc, v3(P[0], P[1], P[2]), c.uv2[2 * (size_t)i], c.uv2[2 * (size_t)i + 1], e2, Jp, Jl, dpos, false);
        const double chi = c.pt_w[i] * (e2[0] * e2[0] + e2[1] * e2[1]);
        c.pt_in[i] = (chi > o.chi2_pt || !dpos) ? 0 : 1;
    }
    for (int i = lane; i < c.nl; i += nl) {
        const double* Q = c.pq6 + 6 * (size_t)i;
        const double* l = c.l3 + 3 * (size_t)i;
        line_edge(o.cam, kc, v3(Q[0], Q[1], Q[2]), v3(Q[3], Q[4], Q[5]), l[0], l[1], l[2], true, e2, Jp, Jl, dpos, false);
        const double chi = c.ln_w[i] * (e2[0] * e2[0] + e2[1] * e2[1]);
        c.ln_in[i] = (chi > o.chi2_ln || !dpos) ? 0 : 1;
    }
    return 0;
}
PLBA_HD int lane_count(const uint8_t* m, int n, int lane, int nl) {
    int k = 0;
    for (int i = lane; i < n; i += nl) k += m[i] ? 1 : 0;
    return k;
}

// ---- the serial pieces (lane 0 writes them into the shared block) ------------------------------------------------------------------------
PLBA_HD void state_copy(const double* s, double* o) {
    for (int k = 0; k < 22; ++k) o[k] = s[k];
    o[22] = o[23] = 0.0;
}
PLBA_HD void state_oplus(const double* s, const double* u15, double* o) {      // NavState::IncSmall: kf_oplus_pvr, then the bias update
    kf_oplus_pvr(s, u15, o);
    for (int k = 0; k < 6; ++k) { o[10 + k] = s[10 + k]; o[16 + k] = s[16 + k] + u15[9 + k]; }
    o[22] = o[23] = 0.0;
}
// EdgeNavStatePrior::computeError (plba_detail::prior_error of the facade, Sophus' normalisations included)
PLBA_HD void prior_error15(const double* p, const double* s, double* e15) {
    for (int k = 0; k < 6; ++k) e15[k] = p[k] - s[k];
    Q4 qp, qs;
    qp.x = p[6]; qp.y = p[7]; qp.z = p[8]; qp.w = p[9];
    qs.x = s[6]; qs.y = s[7]; qs.z = s[8]; qs.w = s[9];
    qp = q_normalized(q_normalized(qp)); qs = q_normalized(q_normalized(qs));
    const Q4 inv = q_normalized(q_conj(qp));
    const V3 w = so3_log(q_normalized(q_mul(q_normalized(inv), qs)));
    e15[6] = w.x; e15[7] = w.y; e15[8] = w.z;
    for (int k = 0; k < 3; ++k) {
        e15[9 + k] = (p[10 + k] + p[16 + k]) - (s[10 + k] + s[16 + k]);
        e15[12 + k] = (p[13 + k] + p[19 + k]) - (s[13 + k] + s[19 + k]);
    }
}
// EdgeNavStatePrior::linearizeOplus into a zeroed 15 x 15: -R, -I, JrInv(rPhi), -I, -I
PLBA_HD void prior_jacobian(const double* s, const double* e15, double* J) {
    Q4 q; q.x = s[6]; q.y = s[7]; q.z = s[8]; q.w = s[9];
    const M3 R = q_to_R(q), Ji = so3_JrInv(v3(e15[6], e15[7], e15[8]));
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            J[r * ND + cc] = -R.a[r * 3 + cc];
            J[(3 + r) * ND + 3 + cc] = (r == cc) ? -1.0 : 0.0;
            J[(6 + r) * ND + 6 + cc] = Ji.a[r * 3 + cc];
        }
    for (int d = 9; d < ND; ++d) J[d * ND + d] = -1.0;
}
// EdgeNavState::linearizeOplus into a zeroed 15 x 30 [d e / d i | d e / d j] (plba_detail::navstate_jacobians)
PLBA_HD void imu_jacobian(const double* si, const double* sj, const double* pre, const double* gw, const double* e15, double* J) {
    pvr_jacobians(si, sj, pre, v3(gw[0], gw[1], gw[2]), e15, J, J + ND, J + 9, N, N);
    for (int d = 9; d < ND; ++d) { J[d * N + d] = -1.0; J[d * N + ND + d] = 1.0; }
}
// the information of the IMU edge, blockdiag(info_pvr81, info_bias36), entry (r, k)
PLBA_HD double imu_info(const Prob& c, int r, int k) {
    if (r < 9) return k < 9 ? c.ipvr[r * 9 + k] : 0.0;
    return k < 9 ? 0.0 : c.ibias[(r - 9) * 6 + (k - 9)];
}
// e^T Omega e as g2o's chi2(): sum_i e_i (sum_j Omega_ij e_j)
PLBA_HD double imu_chi2(const Prob& c, const double* e) {
    double s = 0.0;
    for (int i = 0; i < 9; ++i) { double t = 0.0; for (int j = 0; j < 9; ++j) t += c.ipvr[i * 9 + j] * e[j]; s += e[i] * t; }
    for (int i = 0; i < 6; ++i) { double t = 0.0; for (int j = 0; j < 6; ++j) t += c.ibias[i * 6 + j] * e[9 + j]; s += e[9 + i] * t; }
    return s;
}
PLBA_HD double prior_chi2(const Prob& c, const double* e) {
    double s = 0.0;
    for (int i = 0; i < ND; ++i) { double t = 0.0; for (int j = 0; j < ND; ++j) t += c.pinfo[i * ND + j] * e[j]; s += e[i] * t; }
    return s;
}
// column of the visual 6 x 6 (dP, dPhi) behind column r of the system, or -1
PLBA_HD int vis_col(int r) {
    const int k = r - ND;
    return (k >= 0 && k < 3) ? k : (k >= 6 && k < 9) ? k - 3 : -1;
}

// ---- chi2 alone: the active visual edges, the IMU edge, the prior ----------------------------------------------------------------------
template <class Wave>
PLBA_HD double chi_only(Wave& w, const Prob& c, const Opt& o, const double* si, const double* sj, bool robust) {
    double* sh = w.sh();
    double kc[12];
    kc_load(o, sj, kc);
    Acc a;
    w.sum([&](int lane, int nl, Acc& la) { lane_pass(c, o, kc, false, robust, lane, nl, la); }, a, 1);
    w.par([&](int lane, int) {
        if (lane != 0) return;
        pvr_error(si, sj, c.pre, v3(o.gw[0], o.gw[1], o.gw[2]), sh + SH_E);
        bias_error(si, sj, sh + SH_E + 9);
        if (c.anchor_free) prior_error15(c.pst, si, sh + SH_EP);
    });
    double ci = imu_chi2(c, sh + SH_E), r1;
    if (o.huber_imu > 0.0) huber(ci, o.huber_imu, ci, r1);
    double chi = a.v[0] + ci;
    if (c.anchor_free) chi += prior_chi2(c, sh + SH_EP);
    return chi;
}

// ---- chi2 and the system: H (both triangles) and b of the active edges in [i | j] order; a fixed i leaves zero rows and columns --------
template <class Wave>
PLBA_HD double build(Wave& w, const Prob& c, const Opt& o, const double* si, const double* sj, bool robust) {
    double* sh = w.sh();
    const int o0 = c.anchor_free ? 0 : ND;
    double kc[12];
    kc_load(o, sj, kc);
    Acc a;
    w.sum([&](int lane, int nl, Acc& la) { lane_pass(c, o, kc, true, robust, lane, nl, la); }, a, rp::NACC);
    w.par([&](int lane, int nl) {      // the errors and the visual sums by lane 0; the Jacobians' zeros by all
        for (int q = lane; q < 450 + 225; q += nl) sh[q < 450 ? SH_J + q : SH_JP + (q - 450)] = 0.0;
        if (lane != 0) return;
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q) sh[SH_ACC + q] = a.v[q];
        pvr_error(si, sj, c.pre, v3(o.gw[0], o.gw[1], o.gw[2]), sh + SH_E);
        bias_error(si, sj, sh + SH_E + 9);
        if (c.anchor_free) prior_error15(c.pst, si, sh + SH_EP);
    });
    w.par([&](int lane, int) {
        if (lane != 0) return;
        imu_jacobian(si, sj, c.pre, o.gw, sh + SH_E, sh + SH_J);
        if (c.anchor_free) prior_jacobian(si, sh + SH_EP, sh + SH_JP);
    });
    double ci = imu_chi2(c, sh + SH_E), wi = 1.0;
    if (o.huber_imu > 0.0) huber(ci, o.huber_imu, ci, wi);
    double chi = a.v[0] + ci;
    if (c.anchor_free) chi += prior_chi2(c, sh + SH_EP);
    w.par([&](int lane, int nl) {      // Omega J and Omega e of the IMU edge and of the prior
        for (int q = lane; q < 450 + 15 + (c.anchor_free ? 225 + 15 : 0); q += nl) {
            double t = 0.0;
            if (q < 450) {
                const int r = q / N, cc = q % N;
                for (int k = 0; k < ND; ++k) t += imu_info(c, r, k) * sh[SH_J + k * N + cc];
                sh[SH_OJ + q] = t;
            } else if (q < 465) {
                const int r = q - 450;
                for (int k = 0; k < ND; ++k) t += imu_info(c, r, k) * sh[SH_E + k];
                sh[SH_WE + r] = t;
            } else if (q < 690) {
                const int r = (q - 465) / ND, cc = (q - 465) % ND;
                for (int k = 0; k < ND; ++k) t += c.pinfo[r * ND + k] * sh[SH_JP + k * ND + cc];
                sh[SH_OJP + (q - 465)] = t;
            } else {
                const int r = q - 690;
                for (int k = 0; k < ND; ++k) t += c.pinfo[r * ND + k] * sh[SH_EP + k];
                sh[SH_WEP + r] = t;
            }
        }
    });
    w.par([&](int lane, int nl) {      // the lower triangle and b: the visual sums, + the IMU edge, + the prior
        for (int q = lane; q < 930; q += nl) {
            if (q < 900) {
                const int r = q / N, cc = q % N;
                if (cc > r) continue;
                double h = 0.0;
                if (cc >= o0) {
                    const int vr = vis_col(r), vc = vis_col(cc);
                    if (vr >= 0 && vc >= 0) h = sh[SH_ACC + 1 + vc * 6 - vc * (vc - 1) / 2 + (vr - vc)];      // vc <= vr
                    double t = 0.0;
                    for (int k = 0; k < ND; ++k) t += sh[SH_J + k * N + r] * sh[SH_OJ + k * N + cc];
                    h += wi * t;
                    if (c.anchor_free && r < ND) {
                        double u = 0.0;
                        for (int k = 0; k < ND; ++k) u += sh[SH_JP + k * ND + r] * sh[SH_OJP + k * ND + cc];
                        h += u;
                    }
                }
                sh[SH_H + q] = h;
            } else {
                const int r = q - 900;
                double g = 0.0;
                if (r >= o0) {
                    const int vr = vis_col(r);
                    if (vr >= 0) g = sh[SH_ACC + 22 + vr];
                    double t = 0.0;
                    for (int k = 0; k < ND; ++k) t += sh[SH_J + k * N + r] * sh[SH_WE + k];
                    g += wi * t;
                    if (c.anchor_free && r < ND) {
                        double u = 0.0;
                        for (int k = 0; k < ND; ++k) u += sh[SH_JP + k * ND + r] * sh[SH_WEP + k];
                        g += u;
                    }
                }
                sh[SH_B + r] = -g;
            }
        }
    });
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 900; q += nl) {
            const int r = q / N, cc = q % N;
            if (cc > r) sh[SH_H + q] = sh[SH_H + cc * N + r];
        }
    });
    return chi;
}

// ---- LL^T of rows and columns [lo, hi) of the factor block, in place; false on a pivot that is not > 0 ----------------------------------
// column by column: every row's sum in ascending k into SH_R, then the division; the operations of an entry do not depend on the lanes
template <class Wave>
PLBA_HD bool factor(Wave& w, int lo, int hi) {
    double* sh = w.sh();
    double* L = sh + SH_L;
    for (int j = lo; j < hi; ++j) {
        w.par([&](int lane, int nl) {
            for (int i = j + lane; i < hi; i += nl) {
                double s = L[i * N + j];
                for (int k = lo; k < j; ++k) s -= L[i * N + k] * L[j * N + k];
                sh[SH_R + i] = s;
            }
        });
        const double d = sh[SH_R + j];
        if (!(d > 0.0)) return false;
        const double rd = sqrt(d);
        w.par([&](int lane, int nl) {
            for (int i = j + lane; i < hi; i += nl) L[i * N + j] = (i == j) ? rd : sh[SH_R + i] / rd;
        });
    }
    return true;
}
// (H + lambda I) x = b over [o0, 30) into SH_X; zeros and false when the factorisation fails
template <class Wave>
PLBA_HD bool solve(Wave& w, int o0, double lambda) {
    double* sh = w.sh();
    double* L = sh + SH_L;
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 930; q += nl) {
            if (q < 900) { const int r = q / N, cc = q % N; sh[SH_L + q] = sh[SH_H + q] + (r == cc ? lambda : 0.0); }
            else sh[SH_X + (q - 900)] = 0.0;
        }
    });
    if (!factor(w, o0, N)) return false;
    w.par([&](int lane, int nl) { for (int i = o0 + lane; i < N; i += nl) sh[SH_R + i] = sh[SH_B + i]; });
    for (int k = o0; k < N; ++k) {      // L y = b, column by column
        const double y = sh[SH_R + k] / L[k * N + k];
        w.par([&](int lane, int nl) {
            if (lane == 0) sh[SH_X + k] = y;
            for (int i = k + 1 + lane; i < N; i += nl) sh[SH_R + i] -= L[i * N + k] * y;
        });
    }
    for (int k = N - 1; k >= o0; --k) {      // L^T x = y
        const double x = sh[SH_X + k] / L[k * N + k];
        w.par([&](int lane, int nl) {
            if (lane == 0) sh[SH_X + k] = x;
            for (int i = o0 + lane; i < k; i += nl) sh[SH_X + i] -= L[k * N + i] * x;
        });
    }
    return true;
}

// ---- S = H_jj - H_ji H_ii^-1 H_ij and next_prior_info = J^-T S J^-1 into SH_JP (15 x 15); false = SINGULAR -----------------------------
template <class Wave>
PLBA_HD bool marginal(Wave& w, const Prob& c, const double* sj) {
    double* sh = w.sh();
    double* L = sh + SH_L;
    double* Y = sh + SH_J;       // 15 x 15
    double* S = sh + SH_OJ;      // 15 x 15
    double* T = sh + SH_OJP;     // 15 x 15
    double* A = sh + SH_X;       // R_j^-1
    bool ok = true;
    if (c.anchor_free) {
        w.par([&](int lane, int nl) { for (int q = lane; q < 900; q += nl) sh[SH_L + q] = sh[SH_H + q]; });
        ok = factor(w, 0, ND);
        if (ok) {
            w.par([&](int lane, int nl) {      // Y = L^-1 H_ij, a column per lane
                for (int cc = lane; cc < ND; cc += nl)
                    for (int k = 0; k < ND; ++k) {
                        double s = sh[SH_H + k * N + ND + cc];
                        for (int m = 0; m < k; ++m) s -= L[k * N + m] * Y[m * ND + cc];
                        Y[k * ND + cc] = s / L[k * N + k];
                    }
            });
        }
    }
    if (!ok) return false;
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 225; q += nl) {
            const int r = q / ND, cc = q % ND;
            if (cc > r) continue;
            double s = sh[SH_H + (ND + r) * N + ND + cc];
            if (c.anchor_free) for (int k = 0; k < ND; ++k) s -= Y[k * ND + r] * Y[k * ND + cc];
            S[q] = s;
        }
    });
    w.par([&](int lane, int nl) {      // S's other triangle, its copy for the pivot test, and R_j^-1
        for (int q = lane; q < 225; q += nl) {
            const int r = q / ND, cc = q % ND;
            if (cc > r) S[q] = S[cc * ND + r];
            L[(ND + r) * N + ND + cc] = cc > r ? S[cc * ND + r] : S[q];
        }
        if (lane == 0) {
            Q4 q; q.x = sj[6]; q.y = sj[7]; q.z = sj[8]; q.w = sj[9];
            const M3 Ri = inv3(q_to_R(q));
#pragma unroll
            for (int k = 0; k < 9; ++k) A[k] = Ri.a[k];
        }
    });
    if (!factor(w, ND, N)) return false;
    // D = J^-1 = blockdiag(-R^-1, -I, I, -I, -I); T = S D, then the lower triangle of D^T T
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 225; q += nl) {
            const int r = q / ND, cc = q % ND;
            double t;
            if (cc < 3) t = -(S[r * ND] * A[cc] + S[r * ND + 1] * A[3 + cc] + S[r * ND + 2] * A[6 + cc]);
            else t = (cc >= 6 && cc < 9) ? S[q] : -S[q];
            T[q] = t;
        }
    });
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 225; q += nl) {
            const int r = q / ND, cc = q % ND;
            if (cc > r) continue;
            double t;
            if (r < 3) t = -(A[r] * T[cc] + A[3 + r] * T[ND + cc] + A[6 + r] * T[2 * ND + cc]);
            else t = (r >= 6 && r < 9) ? T[q] : -T[q];
            sh[SH_JP + q] = t;
        }
    });
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 225; q += nl) {
            const int r = q / ND, cc = q % ND;
            if (cc > r) sh[SH_JP + q] = sh[SH_JP + cc * ND + r];
        }
    });
    return true;
}

// ---- one problem ----------------------------------------------------------------------------------------------------------------------
template <class Wave>
PLBA_HD void run(Wave& w, const Prob& c, const Opt& o) {
    double* sh = w.sh();
    const int o0 = c.anchor_free ? 0 : ND;
    int cur = 0;      // the state pair in use: i at SH_S + 2 cur SREC, j behind it
    w.par([&](int lane, int) {
        if (lane != 0) return;
        state_copy(c.si0, sh + SH_S); state_copy(c.sj0, sh + SH_S + SREC);
        for (int k = 0; k < OUT_I; ++k) c.oi[k] = 0;
    });
    int status = OK, trials = 0, failures = 0;
    double lambda = 0.0;
    const double chi_initial = chi_only(w, c, o, sh + SH_S, sh + SH_S + SREC, 0 < o.robust_rounds);
    double chi_final = chi_initial;
    if (!std::isfinite(chi_initial)) status = NONFINITE;
    for (int r = 0; r < o.rounds && status == OK; ++r) {
        const bool robust = r < o.robust_rounds;
        double ni = 2.0;
        int done = 0, stop = STOP_ITERS;
        for (int it = 0; it < o.iters && stop == STOP_ITERS; ++it) {
            const double* si = sh + SH_S + 2 * cur * SREC;
            double chi = build(w, c, o, si, si + SREC, robust);
            if (!std::isfinite(chi)) { status = NONFINITE; stop = STOP_NONFINITE; chi_final = chi; break; }
            if (it == 0) {      // computeLambdaInit, as a new optimize() call would
                if (o.user_lambda_init > 0.0) lambda = o.user_lambda_init;
                else {
                    double md = 0.0;
                    for (int i = o0; i < N; ++i) { const double v = fabs(sh[SH_H + i * N + i]); md = md < v ? v : md; }
                    lambda = o.tau * md;
                }
                ni = 2.0;
            }
            double rho = 0.0;
            int qmax = 0;
            do {
                const bool sok = solve(w, o0, lambda);
                if (!sok) ++failures;
                double* ci = sh + SH_S + 2 * (cur ^ 1) * SREC;
                double temp = DBL_MAX;
                if (sok) {
                    w.par([&](int lane, int) {
                        if (lane != 0) return;
                        if (c.anchor_free) state_oplus(si, sh + SH_X, ci); else state_copy(si, ci);
                        state_oplus(si + SREC, sh + SH_X + ND, ci + SREC);
                    });
                    temp = chi_only(w, c, o, ci, ci + SREC, robust);
                }
                double scale = 1e-3;
                for (int i = o0; i < N; ++i) scale += sh[SH_X + i] * (lambda * sh[SH_X + i] + sh[SH_B + i]);
                rho = (chi - temp) / scale;
                ++trials;
                if (rho > 0.0 && std::isfinite(temp)) {
                    const double t = 2.0 * rho - 1.0;
                    double alpha = 1.0 - t * t * t;
                    alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
                    lambda *= (1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0);
                    ni = 2.0;
                    chi = temp;
                    cur ^= 1;
                    si = sh + SH_S + 2 * cur * SREC;
                } else {
                    lambda *= ni; ni *= 2.0;
                    if (!std::isfinite(lambda)) break;
                }
                ++qmax;
            } while (rho < 0.0 && qmax < o.max_trials);
            ++done;
            chi_final = chi;
            if (qmax == o.max_trials) stop = STOP_TRIALS;
            else if (rho == 0.0) stop = STOP_RHO0;
            else if (!std::isfinite(lambda)) stop = STOP_LAMBDA;
        }
        if (w.leader()) { c.oi[r] = done; c.oi[MAX_ROUNDS + r] = stop; }
        if (status == OK) {      // the gate: every visual edge at the round's estimate
            double kc[12];
            kc_load(o, sh + SH_S + 2 * cur * SREC + SREC, kc);
            w.sum_i([&](int lane, int nl) { return lane_gate(c, o, kc, lane, nl); });
        }
    }
    const double* si = sh + SH_S + 2 * cur * SREC;
    bool have_H = false, have_prior = false;
    if (status == OK) {      // the final linearisation: the active edges, the last round's kernels, no damping
        const int last = o.rounds > 0 ? o.rounds - 1 : 0;
        chi_final = build(w, c, o, si, si + SREC, last < o.robust_rounds);
        if (!std::isfinite(chi_final)) status = NONFINITE;
        else {
            have_H = true;
            have_prior = marginal(w, c, si + SREC);
            if (!have_prior) status = SINGULAR;
        }
    }
    const int n_pt = w.sum_i([&](int lane, int nl) { return lane_count(c.pt_in, c.np, lane, nl); });
    const int n_ln = w.sum_i([&](int lane, int nl) { return lane_count(c.ln_in, c.nl, lane, nl); });
    w.par([&](int lane, int nl) {
        for (int q = lane; q < 900 + 225; q += nl) {
            if (q < 900) c.od[44 + q] = have_H ? sh[SH_H + q] : 0.0;
            else c.od[44 + q] = have_prior ? sh[SH_JP + (q - 900)] : 0.0;
        }
        if (lane != 0) return;
        for (int k = 0; k < 22; ++k) { c.od[k] = si[k]; c.od[22 + k] = si[SREC + k]; }
        c.od[1169] = chi_initial; c.od[1170] = chi_final; c.od[1171] = lambda;
        c.oi[16] = trials; c.oi[17] = failures; c.oi[18] = n_pt; c.oi[19] = n_ln; c.oi[20] = status; c.oi[21] = 0;
    });
}

// the lanes of the host: nl emulated lanes, one after the other (nl = 1: a plain serial loop)
struct HostWave {
    int nl;
    Acc* lanes;      // nl of them
    double* shm;     // SH_TOTAL doubles
    bool leader() const { return true; }
    double* sh() const { return shm; }
    template <class F> void par(F f) { for (int l = 0; l < nl; ++l) f(l, nl); }
    template <class F> void sum(F f, Acc& a, int) {
        for (int l = 0; l < nl; ++l) { rp::acc_zero(lanes[l]); f(l, nl, lanes[l]); }
        rp::tree_sum(lanes, nl);
        a = lanes[0];
    }
    template <class F> int sum_i(F f) { int n = 0; for (int l = 0; l < nl; ++l) n += f(l, nl); return n; }
};

}  // namespace vitrack
}  // namespace plba
