// plba_refine.hip — structure-only landmark refinement (plba_refine_landmarks, include/plba.h): every landmark's own Levenberg-
// Marquardt against FIXED keyframes, all of them in one launch.
//
// Semantics (g2o's StructureOnlySolver::calc is the model; DESIGN.md 9b is the specification): per landmark, over its level-0
// observations, chi2 = sum rho(inv_sigma2 e^T e), H = sum w Jl^T Jl, b = -sum w Jl^T e with w = rho' inv_sigma2 (the first-order
// robustification of k_linearize), damped trials (H + mu I) delta = b, gain ratio rho = (chi2 - chi2') / (delta^T (mu delta + b)),
// accepted iff rho > 0 with rho and chi2' finite: mu *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; else mu *= nu, nu *= 2.  No
// convergence thresholds.  A point is one 3 x 3 system, a line two (one per end point: row 0 depends on sP only, row 1 on eP only)
// under ONE mu, chi2 and decision.
//
// Mapping: RF_G = 8 lanes per landmark, its observations dealt round-robin over the lanes (lane j: j, j + 8, ...; tracks of 2 .. 8 take
// one round), 32 landmarks per 256-thread workgroup.  configs[2]: 24 k landmarks = 3 k waves on 1024 SIMDs, and lanes of one landmark
// never diverge on the track length.  Each lane adds its own observations in ascending order; the eight partial sums of chi2, H and b
// are then added by three DPP steps (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror — the 8-lane units of plba_lm_dev.h), which leave
// the same bits in all eight lanes: the 3 x 3 solves and every decision are computed redundantly and uniformly, with no LDS traffic and
// no barrier inside the loop.  The order of every sum is a function of the window alone.  A trial evaluates the residuals AND the
// Jacobians of the trial state, so an accepted step needs no second pass (one evaluation per trial, not two).
// Camera blocks (kfcam_make, 12 doubles per keyframe) are staged in LDS up to REFINE_KC_LDS_MAX keyframes; beyond, each lane forms its
// observation's block from the keyframe record (24 doubles through L2) with the same function.
#include "plba_internal.h"

namespace plba {
#define DEV __device__ __forceinline__

constexpr int RF_G = 8;                 // lanes per landmark
constexpr int RF_BLOCK = 256;
constexpr int RF_LM = RF_BLOCK / RF_G;  // landmarks per workgroup

template <int CTRL>
DEV double rf_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the 8 lanes of a landmark, the same bits in all of them (every step adds the two operands of a pair in both lanes)
DEV double rf_sum8(double v) {
    v += rf_dpp<0xB1>(v);
    v += rf_dpp<0x4E>(v);
    v += rf_dpp<0x141>(v);
    return v;
}
DEV int rf_sum8_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    return v;
}

// the pivots of sym3_inv's LDL^T of (H + mu I), by its expressions: all positive?  (sym3_inv itself only refuses a zero pivot)
DEV bool rf_pivots_positive(const double* h, double mu) {
    const double a = h[0] + mu, b = h[1], c = h[2], e = h[3] + mu, f = h[4], g = h[5] + mu;
    const double i0 = 1.0 / a;
    const double l10 = b * i0, l20 = c * i0;
    const double d1 = e - l10 * b;
    const double l21 = (f - l20 * b) * (1.0 / d1);
    const double d2 = g - l20 * c - l21 * l21 * d1;
    return a > 0.0 && d1 > 0.0 && d2 > 0.0;
}

struct RfLin { double chi, H[12], b[6]; };      // H: upper triangles [00 01 02 11 12 22] of the point / sP block, then of the eP block

// chi2, H and b of one landmark at x, from this lane's observations and then over the 8 lanes
template <bool KC_LDS>
DEV void rf_linearize(const DevBuf& d, const Robust& rb, const double* s_kc, const double* kf, bool is_pt, int e0, int n, int sub, const double* x, RfLin& o) {
    o.chi = 0.0;
#pragma unroll
    for (int t = 0; t < 12; ++t) o.H[t] = 0.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) o.b[t] = 0.0;
    const int kind = is_pt ? PLBA_EDGE_POINT : PLBA_EDGE_LINE;
    for (int c = sub; c < n; c += RF_G) {
        const int e = e0 + c;
        if (d.ob_level[e] != 0) continue;
        const int k = d.ob_kf[e];
        const double w0 = d.ob_w[e];
        double kcb[KFCAM_STRIDE];
        const double* kc;
        if (KC_LDS) kc = s_kc + k * KFCAM_STRIDE;
        else { kfcam_make(d.cam, kf + (size_t)k * KF_STRIDE, kcb); kc = kcb; }
        double e2[2], Jp[12], Jl[6];
        bool dpos;
        if (is_pt) {
            const double2 uv = reinterpret_cast<const double2*>(d.po_uv)[e];
            point_edge(d.cam, kc, v3(x[0], x[1], x[2]), uv.x, uv.y, e2, Jp, Jl, dpos, true);
        } else {
            const double* l = d.lo_l + (size_t)(e - d.Ep) * 3;
            line_edge(d.cam, kc, v3(x[0], x[1], x[2]), v3(x[3], x[4], x[5]), l[0], l[1], l[2], d.fix_q1 != 0, e2, Jp, Jl, dpos, true);
        }
        const double s = w0 * (e2[0] * e2[0] + e2[1] * e2[1]);
        double r0 = s, r1 = 1.0;
        if (rb.on[kind]) huber(s, rb.delta[kind], r0, r1);
        const double w = w0 * r1;
        o.chi += r0;
        // row 0 (Jl[0..2], e2[0]) and row 1 (Jl[3..5], e2[1]): both into the one block of a point, one each into a line's two blocks
        const double wa0 = w * Jl[0], wa1 = w * Jl[1], wa2 = w * Jl[2], wb0 = w * Jl[3], wb1 = w * Jl[4], wb2 = w * Jl[5];
        o.H[0] += wa0 * Jl[0]; o.H[1] += wa0 * Jl[1]; o.H[2] += wa0 * Jl[2]; o.H[3] += wa1 * Jl[1]; o.H[4] += wa1 * Jl[2]; o.H[5] += wa2 * Jl[2];
        o.b[0] -= wa0 * e2[0]; o.b[1] -= wa1 * e2[0]; o.b[2] -= wa2 * e2[0];
        if (is_pt) {
            o.H[0] += wb0 * Jl[3]; o.H[1] += wb0 * Jl[4]; o.H[2] += wb0 * Jl[5]; o.H[3] += wb1 * Jl[4]; o.H[4] += wb1 * Jl[5]; o.H[5] += wb2 * Jl[5];
            o.b[0] -= wb0 * e2[1]; o.b[1] -= wb1 * e2[1]; o.b[2] -= wb2 * e2[1];
        } else {
            o.H[6] += wb0 * Jl[3]; o.H[7] += wb0 * Jl[4]; o.H[8] += wb0 * Jl[5]; o.H[9] += wb1 * Jl[4]; o.H[10] += wb1 * Jl[5]; o.H[11] += wb2 * Jl[5];
            o.b[3] -= wb0 * e2[1]; o.b[4] -= wb1 * e2[1]; o.b[5] -= wb2 * e2[1];
        }
    }
    o.chi = rf_sum8(o.chi);
#pragma unroll
    for (int t = 0; t < 6; ++t) o.H[t] = rf_sum8(o.H[t]);
#pragma unroll
    for (int t = 0; t < 3; ++t) o.b[t] = rf_sum8(o.b[t]);
    if (!is_pt) {
#pragma unroll
        for (int t = 6; t < 12; ++t) o.H[t] = rf_sum8(o.H[t]);
#pragma unroll
        for (int t = 3; t < 6; ++t) o.b[t] = rf_sum8(o.b[t]);
    }
}

template <bool KC_LDS>
__global__ __launch_bounds__(RF_BLOCK) void k_refine(DevBuf d, Robust rb, RefineArgs a) {
    extern __shared__ double s_kc[];      // K x 12 staged camera blocks (KC_LDS)
    const double* kf = d.kf[a.cur];
    if (KC_LDS) {
        for (int k = threadIdx.x; k < d.K; k += RF_BLOCK) kfcam_make(d.cam, kf + (size_t)k * KF_STRIDE, s_kc + k * KFCAM_STRIDE);
        __syncthreads();
    }
    const int slot = blockIdx.x * RF_LM + (threadIdx.x / RF_G), sub = threadIdx.x % RF_G;
    if (slot >= d.L) return;      // (whole 8-lane units leave together: every DPP step below runs with its unit's lanes all active)
    const bool is_pt = slot < d.Np;
    const int e0 = d.lm_start[slot], n = d.lm_start[slot + 1] - e0;
    int status = PLBA_REFINE_DONE, iters = 0, trials = 0;
    double chi_before = 0.0, chi_after = 0.0;
    if (d.lm_fixed[slot]) status = PLBA_REFINE_FIXED;
    else if (a.select && !a.select[slot]) status = PLBA_REFINE_UNSELECTED;
    else {
        int nact = 0;
        for (int c = sub; c < n; c += RF_G) nact += d.ob_level[e0 + c] == 0 ? 1 : 0;
        if (rf_sum8_i(nact) == 0) status = PLBA_REFINE_NO_OBS;
    }
    if (status == PLBA_REFINE_DONE) {
        const size_t pos = (size_t)(a.lm_pos ? a.lm_pos[slot] : slot) * 6;
        double x[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) x[t] = d.lm[a.cur][pos + t];
        RfLin cur;
        rf_linearize<KC_LDS>(d, rb, s_kc, kf, is_pt, e0, n, sub, x, cur);
        chi_before = chi_after = cur.chi;
        if (!isfinite(cur.chi)) status = PLBA_REFINE_NONFINITE;
        double mu = a.lambda_init, nu = 2.0;
        for (int it = 0; it < a.max_iters && status == PLBA_REFINE_DONE; ++it) {
            bool accepted = false;
            for (int q = 0; q < a.max_trials && !accepted; ++q) {
                ++trials;
                if (rf_pivots_positive(cur.H, mu) && (is_pt || rf_pivots_positive(cur.H + 6, mu))) {
                    double D[6], dx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    sym3_inv(cur.H, mu, D);
                    const V3 d0 = sym3_mul(D, v3(cur.b[0], cur.b[1], cur.b[2]));
                    dx[0] = d0.x; dx[1] = d0.y; dx[2] = d0.z;
                    if (!is_pt) {
                        sym3_inv(cur.H + 6, mu, D);
                        const V3 d1 = sym3_mul(D, v3(cur.b[3], cur.b[4], cur.b[5]));
                        dx[3] = d1.x; dx[4] = d1.y; dx[5] = d1.z;
                    }
                    double xt[6], den = 0.0;
#pragma unroll
                    for (int t = 0; t < 6; ++t) { xt[t] = x[t] + dx[t]; den += dx[t] * (mu * dx[t] + cur.b[t]); }
                    RfLin tr;
                    rf_linearize<KC_LDS>(d, rb, s_kc, kf, is_pt, e0, n, sub, xt, tr);
                    const double rho = (cur.chi - tr.chi) / den;
                    if (isfinite(rho) && rho > 0.0 && isfinite(tr.chi)) {
                        accepted = true;
#pragma unroll
                        for (int t = 0; t < 6; ++t) x[t] = xt[t];
                        cur = tr;
                        const double g = 2.0 * rho - 1.0;
                        mu *= fmax(1.0 / 3.0, 1.0 - g * g * g);
                        nu = 2.0;
                    }
                }
                if (!accepted) { mu *= nu; nu *= 2.0; }
            }
            if (accepted) ++iters;
            else status = PLBA_REFINE_EXHAUSTED;
        }
        chi_after = cur.chi;
        if (sub == 0 && iters > 0) {      // both state images: the trial passes of the next plba_optimize write the other one from this one
            const int nx = is_pt ? 3 : 6;
            for (int t = 0; t < nx; ++t) { d.lm[0][pos + t] = x[t]; d.lm[1][pos + t] = x[t]; }
        }
    }
    if (sub == 0) {
        a.chi[2 * (size_t)slot] = chi_before; a.chi[2 * (size_t)slot + 1] = chi_after;
        a.cnt[3 * (size_t)slot] = status; a.cnt[3 * (size_t)slot + 1] = iters; a.cnt[3 * (size_t)slot + 2] = trials;
    }
}

hipError_t launch_refine(const DevBuf& d, const Robust& rb, const RefineArgs& a, hipStream_t s) {
    if (d.L <= 0) return hipSuccess;
    const dim3 grid((unsigned)((d.L + RF_LM - 1) / RF_LM)), block(RF_BLOCK);
    if (d.K <= REFINE_KC_LDS_MAX) hipLaunchKernelGGL(k_refine<true>, grid, block, (size_t)d.K * KFCAM_STRIDE * sizeof(double), s, d, rb, a);
    else hipLaunchKernelGGL(k_refine<false>, grid, block, 0, s, d, rb, a);
    return hipGetLastError();
}

}  // namespace plba
