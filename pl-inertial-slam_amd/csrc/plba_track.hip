// plba_track.hip — frame-to-frame pose tracking (plba_track_pose, include/plba.h): StereoFrameHandler::optimizePose
// (stvo-pl/src/stereoFrameHandler.cpp:334-419) for B problems in ONE launch, the whole protocol of a problem inside it.
//
// Mapping: one wave (a 64-thread workgroup) per problem, as plba_relpose.hip.  A lane adds its own features (lane, lane + 64, ...; points,
// then lines) into 21 + 6 + 1 fp64 accumulators; the partial sums are added by the fixed butterfly of plba_relpose.hip (quad_perm,
// row_half_mirror, row_mirror inside a DPP row, then lanes ^ 16 and ^ 32), which leaves the same bits in every lane.  Lane 0 runs the
// serial part (exit tests, the pivoted QR, expmap, isGoodSolution's eigenvalues) and its verdict and pose reach the others by lane reads;
// the branch between the refinement and the robust fallback is therefore uniform over the wave.  The order statistics of the cut and of
// the fallback's Cauchy scale are a bitwise radix select (track::select): a lane keeps its residuals in a per-problem slice of the
// call's device block, written and read back by that lane alone with ordinary stores, counts in 63 rounds how many of them fall below
// the bit under test, and the counts are added by the integer butterfly; no LDS, no atomics, no limit on the feature count.
#include <vector>

#include "plba_problem.h"
#include "plba_track_dev.h"

namespace plba {
namespace {

namespace tk = track;
namespace rp = relpose;
constexpr int TK_OUT_D = 12 + 21 + 1 + 6 + 4 + 12;      // per problem: T (R, t), H (upper), err, cov_eig, the cut's statistics, DT (R, t)
constexpr int TK_OUT_I = 10;                            // n_pt, n_ln, iters[3], path, status, good, negdet, -

struct TrackDev {
    tk::Opt o;
    const int32_t *pt_start, *ln_start;
    const double *P3, *uv2, *pt_s2, *pq6, *l3, *se4, *ln_s2, *T0;      // T0: B x 12 or null
    uint8_t *pt_in, *ln_in;
    double *ws_p, *ws_l;      // 2 doubles per point, 2 per line
    double* out_d;
    int32_t* out_i;
};

template <int CTRL>
__device__ __forceinline__ double tk_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, the same bits in all of them: every step adds the two operands of a pair in both of its lanes
__device__ __forceinline__ double tk_sum64(double v) {
    v += tk_dpp<0xB1>(v);
    v += tk_dpp<0x4E>(v);
    v += tk_dpp<0x141>(v);
    v += tk_dpp<0x140>(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int tk_sum64_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

struct DevWave {
    int lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ void share(int& go, rp::Pose& T) const {
#pragma unroll
        for (int i = 0; i < 9; ++i) T.R[i] = __shfl(T.R[i], 0);
#pragma unroll
        for (int i = 0; i < 3; ++i) T.t[i] = __shfl(T.t[i], 0);
        go = __shfl(go, 0);
    }
    template <class F>
    __device__ void sum(F f, rp::Acc& a, int nq) const {      // nq: the entries of a.v in use
        rp::acc_zero(a);
        f(lane, 64, a);
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q)
            if (q < nq) a.v[q] = tk_sum64(a.v[q]);
        a.n = tk_sum64_i(a.n);
    }
    template <class F>
    __device__ int sum_i(F f) const { return tk_sum64_i(f(lane, 64)); }
};

__global__ __launch_bounds__(64) void k_track(TrackDev d) {
    const int b = blockIdx.x;
    const int p0 = d.pt_start[b], l0 = d.ln_start[b];
    tk::Prob c;
    c.rc.np = d.pt_start[b + 1] - p0; c.rc.nl = d.ln_start[b + 1] - l0;
    c.rc.P3 = d.P3 + 3 * (size_t)p0; c.rc.uv2 = d.uv2 + 2 * (size_t)p0; c.rc.pq6 = d.pq6 + 6 * (size_t)l0; c.rc.l3 = d.l3 + 3 * (size_t)l0;
    c.rc.pt_in = d.pt_in + p0; c.rc.ln_in = d.ln_in + l0;
    c.pt_s2 = d.pt_s2 + p0; c.se4 = d.se4 + 4 * (size_t)l0; c.ln_s2 = d.ln_s2 + l0;
    c.res_p = d.ws_p + 2 * (size_t)p0; c.dev_p = c.res_p + c.rc.np;
    c.res_l = d.ws_l + 2 * (size_t)l0; c.dev_l = c.res_l + c.rc.nl;
    DevWave w{(int)threadIdx.x};
    tk::State s;
    tk::run(w, c, d.o, d.T0 ? d.T0 + 12 * (size_t)b : nullptr, s);
    if (threadIdx.x == 0) {
        double* od = d.out_d + (size_t)TK_OUT_D * b;
        for (int i = 0; i < 9; ++i) od[i] = s.T.R[i];
        for (int i = 0; i < 3; ++i) od[9 + i] = s.T.t[i];
        for (int i = 0; i < 21; ++i) od[12 + i] = s.H[i];
        od[33] = s.err;
        for (int i = 0; i < 6; ++i) od[34 + i] = s.cov_eig[i];
        for (int i = 0; i < 4; ++i) od[40 + i] = s.stat[i];
        rp::Pose DT;
        tk::frame_dt(s, DT);
        for (int i = 0; i < 9; ++i) od[44 + i] = DT.R[i];
        for (int i = 0; i < 3; ++i) od[53 + i] = DT.t[i];
        int32_t* oi = d.out_i + (size_t)TK_OUT_I * b;
        oi[0] = s.n_pt; oi[1] = s.n_ln; oi[2] = s.iters[0]; oi[3] = s.iters[1]; oi[4] = s.iters[2];
        oi[5] = s.path; oi[6] = s.status; oi[7] = s.good; oi[8] = s.negdet; oi[9] = 0;
    }
}

size_t al8(size_t b) { return (b + 7) & ~(size_t)7; }
void put16(double* m, const double* R, const double* t) {
    for (int i = 0; i < 3; ++i) { m[i * 4] = R[i * 3]; m[i * 4 + 1] = R[i * 3 + 1]; m[i * 4 + 2] = R[i * 3 + 2]; m[i * 4 + 3] = t[i]; }
    m[12] = m[13] = m[14] = 0.0; m[15] = 1.0;
}

}  // namespace
}  // namespace plba

using namespace plba;

extern "C" {

void plba_track_default_options(plba_track_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_iters = 5; o->max_iters_ref = 10; o->min_features = 10;      // Config::maxIters / maxItersRef / minFeatures, stvo-pl/src/config.cpp:80-86
    o->homog_th = 1e-7; o->min_error = 1e-7; o->min_error_change = 1e-7; o->inlier_k = 4.0;
}

int plba_track_pose(plba_problem* p, const plba_track_options* opt, int B, const int32_t* pt_start, const double* P3, const double* uv2,
                    const double* pt_sigma2, const int32_t* ln_start, const double* sPeP6, const double* l3, const double* spl_epl4,
                    const double* ln_sigma2, double fx, double fy, double cx, double cy, const double* T0_16, uint8_t* pt_inlier,
                    uint8_t* ln_inlier, plba_track_result* out) {
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !out) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: no options or no output");
    if (B < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: B = %d", B);
    if (!pt_start || !ln_start) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: missing start array");
    if (opt->max_iters < 0 || opt->max_iters_ref < 0 || opt->min_features < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: negative iteration or feature count");
    for (const double v : {opt->homog_th, opt->min_error, opt->min_error_change, opt->inlier_k, fx, fy, cx, cy})
        if (!std::isfinite(v)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: an option or an intrinsic is not finite");
    for (const int32_t* st : {pt_start, ln_start}) {
        if (st[0] != 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: a start array does not begin at 0");
        for (int b = 0; b < B; ++b) if (st[b + 1] < st[b]) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: the starts of problem %d descend", b);
    }
    const size_t Np = (size_t)pt_start[B], Nl = (size_t)ln_start[B];
    if ((Np && (!P3 || !uv2 || !pt_sigma2)) || (Nl && (!sPeP6 || !l3 || !spl_epl4 || !ln_sigma2))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: missing feature array");
    auto finite = [](const double* a, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; };
    if (!finite(P3, 3 * Np) || !finite(uv2, 2 * Np) || !finite(pt_sigma2, Np) || !finite(sPeP6, 6 * Nl) || !finite(l3, 3 * Nl) || !finite(spl_epl4, 4 * Nl) ||
        !finite(ln_sigma2, Nl) || (T0_16 && !finite(T0_16, 16 * (size_t)B)))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: non-finite input");
    for (size_t i = 0; i < Np; ++i) if (pt_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: a negative sigma2");
    for (size_t i = 0; i < Nl; ++i) if (ln_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: a negative sigma2");

    // one device block: [starts | features | T0 || masks || results | workspace]; the copy up takes everything before the second bar, the
    // copy down the masks and the results
    const size_t o_ps = 0, o_ls = o_ps + al8(4 * (size_t)(B + 1)), o_P = o_ls + al8(4 * (size_t)(B + 1)), o_uv = o_P + 24 * Np, o_s2p = o_uv + 16 * Np,
                 o_pq = o_s2p + 8 * Np, o_l3 = o_pq + 48 * Nl, o_se = o_l3 + 24 * Nl, o_s2l = o_se + 32 * Nl, o_T0 = o_s2l + 8 * Nl,
                 o_pm = o_T0 + (T0_16 ? 96 * (size_t)B : 0), o_lm = o_pm + al8(Np), o_od = o_lm + al8(Nl), o_oi = o_od + 8 * (size_t)TK_OUT_D * B,
                 o_wp = o_oi + al8(4 * (size_t)TK_OUT_I * B), o_wl = o_wp + 16 * Np, total = o_wl + 16 * Nl;
    const size_t up = o_od, down = o_wp - o_pm;
    PLBA_HIPCK(p, hipSetDevice(p->device));
    hipStream_t s = p->stream;
    DArrStreamScope staged(s, p->have_ctx ? p->ctx.stage : nullptr);
    std::vector<char> h_up, h_down;      // pageable stand-ins when the pinned staging area is missing or too small
    char* hu = (char*)stage_take(up);
    char* hd = (char*)stage_take(down);
    if (!hu) { h_up.resize(up); hu = h_up.data(); }
    if (!hd) { h_down.resize(down); hd = h_down.data(); }
    memset(hu, 0, o_P);
    memcpy(hu + o_ps, pt_start, 4 * (size_t)(B + 1)); memcpy(hu + o_ls, ln_start, 4 * (size_t)(B + 1));
    if (Np) { memcpy(hu + o_P, P3, 24 * Np); memcpy(hu + o_uv, uv2, 16 * Np); memcpy(hu + o_s2p, pt_sigma2, 8 * Np); }
    if (Nl) { memcpy(hu + o_pq, sPeP6, 48 * Nl); memcpy(hu + o_l3, l3, 24 * Nl); memcpy(hu + o_se, spl_epl4, 32 * Nl); memcpy(hu + o_s2l, ln_sigma2, 8 * Nl); }
    if (T0_16)
        for (int b = 0; b < B; ++b) {
            double* t = reinterpret_cast<double*>(hu + o_T0) + 12 * (size_t)b;
            const double* m = T0_16 + 16 * (size_t)b;
            for (int i = 0; i < 3; ++i) { t[i * 3] = m[i * 4]; t[i * 3 + 1] = m[i * 4 + 1]; t[i * 3 + 2] = m[i * 4 + 2]; t[9 + i] = m[i * 4 + 3]; }
        }
    if (pt_inlier) for (size_t i = 0; i < Np; ++i) hu[o_pm + i] = pt_inlier[i] ? 1 : 0; else memset(hu + o_pm, 1, Np);
    if (ln_inlier) for (size_t i = 0; i < Nl; ++i) hu[o_lm + i] = ln_inlier[i] ? 1 : 0; else memset(hu + o_lm, 1, Nl);
    DArr<char> blk;
    PLBA_HIPCK(p, blk.alloc(total, false));
    PLBA_HIPCK(p, hipMemcpyAsync(blk.p, hu, up, hipMemcpyHostToDevice, s));
    TrackDev d;
    d.o.max_iters = opt->max_iters; d.o.max_iters_ref = opt->max_iters_ref; d.o.min_features = opt->min_features;
    d.o.min_error = opt->min_error; d.o.min_error_change = opt->min_error_change; d.o.inlier_k = opt->inlier_k;
    d.o.ro.max_iters = d.o.ro.max_iters_ref = d.o.ro.protocol = 0; d.o.ro.cut = 0.0;
    d.o.ro.homog_th = opt->homog_th; d.o.ro.fx = fx; d.o.ro.fy = fy; d.o.ro.cx = cx; d.o.ro.cy = cy;
    auto dbl = [&](size_t off) { return reinterpret_cast<double*>(blk.p + off); };
    d.pt_start = reinterpret_cast<const int32_t*>(blk.p + o_ps); d.ln_start = reinterpret_cast<const int32_t*>(blk.p + o_ls);
    d.P3 = dbl(o_P); d.uv2 = dbl(o_uv); d.pt_s2 = dbl(o_s2p); d.pq6 = dbl(o_pq); d.l3 = dbl(o_l3); d.se4 = dbl(o_se); d.ln_s2 = dbl(o_s2l);
    d.T0 = T0_16 ? dbl(o_T0) : nullptr;
    d.pt_in = reinterpret_cast<uint8_t*>(blk.p + o_pm); d.ln_in = reinterpret_cast<uint8_t*>(blk.p + o_lm);
    d.out_d = dbl(o_od); d.out_i = reinterpret_cast<int32_t*>(blk.p + o_oi);
    d.ws_p = dbl(o_wp); d.ws_l = dbl(o_wl);
    hipLaunchKernelGGL(k_track, dim3((unsigned)B), dim3(64), 0, s, d);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_HIPCK(p, hipMemcpyAsync(hd, blk.p + o_pm, down, hipMemcpyDeviceToHost, s));
    PLBA_HIPCK(p, plba_stream_wait(p, s));      // the call's one blocking wait

    const double* od = reinterpret_cast<const double*>(hd + (o_od - o_pm));
    const int32_t* oi = reinterpret_cast<const int32_t*>(hd + (o_oi - o_pm));
    for (int b = 0; b < B; ++b) {
        const double* q = od + (size_t)TK_OUT_D * b;
        const int32_t* k = oi + (size_t)TK_OUT_I * b;
        plba_track_result& r = out[b];
        put16(r.T_opt16, q, q + 9);
        put16(r.DT16, q + 44, q + 53);
        tk::State st;
        int n = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) { r.H36[i * 6 + j] = q[12 + n]; r.H36[j * 6 + i] = q[12 + n]; st.H[n] = q[12 + n]; ++n; }
        st.path = k[5]; st.status = k[6]; st.negdet = k[8];
        tk::covariance36(st, r.cov36);      // DT_cov on the host from what came back
        r.err = q[33];
        for (int i = 0; i < 6; ++i) r.cov_eig6[i] = q[34 + i];
        r.pt_mean = q[40]; r.pt_stdv = q[41]; r.ln_mean = q[42]; r.ln_stdv = q[43];
        r.n_inliers_pt = k[0]; r.n_inliers_ln = k[1]; r.iters[0] = k[2]; r.iters[1] = k[3]; r.iters[2] = k[4];
        r.path = k[5]; r.status = k[6]; r.good = k[7];
    }
    if (pt_inlier) memcpy(pt_inlier, hd, Np);
    if (ln_inlier) memcpy(ln_inlier, hd + (o_lm - o_pm), Nl);
    return PLBA_OK;
}

}  // extern "C"
