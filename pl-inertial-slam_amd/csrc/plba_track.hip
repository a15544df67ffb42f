// plba_track.hip — frame-to-frame pose tracking (plba_track_pose, include/plba.h): StereoFrameHandler::optimizePose
// (stvo-pl/src/stereoFrameHandler.cpp:334-419) for B problems in ONE launch, the whole protocol of a problem inside it.
//
// Mapping: one wave (a 64-thread workgroup) per problem, as plba_relpose.hip.  A lane adds its own features (lane, lane + 64, ...; points,
// then lines) into 21 + 6 + 1 fp64 accumulators; the partial sums are added by the fixed butterfly of plba_wave_dev.h (quad_perm,
// row_half_mirror, row_mirror inside a DPP row, then lanes ^ 16 and ^ 32), which leaves the same bits in every lane.  Lane 0 runs the
// serial part (exit tests, the pivoted QR, expmap, isGoodSolution's eigenvalues) and its verdict and pose reach the others by lane reads;
// the branch between the refinement and the robust fallback is therefore uniform over the wave.  The order statistics of the cut and of
// the fallback's Cauchy scale are a bitwise radix select (track::select): a lane keeps its residuals in a per-problem slice of the
// call's device block, written and read back by that lane alone with ordinary stores, counts in 63 rounds how many of them fall below
// the bit under test, and the counts are added by the integer butterfly; no LDS, no atomics, no limit on the feature count.
// The host side of the call (one block, one copy up, one down, one wait) is plba_batch_call.h's.
#include "plba_batch_call.h"
#include "plba_track_dev.h"
#include "plba_wave_dev.h"

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

struct DevWave {
    int lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ void share(int& go, rp::Pose& T) const { go = wave_lead(go, T.R, T.t); }
    template <class F>
    __device__ void sum(F f, rp::Acc& a, int nq) const {      // nq: the entries of a.v in use
        rp::acc_zero(a);
        f(lane, 64, a);
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q)
            if (q < nq) a.v[q] = wave_sum64(a.v[q]);
        a.n = wave_sum64_i(a.n);
    }
    template <class F>
    __device__ int sum_i(F f) const { return wave_sum64_i(f(lane, 64)); }
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
    for (const int32_t* st : {pt_start, ln_start})
        if (const char* why = check_starts(B, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: %s", why);
    const size_t Np = (size_t)pt_start[B], Nl = (size_t)ln_start[B];
    if ((Np && (!P3 || !uv2 || !pt_sigma2)) || (Nl && (!sPeP6 || !l3 || !spl_epl4 || !ln_sigma2))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: missing feature array");
    if (!all_finite(P3, 3 * Np) || !all_finite(uv2, 2 * Np) || !all_finite(pt_sigma2, Np) || !all_finite(sPeP6, 6 * Nl) || !all_finite(l3, 3 * Nl) ||
        !all_finite(spl_epl4, 4 * Nl) || !all_finite(ln_sigma2, Nl) || (T0_16 && !all_finite(T0_16, 16 * (size_t)B)))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: non-finite input");
    for (size_t i = 0; i < Np; ++i) if (pt_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: a negative sigma2");
    for (size_t i = 0; i < Nl; ++i) if (ln_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_track_pose: a negative sigma2");

    // one device block: [starts | features | T0 | masks || results || workspace]; the copy up takes what is before the first bar, the copy
    // down the masks and the results (the masks are in both); the workspace stays on the device
    Layout L;
    const size_t n_st = 4 * ((size_t)B + 1);
    const size_t o_ps = L.take(n_st), o_ls = L.take(n_st), o_P = L.take(24 * Np), o_uv = L.take(16 * Np), o_s2p = L.take(8 * Np), o_pq = L.take(48 * Nl),
                 o_l3 = L.take(24 * Nl), o_se = L.take(32 * Nl), o_s2l = L.take(8 * Nl), o_T0 = L.take(T0_16 ? 96 * (size_t)B : 0), o_pm = L.take(Np),
                 o_lm = L.take(Nl), up_end = L.off, o_od = L.take(8 * (size_t)TK_OUT_D * B), o_oi = L.take(4 * (size_t)TK_OUT_I * B), down_end = L.off,
                 o_wp = L.take(16 * Np), o_wl = L.take(16 * Nl);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_pm, down_end));
    call.put(o_ps, pt_start, n_st); call.put(o_ls, ln_start, n_st);
    call.put(o_P, P3, 24 * Np); call.put(o_uv, uv2, 16 * Np); call.put(o_s2p, pt_sigma2, 8 * Np);
    call.put(o_pq, sPeP6, 48 * Nl); call.put(o_l3, l3, 24 * Nl); call.put(o_se, spl_epl4, 32 * Nl); call.put(o_s2l, ln_sigma2, 8 * Nl);
    if (T0_16)
        for (int b = 0; b < B; ++b) pose_pack12(T0_16 + 16 * (size_t)b, call.up<double>(o_T0) + 12 * (size_t)b);
    mask_normalise(pt_inlier, Np, call.up<uint8_t>(o_pm)); mask_normalise(ln_inlier, Nl, call.up<uint8_t>(o_lm));
    PLBA_TRY(call.upload());
    TrackDev d;
    d.o.max_iters = opt->max_iters; d.o.max_iters_ref = opt->max_iters_ref; d.o.min_features = opt->min_features;
    d.o.min_error = opt->min_error; d.o.min_error_change = opt->min_error_change; d.o.inlier_k = opt->inlier_k;
    d.o.ro.max_iters = d.o.ro.max_iters_ref = d.o.ro.protocol = 0; d.o.ro.cut = 0.0;
    d.o.ro.homog_th = opt->homog_th; d.o.ro.fx = fx; d.o.ro.fy = fy; d.o.ro.cx = cx; d.o.ro.cy = cy;
    d.pt_start = call.dev<int32_t>(o_ps); d.ln_start = call.dev<int32_t>(o_ls);
    d.P3 = call.dev<double>(o_P); d.uv2 = call.dev<double>(o_uv); d.pt_s2 = call.dev<double>(o_s2p);
    d.pq6 = call.dev<double>(o_pq); d.l3 = call.dev<double>(o_l3); d.se4 = call.dev<double>(o_se); d.ln_s2 = call.dev<double>(o_s2l);
    d.T0 = T0_16 ? call.dev<double>(o_T0) : nullptr;
    d.pt_in = call.dev<uint8_t>(o_pm); d.ln_in = call.dev<uint8_t>(o_lm);
    d.out_d = call.dev<double>(o_od); d.out_i = call.dev<int32_t>(o_oi);
    d.ws_p = call.dev<double>(o_wp); d.ws_l = call.dev<double>(o_wl);
    hipLaunchKernelGGL(k_track, dim3((unsigned)B), dim3(64), 0, call.s, d);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());

    const double* od = call.down<double>(o_od);
    const int32_t* oi = call.down<int32_t>(o_oi);
    for (int b = 0; b < B; ++b) {
        const double* q = od + (size_t)TK_OUT_D * b;
        const int32_t* k = oi + (size_t)TK_OUT_I * b;
        plba_track_result& r = out[b];
        pose_unpack16(q, r.T_opt16);
        pose_unpack16(q + 44, r.DT16);
        sym6_expand(q + 12, r.H36);
        tk::State st;
        for (int n = 0; n < 21; ++n) st.H[n] = q[12 + n];
        st.path = k[5]; st.status = k[6]; st.negdet = k[8];
        tk::covariance36(st, r.cov36);      // DT_cov on the host from what came back
        r.err = q[33];
        for (int i = 0; i < 6; ++i) r.cov_eig6[i] = q[34 + i];
        r.pt_mean = q[40]; r.pt_stdv = q[41]; r.ln_mean = q[42]; r.ln_stdv = q[43];
        r.n_inliers_pt = k[0]; r.n_inliers_ln = k[1]; r.iters[0] = k[2]; r.iters[1] = k[3]; r.iters[2] = k[4];
        r.path = k[5]; r.status = k[6]; r.good = k[7];
    }
    if (pt_inlier) memcpy(pt_inlier, call.down<uint8_t>(o_pm), Np);
    if (ln_inlier) memcpy(ln_inlier, call.down<uint8_t>(o_lm), Nl);
    return PLBA_OK;
}

}  // extern "C"
