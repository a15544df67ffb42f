// plba_vitrack.hip — batched visual-inertial tracking (plba_track_inertial, include/plba.h): the motion-only optimisation of two
// consecutive VertexNavState (IMU/g2otypes.h:411-695) for B problems in ONE launch, the whole protocol of a problem inside it.
//
// Mapping: one wave (a 64-thread workgroup) per problem, as plba_track.hip.  A lane adds its own visual edges (lane, lane + 64, ...;
// points, then lines) into 21 + 6 + 1 fp64 accumulators; the partial sums are added by the fixed butterfly of plba_wave_dev.h, which
// leaves the same bits in every lane.  The 30 x 30 system, its factor, the 15 x 30 Jacobian of the IMU edge, the prior's 15 x 15 and both
// copies of the two states live in LDS (27 KB of a workgroup); lane 0 writes the serial pieces (errors, Jacobians, the oplus) there, the
// products Omega J, J^T Omega J, the LL^T columns and the two triangular solves are spread over the lanes in a fixed operation order, a
// barrier between two phases.  What decides a branch (chi2, rho, a pivot's sign) is read from LDS by every lane after the barrier, so
// every branch is uniform over the wave.  No atomics, nothing between workgroups, no spin; every loop is bounded by rounds x iters x
// max_trials and the feature counts.  The host side of the call (one block, one copy up, one down, one wait) is plba_batch_call.h's.
#include "plba_batch_call.h"
#include "plba_vitrack_dev.h"
#include "plba_wave_dev.h"

namespace plba {
namespace {

namespace vt = vitrack;
namespace rp = relpose;

struct VitrackDev {
    vt::Opt o;
    const int32_t *pt_start, *ln_start;
    const double *Pw3, *uv2, *pt_w, *pq6, *l3, *ln_w;
    const double *si, *sj, *pre, *ipvr, *ibias, *pst, *pinfo;      // pst, pinfo: null when no anchor is free
    const uint8_t* anchor_free;
    uint8_t *pt_in, *ln_in;
    char* out;      // B x sizeof(plba_vitrack_result)
};

struct DevWave {
    int lane;
    double* shm;
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ double* sh() const { return shm; }
    template <class F>
    __device__ __forceinline__ void par(F f) const {
        f(lane, 64);
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void sum(F f, rp::Acc& a, int nq) const {      // nq: the entries of a.v in use
        rp::acc_zero(a);
        f(lane, 64, a);
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q)
            if (q < nq) a.v[q] = wave_sum64(a.v[q]);
    }
    template <class F>
    __device__ __forceinline__ int sum_i(F f) const { return wave_sum64_i(f(lane, 64)); }
};

static_assert(sizeof(plba_vitrack_result) == 8 * (size_t)vt::OUT_D + 4 * (size_t)vt::OUT_I, "the kernel writes plba_vitrack_result as it is laid out");
static_assert(offsetof(plba_vitrack_result, H900) == 8 * 44 && offsetof(plba_vitrack_result, chi2_initial) == 8 * 1169 &&
              offsetof(plba_vitrack_result, iterations) == 8 * (size_t)vt::OUT_D && offsetof(plba_vitrack_result, trials) == 8 * (size_t)vt::OUT_D + 64,
              "the kernel writes plba_vitrack_result as it is laid out");

__global__ __launch_bounds__(64) void k_vitrack(VitrackDev d) {
    __shared__ double shm[vt::SH_TOTAL];
    const int b = blockIdx.x;
    const int p0 = d.pt_start[b], l0 = d.ln_start[b];
    vt::Prob c;
    c.np = d.pt_start[b + 1] - p0; c.nl = d.ln_start[b + 1] - l0;
    c.anchor_free = d.anchor_free[b] ? 1 : 0;
    c.Pw3 = d.Pw3 + 3 * (size_t)p0; c.uv2 = d.uv2 + 2 * (size_t)p0; c.pt_w = d.pt_w + p0;
    c.pq6 = d.pq6 + 6 * (size_t)l0; c.l3 = d.l3 + 3 * (size_t)l0; c.ln_w = d.ln_w + l0;
    c.pt_in = d.pt_in + p0; c.ln_in = d.ln_in + l0;
    c.si0 = d.si + 22 * (size_t)b; c.sj0 = d.sj + 22 * (size_t)b;
    c.pre = d.pre + (size_t)PRE_STRIDE * b; c.ipvr = d.ipvr + 81 * (size_t)b; c.ibias = d.ibias + 36 * (size_t)b;
    c.pst = c.anchor_free ? d.pst + 22 * (size_t)b : nullptr; c.pinfo = c.anchor_free ? d.pinfo + 225 * (size_t)b : nullptr;
    char* o = d.out + sizeof(plba_vitrack_result) * (size_t)b;
    c.od = reinterpret_cast<double*>(o); c.oi = reinterpret_cast<int32_t*>(o + 8 * (size_t)vt::OUT_D);
    DevWave w{(int)threadIdx.x, shm};
    vt::run(w, c, d.o);
}

}  // namespace
}  // namespace plba

using namespace plba;

extern "C" {

void plba_vitrack_default_options(plba_vitrack_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->rounds = 4; o->iters = 10; o->max_trials = 10; o->robust_rounds = 2;
    o->tau = 1e-5; o->user_lambda_init = 0.0;
    o->huber_pt = o->huber_ln = (double)(float)sqrt(5.991);      // src/mapHandler.cpp:5896, :5956
    o->huber_imu = 0.0;
    o->chi2_pt = o->chi2_ln = 5.991;      // :6051
}

int plba_track_inertial(plba_problem* p, const plba_vitrack_options* opt, int B, const uint8_t* anchor_free, const double* state_i22, const double* state_j22,
                        const double* preint142, const double* info_pvr81, const double* info_bias36, const double* prior_state22, const double* prior_info225,
                        const double* gw3, const int32_t* pt_start, const double* Pw3, const double* uv2, const double* pt_inv_sigma2, const int32_t* ln_start,
                        const double* sPeP6, const double* l3, const double* ln_inv_sigma2, double fx, double fy, double cx, double cy, const double* Rbc9,
                        const double* Pbc3, uint8_t* pt_inlier, uint8_t* ln_inlier, plba_vitrack_result* out) {
    static const char* const me = "plba_track_inertial";
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !out) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: no options or no output", me);
    if (B < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: B = %d", me, B);
    if (!pt_start || !ln_start) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: missing start array", me);
    if (!state_i22 || !state_j22 || !preint142 || !info_pvr81 || !info_bias36 || !gw3 || !Rbc9 || !Pbc3) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: missing state, IMU or camera array", me);
    if (opt->rounds < 0 || opt->rounds > vt::MAX_ROUNDS) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: rounds = %d outside [0, %d]", me, opt->rounds, vt::MAX_ROUNDS);
    if (opt->iters < 0 || opt->max_trials < 0 || opt->robust_rounds < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: negative iters, max_trials or robust_rounds", me);
    for (const double v : {opt->tau, opt->user_lambda_init, opt->huber_pt, opt->huber_ln, opt->huber_imu, opt->chi2_pt, opt->chi2_ln, fx, fy, cx, cy})
        if (!std::isfinite(v)) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: an option or an intrinsic is not finite", me);
    for (const int32_t* st : {pt_start, ln_start})
        if (const char* why = check_starts(B, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: %s", me, why);
    const size_t Np = (size_t)pt_start[B], Nl = (size_t)ln_start[B], nb = (size_t)B;
    if ((Np && (!Pw3 || !uv2 || !pt_inv_sigma2)) || (Nl && (!sPeP6 || !l3 || !ln_inv_sigma2))) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: missing feature array", me);
    bool any_free = false;
    for (int b = 0; anchor_free && b < B; ++b) any_free = any_free || anchor_free[b];
    if (any_free && (!prior_state22 || !prior_info225)) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: a free anchor without the prior arrays", me);
    if (!all_finite(Pw3, 3 * Np) || !all_finite(uv2, 2 * Np) || !all_finite(pt_inv_sigma2, Np) || !all_finite(sPeP6, 6 * Nl) || !all_finite(l3, 3 * Nl) ||
        !all_finite(ln_inv_sigma2, Nl) || !all_finite(state_i22, 22 * nb) || !all_finite(state_j22, 22 * nb) || !all_finite(preint142, (size_t)PRE_STRIDE * nb) ||
        !all_finite(info_pvr81, 81 * nb) || !all_finite(info_bias36, 36 * nb) || !all_finite(gw3, 3) || !all_finite(Rbc9, 9) || !all_finite(Pbc3, 3))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: non-finite input", me);
    for (int b = 0; any_free && b < B; ++b)
        if (anchor_free[b] && (!all_finite(prior_state22 + 22 * (size_t)b, 22) || !all_finite(prior_info225 + 225 * (size_t)b, 225)))
            PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: non-finite prior", me);
    for (size_t i = 0; i < Np; ++i) if (pt_inv_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: a negative inv_sigma2", me);
    for (size_t i = 0; i < Nl; ++i) if (ln_inv_sigma2[i] < 0.0) PLBA_FAIL(p, PLBA_ERR_INVALID, "%s: a negative inv_sigma2", me);

    // one device block: [starts | features | states, IMU edges, priors, flags | masks || results]; the copy up takes what is before the
    // bar, the copy down the masks and the results (the masks are in both).  A fixed anchor's prior rows are never read: they go up as zeros.
    Layout L;
    const size_t n_st = 4 * (nb + 1);
    const size_t o_ps = L.take(n_st), o_ls = L.take(n_st), o_P = L.take(24 * Np), o_uv = L.take(16 * Np), o_wp = L.take(8 * Np), o_pq = L.take(48 * Nl),
                 o_l3 = L.take(24 * Nl), o_wl = L.take(8 * Nl), o_si = L.take(176 * nb), o_sj = L.take(176 * nb), o_pre = L.take(8 * (size_t)PRE_STRIDE * nb),
                 o_ip = L.take(648 * nb), o_ib = L.take(288 * nb), o_ps22 = L.take(any_free ? 176 * nb : 0), o_pi = L.take(any_free ? 1800 * nb : 0),
                 o_af = L.take(nb), o_pm = L.take(Np), o_lm = L.take(Nl), up_end = L.off, o_out = L.take(sizeof(plba_vitrack_result) * nb), down_end = L.off;
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_pm, down_end));
    call.put(o_ps, pt_start, n_st); call.put(o_ls, ln_start, n_st);
    call.put(o_P, Pw3, 24 * Np); call.put(o_uv, uv2, 16 * Np); call.put(o_wp, pt_inv_sigma2, 8 * Np);
    call.put(o_pq, sPeP6, 48 * Nl); call.put(o_l3, l3, 24 * Nl); call.put(o_wl, ln_inv_sigma2, 8 * Nl);
    call.put(o_si, state_i22, 176 * nb); call.put(o_sj, state_j22, 176 * nb); call.put(o_pre, preint142, 8 * (size_t)PRE_STRIDE * nb);
    call.put(o_ip, info_pvr81, 648 * nb); call.put(o_ib, info_bias36, 288 * nb);
    if (any_free) {
        memset(call.up<char>(o_ps22), 0, (176 * nb + 15) & ~(size_t)15); memset(call.up<char>(o_pi), 0, (1800 * nb + 15) & ~(size_t)15);
        for (int b = 0; b < B; ++b)
            if (anchor_free[b]) {
                memcpy(call.up<double>(o_ps22) + 22 * (size_t)b, prior_state22 + 22 * (size_t)b, 176);
                memcpy(call.up<double>(o_pi) + 225 * (size_t)b, prior_info225 + 225 * (size_t)b, 1800);
            }
    }
    mask_normalise(anchor_free, nb, call.up<uint8_t>(o_af));
    if (!anchor_free) memset(call.up<uint8_t>(o_af), 0, nb);      // no flags: every anchor is fixed
    memset(call.up<uint8_t>(o_af) + nb, 0, (0 - nb) & 15);
    mask_normalise(pt_inlier, Np, call.up<uint8_t>(o_pm)); mask_normalise(ln_inlier, Nl, call.up<uint8_t>(o_lm));
    PLBA_TRY(call.upload());
    VitrackDev d;
    d.o.rounds = opt->rounds; d.o.iters = opt->iters; d.o.max_trials = opt->max_trials; d.o.robust_rounds = opt->robust_rounds;
    d.o.tau = opt->tau; d.o.user_lambda_init = opt->user_lambda_init; d.o.huber_pt = opt->huber_pt; d.o.huber_ln = opt->huber_ln; d.o.huber_imu = opt->huber_imu;
    d.o.chi2_pt = opt->chi2_pt; d.o.chi2_ln = opt->chi2_ln;
    for (int k = 0; k < 3; ++k) d.o.gw[k] = gw3[k];
    d.o.cam.fx = fx; d.o.cam.fy = fy; d.o.cam.cx = cx; d.o.cam.cy = cy;
    cam_set_extrinsics(d.o.cam, Rbc9, Pbc3);
    d.pt_start = call.dev<int32_t>(o_ps); d.ln_start = call.dev<int32_t>(o_ls);
    d.Pw3 = call.dev<double>(o_P); d.uv2 = call.dev<double>(o_uv); d.pt_w = call.dev<double>(o_wp);
    d.pq6 = call.dev<double>(o_pq); d.l3 = call.dev<double>(o_l3); d.ln_w = call.dev<double>(o_wl);
    d.si = call.dev<double>(o_si); d.sj = call.dev<double>(o_sj); d.pre = call.dev<double>(o_pre); d.ipvr = call.dev<double>(o_ip); d.ibias = call.dev<double>(o_ib);
    d.pst = any_free ? call.dev<double>(o_ps22) : nullptr; d.pinfo = any_free ? call.dev<double>(o_pi) : nullptr;
    d.anchor_free = call.dev<uint8_t>(o_af);
    d.pt_in = call.dev<uint8_t>(o_pm); d.ln_in = call.dev<uint8_t>(o_lm);
    d.out = call.dev<char>(o_out);
    hipLaunchKernelGGL(k_vitrack, dim3((unsigned)B), dim3(64), 0, call.s, d);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());

    memcpy(out, call.down<char>(o_out), sizeof(plba_vitrack_result) * nb);
    if (pt_inlier) memcpy(pt_inlier, call.down<uint8_t>(o_pm), Np);
    if (ln_inlier) memcpy(ln_inlier, call.down<uint8_t>(o_lm), Nl);
    return PLBA_OK;
}

}  // extern "C"
