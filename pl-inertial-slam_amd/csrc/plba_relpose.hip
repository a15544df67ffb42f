// plba_relpose.hip — loop-closure candidate verification (plba_relative_pose, include/plba.h): MapHandler::computeRelativePoseRobustGN /
// computeRelativePoseGN (src/mapHandler.cpp:3411-4066) for B candidates in ONE launch, with no read-back between passes.
//
// Mapping: one wave (a 64-thread workgroup) per candidate.  A lane adds its own features (lane, lane + 64, ...; points, then lines) into
// 21 + 6 + 1 fp64 accumulators; the 64 partial sums are added by the fixed butterfly of plba_wave_dev.h — quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror and row_mirror inside a DPP row of 16, then lanes ^ 16 and ^ 32 across the rows — which leaves the same bits in every lane
// and, in lane 0, the balanced tree relpose::tree_sum() spells out for the host.  No atomics: a candidate's result depends on nothing but its own inputs.
// Lane 0 runs the serial part (exit tests, the 6 x 6 pivoted QR, expmap, the composition); its verdict and the 12 pose numbers reach
// the other lanes by lane reads.  The cut is a lane-parallel pass over the same lane -> feature map, so a mask byte is only ever
// touched by one lane.  A candidate is launch- and latency-bound (a handful of dependent passes over a few hundred features): the batch is
// what fills the machine.  The arithmetic is plba_relpose_dev.h, shared with the host check and the plain-C++ drop-in.
// The launch and the host result assembly are also lent to plba_match.hip (plba_verify_loop_candidates) through plba_relpose_launch.h.
// The host side of the call (one block, one copy up, one down, one wait) is plba_batch_call.h's.
#include "plba_batch_call.h"
#include "plba_relpose_launch.h"
#include "plba_wave_dev.h"

namespace plba {
namespace {

namespace rp = relpose;

struct DevWave {
    int lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ int share(int go, rp::Pose& T) const { return wave_lead(go, T.R, T.t); }
    __device__ void pass(const rp::Cand& c, const rp::Opt& o, const rp::Pose& T, rp::Acc& a) const {
        rp::lane_pass(c, o, T, lane, 64, a);
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q) a.v[q] = wave_sum64(a.v[q]);
        a.n = wave_sum64_i(a.n);
    }
    __device__ int count(const rp::Cand& c) const { return wave_sum64_i(rp::lane_count(c, lane, 64)); }
    __device__ int cut(const rp::Cand& c, const rp::Opt& o, const rp::Pose& T) const { return wave_sum64_i(rp::lane_cut(c, o, T, lane, 64)); }
};

__global__ __launch_bounds__(64) void k_relpose(RelposeDev d) {
    const int b = blockIdx.x;
    const int p0 = d.pt_start[b], l0 = d.ln_start[b];
    rp::Cand c;
    c.np = d.pt_start[b + 1] - p0; c.nl = d.ln_start[b + 1] - l0;
    c.P3 = d.P3 + 3 * (size_t)p0; c.uv2 = d.uv2 + 2 * (size_t)p0; c.pq6 = d.pq6 + 6 * (size_t)l0; c.l3 = d.l3 + 3 * (size_t)l0;
    c.pt_in = d.pt_in + p0; c.ln_in = d.ln_in + l0;
    DevWave w{(int)threadIdx.x};
    rp::State s;
    rp::run(w, c, d.o, d.T0 ? d.T0 + 12 * (size_t)b : nullptr, s);
    if (threadIdx.x == 0) {
        double* od = d.out_d + (size_t)RP_OUT_D * b;
        for (int i = 0; i < 9; ++i) od[i] = s.T.R[i];
        for (int i = 0; i < 3; ++i) od[9 + i] = s.T.t[i];
        for (int i = 0; i < 21; ++i) od[12 + i] = s.H[i];
        od[33] = s.e;
        rp::finish(s, d.o.protocol, od + 34, od + 40);
        int32_t* oi = d.out_i + (size_t)RP_OUT_I * b;
        oi[0] = s.n_inl; oi[1] = s.iters[0]; oi[2] = s.iters[1]; oi[3] = s.status;
    }
}

}  // namespace

void relpose_set_options(const plba_relpose_options& opt, double fx, double fy, double cx, double cy, relpose::Opt& o) {
    o.max_iters = opt.max_iters; o.max_iters_ref = opt.max_iters_ref; o.protocol = opt.protocol; o.homog_th = opt.homog_th;
    o.cut = sqrt(opt.chi2_th); o.fx = fx; o.fy = fy; o.cx = cx; o.cy = cy;
}

hipError_t relpose_launch(const RelposeDev& d, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_relpose, dim3((unsigned)B), dim3(64), 0, s, d);
    return hipGetLastError();
}

// the uncertainty and the decision, on the host from what came back (:3593-3628, :3985-4021)
void relpose_assemble(const plba_relpose_options& opt, int n_features, const double* q, const int32_t* oi, plba_relpose_result& r) {
    const rp::Thresholds th{opt.lc_res, opt.lc_unc, opt.lc_inl, opt.lc_trs, opt.lc_rot};
    rp::State st;
    for (int i = 0; i < 9; ++i) st.T.R[i] = q[i];
    for (int i = 0; i < 3; ++i) st.T.t[i] = q[9 + i];
    for (int i = 0; i < 21; ++i) st.H[i] = q[12 + i];
    st.e = q[33];
    st.n_inl = oi[0]; st.iters[0] = oi[1]; st.iters[1] = oi[2]; st.status = oi[3];
    rp::Decision dec;
    rp::decide(st, q + 34, opt.protocol, n_features, th, dec);
    pose_unpack16(q, r.T_inc16);
    const bool ok = dec.status == PLBA_RELPOSE_OK || dec.status == PLBA_RELPOSE_RANK;
    for (int i = 0; i < 6; ++i) r.pose_inc6[i] = ok ? q[40 + i] : 0.0;
    sym6_expand(q + 12, r.H36);
    r.e = st.e;
    for (int i = 0; i < 6; ++i) r.cov_eig6[i] = dec.cov_eig[i];
    r.t = dec.t; r.r = dec.r;
    r.n_inliers = st.n_inl; r.iters[0] = st.iters[0]; r.iters[1] = st.iters[1];
    r.status = dec.status; r.accepted = dec.accepted;
    r.lc_res = dec.lc_res; r.lc_unc = dec.lc_unc; r.lc_inl = dec.lc_inl; r.lc_trs = dec.lc_trs; r.lc_rot = dec.lc_rot;
}

const char* relpose_check_options(const plba_relpose_options& opt, double fx, double fy, double cx, double cy) {
    if (opt.protocol != 0 && opt.protocol != 1) return "protocol is not 0 or 1";
    if (opt.max_iters < 0 || opt.max_iters_ref < 0) return "negative iteration count";
    for (const double v : {opt.homog_th, opt.chi2_th, opt.lc_res, opt.lc_unc, opt.lc_inl, opt.lc_trs, opt.lc_rot, fx, fy, cx, cy})
        if (!std::isfinite(v)) return "an option or an intrinsic is not finite";
    if (opt.chi2_th < 0.0) return "chi2_th < 0";
    return nullptr;
}

}  // namespace plba

using namespace plba;

extern "C" {

void plba_relpose_default_options(plba_relpose_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_iters = 5; o->max_iters_ref = 10; o->homog_th = 1e-7;      // Config::maxIters / maxItersRef / homogTh, stvo-pl/src/config.cpp:80-83
    o->chi2_th = 7.815;                                                // :3569, :3836
    o->protocol = 0;
    o->lc_res = 1.0; o->lc_unc = 0.01; o->lc_inl = 0.3; o->lc_trs = 1.5; o->lc_rot = 35.0;      // src/slamConfig.cpp:73-77
}

int plba_relative_pose(plba_problem* p, const plba_relpose_options* opt, int B, const int32_t* pt_start, const double* P3, const double* uv2,
                       const int32_t* ln_start, const double* sPeP6, const double* l3, double fx, double fy, double cx, double cy,
                       const double* T0_16, uint8_t* pt_inlier, uint8_t* ln_inlier, plba_relpose_result* out) {
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !out) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: no options or no output");
    if (B < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: B = %d", B);
    if (!pt_start || !ln_start) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: missing start array");
    if (const char* why = relpose_check_options(*opt, fx, fy, cx, cy)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: %s", why);
    for (const int32_t* st : {pt_start, ln_start})
        if (const char* why = check_starts(B, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: %s", why);
    const size_t Np = (size_t)pt_start[B], Nl = (size_t)ln_start[B];
    if ((Np && (!P3 || !uv2)) || (Nl && (!sPeP6 || !l3))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: missing feature array");
    if (!all_finite(P3, 3 * Np) || !all_finite(uv2, 2 * Np) || !all_finite(sPeP6, 6 * Nl) || !all_finite(l3, 3 * Nl) || (T0_16 && !all_finite(T0_16, 16 * (size_t)B)))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: non-finite input");

    // one device block: [starts | features | T0 | masks || results]; the copy up takes what is before the bar, the copy down the masks and
    // the results: the masks are in both
    Layout L;
    const size_t n_st = 4 * ((size_t)B + 1);
    const size_t o_ps = L.take(n_st), o_ls = L.take(n_st), o_P = L.take(24 * Np), o_uv = L.take(16 * Np), o_pq = L.take(48 * Nl), o_l3 = L.take(24 * Nl),
                 o_T0 = L.take(T0_16 ? 96 * (size_t)B : 0), o_pm = L.take(Np), o_lm = L.take(Nl), up_end = L.off, o_od = L.take(8 * (size_t)RP_OUT_D * B),
                 o_oi = L.take(4 * (size_t)RP_OUT_I * B);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_pm, L.off));
    call.put(o_ps, pt_start, n_st); call.put(o_ls, ln_start, n_st);
    call.put(o_P, P3, 24 * Np); call.put(o_uv, uv2, 16 * Np); call.put(o_pq, sPeP6, 48 * Nl); call.put(o_l3, l3, 24 * Nl);
    if (T0_16)
        for (int b = 0; b < B; ++b) pose_pack12(T0_16 + 16 * (size_t)b, call.up<double>(o_T0) + 12 * (size_t)b);
    mask_normalise(pt_inlier, Np, call.up<uint8_t>(o_pm)); mask_normalise(ln_inlier, Nl, call.up<uint8_t>(o_lm));
    PLBA_TRY(call.upload());
    RelposeDev d;
    relpose_set_options(*opt, fx, fy, cx, cy, d.o);
    d.pt_start = call.dev<int32_t>(o_ps); d.ln_start = call.dev<int32_t>(o_ls);
    d.P3 = call.dev<double>(o_P); d.uv2 = call.dev<double>(o_uv); d.pq6 = call.dev<double>(o_pq); d.l3 = call.dev<double>(o_l3);
    d.T0 = T0_16 ? call.dev<double>(o_T0) : nullptr;
    d.pt_in = call.dev<uint8_t>(o_pm); d.ln_in = call.dev<uint8_t>(o_lm);
    d.out_d = call.dev<double>(o_od); d.out_i = call.dev<int32_t>(o_oi);
    PLBA_HIPCK(p, relpose_launch(d, B, call.s));
    PLBA_TRY(call.download());

    const double* od = call.down<double>(o_od);
    const int32_t* oi = call.down<int32_t>(o_oi);
    for (int b = 0; b < B; ++b)
        relpose_assemble(*opt, (pt_start[b + 1] - pt_start[b]) + (ln_start[b + 1] - ln_start[b]), od + (size_t)RP_OUT_D * b, oi + (size_t)RP_OUT_I * b, out[b]);
    if (pt_inlier) memcpy(pt_inlier, call.down<uint8_t>(o_pm), Np);
    if (ln_inlier) memcpy(ln_inlier, call.down<uint8_t>(o_lm), Nl);
    return PLBA_OK;
}

}  // extern "C"
