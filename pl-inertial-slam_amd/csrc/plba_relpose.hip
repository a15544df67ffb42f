// plba_relpose.hip — loop-closure candidate verification (plba_relative_pose, include/plba.h): MapHandler::computeRelativePoseRobustGN /
// computeRelativePoseGN (src/mapHandler.cpp:3411-4066) for B candidates in ONE launch, with no read-back between passes.
//
// Mapping: one wave (a 64-thread workgroup) per candidate.  A lane adds its own features (lane, lane + 64, ...; points, then lines) into
// 21 + 6 + 1 fp64 accumulators; the 64 partial sums are added by a butterfly — quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror and
// row_mirror inside a DPP row of 16, then lanes ^ 16 and ^ 32 across the rows — which leaves the same bits in every lane and, in lane 0,
// the balanced tree relpose::tree_sum() spells out for the host.  No atomics: a candidate's result depends on nothing but its own inputs.
// Lane 0 runs the serial part (exit tests, the 6 x 6 pivoted QR, expmap, the composition); its verdict and the 12 pose numbers reach
// the other lanes by lane reads.  The cut is a lane-parallel pass over the same lane -> feature map, so a mask byte is only ever
// touched by one lane.  A candidate is launch- and latency-bound (a handful of dependent passes over a few hundred features): the batch is
// what fills the machine.  The arithmetic is plba_relpose_dev.h, shared with the host check and the plain-C++ drop-in.
// The launch and the host result assembly are also lent to plba_match.hip (plba_verify_loop_candidates) through plba_relpose_launch.h.
#include <vector>

#include "plba_problem.h"
#include "plba_relpose_launch.h"

namespace plba {
namespace {

namespace rp = relpose;

template <int CTRL>
__device__ __forceinline__ double rp_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, the same bits in all of them: every step adds the two operands of a pair in both of its lanes
__device__ __forceinline__ double rp_sum64(double v) {
    v += rp_dpp<0xB1>(v);
    v += rp_dpp<0x4E>(v);
    v += rp_dpp<0x141>(v);
    v += rp_dpp<0x140>(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int rp_sum64_i(int v) {
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
    __device__ int share(int go, rp::Pose& T) const {
#pragma unroll
        for (int i = 0; i < 9; ++i) T.R[i] = __shfl(T.R[i], 0);
#pragma unroll
        for (int i = 0; i < 3; ++i) T.t[i] = __shfl(T.t[i], 0);
        return __shfl(go, 0);
    }
    __device__ void pass(const rp::Cand& c, const rp::Opt& o, const rp::Pose& T, rp::Acc& a) const {
        rp::lane_pass(c, o, T, lane, 64, a);
#pragma unroll
        for (int q = 0; q < rp::NACC; ++q) a.v[q] = rp_sum64(a.v[q]);
        a.n = rp_sum64_i(a.n);
    }
    __device__ int count(const rp::Cand& c) const { return rp_sum64_i(rp::lane_count(c, lane, 64)); }
    __device__ int cut(const rp::Cand& c, const rp::Opt& o, const rp::Pose& T) const { return rp_sum64_i(rp::lane_cut(c, o, T, lane, 64)); }
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

size_t al8(size_t b) { return (b + 7) & ~(size_t)7; }

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
    for (int i = 0; i < 3; ++i) { r.T_inc16[i * 4] = q[i * 3]; r.T_inc16[i * 4 + 1] = q[i * 3 + 1]; r.T_inc16[i * 4 + 2] = q[i * 3 + 2]; r.T_inc16[i * 4 + 3] = q[9 + i]; }
    r.T_inc16[12] = r.T_inc16[13] = r.T_inc16[14] = 0.0; r.T_inc16[15] = 1.0;
    const bool ok = dec.status == PLBA_RELPOSE_OK || dec.status == PLBA_RELPOSE_RANK;
    for (int i = 0; i < 6; ++i) r.pose_inc6[i] = ok ? q[40 + i] : 0.0;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { r.H36[i * 6 + j] = q[12 + k]; r.H36[j * 6 + i] = q[12 + k]; ++k; }
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
    for (const int32_t* st : {pt_start, ln_start}) {
        if (st[0] != 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: a start array does not begin at 0");
        for (int b = 0; b < B; ++b) if (st[b + 1] < st[b]) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: the starts of candidate %d descend", b);
    }
    const size_t Np = (size_t)pt_start[B], Nl = (size_t)ln_start[B];
    if ((Np && (!P3 || !uv2)) || (Nl && (!sPeP6 || !l3))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: missing feature array");
    auto finite = [](const double* a, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false; return true; };
    if (!finite(P3, 3 * Np) || !finite(uv2, 2 * Np) || !finite(sPeP6, 6 * Nl) || !finite(l3, 3 * Nl) || (T0_16 && !finite(T0_16, 16 * (size_t)B)))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_relative_pose: non-finite input");

    // one device block: [starts | features | T0 || masks || results]; the copy up takes everything before the second bar, the copy down
    // everything behind the first
    const size_t o_ps = 0, o_ls = o_ps + al8(4 * (size_t)(B + 1)), o_P = o_ls + al8(4 * (size_t)(B + 1)), o_uv = o_P + 24 * Np, o_pq = o_uv + 16 * Np,
                 o_l3 = o_pq + 48 * Nl, o_T0 = o_l3 + 24 * Nl, o_pm = o_T0 + (T0_16 ? 96 * (size_t)B : 0), o_lm = o_pm + al8(Np), o_od = o_lm + al8(Nl),
                 o_oi = o_od + 8 * (size_t)RP_OUT_D * B, total = o_oi + al8(4 * (size_t)RP_OUT_I * B);
    const size_t up = o_od, down = total - o_pm;
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
    if (Np) { memcpy(hu + o_P, P3, 24 * Np); memcpy(hu + o_uv, uv2, 16 * Np); }
    if (Nl) { memcpy(hu + o_pq, sPeP6, 48 * Nl); memcpy(hu + o_l3, l3, 24 * Nl); }
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
    RelposeDev d;
    relpose_set_options(*opt, fx, fy, cx, cy, d.o);
    d.pt_start = reinterpret_cast<const int32_t*>(blk.p + o_ps); d.ln_start = reinterpret_cast<const int32_t*>(blk.p + o_ls);
    d.P3 = reinterpret_cast<const double*>(blk.p + o_P); d.uv2 = reinterpret_cast<const double*>(blk.p + o_uv);
    d.pq6 = reinterpret_cast<const double*>(blk.p + o_pq); d.l3 = reinterpret_cast<const double*>(blk.p + o_l3);
    d.T0 = T0_16 ? reinterpret_cast<const double*>(blk.p + o_T0) : nullptr;
    d.pt_in = reinterpret_cast<uint8_t*>(blk.p + o_pm); d.ln_in = reinterpret_cast<uint8_t*>(blk.p + o_lm);
    d.out_d = reinterpret_cast<double*>(blk.p + o_od); d.out_i = reinterpret_cast<int32_t*>(blk.p + o_oi);
    PLBA_HIPCK(p, relpose_launch(d, B, s));
    PLBA_HIPCK(p, hipMemcpyAsync(hd, blk.p + o_pm, down, hipMemcpyDeviceToHost, s));
    PLBA_HIPCK(p, plba_stream_wait(p, s));      // the call's one blocking wait

    const double* od = reinterpret_cast<const double*>(hd + (o_od - o_pm));
    const int32_t* oi = reinterpret_cast<const int32_t*>(hd + (o_oi - o_pm));
    for (int b = 0; b < B; ++b)
        relpose_assemble(*opt, (pt_start[b + 1] - pt_start[b]) + (ln_start[b + 1] - ln_start[b]), od + (size_t)RP_OUT_D * b, oi + (size_t)RP_OUT_I * b, out[b]);
    if (pt_inlier) memcpy(pt_inlier, hd, Np);
    if (ln_inlier) memcpy(ln_inlier, hd + (o_lm - o_pm), Nl);
    return PLBA_OK;
}

}  // extern "C"
