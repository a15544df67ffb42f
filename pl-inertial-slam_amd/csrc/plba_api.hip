// plba_api.hip — the C ABI of include/plba.h on top of the HIP kernels (gfx950).
//
// Host side of the hot path: flattens the uploaded graph into device SoA buffers, builds the static
// structure (landmark CSR, keyframe-pair lists for the Schur complement, pose-side index map), and
// drives g2o's Levenberg-Marquardt control flow with every arithmetic step on
// the device; only the control block (a few scalars) crosses PCIe once per damped trial (k_decide writes it into
// mapped host memory, the host polls a sequence number).
// No CPU fallback exists: every entry point that computes needs a HIP device.
#include <atomic>
#include <algorithm>
#include <thread>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>

#include "plba_problem.h"

using namespace plba;

namespace {
char g_create_err[256] = "";
static std::mutex g_ctx_mu;
static std::vector<HostCtx> g_ctx_free;
static std::map<int, hipStream_t> g_lib_stream;
// Parked problems (round 5).  The reference builds a fresh optimizer per local BA (src/mapHandler.cpp:5787-5797), so a drop-in caller
// creates and destroys a plba_problem per call.  plba_destroy parks up to PARK_MAX problems per process instead of freeing them and
// plba_create hands one back with every caller-visible field reset: the device buffers stay allocated and — because the pose-structure
// cache is keyed on CONTENT, not on the handle — the next window with the same pose structure finds it built (0.3 ms per BA call at
// configs[2] for the g2o facade, which can not keep a handle).  That a re-used handle gives bit-identical results to a fresh one is what
// tests/test_gpu_parity.py::test_a_problem_handle_reused_across_windows_matches_fresh_handles pins; with parking every test runs on
// recycled handles.
static std::vector<plba_problem*> g_parked;
static const size_t PARK_MAX = 2;
}  // namespace

// every field a caller can see or set goes back to what a new plba_problem() has; device buffers, the batch blocks, the events and the
// structure cache stay
static void reset_for_reuse(plba_problem* p, const plba_options* opt) {
    marg_discard(p);      // (plba_destroy has done so already)
    plba_bow_discard(p);
    plba_covis_discard(p);
    if (opt) p->opt = *opt; else plba_default_options(&p->opt);
    p->err[0] = 0;
    p->stream = p->ctx.stream; p->own_stream = true;
    p->ev_sample = false; p->trial_counter = 0; p->spec_lin = false; p->lin_in_span = false; p->prof_lin_launches = 0;
    p->marg_dbg.clear(); p->cov_dbg_S.clear(); p->cov_dbg_Sigma.clear(); for (double& v : p->marg_path) v = 0.0;
    p->spec_hll = false;
    p->win.clear(); p->win_next.clear(); p->lm0.clear(); p->lm_fixed.clear();
    p->pr_n = p->pr_nv = 0; p->pr_vid.clear(); p->pr_size.clear(); p->pr_idx.clear(); p->pr_x0.clear(); p->pr_J0.clear(); p->pr_r0.clear();
    p->prior_dev = false; p->prior_changed = false; p->pr_m = 0; p->host_waits = 0;
    for (double& v : p->pgo_sparse) v = 0.0;
    for (double& v : p->lba_sparse) v = 0.0;
    for (double& v : p->pgo_cov) v = 0.0;
    p->pgo_cov_H.clear();
    memset(&p->rob, 0, sizeof p->rob);
    p->rank = 0; p->world = 1; p->xfn = nullptr; p->xuser = nullptr;
    p->dirty = true; p->P = p->Ppad = p->ld = p->L = p->E = 0; p->cur = 0;
    p->carry_obs_pending = false;
    p->ob_pos.clear(); p->flow_epoch = 0;
    p->lm_ok = false; p->lm_grouped = false; ++p->state_epoch; p->res_lm_epoch = 0; p->res_lm.clear(); p->lm_hist.clear();
    p->lm_chi_dirty = false; p->back_epoch = 0; p->lm_disable = false; p->lm_spec = false; p->assembled = false;
    p->chi_E = -1; p->chi_carry = false; p->chi_keep.clear();
    memset(&p->lv, 0, sizeof p->lv);
    p->trace.clear(); p->saved_valid = false;
    memset(p->h_mail, 0, sizeof(Mailbox)); p->mail_seq = 0;
}


#define FAIL(p, code, ...)                                  \
    do {                                                    \
        snprintf((p)->err, sizeof((p)->err), __VA_ARGS__);  \
        return (code);                                      \
    } while (0)
#define HIPCK(p, call)                                                                                        \
    do {                                                                                                      \
        hipError_t e__ = (call);                                                                              \
        if (e__ != hipSuccess) FAIL(p, PLBA_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

static const int TRACE_CAP = 4096;
static const int SCHUR_CHUNK = 256;   // entries of a keyframe pair per k_schur_pairs workgroup (512: no faster)

extern "C" {

void plba_default_options(plba_options* o) {
    memset(o, 0, sizeof(*o));
    o->tau = 1e-5;
    o->good_step_lower = 1. / 3.;
    o->good_step_upper = 2. / 3.;
    o->max_trials = 10;
    o->user_lambda_init = 0.0;
    o->marg_eps = 1e-8;
    o->device = -1;
    o->use_mfma = 1;
    o->factor_block = 32;
    o->factor_flow = 0;
    o->chain_elim = 1;
    o->wide_steps = 0;
    o->band_solve = 1;
    o->marg_exact = 1;
    o->lm_fused = 1;
    o->lm_fused_min_obs = 40000;
}
const char* plba_backend_name(void) { return "hip-gfx950"; }
const char* plba_last_error(const plba_problem* p) { return p ? p->err : g_create_err; }

int plba_create(const plba_options* opt, plba_problem** out) {
    if (!out) { snprintf(g_create_err, sizeof g_create_err, "out is NULL"); return PLBA_ERR_INVALID; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        snprintf(g_create_err, sizeof g_create_err, "no HIP device available (%s); the plba product path has no CPU fallback",
                 e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return PLBA_ERR_DEVICE;
    }
    {   // a parked problem of this device, if there is one
        int want = -1;
        if (opt && opt->device >= 0) {
            if ((e = hipSetDevice(opt->device)) != hipSuccess) { snprintf(g_create_err, sizeof g_create_err, "hipSetDevice(%d): %s", opt->device, hipGetErrorString(e)); return PLBA_ERR_DEVICE; }
        }
        (void)hipGetDevice(&want);
        plba_problem* q = nullptr;
        {
            std::lock_guard<std::mutex> g(g_ctx_mu);
            for (size_t i = g_parked.size(); i-- > 0;)
                if (g_parked[i]->device == want) { q = g_parked[i]; g_parked.erase(g_parked.begin() + (long)i); break; }
        }
        if (q) { reset_for_reuse(q, opt); *out = q; return PLBA_OK; }
    }
    plba_problem* p = new plba_problem();
    p->err[0] = 0;
    if (opt) p->opt = *opt; else plba_default_options(&p->opt);
    memset(&p->rob, 0, sizeof p->rob);
    if (p->opt.device >= 0) {
        if ((e = hipSetDevice(p->opt.device)) != hipSuccess) {
            snprintf(g_create_err, sizeof g_create_err, "hipSetDevice(%d): %s", p->opt.device, hipGetErrorString(e));
            delete p;
            return PLBA_ERR_DEVICE;
        }
    }
    (void)hipGetDevice(&p->device);
    // stream, pinned control block and mapped mailbox come from a process-wide cache: creating and freeing them per BA
    // call (hipHostMalloc / hipHostFree / stream create / destroy synchronise the device and remap memory) costs
    // milliseconds as soon as another problem is alive
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        for (size_t i = 0; i < g_ctx_free.size(); ++i)
            if (g_ctx_free[i].device == p->device) { p->ctx = g_ctx_free[i]; g_ctx_free.erase(g_ctx_free.begin() + (long)i); p->have_ctx = true; break; }
    }
    if (!p->have_ctx) {
        HostCtx c;
        c.device = p->device;
        // ONE library stream per device, shared by every problem that does not bring its own (plba_set_stream).  (The ~20 ms
        // stalls once blamed on idle queues came from pageable host memory handed to hipMemcpy: plba_problem.h, plba_d2h.)
        {
            std::lock_guard<std::mutex> g(g_ctx_mu);
            auto it = g_lib_stream.find(p->device);
            if (it == g_lib_stream.end()) {
                hipStream_t st = nullptr;
                if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) == hipSuccess) it = g_lib_stream.emplace(p->device, st).first;
            }
            if (it != g_lib_stream.end()) { c.stream = it->second; e = hipSuccess; }
        }
        if (e != hipSuccess ||
            (e = hipHostMalloc((void**)&c.h_ctrl, sizeof(Ctrl), hipHostMallocDefault)) != hipSuccess ||
            (e = hipHostMalloc((void**)&c.h_mail, sizeof(Mailbox), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
            (e = hipHostGetDevicePointer((void**)&c.d_mail, c.h_mail, 0)) != hipSuccess) {
            snprintf(g_create_err, sizeof g_create_err, "device initialisation failed: %s", hipGetErrorString(e));
            delete p;
            return PLBA_ERR_DEVICE;
        }
        c.stage = new StageArea;
        const size_t cap = (size_t)64 << 20;
        if (hipHostMalloc((void**)&c.stage->base, cap, hipHostMallocDefault) == hipSuccess) c.stage->cap = cap;      // optional: uploads fall back to pageable copies
        else c.stage->base = nullptr;
        p->ctx = c; p->have_ctx = true;
    }
    p->stream = p->ctx.stream; p->h_ctrl = (Ctrl*)p->ctx.h_ctrl; p->h_mail = (Mailbox*)p->ctx.h_mail; p->d_mail = (Mailbox*)p->ctx.d_mail;
    memset(p->h_mail, 0, sizeof(Mailbox));
    p->mail_seq = 0;
    p->own_stream = true;
    *out = p;
    return PLBA_OK;
}

void plba_destroy(plba_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    marg_discard(p);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    plba_bow_discard(p);
    plba_covis_discard(p);
    if (p->have_ctx) {
        (void)hipStreamSynchronize(p->ctx.stream);
        std::lock_guard<std::mutex> g(g_ctx_mu);
        if (g_parked.size() < PARK_MAX) { g_parked.push_back(p); return; }      // parked with its context, buffers and structure cache (plba_create resets the rest)
        g_ctx_free.push_back(p->ctx);          // kept for the next problem (never freed: a handful of bytes and one stream per concurrent problem)
    }
    if (p->ev_ready) for (auto& e : p->ev) (void)hipEventDestroy(e);
    delete p;
}

int plba_set_stream(plba_problem* p, void* s) {
    if (!p) return PLBA_ERR_INVALID;
    if (p->own_stream && p->stream) (void)hipStreamSynchronize(p->stream);      // the problem's own stream stays with its cached context
    p->stream = (hipStream_t)s;
    p->own_stream = false;
    return PLBA_OK;
}

int plba_set_camera(plba_problem* p, double fx, double fy, double cx, double cy, const double* Rbc, const double* Pbc) {
    if (!p || !Rbc || !Pbc) return PLBA_ERR_INVALID;
    p->win.fx = fx; p->win.fy = fy; p->win.cx = cx; p->win.cy = cy;
    memcpy(p->win.Rbc, Rbc, 72); memcpy(p->win.Pbc, Pbc, 24);
    p->win.have_cam = true; p->dirty = true;
    return PLBA_OK;
}
int plba_set_gravity(plba_problem* p, const double* gw) {
    if (!p || !gw) return PLBA_ERR_INVALID;
    memcpy(p->win.gw, gw, 24);
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_keyframes(plba_problem* p, int K, const int32_t* vid_pvr, const int32_t* vid_bias, const double* P3, const double* V3,
                       const double* q4, const double* bg3, const double* ba3, const double* dbg3, const double* dba3,
                       const uint8_t* fixed_pvr, const uint8_t* fixed_bias) {
    if (!p || K <= 0 || !vid_pvr || !P3 || !V3 || !q4) return PLBA_ERR_INVALID;
    for (int k = 1; k < K; ++k) if (vid_pvr[k] <= vid_pvr[k - 1]) FAIL(p, PLBA_ERR_INVALID, "keyframe vertex ids must be ascending");
    if (!all_finite(P3, 3 * (size_t)K) || !all_finite(V3, 3 * (size_t)K) || !all_finite(q4, 4 * (size_t)K)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite keyframe state");
    p->win.K = K; p->win.carry_kf = false;
    p->win.vid_pvr.assign(vid_pvr, vid_pvr + K);
    p->win.vid_bias.assign(K, -1);
    p->win.kf0.assign((size_t)K * KF_STRIDE, 0.0);
    p->win.fix_pvr.assign(K, 0); p->win.fix_bias.assign(K, 0);
    for (int k = 0; k < K; ++k) {
        double* s = &p->win.kf0[(size_t)k * KF_STRIDE];
        if (vid_bias) p->win.vid_bias[k] = vid_bias[k];
        memcpy(s, P3 + 3 * k, 24); memcpy(s + 3, V3 + 3 * k, 24); memcpy(s + 6, q4 + 4 * k, 32);
        if (bg3) memcpy(s + 10, bg3 + 3 * k, 24);
        if (ba3) memcpy(s + 13, ba3 + 3 * k, 24);
        if (dbg3) memcpy(s + 16, dbg3 + 3 * k, 24);
        if (dba3) memcpy(s + 19, dba3 + 3 * k, 24);
        if (fixed_pvr) p->win.fix_pvr[k] = fixed_pvr[k];
        if (fixed_bias) p->win.fix_bias[k] = fixed_bias[k];
    }
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_points(plba_problem* p, int Np, const double* xyz, const uint8_t* fixed) {
    if (!p || Np < 0 || (Np && !xyz)) return PLBA_ERR_INVALID;
    if (!all_finite(xyz, 3 * (size_t)Np)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite point");
    p->win.Np = Np;
    p->win.pts.assign(xyz, xyz + 3 * (size_t)Np);
    p->win.carry_pts = false;
    p->win.pt_fixed.assign(Np, 0);
    if (fixed) p->win.pt_fixed.assign(fixed, fixed + Np);
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_lines(plba_problem* p, int Nl, const double* l, const uint8_t* fixed) {
    if (!p || Nl < 0 || (Nl && !l)) return PLBA_ERR_INVALID;
    if (!all_finite(l, 6 * (size_t)Nl)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite line");
    p->win.Nl = Nl;
    p->win.lns.assign(l, l + 6 * (size_t)Nl);
    p->win.carry_lns = false;
    p->win.ln_fixed.assign(Nl, 0);
    if (fixed) p->win.ln_fixed.assign(fixed, fixed + Nl);
    p->dirty = true;
    return PLBA_OK;
}
static int check_obs(plba_problem* p, int E, const int32_t* lm, const int32_t* kf, int Nlm) {
    for (int e = 0; e < E; ++e) {
        if (lm[e] < 0 || lm[e] >= Nlm) FAIL(p, PLBA_ERR_INVALID, "observation %d: landmark index out of range", e);
        if (kf[e] < 0 || kf[e] >= p->win.K) FAIL(p, PLBA_ERR_INVALID, "observation %d: keyframe index out of range", e);
        if (e && lm[e] < lm[e - 1]) FAIL(p, PLBA_ERR_INVALID, "observations must be landmark-major (sorted by landmark)");
    }
    for (int e = 0; e < E; ++e)
        for (int f = e + 1; f < E && lm[f] == lm[e]; ++f)
            if (kf[f] == kf[e]) FAIL(p, PLBA_ERR_INVALID, "landmark %d observed twice by keyframe %d", lm[e], kf[e]);
    return PLBA_OK;
}
int plba_set_point_obs(plba_problem* p, int Ep, const int32_t* pt, const int32_t* kf, const double* uv, const double* w) {
    if (!p || Ep < 0 || (Ep && (!pt || !kf || !uv))) return PLBA_ERR_INVALID;
    if (!p->win.K) FAIL(p, PLBA_ERR_STATE, "set_keyframes first");
    int rc = check_obs(p, Ep, pt, kf, p->win.Np);
    if (rc) return rc;
    if (!all_finite(uv, 2 * (size_t)Ep)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite observation");
    p->win.Ep = Ep;
    p->win.po_pt.assign(pt, pt + Ep); p->win.po_kf.assign(kf, kf + Ep);
    p->win.po_uv.assign(uv, uv + 2 * (size_t)Ep);
    p->win.po_w.assign(Ep, 1.0);
    if (w) for (int e = 0; e < Ep; ++e) p->win.po_w[e] = (double)(float)w[e];   // const float& invSigma2 (mapHandler.cpp:5340)
    p->win.carry_po = false;
    p->win.level.assign((size_t)p->win.Ep + p->win.El, 0);      // new edges are level 0 (g2o); a re-used handle does not inherit the previous window's
    p->chi_E = -1; p->chi_carry = false;      // ... and have no cached error
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_line_obs(plba_problem* p, int El, const int32_t* ln, const int32_t* kf, const double* l3, const double* w) {
    if (!p || El < 0 || (El && (!ln || !kf || !l3))) return PLBA_ERR_INVALID;
    if (!p->win.K) FAIL(p, PLBA_ERR_STATE, "set_keyframes first");
    int rc = check_obs(p, El, ln, kf, p->win.Nl);
    if (rc) return rc;
    if (!all_finite(l3, 3 * (size_t)El)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite observation");
    p->win.El = El;
    p->win.lo_ln.assign(ln, ln + El); p->win.lo_kf.assign(kf, kf + El);
    p->win.lo_l.assign(l3, l3 + 3 * (size_t)El);
    p->win.lo_w.assign(El, 1.0);
    if (w) for (int e = 0; e < El; ++e) p->win.lo_w[e] = (double)(float)w[e];
    p->win.carry_lo = false;
    // the new line edges are level 0; the POINT edges' levels stay (set_point_obs -> set_levels(POINT) -> set_line_obs used
    // to drop them).  plba_set_point_obs still resets both ranges: Ep moves the line range's offset.
    p->win.level.resize((size_t)p->win.Ep + p->win.El);
    std::fill(p->win.level.begin() + std::min((size_t)p->win.Ep, p->win.level.size()), p->win.level.end(), (uint8_t)0);
    p->chi_E = -1; p->chi_carry = false;
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_imu_edges(plba_problem* p, int M, const int32_t* ki, const int32_t* kj, const double* pre, const double* ipvr, const double* ibias) {
    if (!p || M < 0 || (M && (!ki || !kj || !pre || !ipvr || !ibias))) return PLBA_ERR_INVALID;
    for (int m = 0; m < M; ++m) {
        if (ki[m] < 0 || ki[m] >= p->win.K || kj[m] < 0 || kj[m] >= p->win.K) FAIL(p, PLBA_ERR_INVALID, "imu edge %d: keyframe index", m);
        if (p->win.vid_bias[ki[m]] < 0 || p->win.vid_bias[kj[m]] < 0) FAIL(p, PLBA_ERR_INVALID, "imu edge %d: keyframe without bias vertex", m);
    }
    if (!all_finite(pre, 142 * (size_t)M) || !all_finite(ipvr, 81 * (size_t)M)) FAIL(p, PLBA_ERR_NUMERIC, "non-finite IMU edge");
    p->win.M = M;
    p->win.imu_i.assign(ki, ki + M); p->win.imu_j.assign(kj, kj + M);
    p->win.imu_pre.assign(pre, pre + 142 * (size_t)M);
    p->win.imu_ipvr.assign(ipvr, ipvr + 81 * (size_t)M);
    p->win.imu_ibias.assign(ibias, ibias + 36 * (size_t)M);
    p->dirty = true;
    return PLBA_OK;
}
int plba_set_prior(plba_problem* p, int n, int nv, const int32_t* vid, const int32_t* size, const int32_t* idx, const double* x0,
                   const double* J0, const double* r0) {
    if (!p) return PLBA_ERR_INVALID;
    // validate, then touch: a refused call leaves the prior — host-made, device-made or still pending — exactly as it was
    int tot = 0, nx = 0;
    if (nv != 0) {
        if (n <= 0 || nv < 0 || !vid || !size || !idx || !x0 || !J0 || !r0) return PLBA_ERR_INVALID;
        for (int i = 0; i < nv; ++i) {
            if (size[i] != 9 && size[i] != 6) FAIL(p, PLBA_ERR_INVALID, "Undefined size of marginalization vertex: %d", size[i]);
            if (idx[i] < 0 || idx[i] + size[i] > n) FAIL(p, PLBA_ERR_INVALID, "prior vertex %d: idx out of range", i);
            nx += size[i] == 9 ? 10 : 6;
            tot += size[i];
        }
        if (tot != n) FAIL(p, PLBA_ERR_INVALID, "prior: sum of kept sizes %d != n %d", tot, n);
    }
    marg_discard(p);      // a pending plba_marginalize_to_prior: waited for, its result dropped
    p->dirty = true;
    p->prior_dev = false; p->prior_changed = false; p->pr_m = 0;
    if (nv == 0) { p->pr_n = 0; p->pr_nv = 0; return PLBA_OK; }
    p->pr_n = n; p->pr_nv = nv;
    p->pr_vid.assign(vid, vid + nv); p->pr_size.assign(size, size + nv); p->pr_idx.assign(idx, idx + nv);
    p->pr_x0.assign(x0, x0 + nx);
    p->pr_J0.assign(J0, J0 + (size_t)n * n);
    p->pr_r0.assign(r0, r0 + n);
    return PLBA_OK;
}
int plba_set_robust(plba_problem* p, plba_edge_kind kind, int enabled, double delta) {
    if (!p || kind < 0 || kind > 4) return PLBA_ERR_INVALID;
    p->rob.on[kind] = enabled;
    p->rob.delta[kind] = delta;
    return PLBA_OK;
}
int plba_set_marg_eps(plba_problem* p, double eps) {
    if (!p || !(eps >= 0.0) || !std::isfinite(eps)) return PLBA_ERR_INVALID;
    p->opt.marg_eps = eps;
    return PLBA_OK;
}
int plba_set_shard(plba_problem* p, int rank, int world, plba_allreduce_fn fn, void* user) {
    if (!p || world < 1 || rank < 0 || rank >= world) return PLBA_ERR_INVALID;
    if (world > 1 && !fn) FAIL(p, PLBA_ERR_INVALID, "a sharded problem needs an all-reduce callback");
    p->rank = rank; p->world = world; p->xfn = fn; p->xuser = user;
    p->dirty = true;
    return PLBA_OK;
}


int plba_dense_solve(plba_problem* p, int n, const double* A, const double* b, double* x, int* ok) {
    if (!p || n <= 0 || !A || !b || !x) return PLBA_ERR_INVALID;
    HIPCK(p, hipSetDevice(p->device));
    const int Ppad = dense_ppad(n), ld = Ppad;
    std::vector<double> h(dense_counts(Ppad, ld).sys_len, 0.0);
    for (int r = 0; r < n; ++r) memcpy(&h[(size_t)r * ld], A + (size_t)r * n, (size_t)n * 8);
    for (int r = n; r < Ppad; ++r) h[(size_t)r * ld + r] = 1.0;
    memcpy(&h[(size_t)Ppad * ld], b, (size_t)n * 8);
    DArr<double> sys;
    DArr<Ctrl> ctrl; DenseWork work;
    DArrStreamScope staged(p->stream, p->have_ctx ? p->ctx.stage : nullptr);      // `h` stays alive until the final wait below
    HIPCK(p, sys.upload(h)); HIPCK(p, ctrl.alloc(1)); HIPCK(p, work.alloc(Ppad, ld, ninv_fits(Ppad)));
    Ctrl c0; memset(&c0, 0, sizeof c0); c0.solver_ok = 1;
    HIPCK(p, plba_h2d(p, ctrl.p, &c0, sizeof c0));
    DevBuf d; memset(&d, 0, sizeof d);
    d.P = n; d.Ppad = Ppad; d.ld = ld; d.sys = sys.p; d.ctrl = ctrl.p; work.bind(d, p->opt);
    launch_cholesky(d, p->opt.use_mfma != 0, 1, p->stream);
    launch_trsv_back(d, p->opt.use_mfma != 0, 1, p->stream);
    HIPCK(p, plba_stream_wait(p, p->stream));
    HIPCK(p, hipGetLastError());
    HIPCK(p, plba_d2h(p, x, work.x.p, (size_t)n * 8));
    HIPCK(p, plba_d2h(p, &c0, ctrl.p, sizeof c0));
    if (ok) *ok = c0.solver_ok;
    return PLBA_OK;
}
int plba_debug_dense_solve(plba_problem* p, int n, const double* A, const double* b, double* x, int* ok) { return plba_dense_solve(p, n, A, b, x, ok); }

}  // extern "C"

// =================================================================================================
// structure + device image
// =================================================================================================
// A few persistent host threads for the structure build: spawning std::threads per call cost more than the work they
// did (8 threads were no faster than 4).  Workers sleep on a condition variable between jobs; run(n, f) executes f(0..n-1)
// with the caller taking index 0.
namespace {
class HostPool {
public:
    static HostPool& get() { static HostPool p; return p; }
    void run(int n, const std::function<void(int)>& f) {
        finish();      // (an asynchronous job of this thread)
        if (n <= 1) { f(0); return; }
        std::lock_guard<std::mutex> serial(run_m_);      // one job at a time (problems on different host threads)
        ensure(n - 1);
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &f; njobs_ = n; next_ = 1; pending_ = n - 1; ++gen_;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
    }
    // start(n, f): the workers take f(0..n-1) while the caller goes on; finish() (the caller helps with what is left) joins.  One
    // asynchronous job at a time; a run() from the same thread in between joins it first.
    void start(int n, std::function<void(int)> f) {
        finish();
        run_m_.lock();
        ensure(std::min(n, 12));
        async_f_ = std::move(f);
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &async_f_; njobs_ = n; next_ = 0; pending_ = n; ++gen_;
        }
        async_owner_.store(std::this_thread::get_id(), std::memory_order_relaxed);
        async_.store(true, std::memory_order_release);      // (finish() on OTHER host threads reads these two: atomics, owner first)
        cv_.notify_all();
    }
    void finish() {
        if (!async_.load(std::memory_order_acquire) || async_owner_.load(std::memory_order_relaxed) != std::this_thread::get_id()) return;
        std::unique_lock<std::mutex> lk(m_);
        while (next_ < njobs_) {
            const int i = next_++;
            lk.unlock();
            async_f_(i);
            lk.lock();
            --pending_;
        }
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
        lk.unlock();
        async_.store(false, std::memory_order_release);
        run_m_.unlock();
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
private:
    void ensure(int workers) {
        while ((int)th_.size() < workers) th_.emplace_back([this] { loop(); });
    }
    // (polling the job generation for a few hundred microseconds before sleeping, with a wake-up call at the start of prepare(), was tried at
    // the end of round 5 — the pool is used twice within half a millisecond per BA call and a futex wake costs 30 - 60 us —: no gain in
    // sequential A/B runs on one box, 3.3 - 3.4 ms per slid call either way; removed)
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return stop_ || (gen_ != seen && next_ < njobs_); });
            if (stop_) return;
            seen = gen_;
            while (next_ < njobs_) {
                const int i = next_++;
                const std::function<void(int)>* f = job_;
                lk.unlock();
                (*f)(i);
                lk.lock();
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_, run_m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    int njobs_ = 0, next_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
    std::function<void(int)> async_f_;
    std::atomic<bool> async_{false};
    std::atomic<std::thread::id> async_owner_{};
};
}  // namespace


// ---- fused landmark-major passes: group structure (plba_lm_dev.h) ---------------------------------------------------------------------
// Landmarks of one kind are ordered by (first keyframe, last keyframe, index) and cut greedily into groups whose observing keyframes
// fit a window of LMF_W (standard groups: landmarks with at most 8 observations) or LMF_W2 = 16 (wide groups: 9 .. 16 observations —
// round 4: the reference's 12-keyframe window with tracks over most of it); the observations are re-listed in that order (static data: measurement, weight, window slot, original
// index), so that a group streams its inputs.  Per group and window-slot pair (p <= q) some landmark couples, one contribution to
// the pose-pair block (kf[p], kf[q]); the gather lists hold them block by block in ascending group order (a fixed summation order).
static bool lm_structure_fits(const plba_problem* p, const std::vector<int32_t>& lm_start) {
    if (p->win.K >= 65536) return false;
    for (int s = 0; s < p->L; ++s) if (lm_start[s + 1] - lm_start[s] > LMF_W2) return false;
    return true;      // (two observations of a landmark in one keyframe are refused at upload; build_lm_groups still checks and returns false)
}
// Three phases.  (1) serial and light: order, group boundaries and windows, offsets.  (2) the gather lists, from the windows alone: every
// pair of free window keyframes of a group is listed — a pair no landmark of the group happens to couple contributes an exact zero
// block — so that neither the lists nor the structure of the reduced system wait for (3) the per-landmark / per-observation tables,
// which the host worker pool fills WHILE prepare() goes on allocating and uploading (the largest single item of a BA call's host side:
// 2.5 ms on one thread at configs[2]); lm_groups_finish() joins before they are uploaded.
static void lm_fill_groups(const plba_problem* p, const std::vector<int32_t>& lm_start, const std::vector<int32_t>& ob_kf, LmHost& H, int t) {
    // (raw pointers: H is a heap object whose vectors' data pointers the loops would reload; keyframe -> window slot through a table per
    // group — up to 256 keyframes — instead of a search per observation: the fill is what prepare() ends up waiting for)
    const int32_t* const ordall = H.ordall.data(); const int32_t* const ls = lm_start.data(); const int32_t* const okf = ob_kf.data();
    const uint8_t* const fixed = p->lm_fixed.data();
    int32_t* const o_slot = H.p_lm_slot; int32_t* const o_ob0 = H.p_lm_ob0; int32_t* const o_orig = H.p_ob_orig; uint8_t* const o_fixed = H.p_lm_fixed; uint8_t* const o_ws8 = H.p_lm_ws8;
    const int wmax = H.wmax;
    const bool use_lut = p->win.K <= 256;
    uint8_t lut[256];
    int bad = 0;
    for (int gi = H.gcut[t]; gi < H.gcut[t + 1]; ++gi) {
        const LmGroup& g = H.grp[gi];
        if (use_lut) for (int w = 0; w < g.nw; ++w) lut[g.kf[w]] = (uint8_t)w;
        int l = g.lm0, ob = H.span_ob0[gi];
        for (int n = H.span_at[gi]; n < H.span_end[gi]; ++n, ++l) {
            const int s = ordall[n];
            o_slot[l] = s; o_fixed[l] = fixed[s]; o_ob0[l] = ob;
            // the 8 lanes of the landmark's unit(s) ARE the window slots: lane w takes the observation made from keyframe kf[w] (its
            // offset in the landmark's range), or none (0xFF) — so a lane's camera block, operand rows and accumulators never move
            uint8_t* w8 = o_ws8 + (size_t)l * wmax;
            memset(w8, 0xFF, (size_t)wmax);
            int nk = 0;
            for (int e = ls[s]; e < ls[s + 1]; ++e, ++ob, ++nk) {
                int w = 0;
                if (use_lut) w = lut[okf[e]];
                else while (g.kf[w] != okf[e]) ++w;      // (<= 8 / 16 window keyframes, all of the landmark's are among them)
                bad |= (w8[w] != 0xFF);      // two observations in one keyframe: not expressible
                w8[w] = (uint8_t)nk;
                o_orig[ob] = e;      // (measurement and weight follow on the DEVICE: k_lm_tables gathers them from the landmark-major arrays)
            }
        }
    }
    if (bad) H.bad[t] = 1;
}
static bool lm_groups_finish(LmHost& H) {      // false: a keyframe observes a landmark twice (refused at upload; checked all the same)
    HostPool::get().finish();
    for (int b : H.bad) if (b) return false;
    return true;
}
static void build_lm_groups(const plba_problem* p, const std::vector<int32_t>& lm_start, const std::vector<int32_t>& ob_kf, LmHost& H) {
    const int K = p->win.K, Np = p->win.Np, Nl = p->win.Nl, Ep = p->win.Ep, L = Np + Nl, E = (int)ob_kf.size();
    H.cov.assign((size_t)K * K, 0);
    const bool gt = (p->opt.diag & PLBA_DIAG_TIMING) != 0;
    auto g0 = std::chrono::steady_clock::now();
    auto glap = [&](const char* what) { if (!gt) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[prepare]   groups: %-18s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - g0).count()); g0 = t; };
    // group size: a workgroup step takes 32 points or 16 lines.
    // Large windows: two workgroups share a CU (registers), so `slots` of them run at once and the launch takes R rounds of groups: the
    // smallest R whose groups stay within 16 steps, the groups sized to fill the R rounds (configs[4]: 8750 workgroup-steps; 8 steps gave
    // 1095 groups = 2.14 rounds, i.e. three — 9 steps give 973, two rounds, 25 % less).
    // Windows that fit ONE round: about one group per CU instead of two — the launch's other workgroups (chain segments, IMU edge blocks:
    // the trial launch's critical path at this size) then do not share their SIMDs with a group.  tools/ab_env.py, configs[2] (1125
    // workgroup-steps incl. lines at 16 per step: 876), ms per LM trial: 2 steps 0.1722, 3 (292 groups) 0.1694, 4 (220 groups + 50 IMU edge
    // blocks + 10 chain segments on 256 CUs) 0.1561, 5 0.1585, 6 0.1611; configs[1]: 1 step 0.1200, 2 (219 groups) 0.1143, 3 0.1181.
    int nwide_pt = 0, nwide_ln = 0;      // landmarks with more than LMF_W observations: wide groups (two units per landmark block)
    for (int s = 0; s < L; ++s) if (lm_start[s + 1] - lm_start[s] > LMF_W) ++(s < Np ? nwide_pt : nwide_ln);
    const bool any_wide = nwide_pt + nwide_ln > 0;
    int steps = 1;
    {
        static int cus = 0;
        if (!cus) { int dev = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256; }
        const int slots = 2 * cus;
        const long wg_steps = (Np - nwide_pt + 31) / 32 + (Nl - nwide_ln + 15) / 16 + (nwide_pt + 15) / 16 + (nwide_ln + 7) / 8;
        const long cap1 = std::max<long>(32, (long)(1.12 * cus) - (p->win.M + 1) - (p->win.M / 4 + 1));      // one group per CU, with room for the IMU edge blocks and the chain segments
        steps = (int)std::max<long>(1, (wg_steps + cap1 - 1) / cap1);
        if (steps > 16) {
            for (int R = 1; R <= 64; ++R) {
                const long cap = (long)(0.97 * R * slots);
                steps = (int)std::max<long>(1, (wg_steps + cap - 1) / cap);
                if (steps <= 16) break;
            }
        }
        steps = std::min(steps, 16);
        if (p->opt.lm_group_steps >= 1 && p->opt.lm_group_steps <= 16) steps = p->opt.lm_group_steps;      // (measurement knob)
    }
    const int gpt = 32 * steps, gln = 16 * steps;      // (a wide group's landmark blocks take two units: half as many per step)
    // wide groups exist only where some landmark has more than LMF_W observations; the gather buffer's layout (pair blocks per group,
    // window slots) is the problem's: 36 / 8 when every group is standard
    H.wmax = any_wide ? LMF_W2 : LMF_W; H.npair = H.wmax * (H.wmax + 1) / 2;
    // ---- phase 1 -----------------------------------------------------------------------------------------------------------------------
    std::vector<int32_t>& kmin = H.kmin; std::vector<int32_t>& kmax = H.kmax; std::vector<int32_t>& ord = H.ord; std::vector<int32_t>& tmp = H.tmp;
    std::vector<int32_t>& cnt = H.cnt; std::vector<int32_t>& ordall = H.ordall; std::vector<int32_t>& stamp = H.stamp;
    kmin.resize(L); kmax.resize(L); cnt.assign(K + 1, 0); stamp.assign(K, -1); ordall.clear();
    H.grp.clear(); H.span_at.clear(); H.span_end.clear(); H.span_ob0.clear();
    H.blk_c.clear(); H.row_c.clear(); H.blk_ij.clear(); H.blk_start.clear(); H.row_kf.clear(); H.row_start.clear();
    {
        const int NTK = E > 60000 ? 8 : E > 20000 ? 4 : 1;      // (independent per landmark: the worker pool takes it in ranges)
        int32_t* kmn = kmin.data(); int32_t* kmx = kmax.data();
        const int32_t* ls = lm_start.data(); const int32_t* ok = ob_kf.data();
        // up to 256 keyframes: the set of a landmark's keyframes as a bit mask too, so that the greedy cut below tests "does this landmark
        // still fit the group's window" with an OR and a popcount per landmark instead of a pass over its observations (round 4: 0.42 ms
        // of a BA call's host side at configs[2], 103 k observations; beyond 256 keyframes the stamp array does it)
        const int NWm = K <= 256 ? (K + 63) / 64 : 0;
        H.kmask.resize((size_t)NWm * L);
        uint64_t* km = H.kmask.data();
        HostPool::get().run(NTK, [=](int t) {
            const int s0 = (int)((long)L * t / NTK), s1 = (int)((long)L * (t + 1) / NTK);
            for (int s = s0; s < s1; ++s) {      // (ob_kf ascends within a landmark when the caller lists observations in keyframe order; not assumed)
                int lo = K, hi = -1;
                uint64_t m[4] = {0, 0, 0, 0};
                for (int e = ls[s]; e < ls[s + 1]; ++e) { lo = std::min(lo, ok[e]); hi = std::max(hi, ok[e]); if (NWm) m[ok[e] >> 6] |= (uint64_t)1 << (ok[e] & 63); }
                kmn[s] = lo; kmx[s] = hi;
                for (int q = 0; q < NWm; ++q) km[(size_t)s * NWm + q] = m[q];
            }
        });
    }
    glap("kmin / kmax");
    int nlm = 0, nob = 0;
    double t_sort = 0.0, t_cut = 0.0;
    for (int kind4 = 0; kind4 < 4; ++kind4) {      // points, wide points, lines, wide lines: every point observation before every line observation (meas_pt / meas_ln)
        const int kind = kind4 >> 1, wide = kind4 & 1, W = wide ? LMF_W2 : LMF_W;
        if (wide && !any_wide) continue;
        const int s0 = kind ? Np : 0, s1 = kind ? L : Np, gmax = (kind ? gln : gpt) / (wide ? 2 : 1);
        // order by (first keyframe, last keyframe, index): two stable counting sorts; landmarks without an edge are not in the graph
        {   // (raw pointers and a counted fill: the vectors are members of a heap object, whose data pointers the loops would reload)
            ord.resize((size_t)(s1 - s0));
            int32_t* o = ord.data(); const int32_t* kx = kmax.data(); const int32_t* lsp = lm_start.data();
            size_t no = 0;
            for (int s = s0; s < s1; ++s) { o[no] = s; no += (kx[s] >= 0) & ((lsp[s + 1] - lsp[s] > LMF_W) == (wide != 0)); }
            ord.resize(no);
        }
        for (int pass = 0; pass < 2; ++pass) {
            const int32_t* key = (pass ? kmin : kmax).data();
            std::fill(cnt.begin(), cnt.end(), 0);
            tmp.resize(ord.size());
            int32_t* c = cnt.data(); const int32_t* o = ord.data(); int32_t* t2 = tmp.data();
            const size_t no = ord.size();
            for (size_t x = 0; x < no; ++x) c[key[o[x]] + 1]++;
            for (int k = 0; k < K; ++k) c[k + 1] += c[k];
            for (size_t x = 0; x < no; ++x) { const int32_t s = o[x]; t2[c[key[s]]++] = s; }
            ord.swap(tmp);
        }
        const int base = (int)ordall.size();
        size_t at = 0;
        const int NWm = (int)(H.kmask.size() / (size_t)std::max(L, 1));
        if (gt) { auto t = std::chrono::steady_clock::now(); t_sort += std::chrono::duration<double, std::milli>(t - g0).count(); g0 = t; }
        while (at < ord.size()) {
            const int gi = (int)H.grp.size();
            int32_t win[LMF_W2];
            int nw = 0, gob = 0;
            size_t end = at;
            if (NWm) {
                uint64_t gm[4] = {0, 0, 0, 0};
                const int32_t* ordp = ord.data(); const uint64_t* kmp = H.kmask.data(); const int32_t* lsp = lm_start.data();
                const size_t nord = ord.size();
                while (end < nord && (int)(end - at) < gmax) {
                    const int s = ordp[end];
                    const uint64_t* m = kmp + (size_t)s * NWm;
                    int cntw = 0;
                    for (int q = 0; q < NWm; ++q) cntw += __builtin_popcountll(gm[q] | m[q]);
                    if (cntw > W) break;
                    for (int q = 0; q < NWm; ++q) gm[q] |= m[q];
                    gob += lsp[s + 1] - lsp[s];
                    ++end;
                }
                for (int q = 0; q < NWm; ++q) for (uint64_t b = gm[q]; b; b &= b - 1) win[nw++] = q * 64 + __builtin_ctzll(b);      // (ascending)
            } else {
                while (end < ord.size() && (int)(end - at) < gmax) {
                    const int s = ord[end];
                    int add = 0;
                    for (int e = lm_start[s]; e < lm_start[s + 1]; ++e) if (stamp[ob_kf[e]] != gi) ++add;      // (a duplicate keyframe inside one landmark is caught in phase 3)
                    if (nw + add > W) break;
                    for (int e = lm_start[s]; e < lm_start[s + 1]; ++e) if (stamp[ob_kf[e]] != gi) { stamp[ob_kf[e]] = gi; win[nw++] = ob_kf[e]; }
                    gob += lm_start[s + 1] - lm_start[s];
                    ++end;
                }
                std::sort(win, win + nw);
            }
            LmGroup g;
            memset(&g, 0, sizeof g);
            g.lm0 = nlm; g.nlm = (int32_t)(end - at); g.nw = nw; g.kind = kind | (wide << 1);
            for (int q = 0; q < LMF_W2; ++q) { g.kf[q] = q < nw ? win[q] : 0; g.off[q] = q < nw ? p->off_pvr[win[q]] : -1; }
            H.grp.push_back(g);
            H.span_at.push_back(base + (int32_t)at); H.span_end.push_back(base + (int32_t)end); H.span_ob0.push_back(nob);
            nlm += (int)(end - at); nob += gob;
            at = end;
        }
        ordall.insert(ordall.end(), ord.begin(), ord.end());
        if (gt) { auto t = std::chrono::steady_clock::now(); t_cut += std::chrono::duration<double, std::milli>(t - g0).count(); g0 = t; }
    }
    if (gt) fprintf(stderr, "[prepare]   groups: order (sorts)      %8.3f ms\n[prepare]   groups: cut + pair lists   %8.3f ms\n", t_sort, t_cut);
    // ---- phase 3: the tables, group by group, on the worker pool; joined by lm_groups_finish() -------------------------------------------------
    const int ngrp = (int)H.grp.size();
    H.n_lm = (size_t)nlm; H.n_ob = (size_t)nob; H.n_meas_pt = 2 * (size_t)Ep; H.n_meas_ln = 3 * (size_t)(E - Ep);
    H.staged = false;
    if (nob > 20000) {      // (small windows: their tables ride in the batched upload block, one copy for all of them)
        H.p_ob_orig = (int32_t*)stage_take(std::max<size_t>(H.n_ob, 1) * 4);
        H.p_lm_slot = (int32_t*)stage_take(std::max<size_t>(H.n_lm, 1) * 4); H.p_lm_ob0 = (int32_t*)stage_take((H.n_lm + 1) * 4);
        H.p_lm_ws8 = (uint8_t*)stage_take(std::max<size_t>(H.n_lm * H.wmax, 1)); H.p_lm_fixed = (uint8_t*)stage_take(std::max<size_t>(H.n_lm, 1));
        H.staged = H.p_ob_orig && H.p_lm_slot && H.p_lm_ob0 && H.p_lm_ws8 && H.p_lm_fixed;      // (a block taken before the area ran out stays unused until the next scope)
    }
    if (!H.staged) {
        H.lm_slot.resize(nlm); H.lm_ob0.resize(nlm + 1); H.lm_ws8.resize((size_t)nlm * H.wmax); H.lm_fixed.resize(nlm); H.ob_orig.resize(nob);
        H.p_lm_slot = H.lm_slot.data(); H.p_lm_ob0 = H.lm_ob0.data(); H.p_lm_ws8 = H.lm_ws8.data(); H.p_lm_fixed = H.lm_fixed.data(); H.p_ob_orig = H.ob_orig.data();
    }
    H.p_lm_ob0[nlm] = nob;
    // more jobs than threads from 60 k observations on: they are dealt dynamically, and the caller takes what is left when it joins (round 4:
    // with 8 jobs on 8 sleeping workers the join had become the critical path of prepare(), 0.1 ms of waiting at configs[2])
    const int NT = E > 400000 ? 32 : E > 60000 ? 16 : E > 20000 ? 4 : 1;
    H.gcut.assign(NT + 1, ngrp);
    H.gcut[0] = 0;
    for (int t = 1, g = 0; t < NT; ++t) { while (g < ngrp && H.span_ob0[g] < (int64_t)nob * t / NT) ++g; H.gcut[t] = g; }
    H.bad.assign(NT, 0);
    glap("table allocation");
    const plba_problem* pp = p; const std::vector<int32_t>* ls = &lm_start; const std::vector<int32_t>* ok = &ob_kf; LmHost* Hp = &H;
    HostPool::get().start(NT, [pp, ls, ok, Hp](int t) { lm_fill_groups(pp, *ls, *ok, *Hp, t); });
    // ---- phase 2, while the workers fill the tables (round 5: it sat inside the cut loop, 0.13 ms the pool spent idle and prepare() then
    // spent waiting for the fill): every group's window's pose pairs and right-hand-side rows, in group order = the fixed summation order
    {
        size_t npairs_tot = 0, nrows_tot = 0;
        for (const LmGroup& g : H.grp) { int nf = 0; for (int q = 0; q < g.nw; ++q) nf += g.off[q] >= 0; npairs_tot += (size_t)nf * (nf + 1) / 2; nrows_tot += nf; }
        H.blk_c.resize(npairs_tot); H.row_c.resize(nrows_tot);
        auto* bc = H.blk_c.data(); auto* rc = H.row_c.data();
        uint8_t* cov = H.cov.data();
        for (int gi = 0; gi < ngrp; ++gi) {
            const LmGroup& g = H.grp[gi];
            for (int q = 0; q < g.nw; ++q) {
                if (g.off[q] < 0) continue;
                for (int pp = 0; pp <= q; ++pp) {
                    if (g.off[pp] < 0) continue;
                    const int i = g.kf[pp], j = g.kf[q];
                    cov[(size_t)i * K + j] = 1; cov[(size_t)j * K + i] = 1;
                    *bc++ = {(int64_t)i * K + j, gi * H.npair + q * (q + 1) / 2 + pp};
                }
                *rc++ = {(int64_t)g.kf[q], gi * H.wmax + q};
            }
        }
    }
    // stable counting sorts by key (K * K resp. K buckets): equal keys stay in group order
    {
        std::vector<int32_t>& c2 = H.c2; std::vector<int32_t>& pos = H.pos;
        c2.assign((size_t)K * K + 1, 0);
        for (const auto& b : H.blk_c) c2[b.first + 1]++;
        for (size_t k = 0; k < (size_t)K * K; ++k) c2[k + 1] += c2[k];
        H.blk_src.resize(H.blk_c.size());
        for (size_t k = 0; k < (size_t)K * K; ++k) if (c2[k + 1] > c2[k]) { const int i = (int)(k / K), j = (int)(k % K); H.blk_ij.push_back((int32_t)(i | (j << 16))); H.blk_start.push_back(c2[k]); }
        H.blk_start.push_back((int32_t)H.blk_c.size());
        pos.assign(c2.begin(), c2.end() - 1);
        for (const auto& b : H.blk_c) H.blk_src[pos[b.first]++] = b.second;
        c2.assign(K + 1, 0);
        for (const auto& r : H.row_c) c2[r.first + 1]++;
        for (int k = 0; k < K; ++k) c2[k + 1] += c2[k];
        H.row_src.resize(H.row_c.size());
        for (int k = 0; k < K; ++k) if (c2[k + 1] > c2[k]) { H.row_kf.push_back(k); H.row_start.push_back(c2[k]); }
        H.row_start.push_back((int32_t)H.row_c.size());
        pos.assign(c2.begin(), c2.end() - 1);
        for (const auto& r : H.row_c) H.row_src[pos[r.first]++] = r.second;
    }
    glap("gather lists");
}

// Padded dimension of the compact dense system.  The block steps are 32 columns wide; the 64-column forms (factor_block 64, wide steps, the
// dataflow factorisation, the 64 x 64 inverses of the substitution-based back-solve for systems beyond 32 steps) need a multiple of 64.  A
// SMALL system — one that stays below 8 tiles even padded to 64, i.e. the plain multi-launch factorisation with the explicit inverse, never the
// band or multi-chain forms (those start at 8 tiles and keep their layouts) — is padded to 32 only (round 4): the reference's own 12-keyframe window has 75 dense dims, 3 tiles instead of 4, one dependent
// launch of ~9 us less in every iteration of ~90.
static int dense_pad(const plba_problem* p, int pd) {
    const bool small32 = p->opt.use_mfma && p->opt.factor_block != 64 && !p->opt.factor_flow && !p->opt.wide_steps && (pd + TILE - 1) / TILE * 2 < 8;
    return small32 ? std::max(32, (pd + 31) / 32 * 32) : ((pd + TILE - 1) / TILE) * TILE;
}
// group-order measurement / weight tables of the fused landmark passes from the landmark-major observation arrays: entry g is observation
// ob_orig[g]; point observations come first in both orders
__global__ void k_lm_tables(const int32_t* __restrict__ ob_orig, int E, int Ep, const double* __restrict__ po_uv, const double* __restrict__ lo_l, const double* __restrict__ ob_w,
                            double* __restrict__ meas_pt, double* __restrict__ meas_ln, double* __restrict__ ob_wt) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E) return;
    const int e = ob_orig[g];
    ob_wt[g] = ob_w[e];
    if (g < Ep) { meas_pt[2 * (size_t)g] = po_uv[2 * (size_t)e]; meas_pt[2 * (size_t)g + 1] = po_uv[2 * (size_t)e + 1]; }
    else for (int c = 0; c < 3; ++c) meas_ln[3 * (size_t)(g - Ep) + c] = lo_l[3 * (size_t)(e - Ep) + c];
}
// grouped landmark storage (LmView::lm_grouped): the three state images in GROUP order from a slot-ordered source; ob_slot -> positions
__global__ void k_lm_permute(const double* __restrict__ src, const int32_t* __restrict__ slot_of_pos, int L, double* __restrict__ out0, double* __restrict__ out1) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= L * 6) return;
    const double v = src[(size_t)slot_of_pos[t / 6] * 6 + t % 6];
    out0[t] = v; out1[t] = v;
}
__global__ void k_remap_slots(int32_t* __restrict__ ob_slot, const int32_t* __restrict__ pos_of_slot, int E) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) ob_slot[e] = pos_of_slot[ob_slot[e]];
}
// Hconst[off(a) + c, off(b) + e] = H[idx(a) + c, idx(b) + e] over the prior's kept vertices that are free in this window (H = J0^T J0, n x n)
__global__ void k_prior_scatter(const double* __restrict__ H, int n, int nv, const int32_t* __restrict__ off, const int32_t* __restrict__ idx, const int32_t* __restrict__ size,
                                double* __restrict__ Hconst, int ld) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n) return;
    const int r = t / n, c = t % n;
    int dr = -1, dc = -1;
    for (int a = 0; a < nv; ++a) {
        if (r >= idx[a] && r < idx[a] + size[a] && off[a] >= 0) dr = off[a] + (r - idx[a]);
        if (c >= idx[a] && c < idx[a] + size[a] && off[a] >= 0) dc = off[a] + (c - idx[a]);
    }
    if (dr >= 0 && dc >= 0) Hconst[(size_t)dr * ld + dc] = H[t];
}
// reads_prior: the caller consumes the prior (plba_optimize, plba_marginalize*, plba_debug_build): a prior that plba_marginalize_to_prior
// changed on an unchanged window rebuilds it, as plba_set_prior would.  The other callers (results, gating, culling) keep the resident window.
static void lm_chi_sync(plba_problem* p);
static int prepare(plba_problem* p, bool reads_prior = false) {
    if (reads_prior && p->prior_changed) p->dirty = true;
    if (!p->dirty) return PLBA_OK;
    if (p->mp) { if (int rc = marg_resolve(p)) return rc; }      // the prior this window reads (plba_marginalize_to_prior)
    const Window& w = p->win;      // read-only here, but for the two repairs of a half-set window: Ep below, the levels' size further down
    if (!w.have_cam || !w.K) FAIL(p, PLBA_ERR_STATE, "camera and keyframes must be set before optimize");
    if ((int)w.po_pt.size() != w.Ep) p->win.Ep = 0;
    HIPCK(p, hipSetDevice(p->device));
    DArrStreamScope zero_fill_on(p->stream, p->have_ctx ? p->ctx.stage : nullptr);      // fresh buffers are cleared, and uploads queued, on the stream their kernels run on
    // the small ones among them in two blocks, one memset and one copy per flush (plba_problem.h, DevBatch)
    struct DevBatchScope {
        DevBatch* prev;
        explicit DevBatchScope(DevBatch* b) : prev(darr_batch()) { darr_batch() = b; }
        ~DevBatchScope() { darr_batch() = prev; }
    };
    if (!p->d_batch_z.p) { HIPCK(p, p->d_batch_z.alloc(DevBatch::ZCAP, false)); HIPCK(p, p->d_batch_u.alloc(DevBatch::UCAP, false)); }
    {
        DevBatch& b = p->batch;
        b.z = p->d_batch_z.p; b.zcap = DevBatch::ZCAP; b.zused = b.zdone = 0; ++b.gen;
        b.uh = (char*)stage_take(DevBatch::UCAP);      // (no pinned staging area: the uploads go one by one)
        b.u = b.uh ? p->d_batch_u.p : nullptr; b.ucap = DevBatch::UCAP; b.uused = b.udone = 0; b.n_batched = 0;
    }
    DevBatchScope batch_small(&p->batch);
    const int K = w.K, Np = w.Np, Nl = w.Nl, Ep = w.Ep, El = w.El, M = w.M;
    const int L = Np + Nl, E = Ep + El;
    p->L = L; p->E = E;
    // the observation arrays may refer to landmarks uploaded later/earlier: re-check ranges
    // ... and a handle that is re-used for the next window keeps every array until it is set again: edges that still refer to the
    // previous window's keyframes are refused here (they were range-checked against the keyframes of THEIR upload)
    // A sharded run must not fail on ONE rank here: each rank holds its own observation shard, and a rank that returned alone
    // would leave the others blocked in the vote below.  The verdict is carried into that all-reduce and every rank fails together.
    bool local_invalid = false;
    auto invalid = [&](const char* fmt, int a, int b, int c, int d2, int e2) { if (!local_invalid) snprintf(p->err, sizeof p->err, fmt, a, b, c, d2, e2); local_invalid = true; };
    for (int e = 0; e < Ep && !local_invalid; ++e) if (w.po_pt[e] >= Np || w.po_kf[e] >= K) invalid("point observation %d refers to point %d of %d / keyframe %d of %d", e, w.po_pt[e], Np, w.po_kf[e], K);
    for (int e = 0; e < El && !local_invalid; ++e) if (w.lo_ln[e] >= Nl || w.lo_kf[e] >= K) invalid("line observation %d refers to line %d of %d / keyframe %d of %d", e, w.lo_ln[e], Nl, w.lo_kf[e], K);
    for (int m = 0; m < M && !local_invalid; ++m)
        if (w.imu_i[m] >= K || w.imu_j[m] >= K || w.vid_bias[w.imu_i[m]] < 0 || w.vid_bias[w.imu_j[m]] < 0)
            invalid("imu edge %d joins keyframes %d and %d of %d (edges of a previous window? set them again, or clear them with M = %d)", m, w.imu_i[m], w.imu_j[m], K, 0);
    if (local_invalid && p->world <= 1) return PLBA_ERR_INVALID;
    if (local_invalid) {      // take part in the window's vote (the first collective of every rank's prepare()) and return with the others
        std::vector<double> vote = {0.0, 1.0, 1.0};
        DArr<double> dvote;
        HIPCK(p, dvote.upload(vote)); HIPCK(p, darr_flush());
        if (int xrc = p->xfn(p->xuser, dvote.p, vote.size(), 0, (void*)p->stream)) { snprintf(p->err, sizeof p->err, "all-reduce callback failed (%d)", xrc); return PLBA_ERR_EXCHANGE; }
        HIPCK(p, plba_stream_wait(p, p->stream));
        return PLBA_ERR_INVALID;      // (p->err holds this rank's finding)
    }
    if ((int)w.level.size() != E) p->win.level.assign(E, 0);
    // A rebuild that keeps the observation arrays — a state, IMU or prior setter after an evaluation pass — keeps the edges' cached chi2
    // (include/plba.h: a level-0 edge uses the error cached by the last evaluation pass; the reference's edge->chi2() reads the cached
    // _error whatever happened to the vertices since).  It is read back from the image about to be rebuilt, whose buffers and views are
    // untouched so far, and uploaded into the new one below.  A window whose observation arrays were set again never takes this path.
    if (p->chi_E == E && E > 0 && !p->chi_carry) {
        lm_chi_sync(p);
        p->chi_keep.resize((size_t)E);
        HIPCK(p, plba_d2h(p, p->chi_keep.data(), p->dv.ob_chi2, (size_t)E * 8));
        p->chi_carry = true;
    }
    const bool ptime = (p->opt.diag & PLBA_DIAG_TIMING) != 0;
    auto pt0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!ptime) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[prepare] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - pt0).count()); pt0 = t; };
    // ---- pose-side index map: non-fixed vertices by ascending id ----------------
    p->off_pvr.assign(K, -1); p->off_bias.assign(K, -1);
    int off = 0;
    for (int k = 0; k < K; ++k) {
        const bool pv = !w.fix_pvr[k];
        const bool bv = w.vid_bias[k] >= 0 && !w.fix_bias[k];
        if (pv && bv && w.vid_bias[k] < w.vid_pvr[k]) { p->off_bias[k] = off; off += 6; p->off_pvr[k] = off; off += 9; }
        else {
            if (pv) { p->off_pvr[k] = off; off += 9; }
            if (bv) { p->off_bias[k] = off; off += 6; }
        }
    }
    p->P = off;
    p->Ppad = dense_ppad(off);
    p->ld = p->Ppad;
    // ---- unified landmark slots / observation arrays ----------------------------------------------------
    if (!p->ctx.lm_host) p->ctx.lm_host = new LmHost;      // (stays with the cached context)
    LmHost& LH = *p->ctx.lm_host;
    // (locals on purpose: kept with the cached context instead, these four made the loops below 4 x SLOWER — 0.085 -> 0.34 – 0.44 ms at
    // configs[2], measured A/B in one process with tools/ab_lib.py; the worker pool reads them asynchronously and they then sit in other cores' caches)
    std::vector<int32_t> ob_kf(E), ob_slot(E), lm_start(L + 1, 0);
    std::vector<double> ob_w(E);
    // (a slid window's measurements and weights are on the device already: plba_slide_window)
    const bool carry_obs = (w.carry_po || Ep == 0) && (w.carry_lo || El == 0) && (w.carry_po || w.carry_lo);
    if ((w.carry_po || w.carry_lo) && !carry_obs) FAIL(p, PLBA_ERR_STATE, "after plba_slide_window set BOTH observation arrays again (plba_set_point_obs and plba_set_line_obs) or neither: the kept measurements live on the device");
    {
        int32_t* okf = ob_kf.data(); int32_t* osl = ob_slot.data(); int32_t* ls = lm_start.data(); double* ow = ob_w.data();
        const int32_t* ppt = w.po_pt.data(); const int32_t* pkf = w.po_kf.data(); const int32_t* lln = w.lo_ln.data(); const int32_t* lkf = w.lo_kf.data();
        for (int e = 0; e < Ep; ++e) { okf[e] = pkf[e]; osl[e] = ppt[e]; ls[ppt[e] + 1]++; }
        for (int e = 0; e < El; ++e) { okf[Ep + e] = lkf[e]; osl[Ep + e] = Np + lln[e]; ls[Np + lln[e] + 1]++; }
        if (!carry_obs) { if (Ep) memcpy(ow, w.po_w.data(), (size_t)Ep * 8); if (El) memcpy(ow + Ep, w.lo_w.data(), (size_t)El * 8); }
        for (int s = 0; s < L; ++s) ls[s + 1] += ls[s];
    }
    // ---- fused landmark-major passes: does the structure fit?  (decided for good once the chain maps exist, below) -----------------
    // lm_fused = 1: from 40 k observations on.  Measured after the third form of the Schur pass (decoupled waves, lane = window slot; ms
    // per LM trial, record-based | fused): configs[0] 9 k observations 0.074 | 0.069, configs[1] 52 k 0.130 | 0.124, configs[2] 103 k
    // 0.179 | 0.169, configs[4] 1.05 M 0.695 | 0.453.  Below the threshold the record-based passes stay: windows of that size are the
    // reference's real ones (12 keyframes, tracks longer than a group's window of 8, which do not fit anyway).  2: whenever the structure fits
    const int lm_min_obs = p->opt.lm_fused_min_obs;
    // A sharded run decides from GLOBAL quantities: the window's observation count against the threshold and whether
    // EVERY rank's landmarks fit the groups — one all-reduce (sum) of [E, "does not fit here"] — so that the ranks of one window cannot
    // take different landmark paths (the collective sequence would still match; nothing tested such a mixed run).
    bool lm_fits = p->opt.lm_fused != 0 && !p->lm_disable && E > 0 && p->opt.chain_elim && p->opt.use_mfma && p->opt.factor_block != 64 && lm_structure_fits(p, lm_start);
    long E_window = E;
    if (p->world > 1) {
        std::vector<double> vote = {(double)E, lm_fits ? 0.0 : 1.0, 0.0};      // [2]: ranks whose shard failed its range checks (above)
        DArr<double> dvote;
        HIPCK(p, dvote.upload(vote)); HIPCK(p, darr_flush());
        if (int xrc = p->xfn(p->xuser, dvote.p, vote.size(), 0, (void*)p->stream)) FAIL(p, PLBA_ERR_EXCHANGE, "all-reduce callback failed (%d)", xrc);
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, vote.data(), dvote.p, vote.size() * 8));
        E_window = (long)vote[0];
        lm_fits = vote[1] == 0.0;
        if (vote[2] != 0.0) {      // some rank's shard does not belong to this window: all ranks return, none enters the next collective alone
            snprintf(p->err, sizeof p->err, "%d rank(s) of the sharded window hold edges that refer to keyframes / landmarks the window does not have", (int)vote[2]);
            return PLBA_ERR_INVALID;
        }
    }
    const bool lm_cand = lm_fits && (p->opt.lm_fused >= 2 || E_window >= lm_min_obs);
    // keyframe-major record positions (stable: landmark order inside a keyframe), in EREC_UNIT = 64-byte units: a point
    // record takes one unit, a line record two, packed back to back (plba_math.h)
    p->ob_pos.assign(lm_cand ? 0 : E, 0);
    if (!lm_cand) {      // (the fused passes write no records)
        std::vector<int32_t> cntk(K + 1, 0);
        for (int e = 0; e < E; ++e) cntk[ob_kf[e] + 1] += (e < Ep) ? 1 : 2;
        for (int k = 0; k < K; ++k) cntk[k + 1] += cntk[k];
        for (int e = 0; e < E; ++e) { p->ob_pos[e] = cntk[ob_kf[e]]; cntk[ob_kf[e]] += (e < Ep) ? 1 : 2; }
    }
    // (a slid window's landmark estimates stay on the device: plba_slide_window left them in d_lm_carry, and the host copy is not formed)
    const bool carry_all = (w.carry_pts || Np == 0) && (w.carry_lns || Nl == 0) && (w.carry_pts || w.carry_lns) && p->d_lm_carry.p && p->d_lm_carry.n >= (size_t)L * 6;
    if ((w.carry_pts || w.carry_lns) && !carry_all) FAIL(p, PLBA_ERR_STATE, "after plba_slide_window set BOTH landmark arrays again (plba_set_points and plba_set_lines) or neither: the kept estimates live on the device");
    p->lm_fixed.assign(L, 0);
    if (!carry_all) {
        p->lm0.assign((size_t)L * 6, 0.0);
        for (int i = 0; i < Np; ++i) memcpy(&p->lm0[(size_t)i * 6], &w.pts[(size_t)i * 3], 24);
        for (int i = 0; i < Nl; ++i) memcpy(&p->lm0[(size_t)(Np + i) * 6], &w.lns[(size_t)i * 6], 48);
    }
    for (int i = 0; i < Np; ++i) p->lm_fixed[i] = w.pt_fixed[i];
    for (int i = 0; i < Nl; ++i) p->lm_fixed[Np + i] = w.ln_fixed[i];
    lap("index maps, slots");
    struct PoolJoin { ~PoolJoin() { HostPool::get().finish(); } } join_tables;      // (declared after the vectors the asynchronous fill reads: joined before they go)
    if (lm_cand) build_lm_groups(p, lm_start, ob_kf, LH);
    else LH.grp.clear();
    lap("landmark groups");
    // ---- keyframe-pair lists for the Schur complement --------------------------------------------------
    // Counting sort of the (landmark, observation a, observation b >= a) triples by keyframe pair, on a few host threads:
    // thread t owns a contiguous range of landmarks with about 1/T of the triples; per-thread pair counts give every thread
    // its own slice of every pair's entry range, in thread (= landmark) order, so the result is the serial one bit for bit.
    std::vector<int32_t> pair_i, pair_j, pair_start;
    int64_t nent = 0;
    std::vector<int32_t> ent_ei_v, ent_ej_v, ent_slot_v;
    int32_t *ent_ei = nullptr, *ent_ej = nullptr, *ent_slot = nullptr;
    bool ent_staged = false;
    if (lm_cand) {
        // the fused passes need no pair-entry lists (3 x 4 bytes x 317 k entries at configs[2], the largest item of this function):
        // only which keyframe pairs are coupled, for the structure of the reduced system
        for (int i = 0; i < K; ++i) for (int j = i; j < K; ++j) if (LH.cov[(size_t)i * K + j]) { pair_i.push_back(i); pair_j.push_back(j); pair_start.push_back(0); }
        pair_start.push_back(0);
    } else {
    const int NT = (E > 60000) ? 8 : (E > 20000) ? 4 : 1;
    std::vector<int> lm_cut(NT + 1, L);
    {
        std::vector<int64_t> tri(L + 1, 0);
        for (int s = 0; s < L; ++s) { const int64_t k = lm_start[s + 1] - lm_start[s]; tri[s + 1] = tri[s] + k * (k + 1) / 2; }
        lm_cut[0] = 0;
        for (int t = 1; t < NT; ++t) lm_cut[t] = (int)(std::lower_bound(tri.begin(), tri.end(), tri[L] * t / NT) - tri.begin());
        for (int t = 1; t <= NT; ++t) lm_cut[t] = std::max(lm_cut[t], lm_cut[t - 1]);
        lm_cut[NT] = L;
    }
    std::vector<int32_t> kfree(E);        // keyframe of an observation, -1 if that keyframe's pose is fixed
    for (int e = 0; e < E; ++e) kfree[e] = p->off_pvr[ob_kf[e]] >= 0 ? ob_kf[e] : -1;
    std::vector<std::vector<int32_t>> tcnt(NT, std::vector<int32_t>((size_t)K * K, 0));
    auto count_range = [&](int t) {
        int32_t* c = tcnt[t].data();
        for (int s = lm_cut[t]; s < lm_cut[t + 1]; ++s)
            for (int a = lm_start[s]; a < lm_start[s + 1]; ++a) {
                const int ka = kfree[a];
                if (ka < 0) continue;
                for (int b = a; b < lm_start[s + 1]; ++b) {
                    const int kb = kfree[b];
                    if (kb < 0) continue;
                    c[ka <= kb ? (size_t)ka * K + kb : (size_t)kb * K + ka]++;
                }
            }
    };
    HostPool::get().run(NT, count_range);
    std::vector<std::vector<int64_t>> tpos(NT, std::vector<int64_t>((size_t)K * K, -1));
    for (int i = 0; i < K; ++i)
        for (int j = i; j < K; ++j) {
            int64_t c = 0;
            for (int t = 0; t < NT; ++t) c += tcnt[t][(size_t)i * K + j];
            if (c == 0) continue;
            pair_i.push_back(i); pair_j.push_back(j); pair_start.push_back((int32_t)nent);
            int64_t o = nent;
            for (int t = 0; t < NT; ++t) { tpos[t][(size_t)i * K + j] = o; o += tcnt[t][(size_t)i * K + j]; }
            nent += c;
        }
    if (nent > 0x7fffffff) FAIL(p, PLBA_ERR_INVALID, "too many Schur pair entries");
    pair_start.push_back((int32_t)nent);
    // the three entry arrays are built straight in the pinned staging area when it has room (3 x 4 bytes x 317 k entries at
    // configs[2]: no pageable copy, no second pass over them)
    ent_ei = (int32_t*)stage_take((size_t)nent * 4); ent_ej = ent_ei ? (int32_t*)stage_take((size_t)nent * 4) : nullptr;
    ent_slot = ent_ej ? (int32_t*)stage_take((size_t)nent * 4) : nullptr;
    ent_staged = ent_slot != nullptr;
    if (!ent_staged) { ent_ei_v.resize((size_t)nent); ent_ej_v.resize((size_t)nent); ent_slot_v.resize((size_t)nent); ent_ei = ent_ei_v.data(); ent_ej = ent_ej_v.data(); ent_slot = ent_slot_v.data(); }
    auto fill_range = [&](int t) {
        int64_t* pos = tpos[t].data();
        for (int s = lm_cut[t]; s < lm_cut[t + 1]; ++s)
            for (int a = lm_start[s]; a < lm_start[s + 1]; ++a) {
                const int ka = kfree[a];
                if (ka < 0) continue;
                for (int b = a; b < lm_start[s + 1]; ++b) {
                    const int kb = kfree[b];
                    if (kb < 0) continue;
                    const bool sw = ka > kb;
                    int64_t& w = pos[sw ? (size_t)kb * K + ka : (size_t)ka * K + kb];
                    ent_ei[(size_t)w] = p->ob_pos[sw ? b : a]; ent_ej[(size_t)w] = p->ob_pos[sw ? a : b]; ent_slot[(size_t)w] = s;
                    ++w;
                }
            }
    };
    HostPool::get().run(NT, fill_range);
    }
    // Co-observation structure of the keyframes: which pose x pose blocks of the reduced system the landmarks' Schur terms can
    // touch.  A sharded run needs the UNION over the ranks (each holds the pairs of its own landmarks only): one all-reduce
    // (max) of a K x K map per upload, after which every rank derives the same assembly / exchange lists and band.
    std::vector<uint8_t> cov((size_t)K * K, 0);
    for (size_t q = 0; q < pair_i.size(); ++q) { cov[(size_t)pair_i[q] * K + pair_j[q]] = 1; cov[(size_t)pair_j[q] * K + pair_i[q]] = 1; }
    if (p->world > 1) {
        // The asynchronous table fill build_lm_groups started holds the worker pool (HostPool::start keeps its job lock until finish()).
        // A rank must not wait in a collective while it holds it: another rank of the SAME process (one thread per problem, plba.h) blocks
        // in HostPool::start / run on its way to this very collective, and neither moves again.  Join the fill first.
        HostPool::get().finish();
        std::vector<double> cd((size_t)K * K);
        for (size_t t = 0; t < cd.size(); ++t) cd[t] = cov[t];
        DArr<double> dcov;
        HIPCK(p, dcov.upload(cd)); HIPCK(p, darr_flush());
        if (int xrc = p->xfn(p->xuser, dcov.p, cd.size(), 1, (void*)p->stream)) FAIL(p, PLBA_ERR_EXCHANGE, "all-reduce callback failed (%d)", xrc);
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, cd.data(), dcov.p, cd.size() * 8));
        for (size_t t = 0; t < cd.size(); ++t) cov[t] = cd[t] != 0.0;
    }
    lap("pair lists (host)");
    // ---- prior bookkeeping ----------------------------------------------------------------------------------------
    std::vector<int32_t> pr_kf(p->pr_nv), pr_isb(p->pr_nv), pr_x0off(p->pr_nv), pr_off(p->pr_nv);
    size_t pr_nx = 0;
    {
        std::map<int, std::pair<int, int>> by_vid;
        for (int k = 0; k < K; ++k) { by_vid[w.vid_pvr[k]] = {k, 0}; if (w.vid_bias[k] >= 0) by_vid[w.vid_bias[k]] = {k, 1}; }
        int xo = 0;
        for (int i = 0; i < p->pr_nv; ++i) {
            auto it = by_vid.find(p->pr_vid[i]);
            if (it == by_vid.end()) FAIL(p, PLBA_ERR_INVALID, "prior vertex id %d not in the window", p->pr_vid[i]);
            pr_kf[i] = it->second.first; pr_isb[i] = it->second.second;
            if ((pr_isb[i] ? 6 : 9) != p->pr_size[i]) FAIL(p, PLBA_ERR_INVALID, "prior vertex %d: size %d does not match its vertex type", i, p->pr_size[i]);
            pr_x0off[i] = xo; xo += p->pr_size[i] == 9 ? 10 : 6;
            pr_off[i] = pr_isb[i] ? p->off_bias[pr_kf[i]] : p->off_pvr[pr_kf[i]];
        }
        pr_nx = (size_t)xo;
    }
    // a prior made by plba_marginalize_to_prior: its numbers [x0 | J0 | r0 | ...] are read where the install left them
    const double* pr_dev = p->prior_dev && p->pr_nv > 0 ? p->d_prd[p->prd_slot].p : nullptr;
    // ---- upload ----------------------------------------------------------------------------------------------------
    const size_t sysn = (size_t)(p->Ppad + TILE) * p->ld;
    if (w.carry_kf) {      // a slid window: the kept keyframes' states never left the device (plba_slide_window)
        if (p->d_kf_carry.n < (size_t)K * KF_STRIDE) FAIL(p, PLBA_ERR_STATE, "carried keyframe states do not fit the window (internal error)");
        for (DArr<double>* dst : {&p->d_kf[0], &p->d_kf[1], &p->d_kf_saved}) { HIPCK(p, dst->alloc((size_t)K * KF_STRIDE, false)); HIPCK(p, hipMemcpyAsync(dst->p, p->d_kf_carry.p, (size_t)K * KF_STRIDE * 8, hipMemcpyDeviceToDevice, p->stream)); }
    } else { HIPCK(p, p->d_kf[0].upload(w.kf0)); HIPCK(p, p->d_kf[1].upload(w.kf0)); HIPCK(p, p->d_kf_saved.upload(w.kf0)); }
    // the landmarks' three images (current, trial, saved): one pass through the staging area, two copies on the device (1.2 MB each at configs[2])
    p->lm_grouped = false;      // (slot order until the fused passes' groups are final, below)
    if (carry_all) {
        const size_t nlm = std::max<size_t>((size_t)L * 6, 1);
        HIPCK(p, p->d_lm[0].alloc(nlm, false)); HIPCK(p, p->d_lm[1].alloc(nlm, false)); HIPCK(p, p->d_lm_saved.alloc(nlm, false));
        for (double* dst : {p->d_lm[0].p, p->d_lm[1].p, p->d_lm_saved.p}) if (L) HIPCK(p, hipMemcpyAsync(dst, p->d_lm_carry.p, (size_t)L * 48, hipMemcpyDeviceToDevice, p->stream));
    } else {
    HIPCK(p, p->d_lm[0].upload(p->lm0));
    if (p->lm0.size() * 8 <= DevBatch::SMALL) { HIPCK(p, p->d_lm[1].upload(p->lm0)); HIPCK(p, p->d_lm_saved.upload(p->lm0)); }
    else {
        HIPCK(p, p->d_lm[1].alloc(p->lm0.size(), false)); HIPCK(p, p->d_lm_saved.alloc(p->lm0.size(), false));
        HIPCK(p, hipMemcpyAsync(p->d_lm[1].p, p->d_lm[0].p, p->lm0.size() * 8, hipMemcpyDeviceToDevice, p->stream));
        HIPCK(p, hipMemcpyAsync(p->d_lm_saved.p, p->d_lm[0].p, p->lm0.size() * 8, hipMemcpyDeviceToDevice, p->stream));
    }
    }
    if (carry_obs) {
        if (p->carry_obs_pending) { p->d_po_uv.swap(p->d_po_uv_c); p->d_lo_l.swap(p->d_lo_l_c); p->d_ob_w.swap(p->d_ob_w_c); p->carry_obs_pending = false;
            p->d_po_uv_c.drop_batched(); p->d_lo_l_c.drop_batched(); p->d_ob_w_c.drop_batched(); }      // (the old buffers become the next slide's destination — unless they lived in the batch blocks, which start over now)
        if (p->d_po_uv.n < 2 * (size_t)Ep || p->d_lo_l.n < 3 * (size_t)El || p->d_ob_w.n < (size_t)E) FAIL(p, PLBA_ERR_STATE, "carried observation arrays do not fit the window (internal error)");
    } else { HIPCK(p, p->d_po_uv.upload(w.po_uv)); HIPCK(p, p->d_lo_l.upload(w.lo_l)); HIPCK(p, p->d_ob_w.upload(ob_w)); }
    HIPCK(p, p->d_ob_kf.upload(ob_kf)); HIPCK(p, p->d_ob_slot.upload(ob_slot)); HIPCK(p, p->d_lm_start.upload(lm_start));
    HIPCK(p, p->d_level.upload(w.level)); HIPCK(p, p->d_lm_fixed.upload(p->lm_fixed));
    const size_t nrec = lm_cand ? 0 : ((size_t)Ep + 2 * (size_t)El) * EREC_UNIT;      // the fused passes write no record table (2 x 70 MB at configs[4])
    if (p->chi_carry && (int)p->chi_keep.size() == E) HIPCK(p, p->d_ob_chi2.upload(p->chi_keep)); else HIPCK(p, p->d_ob_chi2.alloc(E));
    HIPCK(p, p->d_erec.alloc(nrec + EREC)); HIPCK(p, p->d_erec2.alloc(nrec + EREC)); HIPCK(p, p->d_depth.alloc(E));
    HIPCK(p, p->d_lm_active.alloc(L));
    HIPCK(p, p->d_hll.alloc((size_t)L * 12)); HIPCK(p, p->d_bl.alloc((size_t)L * 6)); HIPCK(p, p->d_dinv.alloc((size_t)L * 12));
    HIPCK(p, p->d_tv.alloc((size_t)L * 6)); HIPCK(p, p->d_xl.alloc((size_t)L * 6));
    HIPCK(p, p->d_off_pvr.upload(p->off_pvr)); HIPCK(p, p->d_off_bias.upload(p->off_bias));
    // chunks of at most 256 entries per pair (contiguous, in pair order)
    std::vector<ChunkMeta> ch_pm;          // pair-major order (slot = index): the layout of the partial sums
    for (size_t q = 0; q < pair_i.size(); ++q) {
        const int32_t ch0 = (int32_t)ch_pm.size();
        const int32_t nchq = (pair_start[q + 1] - pair_start[q] + SCHUR_CHUNK - 1) / SCHUR_CHUNK;
        for (int32_t s0 = pair_start[q]; s0 < pair_start[q + 1]; s0 += SCHUR_CHUNK) {
            ChunkMeta m;
            m.slot = (int32_t)ch_pm.size(); m.start = s0; m.end = std::min(s0 + SCHUR_CHUNK, pair_start[q + 1]);
            m.ij = pair_i[q] | (pair_j[q] << 16); m.nch = nchq; m.ch0 = ch0;
            m.oi = p->off_pvr[pair_i[q]]; m.oj = p->off_pvr[pair_j[q]];
            ch_pm.push_back(m);
        }
    }
    // Launch order: XCD-aware.  Workgroups are dealt round-robin over the XCDs (each with its own 4 MiB L2), and a chunk
    // gathers the records of its two keyframes: the pairs (sorted by first keyframe) are cut into SCHUR_XCD runs of
    // equal chunk count, and run x supplies the chunks at launch positions = x (mod SCHUR_XCD), so the records of a
    // keyframe range are fetched into ONE L2 and re-used by all the pairs that touch them (speed only).
    std::vector<ChunkMeta> ch_meta;
    {
        const size_t n = ch_pm.size();
        std::vector<size_t> lo(SCHUR_XCD + 1, n);
        lo[0] = 0;
        for (int x = 1; x < SCHUR_XCD; ++x) {
            size_t cut = std::min(n, (n * x + SCHUR_XCD - 1) / SCHUR_XCD);
            while (cut < n && cut > 0 && ch_pm[cut].ch0 != ch_pm[cut].slot) ++cut;      // cut between pairs
            lo[x] = std::max(cut, lo[x - 1]);
        }
        ch_meta.reserve(n);
        for (size_t q = 0; ch_meta.size() < n; ++q)
            for (int x = 0; x < SCHUR_XCD; ++x)
                if (lo[x] + q < lo[x + 1]) ch_meta.push_back(ch_pm[lo[x] + q]);
    }
    HIPCK(p, p->d_ch_meta.upload(ch_meta));
    HIPCK(p, p->d_schur_part.alloc(ch_meta.size() * 48)); HIPCK(p, p->d_pair_cnt.alloc(ch_meta.size()));
    HIPCK(p, p->d_pair_i.upload(pair_i)); HIPCK(p, p->d_pair_j.upload(pair_j)); HIPCK(p, p->d_pair_start.upload(pair_start));
    if (ent_staged) { HIPCK(p, p->d_ent_pi.upload_staged(ent_ei, (size_t)nent)); HIPCK(p, p->d_ent_pj.upload_staged(ent_ej, (size_t)nent)); HIPCK(p, p->d_ent_slot.upload_staged(ent_slot, (size_t)nent)); }
    else { HIPCK(p, p->d_ent_pi.upload(ent_ei_v)); HIPCK(p, p->d_ent_pj.upload(ent_ej_v)); HIPCK(p, p->d_ent_slot.upload(ent_slot_v)); } HIPCK(p, p->d_ob_pos.upload(p->ob_pos));
    HIPCK(p, p->d_imu_i.upload(w.imu_i)); HIPCK(p, p->d_imu_j.upload(w.imu_j)); HIPCK(p, p->d_imu_pre.upload(w.imu_pre));
    HIPCK(p, p->d_imu_ipvr.upload(w.imu_ipvr)); HIPCK(p, p->d_imu_ibias.upload(w.imu_ibias));
    HIPCK(p, p->d_imu_err.alloc((size_t)M * 16)); HIPCK(p, p->d_imu_chi.alloc((size_t)M * 4));
    HIPCK(p, p->d_pr_kf.upload(pr_kf)); HIPCK(p, p->d_pr_isbias.upload(pr_isb)); HIPCK(p, p->d_pr_size.upload(p->pr_size));
    HIPCK(p, p->d_pr_idx.upload(p->pr_idx)); HIPCK(p, p->d_pr_x0off.upload(pr_x0off)); HIPCK(p, p->d_pr_off.upload(pr_off));
    if (!pr_dev) { HIPCK(p, p->d_pr_x0.upload(p->pr_x0)); HIPCK(p, p->d_pr_J0.upload(p->pr_J0)); HIPCK(p, p->d_pr_r0.upload(p->pr_r0)); }
    HIPCK(p, p->d_pr_err.alloc(p->pr_n)); HIPCK(p, p->d_pr_dx.alloc(p->pr_n)); HIPCK(p, p->d_pr_chi.alloc(1));
    HIPCK(p, p->d_Hconst.alloc((size_t)p->Ppad * p->ld)); HIPCK(p, p->d_Himu.alloc((size_t)p->Ppad * p->ld)); HIPCK(p, p->d_Himu2.alloc((size_t)p->Ppad * p->ld)); HIPCK(p, p->d_bimu2.alloc(p->ld));
    HIPCK(p, p->d_bprior.alloc(p->ld)); HIPCK(p, p->d_bprior2.alloc(p->ld));
    HIPCK(p, p->d_bimu.alloc(p->ld)); HIPCK(p, p->d_sys.alloc(sysn)); HIPCK(p, p->d_bpg.alloc(p->ld)); HIPCK(p, p->work.alloc(p->Ppad, p->ld, false)); p->flow_epoch = 0;      // (the explicit inverse: below, once the solver's path is known)
    const size_t ngrp = LH.grp.size();      // the fused passes leave one partial per landmark group in the same arrays
    HIPCK(p, p->d_chi_part.alloc(std::max((size_t)(E + 255) / 256, ngrp) + 1)); HIPCK(p, p->d_scale_part.alloc(std::max((size_t)(L + 31) / 32 + 32, ngrp) + 1));      // one partial per landmark workgroup (32 landmarks, plba_kernels.hip LML)
    HIPCK(p, p->d_maxd_part.alloc(std::max((size_t)(L + 31) / 32 + 32, ngrp) + 1)); HIPCK(p, p->d_kfdiag.alloc((size_t)K * 6)); HIPCK(p, p->d_posediag.alloc(p->ld));
    HIPCK(p, p->d_red.alloc(8)); HIPCK(p, p->d_ctrl.alloc(1)); HIPCK(p, p->d_trace.alloc(TRACE_CAP)); HIPCK(p, p->d_trace_n.alloc(1));
    lap("alloc + upload");
    if (ptime) fprintf(stderr, "[prepare] pool: %zu hipMalloc, %zu reused so far, %.1f MB cached\n", dev_pool().n_malloc, dev_pool().n_reuse, dev_pool().cached / 1048576.0);
    // ---- kernel argument block -------------------------------------------------------------------------------------
    DevBuf& d = p->dv;
    memset(&d, 0, sizeof d);
    d.K = K; d.Np = Np; d.Nl = Nl; d.L = L; d.Ep = Ep; d.El = El; d.E = E; d.M = M;
    d.P = p->P; d.Ppad = p->Ppad; d.ld = p->ld; d.npairs = (int)pair_i.size(); d.nent = (int)nent; d.nchunks = (int)ch_meta.size();
    d.cam.fx = w.fx; d.cam.fy = w.fy; d.cam.cx = w.cx; d.cam.cy = w.cy;
    cam_set_extrinsics(d.cam, w.Rbc, w.Pbc);
    d.gw = v3(w.gw[0], w.gw[1], w.gw[2]);
    d.fix_q1 = p->opt.fix_line_position_jacobian;
    d.kf[0] = p->d_kf[0].p; d.kf[1] = p->d_kf[1].p; d.lm[0] = p->d_lm[0].p; d.lm[1] = p->d_lm[1].p;
    d.po_uv = p->d_po_uv.p; d.lo_l = p->d_lo_l.p; d.ob_w = p->d_ob_w.p; d.ob_kf = p->d_ob_kf.p; d.ob_slot = p->d_ob_slot.p;
    d.ob_level = p->d_level.p; d.ob_chi2 = p->d_ob_chi2.p; d.erec = p->d_erec.p; d.erec_alt = p->d_erec2.p;
    d.lm_start = p->d_lm_start.p; d.lm_fixed = p->d_lm_fixed.p;
    d.hll = p->d_hll.p; d.bl = p->d_bl.p; d.dinv = p->d_dinv.p; d.tv = p->d_tv.p; d.xl = p->d_xl.p; d.lm_active = p->d_lm_active.p;
    d.kf_off_pvr = p->d_off_pvr.p; d.kf_off_bias = p->d_off_bias.p;
    d.pair_i = p->d_pair_i.p; d.pair_j = p->d_pair_j.p; d.pair_start = p->d_pair_start.p; d.ent_pi = p->d_ent_pi.p; d.ent_pj = p->d_ent_pj.p; d.ent_slot = p->d_ent_slot.p; d.ob_pos = p->d_ob_pos.p;
    d.ch_meta = p->d_ch_meta.p;
    d.schur_part = p->d_schur_part.p; d.pair_cnt = p->d_pair_cnt.p;
    HIPCK(p, p->d_trial_cnt.alloc(2)); d.trial_cnt = p->d_trial_cnt.p; d.back_cnt = reinterpret_cast<unsigned*>(p->d_trial_cnt.p + 1); p->back_epoch = 0;
    d.imu_i = p->d_imu_i.p; d.imu_j = p->d_imu_j.p; d.imu_pre = p->d_imu_pre.p; d.imu_info_pvr = p->d_imu_ipvr.p; d.imu_info_bias = p->d_imu_ibias.p;
    d.imu_err = p->d_imu_err.p; d.imu_chi = p->d_imu_chi.p;
    d.pr_n = p->pr_n; d.pr_nv = p->pr_nv;
    d.pr_kf = p->d_pr_kf.p; d.pr_isbias = p->d_pr_isbias.p; d.pr_size = p->d_pr_size.p; d.pr_idx = p->d_pr_idx.p;
    d.pr_x0off = p->d_pr_x0off.p; d.pr_off = p->d_pr_off.p; d.pr_x0 = p->d_pr_x0.p; d.pr_J0 = p->d_pr_J0.p; d.pr_r0 = p->d_pr_r0.p;
    if (pr_dev) { d.pr_x0 = pr_dev; d.pr_J0 = pr_dev + pr_nx; d.pr_r0 = pr_dev + pr_nx + (size_t)p->pr_n * p->pr_n; }
    d.pr_err = p->d_pr_err.p; d.pr_dx = p->d_pr_dx.p; d.pr_chi = p->d_pr_chi.p;
    d.Hconst = p->d_Hconst.p; d.Himu = p->d_Himu.p; d.bimu = p->d_bimu.p; d.Himu_alt = p->d_Himu2.p; d.bimu_alt = p->d_bimu2.p; d.bprior = p->d_bprior.p; d.bprior_alt = p->d_bprior2.p; d.sys = p->d_sys.p; d.bpg = p->d_bpg.p; p->work.bind(d, p->opt);
    d.chi_part = p->d_chi_part.p; d.scale_part = p->d_scale_part.p; d.maxd_part = p->d_maxd_part.p; d.kfdiag = p->d_kfdiag.p; d.posediag = p->d_posediag.p;
    d.ctrl = p->d_ctrl.p; d.trace = p->d_trace.p; d.trace_cap = TRACE_CAP; d.trace_n = p->d_trace_n.p;
    // ---- structure cache: is this window's pose structure the previous one's? (plba_problem.h, StructCache) ---------------------------------
    std::vector<int32_t> skey;
    {
        skey.reserve(64 + 2 * (size_t)K + 2 * (size_t)M + 4 * (size_t)p->pr_nv + ((size_t)K * K + 3) / 4 * 2 + K);
        for (int v : {K, M, p->pr_nv, p->pr_n, (int)lm_cand, p->world, p->rank, p->opt.chain_elim, p->opt.use_mfma, p->opt.factor_block, p->opt.factor_flow, p->opt.wide_steps, p->opt.band_solve,
                      p->opt.chain_seg, p->opt.twin_max_tiles, (int)(E > 300000), (int)p->lm_disable, p->P}) skey.push_back(v);
        skey.insert(skey.end(), p->off_pvr.begin(), p->off_pvr.end()); skey.insert(skey.end(), p->off_bias.begin(), p->off_bias.end());
        skey.insert(skey.end(), w.imu_i.begin(), w.imu_i.end()); skey.insert(skey.end(), w.imu_j.begin(), w.imu_j.end());
        skey.insert(skey.end(), pr_kf.begin(), pr_kf.end()); skey.insert(skey.end(), pr_isb.begin(), pr_isb.end()); skey.insert(skey.end(), p->pr_size.begin(), p->pr_size.begin() + p->pr_nv); skey.insert(skey.end(), pr_off.begin(), pr_off.end());
        skey.insert(skey.end(), p->pr_idx.begin(), p->pr_idx.begin() + p->pr_nv);
        auto pack = [&](const std::vector<uint8_t>& v) { for (size_t i = 0; i < v.size(); i += 4) { int32_t w = 0; for (size_t j = i; j < std::min(i + 4, v.size()); ++j) w |= (int32_t)(v[j] & 0xFF) << (8 * (j - i)); skey.push_back(w); } };
        pack(cov);
        if (lm_cand) { pack(LH.cov); skey.insert(skey.end(), LH.row_kf.begin(), LH.row_kf.end()); skey.push_back(LH.wmax); }
    }
    const bool sc_hit = p->sc.valid && skey == p->sc.key;
    struct BatchSwitch {      // the structure's buffers come from a batch of their own, and its zero-filled pool buffers are noted
        DevBatch* prev; std::vector<std::pair<void*, size_t>>* prevlog;
        BatchSwitch(DevBatch* b, std::vector<std::pair<void*, size_t>>* log) : prev(darr_batch()), prevlog(darr_zero_log()) { darr_batch() = b; darr_zero_log() = log; }
        ~BatchSwitch() { darr_batch() = prev; darr_zero_log() = prevlog; }
    };
    if (sc_hit) {
        ++p->sc.hits;
        // same structure: the buffers stay; what the miss zero-filled is cleared again (epoch-stamped flags, accumulators, W outside the segments' windows)
        if (p->sbatch.zused) HIPCK(p, hipMemsetAsync(p->sbatch.z, 0, p->sbatch.zused, p->stream));
        for (const auto& zr : p->sc.zero_log) HIPCK(p, hipMemsetAsync(zr.first, 0, zr.second, p->stream));
        p->chain_ok = p->sc.chain_ok;
        d.Ninv = p->sc.Ninv; d.Nwork = p->sc.Nwork; d.dbgbuf = p->sc.dbgbuf; d.alist = p->sc.alist; d.nalist = p->sc.nalist;
        if (p->chain_ok) {      // the dense system's view: this window's arrays, the cached structure's fields
            DevBuf& dd = p->dd; const DevBuf& o = p->sc.dd;
            dd = d;
            dd.P = o.P; dd.Ppad = o.Ppad; dd.ld = o.ld; dd.sys = o.sys; dd.dbgbuf = d.dbgbuf; p->dwork.bind(dd, p->opt);      // the kept workspace (the options are part of the key)
            dd.band = o.band; dd.twin_m0 = o.twin_m0; dd.twin_fac = o.twin_fac; dd.cs_order = o.cs_order; dd.perm = o.perm; dd.xmap = o.xmap; dd.alt = o.alt; dd.alt2 = o.alt2; dd.wtw = o.wtw;
        }
        p->flow_epoch = 0;
    } else {
        ++p->sc.misses;
        p->sc.valid = false; p->sc.zero_log.clear();
        if (!p->d_sbatch_z.p) { BatchSwitch none(nullptr, nullptr); HIPCK(p, p->d_sbatch_z.alloc(DevBatch::ZCAP, false)); HIPCK(p, p->d_sbatch_u.alloc(DevBatch::UCAP, false)); }
        DevBatch& b = p->sbatch;
        b.z = p->d_sbatch_z.p; b.zcap = DevBatch::ZCAP; b.zused = b.zdone = 0; ++b.gen;
        b.uh = (char*)stage_take(DevBatch::UCAP);
        b.u = b.uh ? p->d_sbatch_u.p : nullptr; b.ucap = DevBatch::UCAP; b.uused = b.udone = 0; b.n_batched = 0;
    }
    if (!sc_hit) {
    BatchSwitch structure_scope(&p->sbatch, &p->sc.zero_log);
    // ---- chain-variable elimination (plba_chain.hip): index maps and the compact dense system ---------------------------------
    p->chain_ok = false;
    if (p->opt.chain_elim && p->opt.use_mfma && d.fb == 32 && p->P > 0) {
        // chain-block positions in keyframe order: the velocity (3) + bias (6) dims a keyframe contributes, -1 where fixed
        std::vector<std::array<int32_t, 9>> pos_c;
        std::vector<int32_t> pos_pose, pos_of_kf(K, -1);       // first system index of the position's pose block (-1: fixed)
        for (int k = 0; k < K; ++k) {
            const int op = p->off_pvr[k], ob = p->off_bias[k];
            if (op < 0 && ob < 0) continue;
            std::array<int32_t, 9> c;
            for (int q = 0; q < 3; ++q) c[q] = op >= 0 ? op + 3 + q : -1;
            for (int q = 0; q < 6; ++q) c[3 + q] = ob >= 0 ? ob + q : -1;
            pos_of_kf[k] = (int)pos_c.size();
            pos_c.push_back(c); pos_pose.push_back(op);
        }
        const int npos = (int)pos_c.size();
        bool ok = npos > 0;
        // block-tridiagonal only if every IMU edge joins neighbouring positions
        for (int m = 0; m < M && ok; ++m) {
            const int bi = pos_of_kf[w.imu_i[m]], bj = pos_of_kf[w.imu_j[m]];
            if (bi >= 0 && bj >= 0 && std::abs(bi - bj) > 1) ok = false;
        }
        // a marginalization prior couples the chain dims of its kept vertices with each other: those positions stay dense
        std::vector<char> forced(std::max(npos, 1), 0);
        for (int a = 0; a < p->pr_nv; ++a)
            if (pr_kf[a] >= 0 && pr_kf[a] < K && pos_of_kf[pr_kf[a]] >= 0) forced[pos_of_kf[pr_kf[a]]] = 1;
        // separators: the forced positions, and every position that would make a run of eliminated blocks longer than seg
        auto separators = [&](int seg) {
            std::vector<char> sep(npos, 0);
            int run = 0;
            for (int q = 0; q < npos; ++q) {
                if (forced[q] || run == seg) { sep[q] = 1; run = 0; } else ++run;
            }
            return sep;
        };
        if (ok) {
            // segment length.  Longer segments leave fewer separators dense — fewer tiles for the factorisation — but what counts is the number
            // of DEPENDENT launches of the multi-chain plan, which is not monotonic in it: the band's width in tiles depends on where the
            // segment windows fall on tile boundaries (configs[2]: 4 blocks -> 375 dims, 7 launches; 6 -> 357, 6; 7 -> 348, 7; 8 -> 339, 6).
            // So every candidate gets its dense layout, its band and the plan builder's launch count (twin_plan_launches, plba_twin_plan.h), ~10.3 us per
            // launch; a chain block costs the trial launch ~2.3 us of back-substitution in front of the IMU edge blocks where that path is
            // the launch's critical one (small windows), nothing where the landmark pass is longer.  tools/ab_env.py, one process, medians,
            // configs[2]: 4 -> 0.1720 ms per trial, 5 -> 0.1744, 6 -> 0.1672, 8 -> 0.1708: the order this cost gives.
            int best_seg = 1; double best_cost = 1e300;
            const double block_cost = E > 300000 ? 0.1 : 2.3;
            for (int seg = 1; seg <= CHAIN_SEG; ++seg) {
                const std::vector<char> sp = separators(seg);
                std::vector<int> ds(npos + 1, 0);      // first dense column of each position
                for (int q = 0; q < npos; ++q) {
                    int w = pos_pose[q] >= 0 ? 6 : 0;
                    if (sp[q]) for (int c = 0; c < 9; ++c) w += pos_c[q][c] >= 0;
                    ds[q + 1] = ds[q] + w;
                }
                const int pd = ds[npos], T = dense_pad(p, pd) / 32;
                int hb = 0;
                auto span = [&](int qa, int qb) { if (ds[qb + 1] > ds[qa]) hb = std::max(hb, (ds[qb + 1] - 1) / 32 - ds[qa] / 32); };      // positions qa <= qb couple
                for (int i = 0; i < K; ++i) for (int j2 = i; j2 < K; ++j2)
                    if (cov[(size_t)i * K + j2] && pos_of_kf[i] >= 0 && pos_of_kf[j2] >= 0) span(std::min(pos_of_kf[i], pos_of_kf[j2]), std::max(pos_of_kf[i], pos_of_kf[j2]));
                for (int q = 0, run0 = -1; q <= npos; ++q) {      // a segment's window: the positions around its run of eliminated blocks
                    const bool el = q < npos && !sp[q];
                    if (el && run0 < 0) run0 = q;
                    if (!el && run0 >= 0) { span(std::max(run0 - 1, 0), std::min(q, npos - 1)); run0 = -1; }
                }
                for (int q = 0; q + 1 < npos; ++q) span(q, q + 1);      // IMU edges between neighbours
                { int lo = npos, hi = -1; for (int q = 0; q < npos; ++q) if (forced[q]) { lo = std::min(lo, q); hi = std::max(hi, q); } if (hi >= 0) span(lo, hi); }      // the prior's kept vertices
                const bool twin = p->opt.band_solve == 1 && T <= TWIN_MAX_TILES;
                const int launches = twin ? twin_plan_launches(T, hb) : T;
                const double cost = 10.3 * launches + block_cost * seg;
                if (ptime) fprintf(stderr, "[prepare]   chain segments of %d: %d dense dims, %d tiles, band %d -> %d launches (cost %.1f)\n", seg, pd, T, hb, launches, cost);
                if (cost < best_cost) { best_cost = cost; best_seg = seg; p->seg_launch_est = launches; }
            }
            if (p->opt.chain_seg >= 1 && p->opt.chain_seg <= CHAIN_SEG) best_seg = p->opt.chain_seg;      // (measurement knob)
            const int SEG = best_seg;
            const std::vector<char> is_sep = separators(SEG);
            std::vector<int32_t> cidx, epos, seg_start, seg_col, pidx, ppos, pslot, slotcol((size_t)npos * CHAIN_NSLOT, -1);
            for (int q = 0; q < npos; ++q) {
                const bool sep = is_sep[q] != 0;
                if (pos_pose[q] >= 0) {
                    int sl = 0;
                    for (int c : {0, 1, 2, 6, 7, 8}) { slotcol[(size_t)q * CHAIN_NSLOT + sl] = (int32_t)pidx.size(); pidx.push_back(pos_pose[q] + c); ppos.push_back(q); pslot.push_back(sl++); }
                }
                if (sep) {
                    for (int c = 0; c < 9; ++c) if (pos_c[q][c] >= 0) { slotcol[(size_t)q * CHAIN_NSLOT + 6 + c] = (int32_t)pidx.size(); pidx.push_back(pos_c[q][c]); ppos.push_back(q); pslot.push_back(6 + c); }
                    if (seg_start.empty() || seg_start.back() != (int32_t)epos.size()) seg_start.push_back((int32_t)epos.size());
                } else {
                    if (seg_start.empty()) seg_start.push_back(0);
                    for (int c = 0; c < 9; ++c) cidx.push_back(pos_c[q][c]);
                    epos.push_back(q);
                }
            }
            const int nel = (int)epos.size();
            if (seg_start.empty() || seg_start.back() != nel) seg_start.push_back(nel);
            // drop empty segments (adjacent or leading separators)
            std::vector<int32_t> ss;
            for (size_t q = 0; q < seg_start.size(); ++q) if (q == 0 || seg_start[q] != seg_start[q - 1]) ss.push_back(seg_start[q]);
            seg_start = ss;
            const int nseg = (int)seg_start.size() - 1;
            const int Pd = (int)pidx.size();
            ok = nel > 0 && nseg > 0 && Pd > 0;
            for (int g = 0; g < nseg && ok; ++g) {
                const int pf = epos[seg_start[g]], pl = epos[seg_start[g + 1] - 1];
                int lo = 0, hi = 0;
                while (lo < Pd && ppos[lo] < pf - 1) ++lo;
                hi = lo;
                while (hi < Pd && ppos[hi] <= pl + 1) ++hi;
                seg_col.push_back(lo); seg_col.push_back(hi);
                if (seg_start[g + 1] - seg_start[g] > CHAIN_SEG || hi - lo + 1 > 192) ok = false;
            }
            if (ok) {
                for (int c = 0; c < 9; ++c) cidx.push_back(-1);
                ChainView& cv = p->cv;
                cv.nel = nel; cv.nseg = nseg; cv.npos = npos; cv.Pd = Pd; cv.Pdpad = dense_pad(p, Pd); cv.Wld = ((Pd + 2 + 63) / 64) * 64;
                HIPCK(p, p->d_cidx.upload(cidx)); HIPCK(p, p->d_epos.upload(epos)); HIPCK(p, p->d_seg_start.upload(seg_start)); HIPCK(p, p->d_seg_col.upload(seg_col));
                p->h_pidx = pidx; p->h_seg_col = seg_col;
                HIPCK(p, p->d_pidx.upload(pidx)); HIPCK(p, p->d_ppos.upload(ppos)); HIPCK(p, p->d_pslot.upload(pslot)); HIPCK(p, p->d_slotcol.upload(slotcol));
                {
                    std::vector<int32_t> kf_at(npos, -1), ekf, ukf;
                    for (int k = 0; k < K; ++k) if (pos_of_kf[k] >= 0) kf_at[pos_of_kf[k]] = k;
                    for (int e = 0; e < nel; ++e) ekf.push_back(kf_at[epos[e]]);
                    for (int k = 0; k < K; ++k) if (pos_of_kf[k] < 0 || is_sep[pos_of_kf[k]]) ukf.push_back(k);
                    if (ukf.empty()) ukf.push_back(-1);      // keep the array non-empty; nukf stays 0
                    cv.nukf = (ukf[0] < 0) ? 0 : (int)ukf.size();
                    HIPCK(p, p->d_kfpos.upload(pos_of_kf)); HIPCK(p, p->d_ekf.upload(ekf)); HIPCK(p, p->d_ukf.upload(ukf));
                    {   // chain_back_segment: everything a thread needs to know about the keyframe it updates, in one 80-byte record
                        std::vector<int32_t> bkf((size_t)(nseg * CHAIN_SEG + std::max(cv.nukf, 1)) * 20, -1);
                        auto fill = [&](int32_t* o, int kf, bool eliminated) {
                            o[0] = kf; o[1] = p->off_pvr[kf]; o[2] = p->off_bias[kf];
                            const int q = pos_of_kf[kf];
                            if (q >= 0) {
                                for (int i = 0; i < 6; ++i) o[3 + i] = slotcol[(size_t)q * CHAIN_NSLOT + i];
                                if (!eliminated) for (int i = 0; i < 9; ++i) o[9 + i] = slotcol[(size_t)q * CHAIN_NSLOT + 6 + i];      // a separator's chain dims sit in the dense solution
                            }
                        };
                        for (int g = 0; g < nseg; ++g) for (int t = 0; t < seg_start[g + 1] - seg_start[g]; ++t) fill(&bkf[(size_t)(g * CHAIN_SEG + t) * 20], ekf[seg_start[g] + t], true);
                        for (int u = 0; u < cv.nukf; ++u) fill(&bkf[(size_t)(nseg * CHAIN_SEG + u) * 20], ukf[u], false);
                        HIPCK(p, p->d_bkf.upload(bkf)); cv.bkf = p->d_bkf.p;
                        // per IMU edge: the segment whose back-substitution yields its keyframes' chain dims (-1: both sit in the dense solution) and
                        // the two keyframes' descriptors above (-1: no free dims) — the trial launch's IMU edge blocks form their two trial
                        // states THEMSELVES instead of waiting for the segments' workgroups (pose_edge_block, round 4)
                        std::vector<int32_t> desc_of_kf(K, -1), seg_of_kf(K, -1);
                        for (int g = 0; g < nseg; ++g) for (int t = 0; t < seg_start[g + 1] - seg_start[g]; ++t) { const int kf = ekf[seg_start[g] + t]; desc_of_kf[kf] = g * CHAIN_SEG + t; seg_of_kf[kf] = g; }
                        for (int u = 0; u < cv.nukf; ++u) if (pos_of_kf[ukf[u]] >= 0) desc_of_kf[ukf[u]] = nseg * CHAIN_SEG + u;
                        std::vector<int32_t> iloc((size_t)std::max(M, 1) * 4, -1);
                        bool iloc_ok = true;
                        for (int m = 0; m < M; ++m) {
                            const int ki = w.imu_i[m], kj = w.imu_j[m];
                            const int gi = seg_of_kf[ki], gj = seg_of_kf[kj];
                            if (gi >= 0 && gj >= 0 && gi != gj) iloc_ok = false;      // (cannot happen: a separator sits between two segments)
                            iloc[4 * (size_t)m] = gi >= 0 ? gi : gj; iloc[4 * (size_t)m + 1] = desc_of_kf[ki]; iloc[4 * (size_t)m + 2] = desc_of_kf[kj];
                        }
                        HIPCK(p, p->d_imu_loc.upload(iloc)); cv.imu_loc = iloc_ok ? p->d_imu_loc.p : nullptr;
                    }
                    std::vector<int32_t> trow(2 * (size_t)(cv.Pdpad / 32), 0);
                    for (int tb = 0; tb < cv.Pdpad / 32; ++tb) {
                        int glo = -1, ghi = -1;
                        for (int g = 0; g < nseg; ++g)
                            if (tb * 32 < seg_col[2 * g + 1] && tb * 32 + 32 > seg_col[2 * g]) { if (glo < 0) glo = g; ghi = g; }
                        if (glo >= 0) { trow[2 * tb] = seg_start[glo] * 9; trow[2 * tb + 1] = seg_start[ghi + 1] * 9; }
                    }
                    HIPCK(p, p->d_trow.upload(trow)); cv.trow = p->d_trow.p;
                    cv.kfpos = p->d_kfpos.p; cv.ekf = p->d_ekf.p; cv.ukf = p->d_ukf.p;
                }
                {   // chain_elim_segment's staging as one level of indices (it was three dependent rounds of loads: 11 us of a 19 us segment at
                    // configs[2]).  A fixed-size region per segment, laid out for CHAIN_SEG blocks and padded with -3 (skip): the loads of the
                    // indices then depend on nothing but the kernel arguments
                    constexpr int NB = 3 * CHAIN_NSLOT * 9, REG = CHAIN_SEG * (162 + NB + 9);
                    std::vector<int32_t> esrc((size_t)nseg * REG, -3);
                    const int ld = p->ld, P = p->P;
                    auto code = [&](int a, int b) -> int32_t { const int hi = std::max(a, b), lo = std::min(a, b); return (int32_t)((size_t)hi * ld + lo) | ((a == b && a < P) ? (1 << 30) : 0); };
                    for (int g = 0; g < nseg; ++g) {
                        const int i0 = seg_start[g], n = seg_start[g + 1] - i0;
                        int32_t* oC = &esrc[(size_t)g * REG]; int32_t* oB = oC + CHAIN_SEG * 162; int32_t* oR = oB + CHAIN_SEG * NB;
                        for (int bi = 0; bi < n; ++bi)
                            for (int e = 0; e < 162; ++e) {
                                const int32_t* ci = &cidx[(size_t)(i0 + bi) * 9];
                                const bool nxt = bi + 1 < n;
                                const int ga = e < 81 ? ci[e / 9] : (nxt ? ci[9 + (e - 81) / 9] : -1);
                                const int gb = e < 81 ? ci[e % 9] : ci[(e - 81) % 9];
                                oC[bi * 162 + e] = (ga >= 0 && gb >= 0) ? code(ga, gb) : ((e < 81 && e / 9 == e % 9) ? -2 : -1);
                            }
                        for (int bi = 0; bi < n; ++bi)
                            for (int e = 0; e < NB; ++e) {
                                const int dl = e / (CHAIN_NSLOT * 9), sl = (e / 9) % CHAIN_NSLOT, r = e % 9;
                                const int pos = epos[i0 + bi] + dl - 1;
                                const int col = (pos >= 0 && pos < npos) ? slotcol[(size_t)pos * CHAIN_NSLOT + sl] : -1;
                                const int gi = cidx[(size_t)(i0 + bi) * 9 + r];
                                oB[bi * NB + e] = (col >= 0 && gi >= 0) ? code(gi, pidx[col]) : -1;
                            }
                        for (int idx = 0; idx < n * 9; ++idx) oR[idx] = cidx[(size_t)i0 * 9 + idx] >= 0 ? cidx[(size_t)i0 * 9 + idx] : -1;      // (right-hand side: the system index itself)
                    }
                    if ((size_t)p->Ppad * ld >= ((size_t)1 << 30)) ok = false;      // (the diagonal flag needs bit 30)
                    HIPCK(p, p->d_esrc.upload(esrc));
                    cv.esrc = p->d_esrc.p; cv.esrc_off = nullptr;
                }
                p->d_W.release();      // must come back zero: the kernels only ever write inside each segment's window
                HIPCK(p, p->d_W.alloc((size_t)(nel * 9 + 4) * cv.Wld)); HIPCK(p, p->d_Ldinv.alloc((size_t)nel * 81)); HIPCK(p, p->d_Lsub.alloc((size_t)nel * 81));
                const size_t sysn_d = (size_t)(cv.Pdpad + TILE) * cv.Pdpad;
                HIPCK(p, p->d_sysd.alloc(sysn_d)); HIPCK(p, p->dwork.alloc(cv.Pdpad, cv.Pdpad, ninv_fits(cv.Pdpad)));
                cv.cidx = p->d_cidx.p; cv.epos = p->d_epos.p; cv.seg_start = p->d_seg_start.p; cv.seg_col = p->d_seg_col.p;
                cv.pidx = p->d_pidx.p; cv.ppos = p->d_ppos.p; cv.pslot = p->d_pslot.p; cv.slotcol = p->d_slotcol.p;
                cv.W = p->d_W.p; cv.Ldinv = p->d_Ldinv.p; cv.Lsub = p->d_Lsub.p;
                DevBuf& dd = p->dd;
                dd = d;
                dd.P = cv.Pd; dd.Ppad = cv.Pdpad; dd.ld = cv.Pdpad;
                dd.sys = p->d_sysd.p; p->dwork.bind(dd, p->opt);
                p->chain_ok = true;
            }
        }
    }
    lap("chain maps + buffers");
    d.Ninv = nullptr; d.Nwork = nullptr;
    HIPCK(p, p->d_dbgbuf.alloc(DBGBUF_N)); d.dbgbuf = p->d_dbgbuf.p; p->dd.dbgbuf = d.dbgbuf;
    if (!p->chain_ok && p->P > 0 && ninv_fits(p->Ppad)) { HIPCK(p, p->work.alloc_ninv(p->Ppad, p->ld)); p->work.bind_ninv(d); }
    // ---- structural assembly list (assemble_part): with the chain elimination on, sys is written by the assembly pass and
    // by k_schur_pairs only, so the entries neither of them can make non-zero never need touching again
    d.alist = nullptr; d.nalist = 0;
    if (p->chain_ok) {
        // a bitmap over the Ppad x ld entries, read back in ascending order (was: push + sort + unique, 1.5 ms at configs[2])
        const int ld = p->ld;
        std::vector<uint64_t> bits(((size_t)p->Ppad * ld + 63) / 64, 0);
        auto mark = [&](int idx) { bits[(size_t)idx >> 6] |= 1ull << (idx & 63); };
        auto add_full = [&](const int* dims, int n) {
            for (int a = 0; a < n; ++a) { if (dims[a] < 0) continue; for (int b = 0; b < n; ++b) if (dims[b] >= 0) mark(dims[a] * ld + dims[b]); }
        };
        for (int m = 0; m < M; ++m) {   // IMU PVR edge over [PVR_i | PVR_j | Bias_i], bias edge over [Bias_i | Bias_j]
            const int ki = w.imu_i[m], kj = w.imu_j[m];
            int e1[24], e2[12];
            for (int c = 0; c < 9; ++c) e1[c] = p->off_pvr[ki] >= 0 ? p->off_pvr[ki] + c : -1;
            for (int c = 0; c < 9; ++c) e1[9 + c] = p->off_pvr[kj] >= 0 ? p->off_pvr[kj] + c : -1;
            for (int c = 0; c < 6; ++c) { e1[18 + c] = e2[c] = p->off_bias[ki] >= 0 ? p->off_bias[ki] + c : -1; }
            for (int c = 0; c < 6; ++c) e2[6 + c] = p->off_bias[kj] >= 0 ? p->off_bias[kj] + c : -1;
            add_full(e1, 24); add_full(e2, 12);
        }
        {
            std::vector<int> pd;
            for (int a = 0; a < p->pr_nv; ++a) if (pr_off[a] >= 0) for (int c = 0; c < p->pr_size[a]; ++c) pd.push_back(pr_off[a] + c);
            add_full(pd.data(), (int)pd.size());
        }
        static const int pose6[6] = {0, 1, 2, 6, 7, 8};
        for (size_t q = 0; q < pair_i.size(); ++q) {      // the 6 x 6 blocks k_schur_pairs adds into, both mirror images
            const int oi = p->off_pvr[pair_i[q]], oj = p->off_pvr[pair_j[q]];
            for (int r : pose6) for (int c : pose6) { mark((oi + r) * ld + oj + c); mark((oj + c) * ld + oi + r); }
        }
        if (p->world > 1) {      // a sharded run's all-reduce brings in the OTHER ranks' pair blocks: the global co-observation map
            for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) {
                if (!cov[(size_t)i * K + j] || p->off_pvr[i] < 0 || p->off_pvr[j] < 0) continue;
                for (int r : pose6) for (int c : pose6) mark((p->off_pvr[i] + r) * ld + p->off_pvr[j] + c);
            }
        }
        for (int r = 0; r < p->Ppad; ++r) mark(r * ld + r);
        std::vector<int32_t> al;
        al.reserve(65536);
        for (size_t wd = 0; wd < bits.size(); ++wd) {
            uint64_t v = bits[wd];
            while (v) { al.push_back((int32_t)(wd * 64 + __builtin_ctzll(v))); v &= v - 1; }
        }
        HIPCK(p, p->d_alist.upload(al));
        d.alist = p->d_alist.p; d.nalist = (int)al.size();
        p->h_alist.swap(al);      // kept on the host: the staged upload reads it until the final wait, and the band measurement below
    }
    HIPCK(p, darr_flush());
    }      // (!sc_hit)
    lap("assembly list");
    // ---- fused landmark-major passes: final decision, gather complement of the assembly list, upload --------------------------------
    p->lm_ok = false;
    memset(&p->lv, 0, sizeof p->lv);
    if (lm_cand && !p->chain_ok) {      // the fused passes assemble through the structural list of the chain path: rebuild for the record-based passes
        HostPool::get().finish();      // the asynchronous table fill reads LH, which the nested call clears: join it first
        p->lm_disable = true;
        const int rc2 = prepare(p);
        p->lm_disable = false;
        return rc2;
    }
    std::vector<int32_t> al2;      // (function scope: a queued upload without staging room reads the host vector until the final wait)
    std::vector<uint8_t> colg;
    if (lm_cand && !lm_groups_finish(LH)) {      // (defensive: a keyframe observing a landmark twice — plba_set_*_obs refuses that) rebuild for the record-based passes
        // a sharded run cannot re-enter prepare() on ONE rank (its vote and co-observation all-reduces would have no partners: ADVICE r04).
        // The arrays only change through plba_set_*_obs, whose check_obs refuses such input, so this cannot be reached; if it ever is, fail.
        if (p->world > 1) FAIL(p, PLBA_ERR_STATE, "landmark groups: two observations of one landmark in one keyframe (refused at upload; internal error)");
        p->lm_disable = true;
        const int rc2 = prepare(p);
        p->lm_disable = false;
        return rc2;
    }
    lap("landmark tables joined");
    if (lm_cand && !sc_hit) {
        BatchSwitch structure_scope(&p->sbatch, &p->sc.zero_log);
        const int ld = p->ld;
        // the structural assembly list minus what k_lm_gather writes: the 6 x 6 pose blocks of keyframe pairs some group's window holds
        // (LH.cov) and the right-hand-side columns of the observed keyframes
        std::vector<int32_t> dim_kf(ld, -1);      // system dim -> keyframe, for the six pose dims (dp, dphi) of a free keyframe only
        colg.assign(ld, 0);
        static const int pose6b[6] = {0, 1, 2, 6, 7, 8};
        for (int k = 0; k < K; ++k) if (p->off_pvr[k] >= 0) for (int c : pose6b) dim_kf[p->off_pvr[k] + c] = k;
        for (int32_t k : LH.row_kf) for (int c : pose6b) colg[p->off_pvr[k] + c] = 1;
        al2.reserve(p->h_alist.size());
        {
            int r = 0, r0 = 0, kr = dim_kf[0];      // (the list ascends: the row is tracked, not divided out)
            const uint8_t* covr = kr >= 0 ? &LH.cov[(size_t)kr * K] : nullptr;
            for (int32_t idx : p->h_alist) {
                while (idx >= r0 + ld) { ++r; r0 += ld; kr = r < ld ? dim_kf[r] : -1; covr = kr >= 0 ? &LH.cov[(size_t)kr * K] : nullptr; }
                const int kc = dim_kf[idx - r0];
                if (!(covr && kc >= 0 && covr[kc])) al2.push_back(idx);
            }
        }
        HIPCK(p, p->d_alist2.upload(al2)); HIPCK(p, p->d_col_gather.upload(colg));
        HIPCK(p, darr_flush());
        p->sc.alist2 = p->d_alist2.p; p->sc.nalist2 = (int)al2.size(); p->sc.col_gather = p->d_col_gather.p;
    }
    if (lm_cand) {
        HIPCK(p, p->d_lm_grp.upload(LH.grp));
        if (LH.staged) {      // the tables were filled in the pinned staging area: one asynchronous copy each, no second pass over them
            HIPCK(p, p->d_lmg_slot.upload_staged(LH.p_lm_slot, LH.n_lm)); HIPCK(p, p->d_lmg_ob0.upload_staged(LH.p_lm_ob0, LH.n_lm + 1)); HIPCK(p, p->d_lmg_orig.upload_staged(LH.p_ob_orig, LH.n_ob));
            HIPCK(p, p->d_lmg_ws8.upload_staged(LH.p_lm_ws8, LH.n_lm * LH.wmax)); HIPCK(p, p->d_lmg_fixed.upload_staged(LH.p_lm_fixed, LH.n_lm));
        } else {
            HIPCK(p, p->d_lmg_slot.upload(LH.lm_slot)); HIPCK(p, p->d_lmg_ob0.upload(LH.lm_ob0)); HIPCK(p, p->d_lmg_orig.upload(LH.ob_orig));
            HIPCK(p, p->d_lmg_ws8.upload(LH.lm_ws8)); HIPCK(p, p->d_lmg_fixed.upload(LH.lm_fixed));
        }
        // measurements and weights in group order: gathered on the device from the landmark-major arrays already there (round 5: 3 MB less to
        // fill, stage and send per BA call at configs[2]; a slid window's old observations never come back to the host at all)
        HIPCK(p, p->d_lmg_meas_pt.alloc(std::max<size_t>(LH.n_meas_pt, 1), false)); HIPCK(p, p->d_lmg_meas_ln.alloc(std::max<size_t>(LH.n_meas_ln, 1), false)); HIPCK(p, p->d_lmg_wt.alloc(std::max<size_t>(LH.n_ob, 1), false));
        HIPCK(p, p->d_lmg_level.alloc(E));
        HIPCK(p, p->d_lmg_blk_ij.upload(LH.blk_ij)); HIPCK(p, p->d_lmg_blk_start.upload(LH.blk_start)); HIPCK(p, p->d_lmg_blk_src.upload(LH.blk_src));
        HIPCK(p, p->d_lmg_row_kf.upload(LH.row_kf)); HIPCK(p, p->d_lmg_row_start.upload(LH.row_start)); HIPCK(p, p->d_lmg_row_src.upload(LH.row_src));
        HIPCK(p, p->d_lmg_part.alloc(LH.grp.size() * (size_t)(LH.npair * 36 + LH.wmax * 12))); HIPCK(p, p->d_ob_err.alloc(2 * (size_t)E)); HIPCK(p, p->d_lmg_chi.alloc(E));
        LmView& lv = p->lv;
        p->lm_hist.assign(20, 0.0);      // diagnostics: groups by number of workgroup steps (points 1..8 | lines 1..8), window widths
        for (const LmGroup& g : LH.grp) { const int st = (((g.kind & 1) ? 2 * g.nlm : g.nlm) * ((g.kind & 2) ? 2 : 1) + 31) / 32; p->lm_hist[((g.kind & 1) ? 8 : 0) + std::min(std::max(st, 1), 8) - 1] += 1.0; p->lm_hist[16] += g.nw; p->lm_hist[17] += st; if (g.kind & 2) p->lm_hist[18] += 1.0; }
        lv.ngrp = (int)LH.grp.size(); lv.grp = p->d_lm_grp.p; lv.lm_slot = p->d_lmg_slot.p; lv.lm_ob0 = p->d_lmg_ob0.p; lv.ob_orig = p->d_lmg_orig.p; lv.lm_ws8 = p->d_lmg_ws8.p; lv.wmax = LH.wmax; lv.npair = LH.npair; lv.part_stride = LH.npair * 36 + LH.wmax * 12; lv.lm_fixed_g = p->d_lmg_fixed.p; lv.ob_level_g = p->d_lmg_level.p;
        lv.meas_pt = p->d_lmg_meas_pt.p; lv.meas_ln = p->d_lmg_meas_ln.p; lv.ob_wt = p->d_lmg_wt.p; lv.part = p->d_lmg_part.p; lv.ob_chi_g = p->d_lmg_chi.p; p->lm_chi_dirty = false;
        lv.nblk = (int)LH.blk_ij.size(); lv.blk_ij = p->d_lmg_blk_ij.p; lv.blk_start = p->d_lmg_blk_start.p; lv.blk_src = p->d_lmg_blk_src.p;
        lv.nrow = (int)LH.row_kf.size(); lv.row_kf = p->d_lmg_row_kf.p; lv.row_start = p->d_lmg_row_start.p; lv.row_src = p->d_lmg_row_src.p;
        lv.alist2 = p->sc.alist2; lv.nalist2 = p->sc.nalist2; lv.col_gather = p->sc.col_gather;
        lv.ob_err = nullptr; lv.dbg_out = 0;
        p->lm_ok = lv.ngrp > 0;
        HIPCK(p, darr_flush());
        if (p->lm_ok && L > 0) {
            // grouped landmark storage: position = place in the group tables (ordall), landmarks without an edge behind them
            std::vector<int32_t> pos_of_slot(L, -1), slot_of_pos(L, 0);
            int np = 0;
            for (size_t n = 0; n < LH.n_lm; ++n) { const int sl = LH.ordall[n]; pos_of_slot[sl] = np; slot_of_pos[np++] = sl; }
            for (int sl = 0; sl < L; ++sl) if (pos_of_slot[sl] < 0) { pos_of_slot[sl] = np; slot_of_pos[np++] = sl; }
            HIPCK(p, p->d_lm_pos.upload(pos_of_slot)); HIPCK(p, p->d_lm_ord.upload(slot_of_pos));
            HIPCK(p, darr_flush());
            // (d_lm_saved holds the slot-ordered image just uploaded / carried: source of the permutation, then refreshed from the result)
            hipLaunchKernelGGL(k_lm_permute, dim3((L * 6 + 255) / 256), dim3(256), 0, p->stream, p->d_lm_saved.p, p->d_lm_ord.p, L, p->d_lm[0].p, p->d_lm[1].p);
            HIPCK(p, hipGetLastError());
            HIPCK(p, hipMemcpyAsync(p->d_lm_saved.p, p->d_lm[0].p, (size_t)L * 48, hipMemcpyDeviceToDevice, p->stream));
            if (E) hipLaunchKernelGGL(k_remap_slots, dim3((E + 255) / 256), dim3(256), 0, p->stream, p->d_ob_slot.p, p->d_lm_pos.p, E);
            HIPCK(p, hipGetLastError());
            p->lm_grouped = true; lv.lm_grouped = 1;
        }
        if (p->lm_ok) {
            if (LH.n_ob != (size_t)E) FAIL(p, PLBA_ERR_STATE, "landmark groups list %zu of %d observations (internal error)", LH.n_ob, E);
            hipLaunchKernelGGL(k_lm_tables, dim3((E + 255) / 256), dim3(256), 0, p->stream, p->d_lmg_orig.p, E, Ep, p->d_po_uv.p, p->d_lo_l.p, p->d_ob_w.p, p->d_lmg_meas_pt.p, p->d_lmg_meas_ln.p, p->d_lmg_wt.p);
            HIPCK(p, hipGetLastError());
            launch_lm_level_sync(d, lv, p->stream);
        }
    }
    lap("landmark-group upload");
    // ---- structural exchange list of a sharded run (k_list_pack): every lower-triangle entry of the reduced system that can be
    // non-zero before the factorisation.  Everything else is zero on every rank and need not travel.
    d.xlist = nullptr; d.nxlist = 0;
    if (sc_hit) { d.xlist = p->sc.xlist; d.nxlist = p->sc.nxlist; }
    if (!sc_hit) {
    BatchSwitch structure_scope(&p->sbatch, &p->sc.zero_log);
    if (p->world > 1) {
        std::vector<int32_t> xl;
        const int ld = p->ld;
        auto add_block = [&](const std::vector<int>& dims) {
            for (size_t a = 0; a < dims.size(); ++a)
                for (size_t b = 0; b < dims.size(); ++b)
                    if (dims[a] >= 0 && dims[b] >= 0 && dims[a] >= dims[b]) xl.push_back(dims[a] * ld + dims[b]);
        };
        // pose x pose: the keyframe pairs some rank's landmarks couple (global co-observation map, identical on every rank)
        for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) {
            if (!cov[(size_t)i * K + j] || p->off_pvr[i] < 0 || p->off_pvr[j] < 0) continue;
            for (int r : {0, 1, 2, 6, 7, 8}) for (int c : {0, 1, 2, 6, 7, 8}) {
                const int a = p->off_pvr[i] + r, b2 = p->off_pvr[j] + c;
                if (a >= b2) xl.push_back(a * ld + b2);
            }
        }
        for (int m = 0; m < M; ++m) {   // IMU PVR edge over [PVR_i | PVR_j | Bias_i], bias edge over [Bias_i | Bias_j]
            const int ki = w.imu_i[m], kj = w.imu_j[m];
            std::vector<int> e1, e2;
            for (int c = 0; c < 9; ++c) { e1.push_back(p->off_pvr[ki] >= 0 ? p->off_pvr[ki] + c : -1); }
            for (int c = 0; c < 9; ++c) { e1.push_back(p->off_pvr[kj] >= 0 ? p->off_pvr[kj] + c : -1); }
            for (int c = 0; c < 6; ++c) { e1.push_back(p->off_bias[ki] >= 0 ? p->off_bias[ki] + c : -1); e2.push_back(p->off_bias[ki] >= 0 ? p->off_bias[ki] + c : -1); }
            for (int c = 0; c < 6; ++c) e2.push_back(p->off_bias[kj] >= 0 ? p->off_bias[kj] + c : -1);
            add_block(e1); add_block(e2);
        }
        {   // the prior couples all of its kept dims
            std::vector<int> pd;
            for (int a = 0; a < p->pr_nv; ++a) if (pr_off[a] >= 0) for (int c = 0; c < p->pr_size[a]; ++c) pd.push_back(pr_off[a] + c);
            add_block(pd);
        }
        for (int r = 0; r < p->Ppad; ++r) xl.push_back(r * ld + r);      // lambda / the padding's ones
        std::sort(xl.begin(), xl.end());
        xl.erase(std::unique(xl.begin(), xl.end()), xl.end());
        HIPCK(p, p->d_xlist.upload(xl));
        d.xlist = p->d_xlist.p; d.nxlist = (int)xl.size();
    }
    // ---- band of the compact dense system, measured from the structure; two ways to use it -------------------------------------
    //   T >= 24 tiles: the two-ended sweep inside LDS (plba_band.hip, two workgroups, two launches)
    //   8 <= T < 24  : the two-ended ("twin") form of the multi-launch factorisation (plba_dense.hip): same kernels, the two ends
    //                  of the band eliminated side by side in each launch
    p->band_ok = false; p->twin_ok = false;
    for (double& v : p->plan_twin) v = 0.0;
    p->dd.band = 0; p->dd.twin_m0 = 0; p->dd.twin_fac = nullptr; p->dd.cs_order = nullptr; p->dd.perm = nullptr; p->dd.xmap = nullptr; p->dd.alt = nullptr; p->dd.alt2 = nullptr;
    p->dd.wtw = nullptr;
    if (p->chain_ok && p->lm_ok && p->world <= 1) {      // fused landmark path on one GPU: the chain Schur complement's W^T W tiles are formed in the gather launch
        const int T = p->cv.Pdpad / 32;
        HIPCK(p, p->d_wtw.alloc((size_t)(T * (T + 1) / 2 + T) * 1024, false));
        p->dd.wtw = p->d_wtw.p;
    }
    int plan_hbt = -1;      // (debug_get "solver_plan": the band as measured, -1 = not measured)
    if (p->chain_ok && p->opt.band_solve && !p->dv.flow && !p->dv.wide) {      // (sharded runs: the lists above hold the GLOBAL structure)
        const ChainView& cv = p->cv;
        const int T = cv.Pdpad / 32;
        int hbt = 0;
        if (T >= 8) {
            const std::vector<int32_t>& hpidx = p->h_pidx; const std::vector<int32_t>& hsegcol = p->h_seg_col;
            std::vector<int32_t> dense_of(p->ld, -1);
            for (int c = 0; c < cv.Pd; ++c) dense_of[hpidx[c]] = c;
            // (1) entries the pose-side assembly / the Schur pairs can make non-zero (d.alist), (2) the chain elimination's fill:
            // all dense columns of a segment's window couple with each other
            for (int32_t idx : p->h_alist) {
                const int r = dense_of[idx / p->ld], c = dense_of[idx % p->ld];
                if (r >= 0 && c >= 0) hbt = std::max(hbt, std::abs(r / 32 - c / 32));
            }
            for (int g = 0; g < cv.nseg; ++g) if (hsegcol[2 * g + 1] > hsegcol[2 * g]) hbt = std::max(hbt, (hsegcol[2 * g + 1] - 1) / 32 - hsegcol[2 * g] / 32);
            const int twin_max_t = p->opt.twin_max_tiles > 0 ? p->opt.twin_max_tiles : TWIN_MAX_TILES;      // (experiments: the longest system the twin form takes; default: below the in-LDS threshold)
            const bool twin_pref = p->opt.band_solve == 1 && T <= twin_max_t;
            if (!twin_pref && T >= (p->opt.band_solve >= 2 ? 8 : BAND_MIN_TILES) && band_lds_bytes(cv.Pdpad) <= 160 * 1024 && hbt <= BAND_HB) {      // band_solve = 2 (tests): in LDS from 8 tiles on
                BandView& bv = p->bandv;
                bv.T = T; bv.nA = (T - BAND_HB) / 2; bv.nB = T - BAND_HB - bv.nA;
                HIPCK(p, p->d_band_L.alloc((size_t)2 * T * 4 * 1024, false)); HIPCK(p, p->d_band_y.alloc((size_t)2 * cv.Pdpad, false));
                HIPCK(p, p->d_band_mid.alloc((size_t)2 * (9 * 1024 + 96), false));
                bv.Lband = p->d_band_L.p; bv.y = p->d_band_y.p; bv.mid = p->d_band_mid.p;
                p->band_ok = true;
                p->dd.band = 1;
            } else if (twin_pref && hbt >= 1) {
                if (!p->dd.Ninv) { HIPCK(p, p->dwork.alloc_ninv(cv.Pdpad, cv.Pdpad)); p->dwork.bind_ninv(p->dd); }      // (the multi-chain form keeps the inverse at any length)
                TwinPlan pl;      // (plba_twin_plan.h: chains and separators, the permutation, the tile list of every launch, k_chain_schur's order)
                if (twin_plan_build(T, hbt, pl)) {
                    HIPCK(p, p->d_twin_list.upload(pl.list)); HIPCK(p, p->d_twin_perm.upload(pl.perm)); HIPCK(p, p->d_twin_xmap.upload(pl.xmap)); HIPCK(p, p->d_twin_fac.upload(pl.fac));
                    HIPCK(p, p->d_cs_order.upload(pl.cs_order));
                    HIPCK(p, p->d_twin_alt.alloc((size_t)2 * (cv.Pdpad + TILE) * cv.Pdpad));
                    TwinView& tv = p->twinv;
                    tv.T = T; tv.final0 = pl.final0; tv.nchains = pl.nchains; tv.nlaunch = pl.nlaunch; tv.list = p->d_twin_list.p; tv.off.swap(pl.off);
                    p->dd.twin_m0 = pl.sep0; p->dd.twin_fac = p->d_twin_fac.p; p->dd.cs_order = p->d_cs_order.p; p->dd.perm = p->d_twin_perm.p; p->dd.xmap = p->d_twin_xmap.p;
                    p->dd.alt = p->d_twin_alt.p; p->dd.alt2 = p->d_twin_alt.p + (size_t)(cv.Pdpad + TILE) * cv.Pdpad;
                    p->twin_ok = true;
                    std::copy(pl.summary, pl.summary + 5, p->plan_twin);      // the plan as chosen, for debug_get "solver_plan"
                }
            }
            plan_hbt = hbt;
        }
        if (ptime) fprintf(stderr, "[prepare] dense system: %d dims, %d tiles, band %d sub-diagonal tiles -> %s\n", cv.Pd, T, hbt, p->band_ok ? "banded twisted solve in LDS" : p->twin_ok ? "multi-chain multi-launch factorisation" : "dense path");
        if (ptime && p->twin_ok) fprintf(stderr, "[prepare] %d chains, %d + %d dependent launches\n", p->twinv.nchains, p->twinv.nlaunch, p->twinv.T - p->twinv.final0 - 1);
    }
    p->plan_hbt = plan_hbt;
    HIPCK(p, darr_flush());
    // the structure is complete: remember it
    p->sc.dd = p->dd; p->sc.alist = d.alist; p->sc.nalist = d.nalist; p->sc.xlist = d.xlist; p->sc.nxlist = d.nxlist; p->sc.Ninv = d.Ninv; p->sc.Nwork = d.Nwork; p->sc.dbgbuf = d.dbgbuf;
    p->sc.chain_ok = p->chain_ok; p->sc.key.swap(skey); p->sc.valid = true;
    }      // (!sc_hit)
    if (ptime) fprintf(stderr, "[prepare] pose structure: %s (%ld hits, %ld misses on this handle)\n", sc_hit ? "the previous window's, kept" : "built", p->sc.hits, p->sc.misses);
    lap("exchange list, band");
    // ---- constant part of the pose-side Hessian: prior J0^T J0 scattered over the free kept vertices ----------------------
    if (p->pr_nv > 0 && p->rank == 0) {
        // (round 5: scattered by a kernel.  It was a stream wait, a read-back of H, a 4.7 MB host image of the pose-side matrix and its upload
        // through the bounce buffer — about a millisecond of EVERY BA call of the reference's steady state, which carries a prior.)
        const int n = p->pr_n;
        HIPCK(p, p->d_pr_H.alloc((size_t)n * n)); HIPCK(p, darr_flush());
        launch_ata(d.pr_J0, n, n, p->d_pr_H.p, n, p->stream);
        hipLaunchKernelGGL(k_prior_scatter, dim3((n * n + 255) / 256), dim3(256), 0, p->stream, p->d_pr_H.p, n, p->pr_nv, p->d_pr_off.p, p->d_pr_idx.p, p->d_pr_size.p, p->d_Hconst.p, p->ld);
        HIPCK(p, hipGetLastError());
    }
    HIPCK(p, darr_flush());
    HIPCK(p, plba_stream_wait(p, p->stream));      // the uploads above were queued on the stream from host vectors that end here
    lap("final stream sync");
    if (ptime) fprintf(stderr, "[prepare] %zu small buffers in the batch blocks: %.0f KB cleared, %.0f KB copied\n", p->batch.n_batched, p->batch.zused / 1024.0, p->batch.uused / 1024.0);
    // buffers this window did not re-create must not keep a pointer into the batch blocks, which now hold other buffers (the
    // failure class of the re-used-handle fault of round 4): the conditionally allocated ones are dropped when their stamp is old
    p->d_imu_loc.expire(); p->d_ob_err.expire(); p->work.expire(); p->dwork.expire(); p->d_pr_H.expire();
    p->d_lm_grp.expire(); p->d_lmg_slot.expire(); p->d_lmg_ob0.expire(); p->d_lmg_orig.expire(); p->d_lmg_blk_ij.expire();
    p->d_lmg_blk_start.expire(); p->d_lmg_blk_src.expire(); p->d_lmg_row_kf.expire(); p->d_lmg_row_start.expire(); p->d_lmg_row_src.expire();
    p->d_alist2.expire(); p->d_lmg_ws8.expire(); p->d_lmg_fixed.expire(); p->d_lmg_level.expire(); p->d_col_gather.expire();
    p->d_lmg_meas_pt.expire(); p->d_lmg_meas_ln.expire(); p->d_lmg_wt.expire(); p->d_lmg_chi.expire(); p->d_lmg_part.expire();
    p->d_twin_list.expire(); p->d_twin_perm.expire(); p->d_twin_xmap.expire(); p->d_twin_fac.expire(); p->d_cs_order.expire();
    p->d_xlist.expire(); p->d_alist.expire(); p->d_trow.expire(); p->d_bkf.expire(); p->d_esrc.expire();
    p->d_cidx.expire(); p->d_epos.expire(); p->d_seg_start.expire(); p->d_seg_col.expire(); p->d_pidx.expire(); p->d_ppos.expire();
    p->d_pslot.expire(); p->d_slotcol.expire(); p->d_kfpos.expire(); p->d_ekf.expire(); p->d_ukf.expire();
    p->d_Ldinv.expire(); p->d_Lsub.expire(); p->d_band_y.expire(); p->d_band_mid.expire();
    p->cur = 0;
    p->saved_valid = true;
    p->dirty = false;
    p->chi_E = E; p->chi_carry = false;
    p->prior_changed = false;
    ++p->state_epoch;
    return PLBA_OK;
}

static int exchange(plba_problem* p, double* dev, size_t n, int op) {
    if (p->world <= 1) return PLBA_OK;
    int rc = p->xfn(p->xuser, dev, n, op, (void*)p->stream);
    if (rc) FAIL(p, PLBA_ERR_EXCHANGE, "all-reduce callback failed (%d)", rc);
    return PLBA_OK;
}
static bool owns_pose_edges(const plba_problem* p) { return p->rank == 0; }

static LmParams lm_params(const plba_problem* p) {
    LmParams lp;
    lp.tau = p->opt.tau; lp.lower = p->opt.good_step_lower; lp.upper = p->opt.good_step_upper;
    lp.user_lambda = p->opt.user_lambda_init; lp.max_trials = p->opt.max_trials;
    return lp;
}

// In front of the first iteration of a call (plba_optimize, plba_debug_build): ONE launch resets the control block and clears what the
// first passes add into — bimu, kfdiag, Himu at its structural positions (k_call_setup says why those are enough).  It replaces a
// control-block kernel and three memsets (the one over all of Himu: 4.7 MB at configs[2], a tenth of it structural), each a launch of
// its own on an empty stream.  Without an assembly list (chain_elim = 0) every entry of Himu is assembled, so all of it is cleared.
static int enqueue_call_setup(plba_problem* p) {
    const DevBuf& d = p->dv;
    if (!d.alist) HIPCK(p, hipMemsetAsync(d.Himu, 0, (size_t)d.Ppad * d.ld * 8, p->stream));
    launch_call_setup(d, p->stream);
    return PLBA_OK;
}
// computeActiveErrors + buildSystem for the current estimate (everything lambda-independent)
#define MARK(p, i) do { if ((p)->opt.profile >= 2) HIPCK(p, hipEventRecord((p)->ev[i], (p)->stream)); } while (0)
// profile = 1 samples the factorisation span on every PROFILE_SAMPLE-th trial only: an event pair costs the stream ~8 us of
// bubbles per trial (measured: 11 us between k_chain_schur and the first block step with events, < 1 us without), which
// would be charged to the very throughput the benchmark reports; ms_phase[1] is scaled back to all trials
constexpr int PROFILE_SAMPLE = 8;
#define MARKF(p, i) do { if ((p)->opt.profile >= 2 || ((p)->opt.profile == 1 && (p)->ev_sample)) HIPCK(p, hipEventRecord((p)->ev[i], (p)->stream)); } while (0)
static int enqueue_linearize(plba_problem* p, bool first_iter, int iteration) {
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    // (first iteration: the accumulators were cleared by the call's set-up launch, enqueue_call_setup; later iterations start from the
    // accumulator k_assemble cleared, swapped in on accept)
    MARK(p, 0);
    p->lin_in_span = !p->spec_lin;      // profile = 2: does the span between events 0 and 2 hold a k_linearize<true> launch?
    if (!p->spec_lin) launch_linearize(d, p->cur, true, p->rob, owns_pose_edges(p), s);   // observations + IMU / prior edges, one launch
    p->spec_lin = false;      // else: already enqueued right behind the previous trial's k_decide (plba_optimize)
    MARK(p, 2);
    if (p->spec_hll) p->assembled = true;      // the accepted trial's landmark blocks + assembly ran behind its deciding launch
    else p->assembled = launch_landmark_hll(d, p->cur, !first_iter, owns_pose_edges(p), s);
    p->spec_hll = false;
    if (first_iter) launch_kfdiag(d, p->cur, p->world > 1, s);      // (into the kfdiag the set-up launch cleared)
    // chi2 of the start state (and computeLambdaInit) is only needed on the first iteration of a call.  On later ones it
    // is the chi2 of the trial that was just accepted, evaluated on the very same state: k_decide left it in the control
    // block (already global in a sharded run) together with the iteration / trial counters, so neither the control
    // kernel nor a collective is needed.
    if (!first_iter) { MARK(p, 3); return PLBA_OK; }
    const bool keep_chi = false;
    if (p->world > 1) {
        int rc;
        launch_reduce(d, owns_pose_edges(p), p->d_red.p, s);
        if ((rc = exchange(p, p->d_red.p, 1, 0))) return rc;
        if ((rc = exchange(p, p->d_red.p + 2, 1, 1))) return rc;
        if ((rc = exchange(p, d.posediag, (size_t)d.P, 0))) return rc;
    }
    launch_lambda_init2(d, lm_params(p), p->d_red.p, first_iter, iteration, p->world <= 1, keep_chi, s);
    MARK(p, 3);
    return PLBA_OK;
}
// setLambda + Schur complement (+ optional dense solve, back-substitution, trial update)
static int enqueue_solve(plba_problem* p, bool do_solve, bool need_dinv) {
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    MARK(p, 4);
    if (need_dinv) launch_landmark_dinv(d, s);   // otherwise k_landmark_hll<true> already formed (Hll + lambda I)^-1
    if (need_dinv || !p->assembled) launch_assemble(d, owns_pose_edges(p), s);   // ... and assembled the pose-side system
    p->assembled = false;
    const bool chain_rides = do_solve && p->chain_ok && p->world == 1;      // chain blocks need nothing from the other ranks' landmarks... but the all-reduce carries rank 0's IMU terms
    launch_schur_pairs(d, p->cur, chain_rides ? &p->cv : nullptr, s);
    MARK(p, 5);
    if (p->world > 1) {   // single GPU: k_assemble / k_schur_pairs wrote bp into bpg directly
        // only the entries that can be non-zero before the factorisation (pose x pose, IMU / prior blocks, diagonal) and the two rhs rows travel
        const size_t npk = list_packed_size(d);
        if (p->d_xbuf.n < npk) HIPCK(p, p->d_xbuf.alloc(npk, false));
        launch_list_pack(d, p->d_xbuf.p, false, s);
        int rc = exchange(p, p->d_xbuf.p, npk, 0);
        if (rc) return rc;
        launch_list_pack(d, p->d_xbuf.p, true, s);
        HIPCK(p, hipMemcpyAsync(d.bpg, d.sys + (size_t)(d.Ppad + 1) * d.ld, (size_t)d.ld * 8, hipMemcpyDeviceToDevice, s));
    }
    MARK(p, 6);
    if (!do_solve) return PLBA_OK;
    const int epoch = ++p->flow_epoch;
    if (p->chain_ok) {
        // velocity / bias variables first (block-tridiagonal, one workgroup), then the dense factorisation on the
        // 6-per-keyframe pose system, then the chain back-substitution (plba_chain.hip)
        if (!chain_rides) launch_chain_elim(d, p->cv, s);
        launch_chain_schur(d, p->cv, p->dd, s);
        MARKF(p, 11);
        if (p->band_ok) {
            launch_band_solve(p->dd, p->bandv, s);      // factorisation, forward and backward substitution: two launches
            MARKF(p, 12);
        } else if (p->twin_ok) {
            launch_twin_cholesky(p->dd, p->twinv, s);   // the band's two ends side by side: nA + 1 + (middle - 1) launches instead of T - 1
            MARKF(p, 12);
            launch_trsv_back(p->dd, true, epoch, s);
        } else {
            launch_cholesky(p->dd, true, epoch, s, chain_schur_factors_tile0(p->dd));
            MARKF(p, 12);
            launch_trsv_back(p->dd, true, epoch, s);
        }
    } else {
        MARKF(p, 11);
        launch_cholesky(d, p->opt.use_mfma != 0, epoch, s);
        MARKF(p, 12);
        launch_trsv_back(d, p->opt.use_mfma != 0, epoch, s);
    }
    MARK(p, 7);
    launch_backsub(d, p->cur, p->cur ^ 1, p->chain_ok ? &p->cv : nullptr, p->chain_ok ? p->dd.x : nullptr, s);
    if (!p->chain_ok) launch_update_kf(d, p->cur, p->cur ^ 1, s);
    MARK(p, 8);
    return PLBA_OK;
}

// ---- fused landmark-major passes (options.lm_fused; plba_lm_dev.h): the launches of one LM trial ------------------------------------
//   C  k_lm_schur   chain segments (reading the pose-side accumulators) | groups: linearise + Hll / bl + damped inverse + rank-k update of the group's pose blocks
//   D  k_lm_gather  blocks assembling the rest | pose-pair blocks = pose-side terms + the groups' parts
//      chain Schur, factorisation, back-substitution of the dense system (unchanged)
//   A  k_lm_trial   chain back-substitution segments + keyframe update | groups: landmark back-substitution, update, trial residuals |
//                   IMU / prior edges of the trial state (Jacobians into the idle accumulators; they wait, inside the launch, for the chain
//                   segments that produce the trial keyframes); the LM decision in the launch's last workgroup
// first iteration of a call: pose-side edges + the diagonal pass (chi2, max |H_jj|) + lambda_init instead of nothing before C
static int lm_enqueue_first(plba_problem* p, int iteration) {
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    MARK(p, 0);      // (Himu, bimu, kfdiag: cleared by the call's set-up launch, enqueue_call_setup)
    // one GPU, short window, no per-phase events: lambda_init rides in the diagonal pass's last-arriving workgroup (diag_arrive) instead of
    // in a one-workgroup launch behind it.  The long-window and the sharded form, and profile = 2 (its events 2 | 3 sit between the two), keep their launches.
    const bool ride = p->world <= 1 && p->lv.nrow * 6 <= 256 && p->opt.profile < 2;
    const LambdaInitFusion li{lm_params(p), p->d_red.p, iteration};
    launch_lm_schur(d, p->lv, p->cur, p->rob, true, nullptr, false, s, owns_pose_edges(p), ride ? &li : nullptr);      // (+ the pose-side edges, behind the groups)
    MARK(p, 2);
    if (p->world > 1) {
        launch_lm_gather(d, p->lv, true, false, false, s);      // chi2 (sum), max |Hll_jj| (max) and the pose diagonal (sum) become global before computeLambdaInit, as on the record-based path
        int rc;
        launch_reduce_n(d, owns_pose_edges(p), p->d_red.p, p->lv.ngrp, s);
        launch_posediag(d, s);
        if ((rc = exchange(p, p->d_red.p, 1, 0))) return rc;
        if ((rc = exchange(p, p->d_red.p + 2, 1, 1))) return rc;
        if ((rc = exchange(p, d.posediag, (size_t)d.P, 0))) return rc;
        launch_lambda_init2(d, lm_params(p), p->d_red.p, true, iteration, false, false, s);
    } else if (p->lv.nrow * 6 > 256) {
        // long windows (configs[4]: 200 keyframes): the one-workgroup form below walks 1200 diagonal entries x hundreds of groups, 98 us;
        // the sharded path's launches — a workgroup per keyframe for the diagonal gather — take a quarter of that
        launch_lm_gather(d, p->lv, true, false, false, s);
        launch_reduce_n(d, true, p->d_red.p, p->lv.ngrp, s);
        launch_posediag(d, s);
        launch_lambda_init2(d, lm_params(p), p->d_red.p, true, iteration, false, false, s);
    } else if (!ride) launch_lambda_init_n(d, p->lv, lm_params(p), p->d_red.p, iteration, p->lv.ngrp, s);      // (+ the diagonal gather)
    MARK(p, 3);
    return PLBA_OK;
}
static int lm_enqueue_system(plba_problem* p, const DevBuf& ds, int state, bool spec, bool mark = false) {
    hipStream_t s = p->stream;
    const bool sharded = p->world > 1;
    // one GPU: the chain elimination segments ride in front of the groups (they read the pose-side accumulators directly).  Sharded: the
    // accumulators live on rank 0 alone, so the segments run on the all-reduced system, as a launch of their own behind the exchange
    launch_lm_schur(ds, p->lv, state, p->rob, false, sharded ? nullptr : &p->cv, spec, s);
    if (mark) MARK(p, 5);      // profile = 2: [4, 5] = k_lm_schur alone (the pass over every observation), [5, 6] = gather + assembly
    // (one GPU: the gather launch also forms the W^T W tiles of the chain Schur complement — k_chain_schur then only subtracts them)
    launch_lm_gather(ds, p->lv, false, !sharded || owns_pose_edges(p), spec, s, p->dd.wtw ? &p->cv : nullptr, p->dd.wtw ? &p->dd : nullptr);      // lambda (and the unit padding) from one rank only
    if (sharded) {
        // only the entries that can be non-zero before the factorisation (pose x pose, IMU / prior blocks, diagonal) and the two rhs rows travel
        const size_t npk = list_packed_size(ds);
        if (p->d_xbuf.n < npk) HIPCK(p, p->d_xbuf.alloc(npk, false));
        if (mark) MARK(p, 13);      // profile = 2: [13, 14] = pack + all-reduce + unpack of the structural entries (ms_phase[6])
        launch_list_pack(ds, p->d_xbuf.p, false, s);
        int rc = exchange(p, p->d_xbuf.p, npk, 0);
        if (rc) return rc;
        launch_list_pack(ds, p->d_xbuf.p, true, s);
        HIPCK(p, hipMemcpyAsync(ds.bpg, ds.sys + (size_t)(ds.Ppad + 1) * ds.ld, (size_t)ds.ld * 8, hipMemcpyDeviceToDevice, s));
        if (mark) MARK(p, 14);
        launch_chain_elim(ds, p->cv, s);
    }
    return PLBA_OK;
}
static int lm_enqueue_solve_and_trial(plba_problem* p) {
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    const int epoch = ++p->flow_epoch;
    launch_chain_schur(d, p->cv, p->dd, s, p->dd.wtw != nullptr);
    MARKF(p, 11);
    if (p->band_ok) { launch_band_solve(p->dd, p->bandv, s); MARKF(p, 12); }
    else if (p->twin_ok) { launch_twin_cholesky(p->dd, p->twinv, s); MARKF(p, 12); launch_trsv_back(p->dd, true, epoch, s); }
    else { launch_cholesky(p->dd, true, epoch, s, chain_schur_factors_tile0(p->dd)); MARKF(p, 12); launch_trsv_back(p->dd, true, epoch, s); }
    MARK(p, 7);
    MARK(p, 8);
    return PLBA_OK;
}

// the count the trial launch's pose-side blocks wait for: every chain segment of every k_lm_trial launch so far (lead_wait).
// options.diag bit 2 (fault injection, tests/test_lm_fused.py): a count that is never reached — the wait must run into its bound,
// set Ctrl::sync_fail and fail the call; it must not hang the queue.
static unsigned lm_back_target(plba_problem* p) {
    const unsigned t = (++p->back_epoch) * (unsigned)std::max(p->cv.nseg, 1);
    return (p->opt.diag & PLBA_DIAG_LEAD_WAIT_FAIL) ? t + 1000u : t;
}
static void lm_chi_sync(plba_problem* p) {
    if (p->lm_ok && p->lm_chi_dirty) launch_lm_chi_sync(p->dv, p->lv, p->stream);
    p->lm_chi_dirty = false;
}

extern "C" {

int plba_optimize(plba_problem* p, int max_iters, const volatile uint8_t* abort_flag, plba_stats* out) {
    if (!p) return PLBA_ERR_INVALID;
    auto t0 = std::chrono::steady_clock::now();
    int rc = prepare(p, true);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    plba_stats st;
    memset(&st, 0, sizeof st);
    if ((rc = enqueue_call_setup(p))) return rc;      // (a kernel, not an upload + wait: the call starts without a synchronisation)
    ++p->state_epoch;
    p->trace.clear();
    const LmParams lp = lm_params(p);
    bool ok = true;
    double last_chi = 0.0, lambda = 0.0;
    if (p->opt.profile && !p->ev_ready) {
        for (auto& e : p->ev) HIPCK(p, hipEventCreate(&e));
        p->ev_ready = true;
    }
    auto span = [&](int a, int b) -> double { float ms = 0.f; return hipEventElapsedTime(&ms, p->ev[a], p->ev[b]) == hipSuccess ? (double)ms : 0.0; };
    p->spec_lin = false; p->spec_hll = false;
    double fact_sampled_ms = 0.0;
    int fact_samples = 0;
    p->lm_spec = false;
    for (int it = 0; it < max_iters && !(abort_flag && *abort_flag) && ok && p->lm_ok; ++it) {
        // ---- fused landmark-major passes (see lm_enqueue_* above) ------------------------------------------------------------------
        if (it == 0 && (rc = lm_enqueue_first(p, it))) return rc;
        p->lm_chi_dirty = true;      // (the cached per-observation chi2 now lives in group order: lm_chi_sync before anything reads DevBuf::ob_chi2)
        double rho = 0.0;
        int qmax = 0;
        do {
            p->ev_sample = (p->opt.profile == 1) && (p->trial_counter++ % PROFILE_SAMPLE == 0);
            MARK(p, 4);
            const bool had_spec = p->lm_spec;      // the accepted trial's system is already in the stream
            if (!p->lm_spec && (rc = lm_enqueue_system(p, d, p->cur, false, true))) return rc;
            p->lm_spec = false;
            MARK(p, 6);
            if ((rc = lm_enqueue_solve_and_trial(p))) return rc;
            const int trial = p->cur ^ 1;
            const unsigned long long seq = ++p->mail_seq;
            const bool jac_trial = it + 1 < max_iters;      // not the call's last iteration: the trial's pose-side edges are linearised while they are measured
            DevBuf ds = d;
            if (jac_trial) { std::swap(ds.Himu, ds.Himu_alt); std::swap(ds.bimu, ds.bimu_alt); std::swap(ds.bprior, ds.bprior_alt); }
            DecideFusion df{lp, p->d_red.p, p->d_mail, seq};
            bool spec = false;
            const bool sharded = p->world > 1;
            if (p->opt.profile >= 2 || sharded) {
                launch_lm_trial(ds, p->lv, p->cur, trial, jac_trial, p->rob, &p->cv, p->dd.x, lm_back_target(p), owns_pose_edges(p), nullptr, s);
                MARK(p, 9);
                if (sharded) {      // [chi2, landmark part of the scale] become global; every rank then takes the same decision
                    launch_reduce_n(d, owns_pose_edges(p), p->d_red.p, p->lv.ngrp, s);
                    MARK(p, 15);
                    if ((rc = exchange(p, p->d_red.p, 4, 0))) return rc;      // [chi2, scale, (max diag: unused here), in-launch wait failed on some rank]
                    MARK(p, 16);
                    launch_decide(d, lp, p->d_red.p, false, p->d_mail, seq, s);
                } else launch_decide_n(d, lp, p->d_red.p, p->lv.ngrp, p->d_mail, seq, s);
                MARK(p, 10);
                if (p->opt.profile >= 2) HIPCK(p, plba_stream_wait(p, s));
                else HIPCK(p, mail_wait(p, s, seq));
            } else {
                launch_lm_trial(ds, p->lv, p->cur, trial, jac_trial, p->rob, &p->cv, p->dd.x, lm_back_target(p), true, &df, s);      // the trial's IMU / prior edges (linearised into the idle accumulators) | landmark groups; + the decision
                if (jac_trial) { if ((rc = lm_enqueue_system(p, ds, trial, true))) return rc; spec = true; }      // gated on the device-side decision
                HIPCK(p, mail_wait(p, s, seq));
            }
            if (__atomic_load_n(&p->h_mail->seq, __ATOMIC_ACQUIRE) != seq) FAIL(p, PLBA_ERR_DEVICE, "LM control block was not delivered by the device");
            *p->h_ctrl = p->h_mail->c;
            if ((int)p->trace.size() < TRACE_CAP) p->trace.push_back(p->h_mail->row);      // the trace is kept from the mailbox: no read-back at the end of the call
            if (p->h_ctrl->sync_fail) FAIL(p, PLBA_ERR_DEVICE, "k_lm_trial: the pose-side blocks waited for the chain back-substitution beyond their bound");
            if (p->opt.profile >= 2) st.ms_phase[1] += span(11, 12);
            else if (p->opt.profile == 1 && p->ev_sample) { fact_sampled_ms += span(11, 12); ++fact_samples; }
            if (p->opt.profile >= 2) {
                // [0]: the linearising Schur pass + assembly (launch C) and the gather (launch D) when this trial issued them; [7]: first-iteration passes
                if (qmax == 0 && it == 0) st.ms_phase[7] += span(0, 3);
                if (!had_spec) { st.ms_phase[0] += span(4, 5); ++p->prof_lin_launches; st.ms_phase[2] += span(5, 6); }
                st.ms_phase[3] += span(6, 7); st.ms_phase[4] += span(7, 8); st.ms_phase[5] += span(8, 9); st.ms_phase[7] += span(9, 10);
                if (sharded) {      // the two all-reduces of a trial, out of the phases they sit in
                    const double x1 = had_spec ? 0.0 : span(13, 14), x2 = span(15, 16);
                    st.ms_phase[6] += x1 + x2; st.ms_phase[2] -= x1; st.ms_phase[7] -= x2;
                }
            }
            const Ctrl& c = *p->h_ctrl;
            rho = c.rho;
            lambda = c.lambda;
            st.trials++;
            if (c.accepted) {
                p->cur ^= 1; last_chi = c.current_chi;
                if (jac_trial) { std::swap(p->dv.Himu, p->dv.Himu_alt); std::swap(p->dv.bimu, p->dv.bimu_alt); std::swap(p->dv.bprior, p->dv.bprior_alt); }
                p->lm_spec = spec;
            }
            else if (!std::isfinite(lambda)) break;
            qmax++;
        } while (rho < 0 && qmax < lp.max_trials && !(abort_flag && *abort_flag));
        st.iterations++;
        if (qmax == lp.max_trials || rho == 0 || !std::isfinite(lambda)) { ok = false; st.stop_reason = 1; }
    }
    bool spec_unconsumed = p->lm_spec;      // abort / Terminate right after an accepted step: the gated launches of the next system are still in the stream
    p->lm_spec = false;
    for (int it = 0; it < max_iters && !(abort_flag && *abort_flag) && ok && !p->lm_ok; ++it) {
        if ((rc = enqueue_linearize(p, it == 0, it))) return rc;
        double rho = 0.0;
        int qmax = 0;
        do {
            p->ev_sample = (p->opt.profile == 1) && (p->trial_counter++ % PROFILE_SAMPLE == 0);
            if ((rc = enqueue_solve(p, true, it == 0 || qmax > 0))) return rc;
            const int trial = p->cur ^ 1;
            const unsigned long long seq = ++p->mail_seq;
            // one GPU: the workgroup of the trial-error launch that finishes last takes the LM decision (no k_decide launch)
            const bool decide_rides = p->world <= 1 && p->opt.profile < 2;
            DecideFusion df{lp, p->d_red.p, p->d_mail, seq};
            // One GPU, not the call's last iteration: the trial is LINEARISED while it is measured (k_linearize<true> with the
            // decision riding in its last workgroup) into the idle record table / accumulators, and its landmark blocks +
            // assembly follow gated on that decision; acceptance swaps the tables in, rejection leaves them to be overwritten.
            const bool jac_trial = decide_rides && it + 1 < max_iters;
            bool spec = false, spec_hll = false, jac_sync = false;
            if (jac_trial) {
                DevBuf ds = d;
                std::swap(ds.Himu, ds.Himu_alt); std::swap(ds.bimu, ds.bimu_alt); std::swap(ds.bprior, ds.bprior_alt); std::swap(ds.erec, ds.erec_alt);
                launch_linearize(ds, trial, true, p->rob, owns_pose_edges(p), s, false, &df);
                MARK(p, 9);
                MARK(p, 10);
                spec_hll = launch_landmark_hll(ds, trial, true, owns_pose_edges(p), s, true);      // false: no landmarks, nothing rode
                spec = true;
            } else if (p->world <= 1 && it + 1 < max_iters) {
                // the synchronous form of the same thing (profile >= 2: an event after every phase): the trial is measured by the
                // SAME kernel instance — the two instances round chi2 differently in the last bit — then k_decide, no speculation
                DevBuf ds = d;
                std::swap(ds.Himu, ds.Himu_alt); std::swap(ds.bimu, ds.bimu_alt); std::swap(ds.bprior, ds.bprior_alt); std::swap(ds.erec, ds.erec_alt);
                launch_linearize(ds, trial, true, p->rob, owns_pose_edges(p), s);
                MARK(p, 9);
                launch_decide(d, lp, p->d_red.p, true, p->d_mail, seq, s);
                MARK(p, 10);
                jac_sync = true;
            } else {
                launch_linearize(d, trial, false, p->rob, owns_pose_edges(p), s, false, decide_rides ? &df : nullptr);
                MARK(p, 9);
                if (p->world > 1) {
                    launch_reduce(d, owns_pose_edges(p), p->d_red.p, s);
                    if ((rc = exchange(p, p->d_red.p, 2, 0))) return rc;
                }
                if (!decide_rides) launch_decide(d, lp, p->d_red.p, p->world <= 1, p->d_mail, seq, s);
                MARK(p, 10);
                // The next iteration's linearisation goes out NOW, gated on the decision k_decide leaves in the device control
                // block: if the step was accepted it linearises the trial state (into the accumulators that are swapped in
                // below), if not it returns at once and the retry goes on with the old records.  The host's reaction time
                // (mailbox poll + enqueueing the next launches) hides behind it.  (Sharded runs only: one GPU takes the paths above.)
                if (p->opt.profile < 2 && it + 1 < max_iters) {
                    DevBuf ds = d;
                    std::swap(ds.Himu, ds.Himu_alt); std::swap(ds.bimu, ds.bimu_alt); std::swap(ds.bprior, ds.bprior_alt);
                    launch_linearize(ds, trial, true, p->rob, owns_pose_edges(p), s, true);
                    spec = true;
                }
            }
            if (p->opt.profile >= 2) {
                HIPCK(p, plba_stream_wait(p, s));        // every phase event must have completed before it is read
            } else HIPCK(p, mail_wait(p, s, seq));      // k_decide is the last kernel of the trial and writes the control block into mapped host memory
            if (__atomic_load_n(&p->h_mail->seq, __ATOMIC_ACQUIRE) != seq) FAIL(p, PLBA_ERR_DEVICE, "LM control block was not delivered by the device");
            *p->h_ctrl = p->h_mail->c;
            if ((int)p->trace.size() < TRACE_CAP) p->trace.push_back(p->h_mail->row);      // the trace is kept from the mailbox: no read-back at the end of the call
            if (p->opt.profile >= 2) st.ms_phase[1] += span(11, 12);
            else if (p->opt.profile == 1 && p->ev_sample) { fact_sampled_ms += span(11, 12); ++fact_samples; }
            if (p->opt.profile >= 2) {
                // ms_phase[0] = time inside k_linearize<true> launches, wherever they run: at the head of an iteration only when the
                // accepted trial had not linearised that state already (the call's first iteration, or after a rejection); in the
                // synchronous trial form (jac_sync) the launch between events 8 and 9 IS the linearisation of the trial state.
                // prof_lin_launches counts the launches bracketed, so that time / count is an average launch duration (bench.py).
                if (qmax == 0) { if (p->lin_in_span) { st.ms_phase[0] += span(0, 2); ++p->prof_lin_launches; } st.ms_phase[7] += span(2, 3); }
                st.ms_phase[2] += span(4, 5); st.ms_phase[6] += span(5, 6); st.ms_phase[3] += span(6, 7);
                st.ms_phase[4] += span(7, 8); st.ms_phase[7] += span(9, 10);
                if (jac_sync) { st.ms_phase[0] += span(8, 9); ++p->prof_lin_launches; } else st.ms_phase[5] += span(8, 9);
            }
            const Ctrl& c = *p->h_ctrl;
            rho = c.rho;
            lambda = c.lambda;
            st.trials++;
            if (c.accepted) {
                p->cur ^= 1; last_chi = c.current_chi;
                std::swap(p->dv.Himu, p->dv.Himu_alt); std::swap(p->dv.bimu, p->dv.bimu_alt); std::swap(p->dv.bprior, p->dv.bprior_alt);
                if (jac_trial || jac_sync) std::swap(p->dv.erec, p->dv.erec_alt);
                p->spec_lin = spec || jac_sync; p->spec_hll = spec_hll;
            }
            else if (!std::isfinite(lambda)) break;
            qmax++;
        } while (rho < 0 && qmax < lp.max_trials && !(abort_flag && *abort_flag));
        st.iterations++;
        if (qmax == lp.max_trials || rho == 0 || !std::isfinite(lambda)) { ok = false; st.stop_reason = 1; }
    }
    spec_unconsumed = spec_unconsumed || p->spec_lin || p->spec_hll;
    p->spec_lin = false; p->spec_hll = false;      // an unconsumed one (abort / stop right after an accepted step) only refreshed the records of the current state
    if (spec_unconsumed) HIPCK(p, plba_stream_wait(p, s));      // the call returns with its stream drained (plba_stats.ms_total, plba.h)
    if (p->opt.profile == 1 && fact_samples > 0) st.ms_phase[1] = fact_sampled_ms / fact_samples * st.trials;      // sampled trials scaled to all
    if (abort_flag && *abort_flag && st.stop_reason == 0 && st.iterations < max_iters) st.stop_reason = 2;
    // trace + stats
    const int ntr = (int)p->trace.size();
    if (ntr) {      // (trace rows and the final control block arrived through the mailbox, trial by trial)
        st.chi2_initial = p->trace[0].chi2_current;
        st.chi2_final = p->trace[0].chi2_current;
        for (const auto& r : p->trace) if (r.accepted) st.chi2_final = r.chi2_trial;
        st.solver_failures = p->h_ctrl->n_fail;
        st.lambda_final = p->h_ctrl->lambda;
    } else {
        // no iteration ran: report the chi2 of the current estimate (computeActiveErrors only)
        launch_linearize(d, p->cur, false, p->rob, owns_pose_edges(p), s);
        p->lm_chi_dirty = false;
        launch_reduce(d, owns_pose_edges(p), p->d_red.p, s);
        if (p->world > 1 && (rc = exchange(p, p->d_red.p, 1, 0))) return rc;
        double chi = 0.0;
        HIPCK(p, plba_d2h(p, &chi, p->d_red.p, 8));
        HIPCK(p, plba_stream_wait(p, s));
        st.chi2_initial = st.chi2_final = chi;
    }
    (void)last_chi;
    st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = st;
    return PLBA_OK;
}

int plba_recompute_errors(plba_problem* p) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    launch_linearize(p->dv, p->cur, false, p->rob, owns_pose_edges(p), p->stream);
    p->lm_chi_dirty = false;      // (ob_chi2 was just rewritten in place)
    HIPCK(p, plba_stream_wait(p, p->stream));
    return PLBA_OK;
}

void plba_refine_default_options(plba_refine_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_iters = 5; o->max_trials = 10; o->lambda_init = 1e-2;
}
// The kernel and its mapping: plba_refine.hip.  Here: the checks, the masks in, one launch, the evaluation pass, the per-landmark words out.
int plba_refine_landmarks(plba_problem* p, const plba_refine_options* opt, plba_refine_stats* out) {
    if (!p) return PLBA_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    if (!opt) FAIL(p, PLBA_ERR_INVALID, "plba_refine_landmarks: no plba_refine_options");
    if (opt->max_iters < 1 || opt->max_trials < 1 || !(opt->lambda_init > 0.0) || !std::isfinite(opt->lambda_init))
        FAIL(p, PLBA_ERR_INVALID, "plba_refine_landmarks: max_iters %d, max_trials %d, lambda_init %g (need >= 1, >= 1, a positive finite number)", opt->max_iters, opt->max_trials, opt->lambda_init);
    if (p->world > 1) FAIL(p, PLBA_ERR_INVALID, "plba_refine_landmarks: a sharded problem (plba_set_shard, world %d) is not refined on the device", p->world);
    if (!p->win.have_cam || !p->win.K) FAIL(p, PLBA_ERR_STATE, "plba_refine_landmarks: nothing uploaded");
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const int Np = p->win.Np, Nl = p->win.Nl, L = Np + Nl;
    plba_refine_stats st;
    memset(&st, 0, sizeof st);
    if (L > 0) {
        DArr<uint8_t> d_sel;
        DArr<double> d_chi;
        DArr<int32_t> d_cnt;
        HIPCK(p, d_chi.alloc(2 * (size_t)L, false)); HIPCK(p, d_cnt.alloc(3 * (size_t)L, false));
        if (opt->select_point || opt->select_line) {
            std::vector<uint8_t> sel((size_t)L, 1);
            if (opt->select_point) for (int i = 0; i < Np; ++i) sel[i] = opt->select_point[i] ? 1 : 0;
            if (opt->select_line) for (int i = 0; i < Nl; ++i) sel[(size_t)Np + i] = opt->select_line[i] ? 1 : 0;
            HIPCK(p, d_sel.alloc((size_t)L, false));
            HIPCK(p, plba_h2d(p, d_sel.p, sel.data(), (size_t)L));
        }
        RefineArgs a{};
        a.max_iters = opt->max_iters; a.max_trials = opt->max_trials; a.cur = p->cur; a.lambda_init = opt->lambda_init;
        a.select = d_sel.p; a.lm_pos = p->lm_grouped ? p->d_lm_pos.p : nullptr; a.chi = d_chi.p; a.cnt = d_cnt.p;
        ++p->state_epoch;      // (the getters' mirror is of the previous estimates)
        HIPCK(p, launch_refine(p->dv, p->rob, a, p->stream));
        launch_linearize(p->dv, p->cur, false, p->rob, owns_pose_edges(p), p->stream);      // the evaluation pass of plba_recompute_errors
        p->lm_chi_dirty = false;
        std::vector<double> chi(2 * (size_t)L);
        std::vector<int32_t> cnt(3 * (size_t)L);
        HIPCK(p, plba_d2h(p, chi.data(), d_chi.p, chi.size() * sizeof(double)));      // (waits for the stream: the local buffers may go back to the pool)
        HIPCK(p, plba_d2h(p, cnt.data(), d_cnt.p, cnt.size() * sizeof(int32_t)));
        for (int i = 0; i < L; ++i) {
            const int s = cnt[3 * (size_t)i];
            if (opt->status) opt->status[i] = (uint8_t)s;
            if (opt->iters) opt->iters[i] = cnt[3 * (size_t)i + 1];
            if (opt->trials) opt->trials[i] = cnt[3 * (size_t)i + 2];
            if (s == PLBA_REFINE_FIXED || s == PLBA_REFINE_UNSELECTED || s == PLBA_REFINE_NO_OBS) { ++st.n_skipped; continue; }
            ++st.n_refined;
            st.iterations += cnt[3 * (size_t)i + 1]; st.trials += cnt[3 * (size_t)i + 2];
            if (s == PLBA_REFINE_NONFINITE) continue;
            if (s == PLBA_REFINE_EXHAUSTED) ++st.n_exhausted;
            st.chi2_before += chi[2 * (size_t)i]; st.chi2_after += chi[2 * (size_t)i + 1];
        }
    } else {
        launch_linearize(p->dv, p->cur, false, p->rob, owns_pose_edges(p), p->stream);
        p->lm_chi_dirty = false;
        HIPCK(p, plba_stream_wait(p, p->stream));
    }
    st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (out) *out = st;
    return PLBA_OK;
}

int plba_set_levels(plba_problem* p, plba_edge_kind kind, const uint8_t* level) {
    if (!p || !level) return PLBA_ERR_INVALID;
    if (kind != PLBA_EDGE_POINT && kind != PLBA_EDGE_LINE) FAIL(p, PLBA_ERR_INVALID, "levels only for point/line edges");
    const int E = p->win.Ep + p->win.El;
    if ((int)p->win.level.size() != E) p->win.level.assign(E, 0);
    if (!p->dirty) {   // device copy may have been changed by gate_outliers: refresh the host mirror first
        HIPCK(p, hipSetDevice(p->device));
        HIPCK(p, plba_stream_wait(p, p->stream));
        if (E) HIPCK(p, plba_d2h(p, p->win.level.data(), p->d_level.p, E));
    }
    if (kind == PLBA_EDGE_POINT) memcpy(p->win.level.data(), level, p->win.Ep);
    else memcpy(p->win.level.data() + p->win.Ep, level, p->win.El);
    if (!p->dirty && E) { HIPCK(p, plba_h2d(p, p->d_level.p, p->win.level.data(), E)); if (p->lm_ok) launch_lm_level_sync(p->dv, p->lv, p->stream); }
    return PLBA_OK;
}
int plba_get_levels(plba_problem* p, plba_edge_kind kind, uint8_t* level) {
    if (!p || !level) return PLBA_ERR_INVALID;
    if (kind != PLBA_EDGE_POINT && kind != PLBA_EDGE_LINE) return PLBA_ERR_INVALID;
    const int E = p->win.Ep + p->win.El;
    if ((int)p->win.level.size() != E) p->win.level.assign(E, 0);
    if (!p->dirty && E) {
        HIPCK(p, hipSetDevice(p->device));
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, p->win.level.data(), p->d_level.p, E));
    }
    if (kind == PLBA_EDGE_POINT) memcpy(level, p->win.level.data(), p->win.Ep);
    else memcpy(level, p->win.level.data() + p->win.Ep, p->win.El);
    return PLBA_OK;
}

int plba_gate_outliers(plba_problem* p, double thresh, int* np_out, int* nl_out) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const DevBuf& d = p->dv;
    Ctrl* c = d.ctrl;
    HIPCK(p, hipMemsetAsync(&c->n_gate_pt, 0, 2 * sizeof(int), p->stream));
    lm_chi_sync(p);
    launch_gate(d, p->cur, thresh, p->stream);
    if (p->lm_ok) launch_lm_level_sync(d, p->lv, p->stream);      // the fused passes read the levels in group order
    HIPCK(p, hipMemcpyAsync(p->h_ctrl, d.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, p->stream));
    // the gate is the one place where the device changes the levels: the host mirror follows at once, so that a rebuild of the device image
    // (a state, IMU or prior setter before the next call) uploads the gated levels and not the ones from before the gate
    const int E = p->win.Ep + p->win.El;
    if ((int)p->win.level.size() != E) p->win.level.assign(E, 0);
    if (E) HIPCK(p, hipMemcpyAsync(p->win.level.data(), p->d_level.p, (size_t)E, hipMemcpyDeviceToHost, p->stream));
    HIPCK(p, plba_stream_wait(p, p->stream));
    p->rob.on[PLBA_EDGE_POINT] = 0;    // setRobustKernel(0) on every point / line edge (mapHandler.cpp:6055,6065)
    p->rob.on[PLBA_EDGE_LINE] = 0;
    if (np_out) *np_out = p->h_ctrl->n_gate_pt;
    if (nl_out) *nl_out = p->h_ctrl->n_gate_ln;
    return p->h_ctrl->n_gate_pt + p->h_ctrl->n_gate_ln;
}

int plba_cull_observations(plba_problem* p, double thresh, uint8_t* bad_point, uint8_t* bad_line, int* np_out, int* nl_out) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const DevBuf& d = p->dv;
    const int E = p->win.Ep + p->win.El;
    std::vector<uint8_t> bad((size_t)std::max(E, 1), 0);
    if (E) {
        lm_chi_sync(p);
        launch_cull(d, p->cur, thresh, p->d_depth.p, p->stream);
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, bad.data(), p->d_depth.p, (size_t)E));
    }
    int np = 0, nl = 0;
    for (int e = 0; e < p->win.Ep; ++e) np += bad[e];
    for (int e = 0; e < p->win.El; ++e) nl += bad[p->win.Ep + e];
    if (bad_point && p->win.Ep) memcpy(bad_point, bad.data(), (size_t)p->win.Ep);
    if (bad_line && p->win.El) memcpy(bad_line, bad.data() + p->win.Ep, (size_t)p->win.El);
    if (np_out) *np_out = np;
    if (nl_out) *nl_out = nl;
    return np + nl;
}

int plba_get_edge_chi2(plba_problem* p, plba_edge_kind kind, double* chi2, uint8_t* dpos) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const DevBuf& d = p->dv;
    if (kind == PLBA_EDGE_POINT || kind == PLBA_EDGE_LINE) {
        const int o = kind == PLBA_EDGE_POINT ? 0 : p->win.Ep, n = kind == PLBA_EDGE_POINT ? p->win.Ep : p->win.El;
        // (both kernels queued before the first copy waits: one device round trip per call instead of three)
        if (chi2 && n) lm_chi_sync(p);
        if (dpos && n) launch_depth(d, p->cur, p->d_depth.p, p->stream);
        if (chi2 && n) HIPCK(p, plba_d2h(p, chi2, d.ob_chi2 + o, (size_t)n * 8));
        if (dpos && n) HIPCK(p, plba_d2h(p, dpos, p->d_depth.p + o, n));
    } else if (kind == PLBA_EDGE_IMU_PVR || kind == PLBA_EDGE_IMU_BIAS) {
        std::vector<double> c((size_t)p->win.M * 4);
        if (p->win.M) HIPCK(p, plba_d2h(p, c.data(), d.imu_chi, c.size() * 8));
        for (int m = 0; m < p->win.M; ++m) { if (chi2) chi2[m] = c[(size_t)m * 4 + (kind == PLBA_EDGE_IMU_PVR ? 0 : 1)]; if (dpos) dpos[m] = 1; }
    } else if (kind == PLBA_EDGE_PRIOR) {
        double c = 0.0;
        if (p->pr_nv) HIPCK(p, plba_d2h(p, &c, d.pr_chi, 8));
        if (chi2) chi2[0] = c;
        if (dpos) dpos[0] = 1;
    } else return PLBA_ERR_INVALID;
    return PLBA_OK;
}

int plba_get_trace(plba_problem* p, plba_trace_row* rows, int cap, int* n) {
    if (!p) return PLBA_ERR_INVALID;
    const int c = std::min((int)p->trace.size(), cap);
    if (rows && c > 0) memcpy(rows, p->trace.data(), sizeof(plba_trace_row) * c);
    if (n) *n = (int)p->trace.size();
    return PLBA_OK;
}

// The write-back of a BA call reads keyframes, points AND lines (mapHandler.cpp:6202-6239): ONE read-back per state serves the three getters
// (state_epoch: bumped by every upload, optimize and restore).  The landmark estimates are packed on the device first — a point uses half
// of its 48-byte slot —, the keyframe states ride behind them, everything comes back in one copy and one wait; the requesting call is served
// straight from the pinned bounce buffer, the mirror keeps the rest for the other getters.
// (round 4: three read-backs, 0.20 ms per BA call at configs[2]; round 5: packed landmarks 0.12 ms, with the keyframes in the same copy one
// more device round trip less)
__global__ void k_lm_pack(const double* __restrict__ lm, const int32_t* __restrict__ pos_of_slot /* null: slot order */, int Np, int Nl, const double* __restrict__ kf, int nkf, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int np3 = 3 * Np, nl6 = 6 * Nl;
    if (t < np3) { const int sl = t / 3; out[t] = lm[(size_t)(pos_of_slot ? pos_of_slot[sl] : sl) * 6 + t % 3]; }
    else if (t < np3 + nl6) { const int sl = Np + (t - np3) / 6; out[t] = lm[(size_t)(pos_of_slot ? pos_of_slot[sl] : sl) * 6 + (t - np3) % 6]; }
    else if (t < np3 + nl6 + nkf) out[t] = kf[t - np3 - nl6];
}
// what = 0: keyframes (P3 .. dba3), 1: points (xyz), 2: lines
static int get_results(plba_problem* p, int what, double* xyz, double* lines, double* P3, double* V3, double* q4, double* dbg3, double* dba3) {
    int rc = prepare(p);
    if (rc) return rc;
    const size_t np3 = 3 * (size_t)p->win.Np, nl6 = 6 * (size_t)p->win.Nl, nkf = (size_t)p->win.K * KF_STRIDE, tot = np3 + nl6 + nkf;
    std::vector<double>& h = p->res_lm;      // [points packed | lines packed | keyframe states] of epoch res_lm_epoch
    const double* src = nullptr;
    if (!(p->res_lm_epoch == p->state_epoch && h.size() == tot)) {
        HIPCK(p, hipSetDevice(p->device));
        StageArea* st = p->have_ctx ? p->ctx.stage : nullptr;
        h.resize(tot);
        if (tot) {
            HIPCK(p, p->d_lm_pack.alloc(tot, false));
            hipLaunchKernelGGL(k_lm_pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, p->stream, p->dv.lm[p->cur], p->lm_grouped ? p->d_lm_pos.p : nullptr, p->win.Np, p->win.Nl,
                               p->dv.kf[p->cur], (int)nkf, p->d_lm_pack.p);
            HIPCK(p, hipGetLastError());
            if (st && st->base && tot * 8 <= st->xfer_cap()) {
                HIPCK(p, hipMemcpyAsync(st->xfer(), p->d_lm_pack.p, tot * 8, hipMemcpyDeviceToHost, p->stream));
                HIPCK(p, plba_stream_wait(p, p->stream));
                src = reinterpret_cast<const double*>(st->xfer());      // the requested part goes straight to the caller from here
                memcpy(h.data(), src, tot * 8);
            } else HIPCK(p, plba_d2h(p, h.data(), p->d_lm_pack.p, tot * 8));
        }
        p->res_lm_epoch = p->state_epoch;
    }
    if (!src) src = h.data();
    if (what == 1 && xyz && np3) memcpy(xyz, src, np3 * 8);
    if (what == 2 && lines && nl6) memcpy(lines, src + np3, nl6 * 8);
    if (what == 0) {
        for (int k = 0; k < p->win.K; ++k) {
            const double* s = src + np3 + nl6 + (size_t)k * KF_STRIDE;
            if (P3) memcpy(P3 + 3 * k, s, 24);
            if (V3) memcpy(V3 + 3 * k, s + 3, 24);
            if (q4) memcpy(q4 + 4 * k, s + 6, 32);
            if (dbg3) memcpy(dbg3 + 3 * k, s + 16, 24);
            if (dba3) memcpy(dba3 + 3 * k, s + 19, 24);
        }
    }
    return PLBA_OK;
}
int plba_get_keyframes(plba_problem* p, double* P3, double* V3, double* q4, double* dbg3, double* dba3) {
    if (!p) return PLBA_ERR_INVALID;
    return get_results(p, 0, nullptr, nullptr, P3, V3, q4, dbg3, dba3);
}
int plba_get_points(plba_problem* p, double* xyz) {
    if (!p || !xyz) return PLBA_ERR_INVALID;
    return get_results(p, 1, xyz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int plba_get_lines(plba_problem* p, double* l) {
    if (!p || !l) return PLBA_ERR_INVALID;
    return get_results(p, 2, nullptr, l, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int plba_save_state(plba_problem* p) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    launch_state_copy(p->d_kf_saved.p, p->dv.kf[p->cur], (size_t)p->win.K * KF_STRIDE, p->d_lm_saved.p, p->dv.lm[p->cur], (size_t)p->L * 6, p->stream);      // one launch, not two runtime copies
    HIPCK(p, hipGetLastError());
    return PLBA_OK;
}
int plba_restore_state(plba_problem* p) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    ++p->state_epoch;
    launch_state_copy(p->dv.kf[p->cur], p->d_kf_saved.p, (size_t)p->win.K * KF_STRIDE, p->dv.lm[p->cur], p->d_lm_saved.p, (size_t)p->L * 6, p->stream);
    HIPCK(p, hipGetLastError());
    return PLBA_OK;
}

// ---- plba_slide_window (include/plba.h) ----------------------------------------------------------------------------------------------
// new landmark array = kept slots gathered from the current estimates | added slots from the upload (src < 0: -(1 + index into `add`))
__global__ void k_lm_carry_gather(const double* __restrict__ cur, const int32_t* __restrict__ cur_pos /* slot -> position in `cur`, null: slot order */, const double* __restrict__ add,
                                  const int32_t* __restrict__ src, int Np_new, int L_new, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L_new * 6) return;
    const int slot = i / 6, c = i % 6, sidx = src[slot];
    double v = sidx >= 0 ? cur[(size_t)(cur_pos ? cur_pos[sidx] : sidx) * 6 + c] : add[(size_t)(-1 - sidx) * 6 + c];
    if (slot < Np_new && c >= 3) v = 0.0;      // (a point uses the first half of its slot)
    out[i] = v;
}
// new landmark-major measurement / weight arrays: entry g comes from the old arrays (src >= 0) or from the added observations (-(1 + a))
__global__ void k_obs_carry_gather(const double* __restrict__ po_uv0, const double* __restrict__ lo_l0, const double* __restrict__ ob_w0, int Ep0,
                                   const double* __restrict__ a_uv, const double* __restrict__ a_wp, const double* __restrict__ a_l, const double* __restrict__ a_wl,
                                   const int32_t* __restrict__ src, int Ep1, int El1, double* __restrict__ po_uv1, double* __restrict__ lo_l1, double* __restrict__ ob_w1) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= Ep1 + El1) return;
    const int sidx = src[g];
    if (g < Ep1) {
        const double* m = sidx >= 0 ? po_uv0 + 2 * (size_t)sidx : a_uv + 2 * (size_t)(-1 - sidx);
        po_uv1[2 * (size_t)g] = m[0]; po_uv1[2 * (size_t)g + 1] = m[1];
        ob_w1[g] = sidx >= 0 ? ob_w0[sidx] : a_wp[-1 - sidx];
    } else {
        const int l = g - Ep1;
        const double* m = sidx >= 0 ? lo_l0 + 3 * (size_t)sidx : a_l + 3 * (size_t)(-1 - sidx);
        for (int c = 0; c < 3; ++c) lo_l1[3 * (size_t)l + c] = m[c];
        ob_w1[g] = sidx >= 0 ? ob_w0[(size_t)Ep0 + sidx] : a_wl[-1 - sidx];
    }
}
int plba_get_sizes(const plba_problem* p, int32_t* out6) {
    if (!p || !out6) return PLBA_ERR_INVALID;
    out6[0] = p->win.K; out6[1] = p->win.Np; out6[2] = p->win.Nl; out6[3] = p->win.Ep; out6[4] = p->win.El; out6[5] = p->win.M;
    return PLBA_OK;
}
// Three parts.  PLAN (plba_window.h, pure host code): every check, the keep / drop maps, the merged lists, and the complete next window in
// p->win_next — the resident one is read through a const reference.  STAGE: everything that can return a device error; it writes only
// the slide's own buffers (d_kf_carry, d_lm_carry(_src), d_slide_*, d_obs_carry_src, the d_*_c arrays), none of which a window that is not
// dirty reads.  COMMIT: the two windows are swapped.  After the first write to p->win there is no HIP call and no return but the last
// one: whatever the call returns before that, the handle still holds the previous window, not dirty and usable.
int plba_slide_window(plba_problem* p, const plba_slide* s, int32_t* point_map, int32_t* line_map) {
    if (!p || !s) return PLBA_ERR_INVALID;
    if (p->world > 1) FAIL(p, PLBA_ERR_STATE, "plba_slide_window: a sharded problem takes a fresh upload");
    if (p->dirty || !p->win.K) FAIL(p, PLBA_ERR_STATE, "plba_slide_window: no window is resident on the device (upload one and optimize it first)");
    const bool stime = (p->opt.diag & PLBA_DIAG_TIMING) != 0;
    auto st0 = std::chrono::steady_clock::now();
    auto slap = [&](const char* what) { if (!stime) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[slide] %-30s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - st0).count()); st0 = t; };
    // ---- plan ----------------------------------------------------------------------------------------------------------------------------
    const Window& w0 = p->win;
    const Window& w1 = p->win_next;
    const SlidePlan& pl = p->slide;
    if (int rc = slide_plan(w0, *s, p->win_next, p->slide, p->err, sizeof p->err)) return rc;
    slap("plan (checks, lists, host window)");
    // ---- stage ---------------------------------------------------------------------------------------------------------------------------
    HIPCK(p, hipSetDevice(p->device));
    const int nd = s->n_drop, Kk = w0.K - nd, L1 = w1.Np + w1.Nl, E1 = w1.Ep + w1.El;
    // the slide's uploads go through a pinned area of their own (sized here; kept with the cached context): the copies and the gather
    // kernels are queued and the slide returns WITHOUT waiting for them — prepare() re-uses the general staging area at once, and they
    // overlap its host work.  (No room / no pinned memory: the general area, and one wait at the stage's end.)
    bool own_stage = false;
    if (p->have_ctx) {
        const size_t need = ((size_t)L1 * 4 + (size_t)(s->Np_add + s->Nl_add) * 48 + ((size_t)w0.Ep + w0.El + s->Ep_add + s->El_add) * 4 + (size_t)s->Ep_add * 24 + (size_t)s->El_add * 32 +
                             (size_t)s->K_add * KF_STRIDE * 8 + 8 * 256 + StageArea::XFER) * 5 / 4;
        if (!p->ctx.slide_stage) p->ctx.slide_stage = new StageArea;
        StageArea* ss = p->ctx.slide_stage;
        if (ss->cap < need) {
            if (ss->base) { (void)hipHostFree(ss->base); ss->base = nullptr; ss->cap = 0; }
            const size_t cap = std::max<size_t>((need + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1), (size_t)8 << 20);
            if (hipHostMalloc((void**)&ss->base, cap, hipHostMallocDefault) == hipSuccess) ss->cap = cap; else ss->base = nullptr;
        }
        own_stage = ss->base != nullptr && ss->cap >= need;
    }
    // (a queued upload that found no staging room reads its host vector until the wait below: the plan's vectors are the problem's)
    DArrStreamScope staged(p->stream, own_stage ? p->ctx.slide_stage : (p->have_ctx ? p->ctx.stage : nullptr));
    // keyframes: the kept ones' current states are copied ON THE DEVICE behind the added ones' upload
    HIPCK(p, p->d_kf_carry.alloc((size_t)w1.K * KF_STRIDE, false));
    HIPCK(p, hipMemcpyAsync(p->d_kf_carry.p, p->dv.kf[p->cur] + (size_t)nd * KF_STRIDE, (size_t)Kk * KF_STRIDE * 8, hipMemcpyDeviceToDevice, p->stream));
    if (s->K_add) { HIPCK(p, p->d_slide_kf.upload(pl.kf_add)); HIPCK(p, hipMemcpyAsync(p->d_kf_carry.p + (size_t)Kk * KF_STRIDE, p->d_slide_kf.p, (size_t)s->K_add * KF_STRIDE * 8, hipMemcpyDeviceToDevice, p->stream)); }
    slap("keyframes");
    // landmarks: the new array is gathered ON THE DEVICE from the current estimates; only the added ones go up
    HIPCK(p, p->d_lm_carry_src.upload(pl.src_lm)); HIPCK(p, p->d_slide_lm.upload(pl.add_lm));
    HIPCK(p, p->d_lm_carry.alloc(std::max<size_t>((size_t)L1 * 6, 1), false));
    if (L1) hipLaunchKernelGGL(k_lm_carry_gather, dim3((L1 * 6 + 255) / 256), dim3(256), 0, p->stream, p->dv.lm[p->cur], p->lm_grouped ? p->d_lm_pos.p : nullptr, p->d_slide_lm.p, p->d_lm_carry_src.p, w1.Np, L1, p->d_lm_carry.p);
    HIPCK(p, hipGetLastError());
    slap("landmark carry");
    // measurements and weights: gathered on the device from the old landmark-major arrays + the added observations
    {
        DArr<double>& dadd = p->d_slide_ob;
        HIPCK(p, p->d_obs_carry_src.upload(pl.src_ob)); HIPCK(p, dadd.upload(pl.add_ob));
        HIPCK(p, p->d_po_uv_c.alloc(std::max<size_t>(2 * (size_t)w1.Ep, 1), false)); HIPCK(p, p->d_lo_l_c.alloc(std::max<size_t>(3 * (size_t)w1.El, 1), false)); HIPCK(p, p->d_ob_w_c.alloc(std::max<size_t>((size_t)E1, 1), false));
        const size_t o_wp = 2 * (size_t)s->Ep_add, o_l = o_wp + s->Ep_add, o_wl = o_l + 3 * (size_t)s->El_add;
        if (E1) hipLaunchKernelGGL(k_obs_carry_gather, dim3((E1 + 255) / 256), dim3(256), 0, p->stream, p->d_po_uv.p, p->d_lo_l.p, p->d_ob_w.p, w0.Ep, dadd.p, dadd.p + o_wp, dadd.p + o_l, dadd.p + o_wl,
                                   p->d_obs_carry_src.p, w1.Ep, w1.El, p->d_po_uv_c.p, p->d_lo_l_c.p, p->d_ob_w_c.p);
        HIPCK(p, hipGetLastError());
        if (!own_stage) HIPCK(p, plba_stream_wait(p, p->stream));      // (shared staging area: every queued copy must have left it before prepare() writes it again)
    }
    slap("observation carry");
    // ---- commit: nothing below can fail -----------------------------------------------------------------------------------------------------
    std::swap(p->win, p->win_next);
    p->carry_obs_pending = true;
    p->chi_E = -1; p->chi_carry = false;      // (all edges are level 0 again and none has been evaluated)
    p->dirty = true;
    if (point_map) memcpy(point_map, pl.pmap.data(), pl.pmap.size() * 4);
    if (line_map) memcpy(line_map, pl.lmap.data(), pl.lmap.size() * 4);
    return PLBA_OK;
}

int plba_marginalize(plba_problem* p, int first_kf, int max_edges, plba_prior* out) {
    if (!p || !out) return PLBA_ERR_INVALID;
    int rc = prepare(p, true);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    return marginalize_device(p, first_kf, max_edges, out);
}
int plba_marginalize_factors(plba_problem* p, int n_imu, const int32_t* imu_edges, int n_pt, const int32_t* point_edges,
                             int n_ln, const int32_t* line_edges, int use_prior, int n_drop, const int32_t* drop_vid, plba_prior* out) {
    if (!p || !out || n_imu < 0 || n_pt < 0 || n_ln < 0 || n_drop < 0) return PLBA_ERR_INVALID;
    int rc = prepare(p, true);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    std::vector<int> im(imu_edges, imu_edges + n_imu), pt(point_edges, point_edges + n_pt), ln(line_edges, line_edges + n_ln), dr(drop_vid, drop_vid + n_drop);
    return marginalize_factors_device(p, im, pt, ln, use_prior != 0, dr, out);
}
int plba_marginalize_to_prior(plba_problem* p, int first_kf, int max_edges, int32_t* out3) {
    if (!p) return PLBA_ERR_INVALID;
    if (p->world > 1) FAIL(p, PLBA_ERR_STATE, "plba_marginalize_to_prior: a sharded problem is not marginalized on the device");
    if (first_kf < 0 || first_kf >= p->win.K) FAIL(p, PLBA_ERR_INVALID, "marginalize: first_kf out of range");      // (before prepare(): window and prior untouched)
    int rc = prepare(p, true);      // (resolves the previous one: its result is this call's old prior)
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    if ((rc = marginalize_device(p, first_kf, max_edges, nullptr))) return rc;
    if (out3) { out3[0] = p->pr_n; out3[1] = p->pr_m; out3[2] = p->pr_nv; }
    return PLBA_OK;
}
int plba_compute_marginals(plba_problem* p, plba_marginals* m) {
    if (!p) return PLBA_ERR_INVALID;
    if (!m) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: no plba_marginals");
    if (p->world > 1) FAIL(p, PLBA_ERR_STATE, "plba_compute_marginals: a sharded problem has no marginals on the device");
    if (!p->win.have_cam || !p->win.K) FAIL(p, PLBA_ERR_STATE, "plba_compute_marginals: nothing uploaded");
    const bool want_pair = (m->want & 2) && m->n_pairs > 0;
    if ((m->want & 2) && m->n_pairs < 0) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: n_pairs < 0");
    if (want_pair && (!m->pairs || !m->pair_cov)) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: pairs / pair_cov missing");
    if (want_pair)
        for (int q = 0; q < 2 * m->n_pairs; ++q)
            if (m->pairs[q] < 0 || m->pairs[q] >= p->win.K) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: pair %d names keyframe slot %d of %d", q / 2, m->pairs[q], p->win.K);
    if ((m->want & 1) && !m->kf_cov) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: kf_cov missing");
    if ((m->want & 4) && p->win.Np && !m->pt_cov) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: pt_cov missing");
    if ((m->want & 8) && p->win.Nl && !m->ln_cov) FAIL(p, PLBA_ERR_INVALID, "plba_compute_marginals: ln_cov missing");
    int rc = prepare(p, true);      // (slid window, pending prior: as plba_optimize would see them)
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    return cov_run(p, m);
}
int plba_get_prior(plba_problem* p, plba_prior* out) {
    if (!p || !out) return PLBA_ERR_INVALID;
    memset(out, 0, sizeof *out);
    if (p->mp) { if (int rc = marg_resolve(p)) return rc; }
    if (p->pr_nv == 0) FAIL(p, PLBA_ERR_STATE, "plba_get_prior: the problem holds no prior");
    const int n = p->pr_n, nv = p->pr_nv;
    size_t nx = 0;
    for (int i = 0; i < nv; ++i) nx += p->pr_size[i] == 9 ? 10 : 6;
    std::vector<double> h;
    if (p->prior_dev) {      // [x0 | J0 | r0 | A' | b'] in one read-back
        HIPCK(p, hipSetDevice(p->device));
        h.resize(nx + 2 * (size_t)n * n + 2 * (size_t)n);
        HIPCK(p, plba_d2h(p, h.data(), p->d_prd[p->prd_slot].p, h.size() * 8));
    }
    out->n = n; out->m = p->prior_dev ? p->pr_m : 0; out->nv = nv;
    out->vid = (int32_t*)calloc(nv + 1, 4); out->size = (int32_t*)calloc(nv + 1, 4); out->idx = (int32_t*)calloc(nv + 1, 4);
    memcpy(out->vid, p->pr_vid.data(), (size_t)nv * 4); memcpy(out->size, p->pr_size.data(), (size_t)nv * 4); memcpy(out->idx, p->pr_idx.data(), (size_t)nv * 4);
    out->x0 = (double*)calloc(nx + 1, 8); out->J0 = (double*)malloc(((size_t)n * n + 1) * 8); out->r0 = (double*)malloc((size_t)(n + 1) * 8);
    if (p->prior_dev) {
        const double* q = h.data();
        memcpy(out->x0, q, nx * 8); q += nx;
        memcpy(out->J0, q, (size_t)n * n * 8); q += (size_t)n * n;
        memcpy(out->r0, q, (size_t)n * 8); q += n;
        out->Ar = (double*)malloc(((size_t)n * n + 1) * 8); out->br = (double*)malloc((size_t)(n + 1) * 8);
        memcpy(out->Ar, q, (size_t)n * n * 8); q += (size_t)n * n;
        memcpy(out->br, q, (size_t)n * 8);
    } else {
        memcpy(out->x0, p->pr_x0.data(), nx * 8); memcpy(out->J0, p->pr_J0.data(), (size_t)n * n * 8); memcpy(out->r0, p->pr_r0.data(), (size_t)n * 8);
    }
    return PLBA_OK;
}
void plba_prior_free(plba_prior* pr) {
    if (!pr) return;
    free(pr->vid); free(pr->size); free(pr->idx); free(pr->x0); free(pr->J0); free(pr->r0); free(pr->Ar); free(pr->br);
    memset(pr, 0, sizeof *pr);
}

// ---- diagnostics ------------------------------------------------------------------------------------------------------
int plba_debug_build(plba_problem* p, double lambda, int do_solve) {
    if (!p) return PLBA_ERR_INVALID;
    int rc = prepare(p, true);
    if (rc) return rc;
    HIPCK(p, hipSetDevice(p->device));
    const DevBuf& d = p->dv;
    Ctrl c0;
    memset(&c0, 0, sizeof c0);
    c0.solver_ok = 1; c0.ni = 2.0;
    if ((rc = enqueue_call_setup(p))) return rc;
    HIPCK(p, plba_h2d(p, d.ctrl, &c0, sizeof c0));
    if (p->lm_ok) {      // fused landmark-major passes, with the diagnostic outputs the parity tests read (Hll, bl, residuals, xl)
        p->lv.dbg_out = 1; p->lv.ob_err = p->d_ob_err.p;
        if ((rc = lm_enqueue_first(p, 0))) return rc;
        p->lm_chi_dirty = true;
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, &c0, d.ctrl, sizeof c0));
        c0.lambda = lambda;
        HIPCK(p, plba_h2d(p, d.ctrl, &c0, sizeof c0));
        rc = lm_enqueue_system(p, d, p->cur, false);
        if (!rc && do_solve) {
            rc = lm_enqueue_solve_and_trial(p);
            if (!rc) launch_lm_trial(d, p->lv, p->cur, p->cur ^ 1, false, p->rob, &p->cv, p->dd.x, lm_back_target(p), true, nullptr, p->stream);      // (errors only: the accumulators keep the built system)
        }
        p->lv.dbg_out = 0; p->lv.ob_err = nullptr;
        if (rc) return rc;
        HIPCK(p, plba_stream_wait(p, p->stream));
        HIPCK(p, plba_d2h(p, p->h_ctrl, d.ctrl, sizeof(Ctrl)));
        return PLBA_OK;
    }
    if ((rc = enqueue_linearize(p, true, 0))) return rc;
    HIPCK(p, plba_stream_wait(p, p->stream));
    HIPCK(p, plba_d2h(p, &c0, d.ctrl, sizeof c0));
    c0.lambda = lambda;
    HIPCK(p, plba_h2d(p, d.ctrl, &c0, sizeof c0));
    if ((rc = enqueue_solve(p, do_solve != 0, true))) return rc;
    HIPCK(p, plba_stream_wait(p, p->stream));
    HIPCK(p, plba_d2h(p, p->h_ctrl, d.ctrl, sizeof(Ctrl)));
    return PLBA_OK;
}

int plba_debug_get(plba_problem* p, const char* what, double* out, size_t cap, size_t* n) {
    if (!p || !what) return PLBA_ERR_INVALID;
    const std::string w(what);
    if (w == "host_waits") {      // (read without waiting for anything)
        if (n) *n = 1;
        if (out && cap) *out = (double)p->host_waits;
        return PLBA_OK;
    }
    if (w == "pgo_sparse") {      // (host-side record of the last plba_optimize_pose_graph: the pose graph uploads no window)
        if (n) *n = 8;
        for (size_t i = 0; out && i < cap && i < 8; ++i) out[i] = p->pgo_sparse[i];
        return PLBA_OK;
    }
    if (w == "pgo_cov") {         // (host-side record of the last plba_pose_graph_marginals)
        if (n) *n = 8;
        for (size_t i = 0; out && i < cap && i < 8; ++i) out[i] = p->pgo_cov[i];
        return PLBA_OK;
    }
    if (w == "pgo_cov_H") {       // (its Hblk, kept under PLBA_DIAG_PGO_COV_DUMP; empty otherwise)
        if (n) *n = p->pgo_cov_H.size();
        for (size_t i = 0; out && i < cap && i < p->pgo_cov_H.size(); ++i) out[i] = p->pgo_cov_H[i];
        return PLBA_OK;
    }
    if (w == "lba_sparse") {      // (host-side record of the last plba_lba_visual)
        if (n) *n = 8;
        for (size_t i = 0; out && i < cap && i < 8; ++i) out[i] = p->lba_sparse[i];
        return PLBA_OK;
    }
    if (w == "bow_db") {       // (host-side record of the place-recognition database)
        double d5[5];
        plba_bow_describe(p, d5);
        if (n) *n = 5;
        for (size_t i = 0; out && i < cap && i < 5; ++i) out[i] = d5[i];
        return PLBA_OK;
    }
    if (w == "covis_map") {    // (host-side record of the resident covisibility map)
        double d6[6];
        plba_covis_describe(p, d6);
        if (n) *n = 6;
        for (size_t i = 0; out && i < cap && i < 6; ++i) out[i] = d6[i];
        return PLBA_OK;
    }
    if (p->dirty) FAIL(p, PLBA_ERR_STATE, "debug_get before debug_build/optimize");
    if (w == "marg_path" && p->mp) { if (int rc = marg_resolve(p)) return rc; }      // (after the check: a refused call changes nothing)
    HIPCK(p, hipSetDevice(p->device));
    HIPCK(p, plba_stream_wait(p, p->stream));
    const DevBuf& d = p->dv;
    std::vector<double> v;
    auto fetch = [&](const double* dev, size_t cnt, std::vector<double>& h) -> hipError_t {
        h.resize(cnt);
        return cnt ? plba_d2h(p, h.data(), dev, cnt * 8) : hipSuccess;
    };
    const size_t P = p->P, ld = p->ld;
    if (w == "Hschur") {
        std::vector<double> h;
        HIPCK(p, fetch(d.sys, (size_t)p->Ppad * ld, h));
        v.resize(P * P);
        for (size_t r = 0; r < P; ++r) for (size_t c = 0; c < P; ++c) v[r * P + c] = h[r * ld + c];
    } else if (w == "bschur") { std::vector<double> h; HIPCK(p, fetch(d.sys + (size_t)p->Ppad * ld, ld, h)); v.assign(h.begin(), h.begin() + P); }
    else if (w == "bp") { std::vector<double> h; HIPCK(p, fetch(d.bpg, ld, h)); v.assign(h.begin(), h.begin() + P); }
    else if (w == "x") {
        std::vector<double> hx, hl; std::vector<uint8_t> act(p->L);
        HIPCK(p, fetch(d.x, ld, hx)); HIPCK(p, fetch(d.xl, (size_t)p->L * 6, hl));
        if (p->L) HIPCK(p, plba_d2h(p, act.data(), d.lm_active, p->L));
        v.assign(hx.begin(), hx.begin() + P);
        for (int s = 0; s < p->L; ++s) if (act[s]) for (int t = 0; t < (s < p->win.Np ? 3 : 6); ++t) v.push_back(hl[(size_t)s * 6 + t]);
    } else if (w == "hll_pt" || w == "hll_ln") {
        std::vector<double> h; HIPCK(p, fetch(d.hll, (size_t)p->L * 12, h));
        if (w == "hll_pt") {
            v.resize((size_t)p->win.Np * 9);
            for (int i = 0; i < p->win.Np; ++i) { const double* u = &h[(size_t)i * 12]; double* o = &v[(size_t)i * 9];
                o[0] = u[0]; o[1] = u[1]; o[2] = u[2]; o[3] = u[1]; o[4] = u[3]; o[5] = u[4]; o[6] = u[2]; o[7] = u[4]; o[8] = u[5]; }
        } else {
            v.assign((size_t)p->win.Nl * 36, 0.0);
            for (int i = 0; i < p->win.Nl; ++i) { const double* u = &h[(size_t)(p->win.Np + i) * 12]; double* o = &v[(size_t)i * 36];
                for (int b = 0; b < 2; ++b) { const double* q = u + 6 * b; const int z = b * 3;
                    o[(z + 0) * 6 + z + 0] = q[0]; o[(z + 0) * 6 + z + 1] = q[1]; o[(z + 0) * 6 + z + 2] = q[2];
                    o[(z + 1) * 6 + z + 0] = q[1]; o[(z + 1) * 6 + z + 1] = q[3]; o[(z + 1) * 6 + z + 2] = q[4];
                    o[(z + 2) * 6 + z + 0] = q[2]; o[(z + 2) * 6 + z + 1] = q[4]; o[(z + 2) * 6 + z + 2] = q[5]; } }
        }
    } else if (w == "bl_pt" || w == "bl_ln") {
        std::vector<double> h; HIPCK(p, fetch(d.bl, (size_t)p->L * 6, h));
        if (w == "bl_pt") { v.resize((size_t)p->win.Np * 3); for (int i = 0; i < p->win.Np; ++i) memcpy(&v[(size_t)i * 3], &h[(size_t)i * 6], 24); }
        else { v.resize((size_t)p->win.Nl * 6); for (int i = 0; i < p->win.Nl; ++i) memcpy(&v[(size_t)i * 6], &h[(size_t)(p->win.Np + i) * 6], 48); }
    } else if (w == "err_pvr" || w == "err_bias") {
        std::vector<double> h; HIPCK(p, fetch(d.imu_err, (size_t)p->win.M * 16, h));
        const int o = w == "err_pvr" ? 0 : 9, nn = w == "err_pvr" ? 9 : 6;
        v.resize((size_t)p->win.M * nn);
        for (int m = 0; m < p->win.M; ++m) memcpy(&v[(size_t)m * nn], &h[(size_t)m * 16 + o], nn * 8);
    } else if (w == "err_prior") { HIPCK(p, fetch(d.pr_err, p->pr_nv ? p->pr_n : 0, v)); }
    else if ((w == "err_pt" || w == "err_ln") && p->lm_ok) {      // the fused passes keep no record table: residuals left by the first-iteration pass of debug_build
        std::vector<double> h; HIPCK(p, fetch(p->d_ob_err.p, 2 * (size_t)p->E, h));
        if (w == "err_pt") v.assign(h.begin(), h.begin() + 2 * (size_t)p->win.Ep);
        else { v.assign((size_t)p->win.El * 3, 0.0); for (int e = 0; e < p->win.El; ++e) { v[3 * (size_t)e] = h[2 * (size_t)(p->win.Ep + e)]; v[3 * (size_t)e + 1] = h[2 * (size_t)(p->win.Ep + e) + 1]; } }
    }
    else if (w == "err_pt" || w == "err_ln") {
        std::vector<double> h; HIPCK(p, fetch(d.erec, ((size_t)p->win.Ep + 2 * (size_t)p->win.El) * EREC_UNIT, h));
        if (w == "err_pt") { v.resize((size_t)p->win.Ep * 2); for (int e = 0; e < p->win.Ep; ++e) { const size_t o = (size_t)p->ob_pos[e] * EREC_UNIT; v[2 * (size_t)e] = h[o + EREC_PT_E0]; v[2 * (size_t)e + 1] = h[o + EREC_PT_E0 + 1]; } }      // 64-byte point record
        else { v.assign((size_t)p->win.El * 3, 0.0); for (int e = 0; e < p->win.El; ++e) { const size_t o = (size_t)p->ob_pos[p->win.Ep + e] * EREC_UNIT; v[3 * (size_t)e] = h[o + 13]; v[3 * (size_t)e + 1] = h[o + 14]; } }
    } else if (w == "erec") {
        if (p->lm_ok) FAIL(p, PLBA_ERR_STATE, "\"erec\": the fused landmark passes keep no record table");
        HIPCK(p, fetch(d.erec, ((size_t)p->win.Ep + 2 * (size_t)p->win.El) * EREC_UNIT, v));
    }
    else if (w == "stamps") { HIPCK(p, fetch(d.maxd_part, 80, v)); }
    else if (w == "dbgbuf") { HIPCK(p, fetch(d.dbgbuf, DBGBUF_N, v)); }
    else if (w == "pose_dim") v = {(double)p->P};
    else if (w == "marg_path") v.assign(p->marg_path, p->marg_path + 5);
    else if (w == "prof_lin_launches") v = {(double)p->prof_lin_launches};
    else if (w == "lm_groups") v = p->lm_hist;
    else if (w == "lm_fused") v = {(double)(p->lm_ok ? 1 : 0), (double)p->lv.ngrp, (double)p->lv.nblk, p->lm_ok && p->lm_hist.size() > 18 ? p->lm_hist[18] : 0.0 /* wide groups */};
    else if (w == "marg_J") v = p->marg_dbg;
    else if (w == "cov_S") v = p->cov_dbg_S;
    else if (w == "cov_Sigma") v = p->cov_dbg_Sigma;
    else if (w == "dense_dim") v = {(double)(p->chain_ok ? p->cv.Pd : p->P)};
    else if (w == "band") v = {(double)(p->band_ok ? 1 : 0)};
    else if (w == "twin") v = {(double)(p->twin_ok ? 1 : 0)};
    else if (w == "solver_plan") {      // which form of the reduced-camera solve this window takes (tests/test_solver_accuracy.py):
        // [0] form: 0 = the pose system itself (no chain elimination), 1 = compact system, one launch per tile, 2 = multi-chain, 3 = in-LDS band
        // [1] 32-column tiles of the system factored  [2] explicit L^-T in use  [3] sub-diagonal tiles of the band (-1: not measured)
        // [4] first-stage chains  [5] nested second stage  [6..8] separator widths in tiles  [9] nA  [10] nB (band sweeps)
        const bool ninv = !p->band_ok && (p->chain_ok ? p->dd.Ninv : p->dv.Ninv) != nullptr;
        v = {(double)(p->band_ok ? 3 : p->twin_ok ? 2 : p->chain_ok ? 1 : 0), (double)((p->chain_ok ? p->cv.Pdpad : p->Ppad) / 32), ninv ? 1.0 : 0.0, (double)p->plan_hbt,
             p->plan_twin[0], p->plan_twin[1], p->plan_twin[2], p->plan_twin[3], p->plan_twin[4], (double)(p->band_ok ? p->bandv.nA : 0), (double)(p->band_ok ? p->bandv.nB : 0)};
    }
    else if (w == "fact_launches_estimate") v = {(double)p->seg_launch_est};      // what the segment-length choice expected (twin_plan_launches, plba_twin_plan.h): fact_launches + 1 when the plan is built
    else if (w == "fact_launches") {      // dependent launches of one factorisation between the profile events 11 and 12 (bench.py's roofline)
        if (p->band_ok) v = {2.0};
        else if (p->twin_ok) v = {(double)(p->twinv.nlaunch + (p->twinv.T - p->twinv.final0 - 1))};
        else v = {-1.0};
    }
    else if (w == "chi2") { HIPCK(p, plba_d2h(p, p->h_ctrl, d.ctrl, sizeof(Ctrl))); v = {p->h_ctrl->current_chi}; }
    else if (w == "maxdiag") { HIPCK(p, plba_d2h(p, p->h_ctrl, d.ctrl, sizeof(Ctrl))); v = {p->h_ctrl->maxdiag}; }
    else if (w == "solver_ok") { HIPCK(p, plba_d2h(p, p->h_ctrl, d.ctrl, sizeof(Ctrl))); v = {(double)p->h_ctrl->solver_ok}; }
    else FAIL(p, PLBA_ERR_INVALID, "debug_get: unknown buffer '%s'", what);
    if (n) *n = v.size();
    if (out) { const size_t c = std::min(v.size(), cap); if (c) memcpy(out, v.data(), c * 8); }
    return PLBA_OK;
}

}  // extern "C"
