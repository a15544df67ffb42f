// plba_pgo.hip — SURVEY §8f row 4: the loop-closure pose graph of loopClosureOptimizationCovGraphG2O / ...EssGraphG2O
// (src/mapHandler.cpp:4068-4528) on gfx950: g2o VertexSE3 / EdgeSE3 as include/plba_g2o/types_slam3d.h restates them, under
// the Levenberg loop of SparseOptimizer::optimizeHost (include/plba_g2o/g2o_compat.h), edges to solve on the device.
//
// Layout (n free vertices = those an edge touches that are not fixed, in ascending vertex order; P = 6 n):
//   X, Xs     nv x 12        estimates (R row-major, t) and the backup of the trial's free vertices; cnt: nv oplus counters
//   erec      ne x 120       per edge  A00 = J0^T O J0 | A11 = J1^T O J1 | A10 = J1^T O J0 | g0 = J0^T O e | g1 = J1^T O e
//   echi      ne             per edge  e^T O e of the last evaluation
//   blocks    nblk           every nonzero 6 x 6 block of H (row vertex >= column vertex) with its (edge, slot) sources in edge
//                            order, built once on the host; Hblk (nblk x 36) and b (P) = their undamped sums
//   blkmap    n x n          block id * 2 (+ 1: the transposed block), -1: structurally zero
//   sys       (Ppad + 64) x ld   the damped system in the layout launch_cholesky / launch_trsv_back take, b in row Ppad
//
// One STEP = one LM trial; the host enqueues steps and polls the mapped mailbox one step behind (it never waits on the step it
// has just enqueued, so the device never idles on the host).  A step is
//   k_pgo_edges<jac>      (only when an iteration starts)  error, Jacobians, weighted blocks per edge      thread per edge
//   k_pgo_sum             (only when an iteration starts)  Hblk, b: each block's sources summed in edge order   wave per block
//   k_pgo_iter            (only when an iteration starts)  currentChi, lambda init (computeLambdaInit)        one workgroup
//   k_pgo_fill            sys = H + lambda I (both triangles), unit padding, b; the identity once the run is over
//   launch_cholesky / launch_trsv_back (plba_dense.hip)   x, solver_ok
//   k_pgo_update          backup, X <- X fromVectorMQT(x) (x = 0 after a failed factorisation), orthogonalizeAfter
//   k_pgo_edges<errors>   the trial's chi2 per edge
//   k_pgo_decide          tempChi, scale, rho, the g2o lambda schedule, restore on rejection, trace row, loop exits, mailbox
// options.pgo_solver = 1 replaces k_pgo_fill + launch_cholesky + launch_trsv_back by the multifrontal solve of plba_pgo_sparse.h
// (no blkmap and no dense image; the structure is analysed once per call on the host and held on the device by a PgoSparseWork).
// Every kernel but the factorisation returns at once after the run has ended (PgoCtl::done).  Nothing of O(P^2) or O(E)
// crosses PCIe between the upload and the read-back of the poses, the control block and the trace.
// Bit-reproducible: no floating-point atomics; every sum has one owner and a fixed order.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "plba_internal.h"
#include "plba_pgo_cov.h"
#include "plba_pgo_dev.h"
#include "plba_pgo_sparse_dev.h"
#include "plba_problem.h"

#define HIPCK(p, call) PLBA_HIPCK(p, call)
#define FAIL(p, code, ...) PLBA_FAIL(p, code, __VA_ARGS__)

namespace plba {
namespace {

using namespace pgo_dev;      // the per-edge evaluation and the per-vertex update (plba_pgo_dev.h)

// device-side control: the Ctrl the factorisation reports solver_ok into, + the loop state of optimizeHost
struct PgoCtl {
    Ctrl c;                 // lambda, ni, current_chi, temp_chi, scale, rho, maxdiag; accepted, solver_ok, iteration, trial, n_fail
    double chi2_initial, chi2_final, lambda_final;
    int lin;                // 1: the next step starts an iteration (linearise, sum, currentChi)
    int done, iters, trials, stop_reason, n_trace, pad0, pad1;
};
struct PgoHead { int done, iters, trials, pad; };
using PgoMail = MailOver<PgoHead>;      // laid over the problem's mapped Mailbox (plba_mailbox.h)

struct PgoDev {
    int nv, ne, n, P, Ppad, ld, nblk, max_iters, max_trials, trace_cap;
    double tau, lower, upper, user_lambda;
    double* X;                  // nv x 12
    double* Xs;                 // nv x 12 (free vertices only)
    int* cnt;                   // nv
    const int32_t* free_v;      // n: vertex of each free rank
    const int32_t* ei;          // ne
    const int32_t* ej;
    const double* Zi;           // ne x 12: inverse measurements
    const double* info;         // ne x 36
    double* erec;               // ne x PGO_REC
    double* echi;               // ne
    const int32_t* blk_start;   // nblk + 1
    const int32_t* blk_src;     // edge * 4 + slot (0 A00, 1 A11, 2 A10, 3 A10^T)
    const int32_t* blk_diag;    // nblk: 1 = a diagonal block (carries b)
    const int32_t* blk_row;     // nblk: free rank of the block row
    const int32_t* dg_blk;      // n: diagonal block of each free rank
    const int32_t* blkmap;      // n x n
    double* Hblk;               // nblk x 36
    double* b;                  // P
    double* sys;
    const double* x;            // dense solution
    PgoCtl* ctl;
    PgoMail* mail;
    plba_trace_row* trace;
};

// EdgeSE3::computeError (+ linearizeOplus and the weighted blocks of buildHost when JAC), a thread per edge: the text pgo_edge_eval
// (plba_pgo_dev.h) runs on the host, included here and not called so that the kernel's FMA pairing, and with it every bit, stays as it was
template <bool JAC>
__global__ __launch_bounds__(64) void k_pgo_edges(PgoDev d) {
    if (d.ctl->done || (JAC && !d.ctl->lin)) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= d.ne) return;
    const Iso Xi = iso_load(d.X + (size_t)12 * d.ei[k]), Xj = iso_load(d.X + (size_t)12 * d.ej[k]), Zi = iso_load(d.Zi + (size_t)12 * k);
#define PGO_EDGE_OM (d.info + (size_t)36 * k)
#define PGO_EDGE_CHI d.echi[k]
#define PGO_EDGE_REC (d.erec + (size_t)PGO_REC * k)
#include "plba_pgo_edge_body.inc"
#undef PGO_EDGE_OM
#undef PGO_EDGE_CHI
#undef PGO_EDGE_REC
}

// Hblk, b: a wave per block, lane l < 36 owns entry l, lanes 36..41 the block's b (diagonal blocks); sources in edge order
__global__ __launch_bounds__(256) void k_pgo_sum(PgoDev d) {
    if (d.ctl->done || !d.ctl->lin) return;
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (blk >= d.nblk || l >= 42) return;
    if (l >= 36 && !d.blk_diag[blk]) return;
    const int r = (l < 36) ? l / 6 : l - 36, c = l % 6;
    double acc = 0.0;
    for (int s = d.blk_start[blk]; s < d.blk_start[blk + 1]; ++s) {
        const int src = d.blk_src[s], k = src >> 2, slot = src & 3;
        const double* rec = d.erec + (size_t)PGO_REC * k;
        if (l >= 36) acc -= rec[(slot == 0 ? 108 : 114) + r];
        else acc += pgo_block_term(rec, slot, r, c);
    }
    if (l < 36) d.Hblk[(size_t)36 * blk + l] = acc;
    else d.b[6 * d.blk_row[blk] + r] = acc;
}

// fixed-order sum over one workgroup of 256: thread t takes t, t + 256, ... in order, then a fixed tree
__device__ double wg_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ double chi_total(const PgoDev& d, double* sh) {
    double v = 0.0;
    for (int k = threadIdx.x; k < d.ne; k += 256) v += d.echi[k];
    return wg_sum(v, sh);
}

// start of an iteration: currentChi = activeRobustChi2 of the linearised state; computeLambdaInit in the first one
__global__ __launch_bounds__(256) void k_pgo_iter(PgoDev d) {
    __shared__ double sh[256];
    if (d.ctl->done || !d.ctl->lin) return;
    const double chi = chi_total(d, sh);
    double md = 0.0;
    if (d.ctl->iters == 0)
        for (int i = threadIdx.x; i < d.P; i += 256) md = fmax(md, fabs(d.Hblk[(size_t)36 * d.dg_blk[i / 6] + (i % 6) * 7]));
    sh[threadIdx.x] = md;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        PgoCtl* g = d.ctl;
        g->c.current_chi = chi;
        if (g->iters == 0) {
            g->chi2_initial = chi;
            g->c.maxdiag = sh[0];
            g->c.lambda = d.user_lambda > 0 ? d.user_lambda : d.tau * sh[0];
            g->c.ni = 2.0;
        }
        g->c.trial = 0;
        g->lin = 0;
    }
}

// sys = H + lambda I over the whole (Ppad + 64) x ld image (the factorisation works in place, so every trial writes all of it)
__global__ __launch_bounds__(256) void k_pgo_fill(PgoDev d) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= d.ld) return;
    const bool done = d.ctl->done != 0;
    if (r == 0 && c == 0) d.ctl->c.solver_ok = 1;
    double v = 0.0;
    if (done) v = (r < d.Ppad && r == c) ? 1.0 : 0.0;      // the run has ended: the (ungated) factorisation behind gets the identity
    else if (r < d.P) {
        if (c < d.P) {
            const int id = d.blkmap[(size_t)(r / 6) * d.n + c / 6];
            if (id >= 0) v = d.Hblk[(size_t)36 * (id >> 1) + ((id & 1) ? (c % 6) * 6 + r % 6 : (r % 6) * 6 + c % 6)];
            if (r == c) v += d.ctl->c.lambda;
        }
    } else if (r < d.Ppad) v = (r == c) ? 1.0 : 0.0;
    else if (r == d.Ppad) v = (c < d.P) ? d.b[c] : 0.0;
    d.sys[(size_t)r * d.ld + c] = v;
}

// push + oplus of the free vertices (VertexSE3::oplusImpl, the counter counts every call, rejected trials included)
__global__ __launch_bounds__(64) void k_pgo_update(PgoDev d) {
    if (d.ctl->done) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= d.n) return;
    const int v = d.free_v[k];
    double* xp = d.X + (size_t)12 * v;
    double* sp = d.Xs + (size_t)12 * v;
#pragma unroll
    for (int i = 0; i < 12; ++i) sp[i] = xp[i];
    double u[6];
    const bool ok = d.ctl->c.solver_ok != 0;      // a failed factorisation: the host path's x = 0
#pragma unroll
    for (int i = 0; i < 6; ++i) u[i] = ok ? d.x[6 * k + i] : 0.0;
    pgo_vertex_oplus(xp, u, d.cnt + v);
}

__device__ void pgo_deliver(const PgoDev& d, unsigned long long seq) {
    d.mail->c.done = d.ctl->done; d.mail->c.iters = d.ctl->iters; d.mail->c.trials = d.ctl->trials;
    __threadfence_system();
    __hip_atomic_store(&d.mail->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// end of a trial: the Levenberg branch of optimizeHost, then the loop exits
__global__ __launch_bounds__(256) void k_pgo_decide(PgoDev d, unsigned long long seq) {
    __shared__ double sh[256];
    __shared__ int s_reject;
    PgoCtl* g = d.ctl;
    if (g->done) { if (threadIdx.x == 0) pgo_deliver(d, seq); return; }
    const double lambda = g->c.lambda;
    const bool ok = g->c.solver_ok != 0;
    const double chi = chi_total(d, sh);
    double sp = 0.0;
    if (ok) for (int j = threadIdx.x; j < d.P; j += 256) sp += d.x[j] * (lambda * d.x[j] + d.b[j]);
    sp = wg_sum(sp, sh);
    if (threadIdx.x == 0) {
        double tempChi = chi;
        if (!ok) tempChi = 1.7976931348623157e308;      // DBL_MAX
        const double scale = 1e-3 + sp;
        const double rho = (g->c.current_chi - tempChi) / scale;
        const bool acc = rho > 0 && isfinite(tempChi);
        plba_trace_row row;
        row.iteration = g->iters; row.trial = g->c.trial; row.accepted = acc ? 1 : 0; row.solver_ok = ok ? 1 : 0;
        row.lambda = lambda; row.chi2_current = g->c.current_chi; row.chi2_trial = tempChi; row.scale = scale; row.rho = rho;
        if (g->n_trace < d.trace_cap) d.trace[g->n_trace] = row;
        g->n_trace += 1;
        g->trials += 1;
        if (!ok) g->c.n_fail += 1;
        g->c.temp_chi = tempChi; g->c.scale = scale; g->c.rho = rho; g->c.accepted = acc ? 1 : 0;
        bool brk = false;
        if (acc) {
            double alpha = 1.0 - pow(2 * rho - 1, 3);
            alpha = fmin(alpha, d.upper);
            g->c.lambda = lambda * fmax(d.lower, alpha);
            g->c.ni = 2.0;
            g->c.current_chi = tempChi;
        } else {
            g->c.lambda = lambda * g->c.ni;
            g->c.ni *= 2.0;
            brk = !isfinite(g->c.lambda);
        }
        s_reject = acc ? 0 : 1;
        int qmax = g->c.trial;
        if (!brk) ++qmax;
        g->c.trial = qmax;
        if (brk || !(rho < 0 && qmax < d.max_trials)) {      // the iteration ends
            g->iters += 1;
            g->chi2_final = g->c.current_chi; g->lambda_final = g->c.lambda;
            if (qmax == d.max_trials || rho == 0 || !isfinite(g->c.lambda)) { g->stop_reason = 1; g->done = 1; }
            else if (g->iters >= d.max_iters) g->done = 1;
            else g->lin = 1;
        }
    }
    __syncthreads();
    if (s_reject)      // pop
        for (int i = threadIdx.x; i < 12 * d.n; i += 256) { const size_t o = (size_t)12 * d.free_v[i / 12] + i % 12; d.X[o] = d.Xs[o]; }
    if (threadIdx.x == 0) pgo_deliver(d, seq);
}

// max_iters = 0 or nothing to optimise: chi2 only
__global__ __launch_bounds__(256) void k_pgo_chi_only(PgoDev d) {
    __shared__ double sh[256];
    const double chi = chi_total(d, sh);
    if (threadIdx.x == 0) { d.ctl->chi2_initial = chi; d.ctl->chi2_final = chi; }
}

// plba_pose_graph_marginals, after a failed factorisation: behind a launch of k_sps_factor, notes the first tag at which solver_ok is 0
__global__ void k_pgo_cov_mark(const Ctrl* c, int* rec, int tag) {
    if (!c->solver_ok && *rec < 0) *rec = tag;
}

struct HIso { double R[9], t[3]; };
HIso h_load(const double* p) { HIso a; memcpy(a.R, p, 72); memcpy(a.t, p + 9, 24); return a; }
void h_store(const HIso& a, double* p) { memcpy(p, a.R, 72); memcpy(p + 9, a.t, 24); }
// slam3d_detail::mul / inv on the host (same products as plba::mul, no contraction into FMAs on the host)
HIso h_mul(const HIso& a, const HIso& b) {
    M3 A, Bm; memcpy(A.a, a.R, 72); memcpy(Bm.a, b.R, 72);
    const M3 R = mul(A, Bm);
    const V3 t = mul(A, v3(b.t[0], b.t[1], b.t[2])) + v3(a.t[0], a.t[1], a.t[2]);
    HIso r; memcpy(r.R, R.a, 72); r.t[0] = t.x; r.t[1] = t.y; r.t[2] = t.z;
    return r;
}
HIso h_inv(const HIso& a) {
    M3 A; memcpy(A.a, a.R, 72);
    const M3 Rt = transpose(A);
    const V3 x = mul(Rt, v3(a.t[0], a.t[1], a.t[2]));
    HIso r; memcpy(r.R, Rt.a, 72); r.t[0] = -x.x; r.t[1] = -x.y; r.t[2] = -x.z;
    return r;
}

// What both pose-graph entry points build from the graph on the host: the checks of the graph, the free ranks (the vertices an edge
// touches that are not fixed, in ascending vertex order) and, when asked for, every nonzero 6 x 6 block of H (row rank >= column rank,
// ascending) with its (edge, slot) sources in edge order.  dense_map: blkmap too, for the dense solver's fill.
struct PgoGraphSetup {
    int n = 0;                                        // free vertices
    std::vector<int32_t> fr, free_v;                  // free rank of each vertex (-1: fixed or untouched), vertex of each free rank
    std::vector<int32_t> blk_start, blk_src, blk_diag, blk_row, blk_col, dg_blk, blkmap;
};
int pgo_graph_setup(plba_problem* p, const plba_pose_graph* g, const char* who, bool want_blocks, bool dense_map, PgoGraphSetup& u) {
    const int nv = g->nv, ne = g->ne;
    if (nv <= 0 || ne < 0) FAIL(p, PLBA_ERR_INVALID, "%s: nv = %d, ne = %d", who, nv, ne);
    if (!g->pose12 || (ne > 0 && (!g->ei || !g->ej || !g->meas12))) FAIL(p, PLBA_ERR_INVALID, "%s: missing array", who);
    for (size_t i = 0; i < (size_t)12 * nv; ++i)
        if (!std::isfinite(g->pose12[i])) FAIL(p, PLBA_ERR_INVALID, "%s: pose of vertex %d is not finite", who, (int)(i / 12));
    for (int k = 0; k < ne; ++k) {
        if (g->ei[k] < 0 || g->ei[k] >= nv || g->ej[k] < 0 || g->ej[k] >= nv) FAIL(p, PLBA_ERR_INVALID, "%s: edge %d names a vertex out of range", who, k);
        if (g->ei[k] == g->ej[k]) FAIL(p, PLBA_ERR_INVALID, "%s: edge %d joins vertex %d to itself", who, k, g->ei[k]);
        for (int i = 0; i < 12; ++i) if (!std::isfinite(g->meas12[(size_t)12 * k + i])) FAIL(p, PLBA_ERR_INVALID, "%s: measurement of edge %d is not finite", who, k);
        if (g->info36) for (int i = 0; i < 36; ++i) if (!std::isfinite(g->info36[(size_t)36 * k + i])) FAIL(p, PLBA_ERR_INVALID, "%s: information of edge %d is not finite", who, k);
    }
    std::vector<int32_t>& fr = u.fr; std::vector<int32_t>& free_v = u.free_v;
    fr.assign(nv, -1); free_v.clear();
    {
        std::vector<char> touched(nv, 0);
        for (int k = 0; k < ne; ++k) { touched[g->ei[k]] = 1; touched[g->ej[k]] = 1; }
        for (int v = 0; v < nv; ++v) if (touched[v] && !(g->fixed && g->fixed[v] != 0)) { fr[v] = (int32_t)free_v.size(); free_v.push_back(v); }
    }
    const int n = u.n = (int)free_v.size();
    std::vector<int32_t>&blk_start = u.blk_start, &blk_src = u.blk_src, &blk_diag = u.blk_diag, &blk_row = u.blk_row, &blk_col = u.blk_col, &dg_blk = u.dg_blk, &blkmap = u.blkmap;
    blk_start.clear(); blk_src.clear(); blk_diag.clear(); blk_row.clear(); blk_col.clear(); dg_blk.clear(); blkmap.clear();
    if (want_blocks && n > 0) {
        struct Src { int32_t r, c, src; };
        std::vector<Src> s;
        s.reserve((size_t)3 * ne);
        for (int k = 0; k < ne; ++k) {
            const int a = fr[g->ei[k]], b = fr[g->ej[k]];
            if (a >= 0) s.push_back({a, a, 4 * k + 0});
            if (b >= 0) s.push_back({b, b, 4 * k + 1});
            if (a >= 0 && b >= 0) { if (b > a) s.push_back({b, a, 4 * k + 2}); else s.push_back({a, b, 4 * k + 3}); }
        }
        std::stable_sort(s.begin(), s.end(), [](const Src& x, const Src& y) { return x.r != y.r ? x.r < y.r : x.c < y.c; });   // edge order within a block
        if (dense_map) blkmap.assign((size_t)n * n, -1);
        dg_blk.assign(n, -1);
        for (size_t i = 0; i < s.size(); ++i) {
            if (i == 0 || s[i].r != s[i - 1].r || s[i].c != s[i - 1].c) {
                const int id = (int)blk_row.size();
                blk_start.push_back((int32_t)i); blk_row.push_back(s[i].r); blk_col.push_back(s[i].c); blk_diag.push_back(s[i].r == s[i].c ? 1 : 0);
                if (dense_map) {
                    blkmap[(size_t)s[i].r * n + s[i].c] = 2 * id;
                    if (s[i].r != s[i].c) blkmap[(size_t)s[i].c * n + s[i].r] = 2 * id + 1;
                }
                if (s[i].r == s[i].c) dg_blk[s[i].r] = id;
            }
            blk_src.push_back(s[i].src);
        }
        blk_start.push_back((int32_t)s.size());
    }
    return PLBA_OK;
}

// What k_pgo_edges reads of the edges of a graph that has passed pgo_graph_setup: the inverse measurements, the information matrices
// (the identity where the graph gives none) and the endpoints.  Without an edge all four stay empty (DArr::upload: one zeroed element).
struct PgoEdges { std::vector<double> Zi, info; std::vector<int32_t> ei, ej; };
PgoEdges pgo_stage_edges(const plba_pose_graph* g) {
    const int ne = g->ne; PgoEdges e;
    e.Zi.assign((size_t)12 * ne, 0.0); e.info.assign((size_t)36 * ne, 0.0);
    for (int k = 0; k < ne; ++k) {
        h_store(h_inv(h_load(g->meas12 + (size_t)12 * k)), &e.Zi[(size_t)12 * k]);
        if (g->info36) memcpy(&e.info[(size_t)36 * k], g->info36 + (size_t)36 * k, 36 * 8);
        else for (int i = 0; i < 6; ++i) e.info[(size_t)36 * k + 7 * i] = 1.0;
    }
    if (ne > 0) { e.ei.assign(g->ei, g->ei + ne); e.ej.assign(g->ej, g->ej + ne); }
    return e;
}

}  // namespace
}  // namespace plba

using namespace plba;

extern "C" {

int plba_optimize_pose_graph(plba_problem* p, plba_pose_graph* g, int max_iters, double user_lambda_init, int initial_guess,
                             plba_stats* out, plba_trace_row* trace, int trace_cap, int* n_trace) {
    if (!p) return PLBA_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    for (double& v : p->pgo_sparse) v = 0.0;      // (a refused call leaves an all-zero record)
    if (!g || !out) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: no graph or no stats");
    if (trace_cap < 0 || (trace_cap > 0 && !trace)) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: trace_cap > 0 without a trace");
    if (max_iters < 0) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: max_iters < 0");
    if (p->opt.pgo_solver != 0 && p->opt.pgo_solver != 1) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: options.pgo_solver = %d", p->opt.pgo_solver);
    if (!std::isfinite(user_lambda_init)) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: user_lambda_init is not finite");
    const int nv = g->nv, ne = g->ne;
    PgoGraphSetup gs;
    if (int rc = pgo_graph_setup(p, g, "plba_optimize_pose_graph", max_iters > 0, p->opt.pgo_solver != 1, gs)) return rc;
    auto is_fixed = [&](int v) { return g->fixed && g->fixed[v] != 0; };

    // ---- host: estimates, initial guess, active set, block structure --------------------------------------------------------------
    std::vector<double> X(g->pose12, g->pose12 + (size_t)12 * nv);
    if (initial_guess && ne > 0) {
        // the facade's computeInitialGuess (g2o_compat.h): frontier = fixed vertices in the order the edges name them; each `from` of a
        // frontier scans its edges in insertion order: to = from Z (from is vertex 0) or from Z^-1; O(V + E) with incident-edge lists
        std::vector<int32_t> inc_start(nv + 1, 0), inc((size_t)2 * ne);
        for (int k = 0; k < ne; ++k) { ++inc_start[g->ei[k] + 1]; ++inc_start[g->ej[k] + 1]; }
        for (int v = 0; v < nv; ++v) inc_start[v + 1] += inc_start[v];
        { std::vector<int32_t> cur(inc_start.begin(), inc_start.end() - 1); for (int k = 0; k < ne; ++k) { inc[cur[g->ei[k]]++] = k; inc[cur[g->ej[k]]++] = k; } }
        std::vector<char> done(nv, 0);
        std::vector<int> front, next;
        for (int k = 0; k < ne; ++k) for (int v : {g->ei[k], g->ej[k]}) if (is_fixed(v) && !done[v]) { done[v] = 1; front.push_back(v); }
        while (!front.empty()) {
            next.clear();
            for (int from : front)
                for (int q = inc_start[from]; q < inc_start[from + 1]; ++q) {
                    const int k = inc[q];
                    const int to = g->ei[k] == from ? g->ej[k] : g->ei[k];
                    if (done[to] || is_fixed(to)) continue;
                    const HIso Z = h_load(g->meas12 + (size_t)12 * k);
                    h_store(h_mul(h_load(&X[(size_t)12 * from]), g->ei[k] == from ? Z : h_inv(Z)), &X[(size_t)12 * to]);
                    done[to] = 1; next.push_back(to);
                }
            front.swap(next);
        }
    }
    std::vector<int32_t>& free_v = gs.free_v;
    const int n = gs.n, P = 6 * n;
    const bool run = max_iters > 0 && n > 0, sparse = p->opt.pgo_solver == 1;
    std::vector<int32_t>&blk_start = gs.blk_start, &blk_src = gs.blk_src, &blk_diag = gs.blk_diag, &blk_row = gs.blk_row, &blk_col = gs.blk_col, &dg_blk = gs.dg_blk, &blkmap = gs.blkmap;
    const int nblk = (int)blk_row.size();
    PgoSparsePlan plan; double ms_analysis = 0.0;
    if (sparse) {
        p->pgo_sparse[0] = 1.0;
        if (run) {
            const auto ta = std::chrono::steady_clock::now();
            if (!pgo_sparse_analyse(n, blk_row, blk_col, plan)) FAIL(p, PLBA_ERR_INVALID, "plba_optimize_pose_graph: the sparse analysis failed its checks");
            ms_analysis = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
        }
    }

    // ---- device ------------------------------------------------------------------------------------------------------------------
    HIPCK(p, hipSetDevice(p->device));
    hipStream_t s = p->stream;
    const int Ppad = dense_ppad(P), ld = Ppad;
    const size_t sysn = run && !sparse ? (size_t)(Ppad + TILE) * ld : 1;
    const PgoEdges he = pgo_stage_edges(g);
    DArr<double> dX, dXs, dZi, dInfo, dErec, dEchi, dHblk, db, sys, xx /* the sparse solve's */;
    DArr<int32_t> dfree, dei, dej, dbs, dbsrc, dbdiag, dbrow, ddg, dmap;
    DArr<int> dcnt; DenseWork work; PgoSparseWork swork;
    DArr<PgoCtl> dctl;
    DArr<plba_trace_row> dtrace;
    PgoCtl c0; memset(&c0, 0, sizeof c0);
    c0.lin = 1; c0.c.solver_ok = 1;
    std::vector<PgoCtl> hc0(1, c0);
    {
        DArrStreamScope staged(s, p->have_ctx ? p->ctx.stage : nullptr);      // host vectors above stay alive until the wait below
        HIPCK(p, dX.upload(X)); HIPCK(p, dXs.alloc((size_t)12 * nv)); HIPCK(p, dcnt.alloc(nv));
        HIPCK(p, dZi.upload(he.Zi)); HIPCK(p, dInfo.upload(he.info)); HIPCK(p, dei.upload(he.ei)); HIPCK(p, dej.upload(he.ej));
        HIPCK(p, dEchi.alloc(std::max(ne, 1))); HIPCK(p, dctl.upload(hc0)); HIPCK(p, dtrace.alloc(std::max(trace_cap, 1)));
        if (run) {
            HIPCK(p, dfree.upload(free_v)); HIPCK(p, dbs.upload(blk_start)); HIPCK(p, dbsrc.upload(blk_src));
            HIPCK(p, dbdiag.upload(blk_diag)); HIPCK(p, dbrow.upload(blk_row)); HIPCK(p, ddg.upload(dg_blk));
            if (!sparse) HIPCK(p, dmap.upload(blkmap));
            HIPCK(p, dErec.alloc((size_t)PGO_REC * std::max(ne, 1))); HIPCK(p, dHblk.alloc((size_t)36 * std::max(nblk, 1))); HIPCK(p, db.alloc(P));
            if (sparse) {
                HIPCK(p, xx.alloc(P)); HIPCK(p, swork.upload(plan));
            } else {
                HIPCK(p, sys.alloc(sysn, false)); HIPCK(p, work.alloc(Ppad, ld, ninv_fits(Ppad)));
            }
        }
        HIPCK(p, plba_stream_wait(p, s));
    }
    PgoDev d; memset(&d, 0, sizeof d);
    d.nv = nv; d.ne = ne; d.n = n; d.P = P; d.Ppad = Ppad; d.ld = ld; d.nblk = nblk; d.max_iters = max_iters; d.max_trials = p->opt.max_trials; d.trace_cap = trace_cap;
    d.tau = p->opt.tau; d.lower = p->opt.good_step_lower; d.upper = p->opt.good_step_upper; d.user_lambda = user_lambda_init;
    d.X = dX.p; d.Xs = dXs.p; d.cnt = dcnt.p; d.free_v = dfree.p; d.ei = dei.p; d.ej = dej.p; d.Zi = dZi.p; d.info = dInfo.p;
    d.erec = dErec.p; d.echi = dEchi.p; d.blk_start = dbs.p; d.blk_src = dbsrc.p; d.blk_diag = dbdiag.p; d.blk_row = dbrow.p; d.dg_blk = ddg.p; d.blkmap = dmap.p;
    d.Hblk = dHblk.p; d.b = db.p; d.sys = sys.p; d.x = sparse ? xx.p : work.x.p; d.ctl = dctl.p; d.mail = reinterpret_cast<PgoMail*>(p->d_mail); d.trace = dtrace.p;
    PgoSparseDev sd; memset(&sd, 0, sizeof sd);
    if (sparse && run) {
        swork.bind(sd); sd.Hblk = dHblk.p; sd.b = db.p; sd.x = xx.p; sd.c = &dctl.p->c; sd.done = &dctl.p->done;
        size_t bytes = swork.bytes();
        auto add = [&](const auto& a) { bytes += a.n * sizeof(*a.p); };
        add(dX); add(dXs); add(dcnt); add(dZi); add(dInfo); add(dei); add(dej); add(dEchi); add(dctl); add(dtrace); add(dfree); add(dbs); add(dbsrc);
        add(dbdiag); add(dbrow); add(ddg); add(dErec); add(dHblk); add(db); add(xx);
        pgo_sparse_record(p->pgo_sparse, n, plan, bytes, ms_analysis);
    }
    DevBuf dd; memset(&dd, 0, sizeof dd);
    dd.P = P; dd.Ppad = Ppad; dd.ld = ld; dd.sys = sys.p; dd.ctrl = &dctl.p->c; work.bind(dd, p->opt);

    const dim3 eg((unsigned)((std::max(ne, 1) + 63) / 64)), vg((unsigned)((n + 63) / 64)), bg((unsigned)((std::max(nblk, 1) + 3) / 4)), fg((unsigned)((ld + 255) / 256), (unsigned)(Ppad + TILE));
    if (!run) {
        if (ne > 0) hipLaunchKernelGGL(k_pgo_edges<false>, eg, dim3(64), 0, s, d);
        hipLaunchKernelGGL(k_pgo_chi_only, dim3(1), dim3(256), 0, s, d);
    } else {
        const int max_steps = max_iters * std::max(p->opt.max_trials, 1);
        volatile PgoMail* hm = reinterpret_cast<volatile PgoMail*>(p->h_mail);
        const unsigned long long seq0 = mail_reserve(p, (unsigned long long)max_steps);
        for (int step = 0; step < max_steps; ++step) {
            const unsigned long long seq = seq0 + (unsigned long long)step + 1;
            hipLaunchKernelGGL(k_pgo_edges<true>, eg, dim3(64), 0, s, d);
            hipLaunchKernelGGL(k_pgo_sum, bg, dim3(256), 0, s, d);
            hipLaunchKernelGGL(k_pgo_iter, dim3(1), dim3(256), 0, s, d);
            if (sparse) pgo_sparse_launch(sd, plan, s);
            else {
                hipLaunchKernelGGL(k_pgo_fill, fg, dim3(256), 0, s, d);
                launch_cholesky(dd, p->opt.use_mfma != 0, step + 1, s);      // (not gated: after the run has ended it factors the identity, at most one step of it)
                launch_trsv_back(dd, p->opt.use_mfma != 0, step + 1, s);
            }
            hipLaunchKernelGGL(k_pgo_update, vg, dim3(64), 0, s, d);
            hipLaunchKernelGGL(k_pgo_edges<false>, eg, dim3(64), 0, s, d);
            hipLaunchKernelGGL(k_pgo_decide, dim3(1), dim3(256), 0, s, d, seq);
            HIPCK(p, hipGetLastError());
            // one step behind: has step - 1 ended the run?  (this step is in the queue already; what the mailbox held before is <= seq0)
            if (step > 0) { HIPCK(p, mail_wait(p, s, seq - 1)); if (hm->c.done) break; }
        }
    }
    HIPCK(p, plba_stream_wait(p, s));
    HIPCK(p, hipGetLastError());
    PgoCtl cend;
    HIPCK(p, plba_d2h(p, X.data(), dX.p, (size_t)12 * nv * 8));
    HIPCK(p, plba_d2h(p, &cend, dctl.p, sizeof cend));
    const int nrow = std::min(cend.n_trace, trace_cap);
    if (nrow > 0) HIPCK(p, plba_d2h(p, trace, dtrace.p, (size_t)nrow * sizeof(plba_trace_row)));
    memcpy(g->pose12, X.data(), (size_t)12 * nv * 8);
    memset(out, 0, sizeof *out);
    out->iterations = cend.iters; out->trials = cend.trials; out->stop_reason = cend.stop_reason; out->solver_failures = cend.c.n_fail;
    out->chi2_initial = cend.chi2_initial; out->chi2_final = cend.chi2_final; out->lambda_final = cend.lambda_final;
    out->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_trace) *n_trace = cend.n_trace;
    return PLBA_OK;
}

// Marginal covariances of the graph at g->pose12 (include/plba.h): one linearisation by the kernels above, the multifrontal
// factorisation of plba_pgo_sparse.hip at lambda = 0, the selected inversion of plba_pgo_cov.hip, one read-back.
int plba_pose_graph_marginals(plba_problem* p, const plba_pose_graph* g, plba_pgo_marginals* m) {
    if (!p) return PLBA_ERR_INVALID;
    static const char who[] = "plba_pose_graph_marginals";
    for (double& v : p->pgo_cov) v = 0.0;      // (a refused or failed call leaves an all-zero record)
    p->pgo_cov_H.clear();
    if (!g || !m) FAIL(p, PLBA_ERR_INVALID, "%s: no graph or no request", who);
    const bool want_v = (m->want & 1) != 0, want_p = (m->want & 2) != 0;
    if (!want_v && !want_p) FAIL(p, PLBA_ERR_INVALID, "%s: want = %d asks for nothing", who, m->want);
    if (m->n_pairs < 0) FAIL(p, PLBA_ERR_INVALID, "%s: n_pairs = %d", who, m->n_pairs);
    if ((want_v && !m->v_cov) || (want_p && (!m->pair_cov || (m->n_pairs > 0 && !m->pairs)))) FAIL(p, PLBA_ERR_INVALID, "%s: a requested bit without its buffer", who);
    PgoGraphSetup gs;
    if (int rc = pgo_graph_setup(p, g, who, true, false, gs)) return rc;
    const int nv = g->nv, ne = g->ne, n = gs.n, P = 6 * n, npairs = want_p ? m->n_pairs : 0;
    for (int k = 0; k < npairs; ++k)
        if (m->pairs[2 * k] < 0 || m->pairs[2 * k] >= nv || m->pairs[2 * k + 1] < 0 || m->pairs[2 * k + 1] >= nv) FAIL(p, PLBA_ERR_INVALID, "%s: pair %d names a vertex out of range", who, k);
    const int nblk = (int)gs.blk_row.size();

    // ---- host: the plan, the statuses and the places of the requested blocks --------------------------------------------------------
    PgoSparsePlan plan;
    PgoCovPlan cp;
    double ms_analysis = 0.0;
    if (n > 0) {
        const auto ta = std::chrono::steady_clock::now();
        if (!pgo_sparse_analyse(n, gs.blk_row, gs.blk_col, plan) || !pgo_cov_prepare(plan, cp)) FAIL(p, PLBA_ERR_INTERNAL, "%s: the sparse analysis failed its checks", who);
        ms_analysis = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
    }
    auto vstat = [&](int v) -> uint8_t { return gs.fr[v] >= 0 ? 0 : (g->fixed && g->fixed[v] != 0) ? 1 : 2; };
    const int n_items = (want_v ? nv : 0) + npairs;
    std::vector<uint8_t> status((size_t)std::max(n_items, 1), 0);
    std::vector<PgoCovPlace> places((size_t)std::max(n_items, 1), PgoCovPlace{-1, 0, 0, 0});
    std::vector<int32_t> ranks((size_t)2 * places.size(), 0);
    int32_t n_status[4] = {0, 0, 0, 0};
    for (int v = 0; v < nv; ++v) ++n_status[vstat(v)];
    {
        size_t it = 0;
        if (want_v)
            for (int v = 0; v < nv; ++v, ++it) {
                status[it] = vstat(v);
                if (!status[it]) { places[it] = pgo_cov_locate(plan, cp, gs.fr[v], gs.fr[v]); ranks[2 * it] = ranks[2 * it + 1] = gs.fr[v]; }
            }
        for (int k = 0; k < npairs; ++k, ++it) {
            const int i = m->pairs[2 * k], j = m->pairs[2 * k + 1];
            const uint8_t si = vstat(i), sj = vstat(j);
            if (si == 2 || sj == 2) status[it] = 2;
            else if (si == 1 || sj == 1) status[it] = 1;
            else {
                places[it] = pgo_cov_locate(plan, cp, gs.fr[i], gs.fr[j]);
                ranks[2 * it] = gs.fr[i]; ranks[2 * it + 1] = gs.fr[j];
                if (places[it].front < 0) { status[it] = 3; ++n_status[3]; }
            }
        }
    }
    if (n > 0 && !pgo_cov_check(plan, cp, places, ranks)) FAIL(p, PLBA_ERR_INTERNAL, "%s: the plan of the selected inversion failed its index checks", who);

    // ---- device ------------------------------------------------------------------------------------------------------------------
    HIPCK(p, hipSetDevice(p->device));
    hipStream_t s = p->stream;
    std::vector<double> X(g->pose12, g->pose12 + (size_t)12 * nv);
    const PgoEdges he = pgo_stage_edges(g);      // (these and the block lists go up only with a free vertex, and then none of them is empty)
    std::vector<int32_t> hplace((size_t)4 * places.size());
    for (size_t i = 0; i < places.size(); ++i) { hplace[4 * i] = places[i].front; hplace[4 * i + 1] = places[i].rpos; hplace[4 * i + 2] = places[i].cpos; hplace[4 * i + 3] = places[i].transposed; }
    DArr<double> dX, dZi, dInfo, dErec, dEchi, dHblk, db, dG, dOut;
    DArr<int32_t> dei, dej, dbs, dbsrc, dbdiag, dbrow, dplace, dpar;
    DArr<long long> dgoff; PgoSparseWork swork;
    DArr<uint8_t> dstatus;
    DArr<PgoCtl> dctl;
    DArr<int> drec;
    constexpr size_t HEAD = 32;      // doubles in front of the results: the control block as it stands behind the last launch
    static_assert(sizeof(PgoCtl) <= HEAD * sizeof(double), "the control block fits the head of the read-back");
    PgoCtl c0; memset(&c0, 0, sizeof c0);
    c0.lin = 1; c0.c.solver_ok = 1;      // (lambda = 0: no damping)
    std::vector<PgoCtl> hc0(1, c0);
    std::vector<int> hrec(1, -1);
    {
        // (no wait behind the uploads: the host vectors above live until the read-back below, the call's one blocking wait, has drained the stream)
        DArrStreamScope staged(s, p->have_ctx ? p->ctx.stage : nullptr);
        HIPCK(p, dctl.upload(hc0)); HIPCK(p, drec.upload(hrec)); HIPCK(p, dplace.upload(hplace)); HIPCK(p, dstatus.upload(status));
        HIPCK(p, dOut.alloc(HEAD + (size_t)36 * std::max(n_items, 1), false));
        if (n > 0) {
            HIPCK(p, dX.upload(X)); HIPCK(p, dZi.upload(he.Zi)); HIPCK(p, dInfo.upload(he.info)); HIPCK(p, dei.upload(he.ei)); HIPCK(p, dej.upload(he.ej));
            HIPCK(p, dEchi.alloc(std::max(ne, 1))); HIPCK(p, dErec.alloc((size_t)PGO_REC * std::max(ne, 1)));
            HIPCK(p, dbs.upload(gs.blk_start)); HIPCK(p, dbsrc.upload(gs.blk_src)); HIPCK(p, dbdiag.upload(gs.blk_diag)); HIPCK(p, dbrow.upload(gs.blk_row));
            HIPCK(p, dHblk.alloc((size_t)36 * std::max(nblk, 1))); HIPCK(p, db.alloc(P));
            HIPCK(p, swork.upload(plan)); HIPCK(p, dpar.upload(cp.parent)); HIPCK(p, dgoff.upload(cp.g_off)); HIPCK(p, dG.alloc((size_t)cp.gsize, false));
        }
    }
    PgoDev d; memset(&d, 0, sizeof d);
    d.nv = nv; d.ne = ne; d.n = n; d.P = P; d.nblk = nblk;
    d.X = dX.p; d.ei = dei.p; d.ej = dej.p; d.Zi = dZi.p; d.info = dInfo.p; d.erec = dErec.p; d.echi = dEchi.p;
    d.blk_start = dbs.p; d.blk_src = dbsrc.p; d.blk_diag = dbdiag.p; d.blk_row = dbrow.p; d.Hblk = dHblk.p; d.b = db.p; d.ctl = dctl.p;
    PgoSparseDev sd; memset(&sd, 0, sizeof sd);
    swork.bind(sd); sd.Hblk = dHblk.p; sd.b = db.p; sd.c = &dctl.p->c; sd.done = &dctl.p->done;
    PgoCovDev cd; memset(&cd, 0, sizeof cd);
    cd.parent = dpar.p; cd.g_off = dgoff.p; cd.G = dG.p; cd.n_items = n_items; cd.place = dplace.p; cd.status = dstatus.p; cd.out = dOut.p + HEAD;
    size_t bytes = swork.bytes();
    {
        auto add = [&](const auto& a) { bytes += a.n * sizeof(*a.p); };
        add(dX); add(dZi); add(dInfo); add(dErec); add(dEchi); add(dHblk); add(db); add(dG); add(dOut); add(dei); add(dej); add(dbs);
        add(dbsrc); add(dbdiag); add(dbrow); add(dplace); add(dpar); add(dgoff); add(dstatus); add(dctl); add(drec);
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_pgo_edges<true>, dim3((unsigned)((std::max(ne, 1) + 63) / 64)), dim3(64), 0, s, d);
        hipLaunchKernelGGL(k_pgo_sum, dim3((unsigned)((std::max(nblk, 1) + 3) / 4)), dim3(256), 0, s, d);
        pgo_sparse_launch_assemble(sd, plan, s);
        pgo_sparse_launch_factor_levels(sd, plan, s);
    }
    pgo_cov_launch(sd, cd, plan, s);      // (nothing to invert without a free vertex: the zeros and NaNs of the statuses alone)
    HIPCK(p, hipMemcpyAsync(dOut.p, dctl.p, sizeof(PgoCtl), hipMemcpyDeviceToDevice, s));
    HIPCK(p, hipGetLastError());
    // the one read-back: control block and results together, into host memory; the caller's buffers only after the verdict
    std::vector<double> hall(HEAD + (size_t)36 * std::max(n_items, 1));
    HIPCK(p, plba_d2h(p, hall.data(), dOut.p, hall.size() * 8));
    PgoCtl cend;
    memcpy(&cend, hall.data(), sizeof cend);
    const double* hout = hall.data() + HEAD;
    if (!cend.c.solver_ok) {
        // which front (failure path only): assembled again and factored one front per launch in the order of the levels, in the same
        // arithmetic (a front reads its children alone), with a one-thread note of the first launch behind which solver_ok is 0
        int ef = -1;
        pgo_sparse_launch_assemble(sd, plan, s);
        for (int e = 0; e < plan.nfront; ++e) {
            pgo_sparse_launch_factor(sd, e, 1, s);
            hipLaunchKernelGGL(k_pgo_cov_mark, dim3(1), dim3(1), 0, s, &dctl.p->c, drec.p, e);
        }
        HIPCK(p, hipGetLastError());
        HIPCK(p, plba_d2h(p, &ef, drec.p, sizeof ef));
        if (ef >= 0 && ef < plan.nfront) {
            const int f = plan.lv[ef], npv = plan.f_np[f] / 6;
            const int32_t* rw = plan.rows.data() + plan.f_row0[f];
            FAIL(p, PLBA_ERR_NUMERIC, "%s: a pivot of the factorisation is not > 0 or not finite in front %d of %d (level %d of %d, dimension %d, %d pivot vertices %d .. %d)",
                 who, f, plan.nfront, cp.level[f], plan.nlev, plan.f_m[f], npv, gs.free_v[rw[0]], gs.free_v[rw[npv - 1]]);
        }
        FAIL(p, PLBA_ERR_NUMERIC, "%s: a pivot of the factorisation is not > 0 or not finite (front not identified)", who);
    }
    if ((p->opt.diag & PLBA_DIAG_PGO_COV_DUMP) && n > 0) {      // host copy for plba_debug_get("pgo_cov_H"): read only, the launches are the same
        p->pgo_cov_H.resize((size_t)36 * nblk);
        HIPCK(p, plba_d2h(p, p->pgo_cov_H.data(), dHblk.p, p->pgo_cov_H.size() * 8));
    }
    // ---- every check has passed: the caller's buffers -----------------------------------------------------------------------------
    size_t it0 = 0;
    if (want_v) {
        memcpy(m->v_cov, hout, (size_t)36 * nv * 8);
        if (m->v_status) memcpy(m->v_status, status.data(), (size_t)nv);
        it0 = (size_t)nv;
    }
    if (want_p && npairs > 0) {
        memcpy(m->pair_cov, hout + 36 * it0, (size_t)36 * npairs * 8);
        if (m->pair_status) memcpy(m->pair_status, status.data() + it0, (size_t)npairs);
    }
    for (int i = 0; i < 4; ++i) m->n_status[i] = n_status[i];
    pgo_sparse_record(p->pgo_cov, n, plan, bytes, ms_analysis);
    return PLBA_OK;
}

}  // extern "C"
