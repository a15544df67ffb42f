// plba_pgo_sparse.hip — the multifrontal solve of plba_optimize_pose_graph's sparse path (options.pgo_solver = 1); the host analysis,
// the layout and the kernel sequence are described in plba_pgo_sparse.h; PgoSparseDev and the launchers are declared in plba_pgo_sparse_dev.h.
// One workgroup of 256 per front.  A frontal matrix lives in global memory (L2-resident for the fronts of a keyframe chain; fronts of
// any size, a fully connected graph's included, take the same path).  Every entry has one owner and every sum a fixed order: the
// extend-add runs child by child with a barrier between, the pivot columns and the trailing update F22 - L21 L21^T sum over k in
// column order on the matrix cores (v_mfma_f64_16x16x4_f64, one wave per 16 x 16 tile).  No floating-point atomics.
// Every kernel returns at once after the run has ended (PgoCtl::done).
#include <cmath>

#include "plba_pgo_sparse_dev.h"

namespace plba {
namespace {

constexpr int SPT = 256;
typedef double double4v __attribute__((ext_vector_type(4)));

// column-major frontal matrix: entry (r, c), r >= c
#define FX(F, m, r, c) (F)[(long long)(c) * (m) + (r)]

// zero the lower triangle, the Hblk blocks the front owns (transposed where the elimination order puts the column vertex first),
// lambda on the diagonal (as k_pgo_fill: Hblk entry + lambda), b on the pivot rows
__global__ __launch_bounds__(SPT) void k_sps_assemble(PgoSparseDev d) {
    if (*d.done) return;
    const int f = blockIdx.x, m = d.f_m[f], np = d.f_np[f];
    if (f == 0 && threadIdx.x == 0) d.c->solver_ok = 1;
    double* F = d.F + d.f_off[f];
    double* R = d.R + d.f_roff[f];
    const int32_t* rw = d.rows + d.f_row0[f];
    for (long long t = threadIdx.x; t < (long long)m * m; t += SPT)
        if (t % m >= t / m) F[t] = 0.0;
    for (int t = threadIdx.x; t < m; t += SPT) R[t] = t < np ? d.b[6 * rw[t / 6] + t % 6] : 0.0;
    __syncthreads();
    const double lam = d.c->lambda;
    const int a0 = d.as_start[f], na = d.as_start[f + 1] - a0;
    for (int t = threadIdx.x; t < 36 * na; t += SPT) {
        const int32_t* e = d.as + 3 * (a0 + t / 36);
        const int l = t % 36, i = l / 6, j = l % 6;
        if (e[1] == e[2] && i < j) continue;
        int r = 6 * e[1] + i, c = 6 * e[2] + j;
        if (r < c) { const int q = r; r = c; c = q; }
        double v = d.Hblk[(long long)36 * e[0] + l];
        if (r == c) v += lam;
        FX(F, m, r, c) = v;
    }
}

// one level of the tree, bottom-up: extend-add, partial Cholesky of the np pivot columns (right-hand side carried along), F22 - L21 L21^T
__global__ __launch_bounds__(SPT) void k_sps_factor(PgoSparseDev d, int l0) {
    if (*d.done) return;
    const int f = d.lv[l0 + blockIdx.x], m = d.f_m[f], np = d.f_np[f];
    double* __restrict__ F = d.F + d.f_off[f];
    double* __restrict__ R = d.R + d.f_roff[f];
    for (int q = d.ch_start[f]; q < d.ch_start[f + 1]; ++q) {      // children in their fixed order
        const int c = d.ch[q], mc = d.f_m[c], npc = d.f_np[c], nu = mc - npc;
        const double* __restrict__ Fc = d.F + d.f_off[c];
        const double* __restrict__ Rc = d.R + d.f_roff[c];
        const int32_t* um = d.umap + d.f_row0[c] + npc / 6;
        for (long long t = threadIdx.x; t < (long long)nu * nu; t += SPT) {
            const int a = (int)(t % nu), bb = (int)(t / nu);
            if (a < bb) continue;
            const int pa = 6 * um[a / 6] + a % 6, pb = 6 * um[bb / 6] + bb % 6;      // (the map is increasing: pa > pb)
            FX(F, m, pa, pb) += FX(Fc, mc, npc + a, npc + bb);
        }
        for (int a = threadIdx.x; a < nu; a += SPT) R[6 * um[a / 6] + a % 6] += Rc[npc + a];
        __syncthreads();
    }
    // left-looking over the pivot columns, one vertex (6 columns) at a time: the block's columns less L(:, 0:j0) L(j0:j0+6, 0:j0)^T on
    // the matrix cores (v_mfma_f64_16x16x4_f64: a wave per 16-row tile, B = the block's 6 rows padded to 16, k in column order); the
    // 6 x 6 diagonal block is factored by every thread alike (from LDS), the rows below solved against it by their owners; the
    // right-hand side takes the previous block's update on the way (y = L^-1 b)
    __shared__ double s_blk[36], s_r[6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    for (int j0 = 0; j0 < np; j0 += 6) {
        for (int t = wv; t < (m - j0 + 15) / 16; t += SPT / 64) {
            const int ra = j0 + 16 * t + li;
            double4v acc = (double4v){0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < j0; k0 += 4) {
                const int k = k0 + lk;
                const double av = (ra < m && k < j0) ? FX(F, m, ra, k) : 0.0;
                const double bv = (li < 6 && k < j0) ? FX(F, m, j0 + li, k) : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {      // result (row lk + 4 v, column li) of the tile
                const int i = j0 + 16 * t + lk + 4 * v;
                if (li >= 6 || i >= m || li > i - j0) continue;
                const double val = FX(F, m, i, j0 + li) - acc[v];
                if (i < j0 + 6) s_blk[(i - j0) * 6 + li] = val;
                else FX(F, m, i, j0 + li) = val;
            }
        }
        for (int i = j0 + threadIdx.x; i < m; i += SPT) {
            double r = R[i];
            if (j0 > 0)
#pragma unroll
                for (int c = 0; c < 6; ++c) r -= FX(F, m, i, j0 - 6 + c) * R[j0 - 6 + c];
            if (i < j0 + 6) s_r[i - j0] = r;
            else R[i] = r;
        }
        __syncthreads();
        double Lb[36], y[6];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 6; ++c) {      // Cholesky of the diagonal block, forward substitution of its right-hand side
            double dcc = s_blk[c * 6 + c];
            for (int q = 0; q < c; ++q) dcc -= Lb[c * 6 + q] * Lb[c * 6 + q];
            bad = bad || !(dcc > 0.0) || !isfinite(dcc);
            const double lcc = sqrt(dcc);
            Lb[c * 6 + c] = lcc;
            for (int r = c + 1; r < 6; ++r) {
                double v = s_blk[r * 6 + c];
                for (int q = 0; q < c; ++q) v -= Lb[r * 6 + q] * Lb[c * 6 + q];
                Lb[r * 6 + c] = v / lcc;
            }
            double v = s_r[c];
            for (int q = 0; q < c; ++q) v -= Lb[c * 6 + q] * y[q];
            y[c] = v / lcc;
        }
        if (bad) {      // (uniform: every thread factored the same block)
            if (threadIdx.x == 0) d.c->solver_ok = 0;
            return;
        }
        for (int i = j0 + threadIdx.x; i < m; i += SPT) {
            if (i < j0 + 6) {      // (static register indices: the row is selected, not indexed)
#pragma unroll
                for (int r = 0; r < 6; ++r)
                    if (r == i - j0) {
#pragma unroll
                        for (int c = 0; c <= r; ++c) FX(F, m, i, j0 + c) = Lb[r * 6 + c];
                        R[i] = y[r];
                    }
            } else {
                double l[6];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    double v = FX(F, m, i, j0 + c);
                    for (int q = 0; q < c; ++q) v -= l[q] * Lb[c * 6 + q];
                    l[c] = v / Lb[c * 6 + c];
                    FX(F, m, i, j0 + c) = l[c];
                }
            }
        }
        __syncthreads();
    }
    if (np > 0)      // the last block's update of the right-hand side's update rows
        for (int i = np + threadIdx.x; i < m; i += SPT) {
            double r = R[i];
#pragma unroll
            for (int c = 0; c < 6; ++c) r -= FX(F, m, i, np - 6 + c) * R[np - 6 + c];
            R[i] = r;
        }
    // F22 -= L21 L21^T on the matrix cores: a wave per 16 x 16 tile of the lower triangle, k over the pivot columns in order
    const int nu = m - np, nt = (nu + 15) / 16;
    for (int t = wv; t < nt * (nt + 1) / 2; t += SPT / 64) {
        int ti = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (ti * (ti + 1) / 2 > t) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        const int tj = t - ti * (ti + 1) / 2, ra = 16 * ti + li, rb = 16 * tj + li;
        double4v acc = (double4v){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < np; k0 += 4) {
            const int k = k0 + lk;
            const double av = (ra < nu && k < np) ? FX(F, m, np + ra, k) : 0.0;
            const double bv = (rb < nu && k < np) ? FX(F, m, np + rb, k) : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int a = 16 * ti + lk + 4 * v, bb = rb;
            if (a < nu && a >= bb) FX(F, m, np + a, np + bb) -= acc[v];
        }
    }
}

// one level, top-down: L11^T x1 = y1 - L21^T x2 (x2 from the ancestors, in free-vertex order in d.x); nothing after a failed factorisation
__global__ __launch_bounds__(SPT) void k_sps_back(PgoSparseDev d, int l0) {
    if (*d.done || !d.c->solver_ok) return;
    const int f = d.lv[l0 + blockIdx.x], m = d.f_m[f], np = d.f_np[f];
    const double* F = d.F + d.f_off[f];
    double* R = d.R + d.f_roff[f];
    const int32_t* rw = d.rows + d.f_row0[f];
    for (int i = threadIdx.x; i < np; i += SPT) {
        double acc = R[i];
        for (int a = np; a < m; ++a) acc -= FX(F, m, a, i) * d.x[6 * rw[a / 6] + a % 6];
        R[i] = acc;
    }
    __syncthreads();
    for (int j0 = np - 6; j0 >= 0; j0 -= 6) {      // a vertex at a time: every thread solves the 6 x 6 block alike, owners update above
        double x[6];
#pragma unroll
        for (int c = 5; c >= 0; --c) {
            double v = R[j0 + c];
            for (int r = c + 1; r < 6; ++r) v -= FX(F, m, j0 + r, j0 + c) * x[r];
            x[c] = v / FX(F, m, j0 + c, j0 + c);
        }
        for (int q = threadIdx.x; q < j0; q += SPT) {
            double v = R[q];
#pragma unroll
            for (int c = 0; c < 6; ++c) v -= FX(F, m, j0 + c, q) * x[c];
            R[q] = v;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) if ((int)threadIdx.x == c) d.x[6 * rw[j0 / 6] + c] = x[c];
        __syncthreads();
    }
}

#undef FX

}  // namespace

void pgo_sparse_launch_assemble(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s) {
    hipLaunchKernelGGL(k_sps_assemble, dim3((unsigned)pl.nfront), dim3(SPT), 0, s, d);
}

void pgo_sparse_launch_factor(const PgoSparseDev& d, int l0, int count, hipStream_t s) {
    hipLaunchKernelGGL(k_sps_factor, dim3((unsigned)count), dim3(SPT), 0, s, d, l0);
}

void pgo_sparse_launch_factor_levels(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s) {
    for (int l = 0; l < pl.nlev; ++l) pgo_sparse_launch_factor(d, pl.lv_start[l], pl.lv_start[l + 1] - pl.lv_start[l], s);
}

void pgo_sparse_launch(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s) {
    pgo_sparse_launch_assemble(d, pl, s);
    pgo_sparse_launch_factor_levels(d, pl, s);
    for (int l = pl.nlev - 1; l >= 0; --l)
        hipLaunchKernelGGL(k_sps_back, dim3((unsigned)(pl.lv_start[l + 1] - pl.lv_start[l])), dim3(SPT), 0, s, d, pl.lv_start[l]);
}

}  // namespace plba
