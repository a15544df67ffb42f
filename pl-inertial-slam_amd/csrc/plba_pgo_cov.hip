// plba_pgo_cov.hip — the selected inversion behind plba_pose_graph_marginals: the mirror image of k_sps_factor (plba_pgo_sparse.hip).
// After the factorisation the fronts hold L; the levels are run again top-down and every front's storage is turned in place into the
// entries of H^-1 on the pattern of L (Takahashi's recurrence; the layout and the host side are in plba_pgo_cov.h).
// One workgroup of 256 per front, fronts of any size.  Every entry has one owner and every sum a fixed order: the hot product Z_SS G
// runs on the matrix cores (v_mfma_f64_16x16x4_f64, a wave per 16-row tile of S, the six columns of G padded to 16, k over S in
// increasing order), the 6 x 6 pieces are computed by every thread alike.  No floating-point atomics.
// Both kernels return at once after a failed factorisation (Ctrl::solver_ok = 0).
#include <cmath>

#include "plba_internal.h"
#include "plba_pgo_cov.h"
#include "plba_pgo_sparse_dev.h"

namespace plba {
namespace {

constexpr int SPT = 256;
constexpr int NPART = SPT / 36;      // 7 partial sums per entry of G^T Z_Sj
typedef double double4v __attribute__((ext_vector_type(4)));

// column-major frontal matrix: entry (r, c), r >= c
#define FX(F, m, r, c) (F)[(long long)(c) * (m) + (r)]

// one level of the tree, top-down
__global__ __launch_bounds__(SPT) void k_sps_selinv(PgoSparseDev d, PgoCovDev cv, int l0) {
    if (*d.done || !d.c->solver_ok) return;
    const int f = d.lv[l0 + blockIdx.x], m = d.f_m[f], np = d.f_np[f], nu = m - np;
    double* __restrict__ F = d.F + d.f_off[f];
    double* __restrict__ G = cv.G + cv.g_off[f];
    if (nu > 0) {      // Z22 from the parent, whose lower triangle is complete (the map is increasing: lower maps to lower)
        const int pr = cv.parent[f], mp = d.f_m[pr];
        const double* __restrict__ Fp = d.F + d.f_off[pr];
        const int32_t* um = d.umap + d.f_row0[f] + np / 6;
        for (long long t = threadIdx.x; t < (long long)nu * nu; t += SPT) {
            const int a = (int)(t % nu), bb = (int)(t / nu);
            if (a < bb) continue;
            FX(F, m, np + a, np + bb) = FX(Fp, mp, 6 * um[a / 6] + a % 6, 6 * um[bb / 6] + bb % 6);
        }
        __syncthreads();
    }
    __shared__ double s_L[36], s_part[NPART][36];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    for (int j0 = np - 6; j0 >= 0; j0 -= 6) {      // the pivot vertices, last to first; S = the rows s0 .. m - 1
        const int s0 = j0 + 6, ns = m - s0;
        if (threadIdx.x < 36) { const int r = threadIdx.x / 6, c = threadIdx.x % 6; s_L[threadIdx.x] = r >= c ? FX(F, m, j0 + r, j0 + c) : 0.0; }
        __syncthreads();
        double W[36];      // L_jj^-1 (lower), by every thread alike
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                if (r < c) { W[r * 6 + c] = 0.0; continue; }
                double v = r == c ? 1.0 : 0.0;
#pragma unroll
                for (int k = c; k < r; ++k) v -= s_L[r * 6 + k] * W[k * 6 + c];
                W[r * 6 + c] = v / s_L[r * 6 + r];
            }
        for (int i = threadIdx.x; i < ns; i += SPT) {      // G = L_Sj L_jj^-1, a row per owner
            double l[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) l[k] = FX(F, m, s0 + i, j0 + k);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double v = 0.0;
#pragma unroll
                for (int k = c; k < 6; ++k) v += l[k] * W[k * 6 + c];
                G[(long long)i * 6 + c] = v;
            }
        }
        __syncthreads();
        // Z_Sj = - Z_SS G over L_Sj: Z_SS is a lower triangle, an entry above the diagonal is read at its transposed place
        for (int t = wv; t < (ns + 15) / 16; t += SPT / 64) {
            const int ra = s0 + 16 * t + li;
            double4v acc = (double4v){0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < ns; k0 += 4) {
                const int k = k0 + lk, ck = s0 + k;
                double av = 0.0, bv = 0.0;
                if (ra < m && k < ns) av = ra >= ck ? FX(F, m, ra, ck) : FX(F, m, ck, ra);
                if (li < 6 && k < ns) bv = G[(long long)k * 6 + li];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {      // result (row lk + 4 v, column li) of the tile
                const int i = 16 * t + lk + 4 * v;
                if (li < 6 && i < ns) FX(F, m, s0 + i, j0 + li) = -acc[v];
            }
        }
        __syncthreads();
        // G^T Z_Sj (lower triangle): NPART partial sums per entry, each over its rows of S in increasing order, then summed in order
        if (threadIdx.x < 36 * NPART) {
            const int e = threadIdx.x % 36, part = threadIdx.x / 36, a = e / 6, b = e % 6;
            double v = 0.0;
            if (a >= b) for (int k = part; k < ns; k += NPART) v += G[(long long)k * 6 + a] * FX(F, m, s0 + k, j0 + b);
            s_part[part][e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {      // Z_jj = L_jj^-T L_jj^-1 - G^T Z_Sj, by every thread alike; entry (a, b) stored by thread 6 a + b
                double v = 0.0, g = 0.0;
#pragma unroll
                for (int k = a; k < 6; ++k) v += W[k * 6 + a] * W[k * 6 + b];
#pragma unroll
                for (int q = 0; q < NPART; ++q) g += s_part[q][a * 6 + b];
                if ((int)threadIdx.x == a * 6 + b) FX(F, m, j0 + a, j0 + b) = v - g;
            }
        __syncthreads();
    }
}

// the requested blocks from their places: a thread per entry; diagonal blocks mirrored, pair blocks transposed where the stored one is (j, i)
__global__ __launch_bounds__(SPT) void k_sps_covout(PgoSparseDev d, PgoCovDev cv) {
    if (*d.done || !d.c->solver_ok) return;
    const long long t = (long long)blockIdx.x * SPT + threadIdx.x;
    if (t >= 36LL * cv.n_items) return;
    const int it = (int)(t / 36), l = (int)(t % 36);
    const int st = cv.status[it];
    double v = 0.0;
    if (st >= 2) v = __builtin_nan("");
    else if (st == 0) {
        const int32_t* pc = cv.place + 4 * (long long)it;
        int a = l / 6, b = l % 6;
        if (pc[3]) { const int q = a; a = b; b = q; }
        int r = 6 * pc[1] + a, c = 6 * pc[2] + b;
        if (r < c) { const int q = r; r = c; c = q; }      // (a diagonal block: one triangle is stored)
        v = FX(d.F + d.f_off[pc[0]], d.f_m[pc[0]], r, c);
    }
    cv.out[t] = v;
}

#undef FX

}  // namespace

void pgo_cov_launch(const PgoSparseDev& d, const PgoCovDev& c, const PgoSparsePlan& pl, hipStream_t s) {
    for (int l = pl.nlev - 1; l >= 0; --l)
        hipLaunchKernelGGL(k_sps_selinv, dim3((unsigned)(pl.lv_start[l + 1] - pl.lv_start[l])), dim3(SPT), 0, s, d, c, pl.lv_start[l]);
    if (c.n_items > 0) hipLaunchKernelGGL(k_sps_covout, dim3((unsigned)((36LL * c.n_items + SPT - 1) / SPT)), dim3(SPT), 0, s, d, c);
}

}  // namespace plba
