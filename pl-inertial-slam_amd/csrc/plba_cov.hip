// plba_cov.hip — marginal covariances of keyframes and landmarks at the current estimate (plba_compute_marginals).
//
// Nothing of the LM state is written: every launch below reads the estimates, the observations and the pose-side structure
// of the problem and writes scratch buffers of this call only.
//   1. pose side: the IMU / prior edges (k_pose_edges, k_prior of plba_kernels.hip) into a scratch accumulator, + Hconst
//   2. k_cov_lm: per landmark, its active edges relinearised (point_edge / line_edge, the LM's Huber weights and levels),
//      the undamped Hll reduced to the landmark's coordinates (points: xyz; lines: the 4-dimensional subspace B orthogonal
//      to the line at both endpoints), its Cholesky factor Lr, and per observation  H_a = Jp^T w Jp,  Y_a = W_a Lr^-T
//   3. k_cov_pairs: S = Hpp - sum Hpl Hr^-1 Hlp, one workgroup per pose block, entries summed in a fixed order
//   4. S = L L^T with the explicit inverse N = L^-T: the dense fp64 MFMA factorisation of plba_dense.hip (k_chol32 with its
//      identity rows), whose last block step k_cov_nlast completes; k_cov_pivots: the positive-definiteness test against S's
//      diagonal; k_cov_syrk: Sigma_pp = N N^T on the matrix cores
//   5. k_cov_landmark: Sigma_ll = B Lr^-T (I + sum_ab Y_a^T Sigma(a, b) Y_b) Lr^-1 B^T
//   6. k_cov_gather: keyframe / pair blocks in slot order into one buffer, read back once.
// Bit-reproducible: the new kernels use no floating-point atomics (every output element has one writer and a fixed summation
// order); the reused k_pose_edges accumulates with atomicAdd, but onto zero and at most two adds per address, whose sum does not
// depend on their order.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "plba_problem.h"

namespace plba {

#define CDEV __device__ __forceinline__

namespace {

typedef double double4v __attribute__((ext_vector_type(4)));
constexpr int CB = 32;         // block width of the dense factorisation (k_chol32)
constexpr int REC = 60;        // per observation: H_a (6 x 6) | Y_a (6 x 4)
constexpr int LMREC = 40;      // per landmark: Lr^-1 (4 x 4) | B (6 x 4)
constexpr double PIV_REL = 1e-12;     // a landmark's reduced Hll is degenerate below this pivot / largest diagonal
constexpr double S_PIV_REL = 1e-14;   // the pose system is not positive definite below this pivot / its diagonal entry

CDEV int pmap(int r) { return r < 3 ? r : r + 3; }      // (dp, dphi) row of an observation Jacobian -> PVR tangent index (dp dv dphi)

// one observation at the current estimate: returns false when the edge is not active (level != 0)
CDEV bool cov_edge(const DevBuf& d, int state, const Robust& rb, int e, double jl[2][6], double jp[2][6], double& w) {
    if (d.ob_level[e] != 0) return false;
    const double* L = d.lm[state] + (size_t)d.ob_slot[e] * 6;
    double kc[KFCAM_STRIDE];
    kfcam_make(d.cam, d.kf[state] + (size_t)d.ob_kf[e] * KF_STRIDE, kc);
    double e2[2], Jp[12], Jl[6];
    bool dpos;
    const bool is_pt = e < d.Ep;
    if (is_pt) point_edge(d.cam, kc, v3(L[0], L[1], L[2]), d.po_uv[2 * (size_t)e], d.po_uv[2 * (size_t)e + 1], e2, Jp, Jl, dpos, true);
    else {
        const double* l = d.lo_l + (size_t)(e - d.Ep) * 3;
        line_edge(d.cam, kc, v3(L[0], L[1], L[2]), v3(L[3], L[4], L[5]), l[0], l[1], l[2], d.fix_q1 != 0, e2, Jp, Jl, dpos, true);
    }
    const double w0 = d.ob_w[e];
    const double chi = w0 * (e2[0] * e2[0] + e2[1] * e2[1]);
    const int kind = is_pt ? PLBA_EDGE_POINT : PLBA_EDGE_LINE;
    double r0 = chi, r1 = 1.0;
    if (rb.on[kind]) huber(chi, rb.delta[kind], r0, r1);
    w = w0 * r1;
    for (int i = 0; i < 2; ++i)
        for (int c = 0; c < 6; ++c) { jp[i][c] = Jp[i * 6 + c]; jl[i][c] = 0.0; }
    if (is_pt) { for (int i = 0; i < 2; ++i) for (int c = 0; c < 3; ++c) jl[i][c] = Jl[i * 3 + c]; }
    else { for (int c = 0; c < 3; ++c) { jl[0][c] = Jl[c]; jl[1][3 + c] = Jl[3 + c]; } }
    return true;
}

// ---- 2. landmark elimination (one thread per landmark slot) -------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cov_lm(DevBuf d, int state, Robust rb, double* __restrict__ rec, double* __restrict__ lmrec, int* __restrict__ stat) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= d.L) return;
    const bool is_pt = l < d.Np;
    const int nd = is_pt ? 3 : 6, r = is_pt ? 3 : 4;
    const int e0 = d.lm_start[l], e1 = d.lm_start[l + 1];
    double H[6][6];
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) H[a][b] = 0.0;
    int nact = 0;
    double jl[2][6], jp[2][6], w;
    for (int e = e0; e < e1; ++e) {
        if (!cov_edge(d, state, rb, e, jl, jp, w)) continue;
        ++nact;
        for (int a = 0; a < nd; ++a)
            for (int b = 0; b < nd; ++b) H[a][b] += w * (jl[0][a] * jl[0][b] + jl[1][a] * jl[1][b]);
    }
    int st = d.lm_fixed[l] ? 1 : (nact < 2 ? 2 : 0);
    double B[6][4], Li[4][4];
    for (int a = 0; a < 6; ++a) for (int q = 0; q < 4; ++q) B[a][q] = 0.0;
    for (int a = 0; a < 4; ++a) for (int q = 0; q < 4; ++q) Li[a][q] = 0.0;
    if (st == 0) {
        if (is_pt) { for (int a = 0; a < 3; ++a) B[a][a] = 1.0; }
        else {      // N: orthonormal basis of the plane orthogonal to the line direction, the same at both endpoints
            const double* X = d.lm[state] + (size_t)d.ob_slot[e0] * 6;
            V3 dv = v3(X[3] - X[0], X[4] - X[1], X[5] - X[2]);
            const double dn = sqrt(dv.x * dv.x + dv.y * dv.y + dv.z * dv.z);
            dv = v3(dv.x / dn, dv.y / dn, dv.z / dn);
            const double ax = fabs(dv.x), ay = fabs(dv.y), az = fabs(dv.z);
            const V3 a = (ax <= ay && ax <= az) ? v3(1, 0, 0) : (ay <= az ? v3(0, 1, 0) : v3(0, 0, 1));
            V3 n1 = cross(dv, a);
            const double n1n = sqrt(n1.x * n1.x + n1.y * n1.y + n1.z * n1.z);
            n1 = v3(n1.x / n1n, n1.y / n1n, n1.z / n1n);
            const V3 n2 = cross(dv, n1);
            const double N[3][2] = {{n1.x, n2.x}, {n1.y, n2.y}, {n1.z, n2.z}};
            for (int c = 0; c < 3; ++c) for (int q = 0; q < 2; ++q) { B[c][q] = N[c][q]; B[3 + c][2 + q] = N[c][q]; }
        }
        double Hr[4][4], HB[6][4];
        for (int a = 0; a < nd; ++a)
            for (int q = 0; q < r; ++q) { double s = 0.0; for (int c = 0; c < nd; ++c) s += H[a][c] * B[c][q]; HB[a][q] = s; }
        double dmax = 0.0;
        for (int p = 0; p < r; ++p)
            for (int q = 0; q < r; ++q) { double s = 0.0; for (int a = 0; a < nd; ++a) s += B[a][p] * HB[a][q]; Hr[p][q] = s; }
        for (int p = 0; p < r; ++p) dmax = fmax(dmax, Hr[p][p]);
        double Lr[4][4];
        for (int p = 0; p < 4; ++p) for (int q = 0; q < 4; ++q) Lr[p][q] = 0.0;
        for (int j = 0; j < r && st == 0; ++j) {
            double piv = Hr[j][j];
            for (int t = 0; t < j; ++t) piv -= Lr[j][t] * Lr[j][t];
            if (!(piv > PIV_REL * dmax)) { st = 3; break; }
            Lr[j][j] = sqrt(piv);
            for (int i = j + 1; i < r; ++i) {
                double s = Hr[i][j];
                for (int t = 0; t < j; ++t) s -= Lr[i][t] * Lr[j][t];
                Lr[i][j] = s / Lr[j][j];
            }
        }
        if (st == 0)
            for (int c = 0; c < r; ++c) {      // column c of Lr^-1 (forward substitution)
                Li[c][c] = 1.0 / Lr[c][c];
                for (int i = c + 1; i < r; ++i) {
                    double s = 0.0;
                    for (int t = c; t < i; ++t) s += Lr[i][t] * Li[t][c];
                    Li[i][c] = -s / Lr[i][i];
                }
            }
    }
    stat[l] = st;
    double* lr = lmrec + (size_t)l * LMREC;
    for (int p = 0; p < 4; ++p) for (int q = 0; q < 4; ++q) lr[p * 4 + q] = Li[p][q];
    for (int a = 0; a < 6; ++a) for (int q = 0; q < 4; ++q) lr[16 + a * 4 + q] = B[a][q];
    for (int e = e0; e < e1; ++e) {
        double* o = rec + (size_t)e * REC;
        const bool use = (st == 0 || st == 1) && d.kf_off_pvr[d.ob_kf[e]] >= 0 && cov_edge(d, state, rb, e, jl, jp, w);
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) o[a * 6 + b] = use ? w * (jp[0][a] * jp[0][b] + jp[1][a] * jp[1][b]) : 0.0;
        double Wm[6][4];
        for (int a = 0; a < 6; ++a)
            for (int q = 0; q < 4; ++q) {
                double s = 0.0;
                if (use && st == 0 && q < r)
                    for (int i = 0; i < 2; ++i) { double jb = 0.0; for (int c = 0; c < nd; ++c) jb += jl[i][c] * B[c][q]; s += jp[i][a] * jb; }
                Wm[a][q] = w * s;
            }
        for (int a = 0; a < 6; ++a)
            for (int q = 0; q < 4; ++q) {      // Y = W Lr^-T
                double s = 0.0;
                for (int t = 0; t <= q; ++t) s += Wm[a][t] * Li[q][t];
                o[36 + a * 4 + q] = (use && st == 0) ? s : 0.0;
            }
    }
}

// ---- 1 + 3. the pose system --------------------------------------------------------------------------------------------------
// S (rows < Ppad of the augmented Ppad x ld system the dense factorisation takes; its right-hand-side rows stay zero) and the
// diagonal of S before the factorisation (the positive-definiteness test)
__global__ void k_cov_init(const double* __restrict__ Himu, const double* __restrict__ Hconst, int P, int ldh, double* __restrict__ S, int Pp, double* __restrict__ d0) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)Pp * Pp) return;
    const int r = (int)(t / Pp), c = (int)(t % Pp);
    const int a = r >= c ? r : c, b = r >= c ? c : r;      // (the lower triangle's value in both: S exactly symmetric, as the factorisation reads both)
    const double v = (r < P && c < P) ? Himu[(size_t)a * ldh + b] + Hconst[(size_t)a * ldh + b] : (r == c ? 1.0 : 0.0);
    S[t] = v;
    if (r == c) d0[r] = v;
}
// blk: [oi, oj, first entry, end entry] per pose block (oi >= oj); ent: observation pairs (a, b), kf(a) owns oi, kf(b) owns oj
__global__ __launch_bounds__(64) void k_cov_pairs(const int32_t* __restrict__ blk, const int32_t* __restrict__ ent, const double* __restrict__ rec, double* __restrict__ S, int Pp,
                                                  double* __restrict__ d0) {
    const int4 bk = reinterpret_cast<const int4*>(blk)[blockIdx.x];
    const int t = threadIdx.x;
    if (t >= 36) return;
    const int r = t / 6, c = t % 6;
    if (bk.x == bk.y && c > r) return;      // lower triangle only
    double s = 0.0;
    for (int q = bk.z; q < bk.w; ++q) {
        const int a = ent[2 * q], b = ent[2 * q + 1];
        const double* ya = rec + (size_t)a * REC + 36 + r * 4;
        const double* yb = rec + (size_t)b * REC + 36 + c * 4;
        if (a == b) s += rec[(size_t)a * REC + r * 6 + c];
        s -= ya[0] * yb[0] + ya[1] * yb[1] + ya[2] * yb[2] + ya[3] * yb[3];
    }
    const int gr = bk.x + pmap(r), gc = bk.y + pmap(c);
    const size_t o = (size_t)gr * Pp + gc;
    S[o] += s;
    if (gr != gc) S[(size_t)gc * Pp + gr] = S[o];      // the mirror: no other workgroup writes it
    if (bk.x == bk.y && r == c) d0[bk.x + pmap(r)] = S[o];
}

// ---- 4. S = L L^T with N = L^-T (plba_dense.hip: k_chol32 with the identity rows, launch_cholesky), Sigma_pp = N N^T ---------
// The factorisation launches leave row block j of N in Ninv from column block j on, for every block but the last; its last block
// step (panels only) is the one k_back_gemv folds into the back-substitution.  Here it is completed explicitly:
//   N(c, T) = R(c, T) M^T  (R: the row's unsolved last block in Nwork, M = L(T,T)^-1 as published in Linv32),  N(T, T) = M^T.
__global__ __launch_bounds__(256) void k_cov_nlast(DevBuf d) {
    const int c0 = d.Ppad - CB;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)d.Ppad * CB) return;
    const int c = (int)(t / CB), j = (int)(t % CB);
    const double* M = d.Linv32 + (size_t)(c0 / CB) * CB * CB;
    double v;
    if (c < c0) {
        const double* R = d.Nwork + (size_t)c * d.ld + c0;
        v = 0.0;
        for (int q = 0; q <= j; ++q) v = fma(R[q], M[j * CB + q], v);      // (M lower triangular)
    } else v = c - c0 <= j ? M[j * CB + (c - c0)] : 0.0;
    d.Ninv[(size_t)c * d.ld + c0 + j] = v;
}
// The first free dimension whose pivot L_jj^2 = 1 / M_jj^2 is not above S_PIV_REL x S_jj (or that the factorisation flagged); P: none
__global__ __launch_bounds__(256) void k_cov_pivots(DevBuf d, const double* __restrict__ d0, int* __restrict__ fail) {
    // (a dimension without any constraint has a zero row: named exactly by its zero diagonal entry; the factorisation replaces a failed
    // pivot by 1 and goes on, so the pivots that follow it in its tile are not meaningful)
    __shared__ int sz, sf;
    if (threadIdx.x == 0) { sz = INT_MAX; sf = INT_MAX; }
    __syncthreads();
    int fz = INT_MAX, f = INT_MAX;
    for (int j = threadIdx.x; j < d.P; j += blockDim.x) {
        const double m = d.Linv32[(size_t)(j / CB) * CB * CB + (j % CB) * (CB + 1)];
        const double piv = 1.0 / (m * m);
        if (!(d0[j] > 0.0)) fz = min(fz, j);
        if (!(piv > S_PIV_REL * d0[j]) || !(piv > 0.0) || !(piv < INFINITY)) f = min(f, j);
    }
    atomicMin(&sz, fz);
    atomicMin(&sf, f);
    __syncthreads();
    if (threadIdx.x == 0) *fail = sz != INT_MAX ? sz : sf != INT_MAX ? sf : (d.ctrl->solver_ok ? -1 : d.P);
}
// Sigma(i, j) = sum_{k >= i} N(i, k) N(j, k)^T for the 32 x 32 tiles j <= i, on the matrix cores (v_mfma_f64_16x16x4_f64): wave
// (tr, tc) forms the 16 x 16 quadrant rows tr, columns tc.  A[m][kk] = N[row_i + m][k0 + kk], B[kk][n] = N[row_j + n][k0 + kk]:
// lane l supplies row l & 15, k index l >> 4 (cdna_hip_programming.md, the 16x16x4 f64 operand maps); D: row (l >> 4) + 4 v,
// column l & 15.  N(i, k) is read only from column block i on, where Ninv holds it (upper triangular, zeros below the diagonal).
// Written to both triangles; a diagonal tile's element and its mirror come from the same lane (one writer per address).
__global__ __launch_bounds__(256) void k_cov_syrk(const double* __restrict__ N, int ld, int Pp, double* __restrict__ Sig) {
    const int i = blockIdx.y, j = blockIdx.x;
    if (j > i) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4, tr = wv >> 1, tc = wv & 1;
    const double* Ar = N + (size_t)(i * CB + tr * 16 + li) * ld;
    const double* Br = N + (size_t)(j * CB + tc * 16 + li) * ld;
    double4v acc = (double4v){0.0, 0.0, 0.0, 0.0};
    for (int k0 = i * CB; k0 < Pp; k0 += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ar[k0 + lk], Br[k0 + lk], acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int a = i * CB + tr * 16 + lk + 4 * v, b = j * CB + tc * 16 + li;
        if (i == j && b > a) continue;
        Sig[(size_t)a * Pp + b] = acc[v];
        Sig[(size_t)b * Pp + a] = acc[v];
    }
}

// ---- 5. landmark covariances (one thread per landmark slot) ----------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cov_landmark(DevBuf d, const double* __restrict__ rec, const double* __restrict__ lmrec, const int* __restrict__ stat,
                                                     const double* __restrict__ Sig, int Pp, double* __restrict__ out_pt, double* __restrict__ out_ln, double* __restrict__ out_st) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= d.L) return;
    const bool is_pt = l < d.Np;
    const int nd = is_pt ? 3 : 6, r = is_pt ? 3 : 4;
    double* o = is_pt ? out_pt + (size_t)l * 9 : out_ln + (size_t)(l - d.Np) * 36;
    const int st = stat[l];
    out_st[l] = (double)st;
    if (st != 0) {
        const double v = st == 1 ? 0.0 : __builtin_nan("");
        for (int q = 0; q < nd * nd; ++q) o[q] = v;
        return;
    }
    const int e0 = d.lm_start[l], e1 = d.lm_start[l + 1];
    double M[4][4];
    for (int p = 0; p < 4; ++p) for (int q = 0; q < 4; ++q) M[p][q] = p == q ? 1.0 : 0.0;
    for (int a = e0; a < e1; ++a) {
        const int oa = d.kf_off_pvr[d.ob_kf[a]];
        if (oa < 0 || d.ob_level[a] != 0) continue;
        const double* ya = rec + (size_t)a * REC + 36;
        for (int b = e0; b < e1; ++b) {
            const int ob = d.kf_off_pvr[d.ob_kf[b]];
            if (ob < 0 || d.ob_level[b] != 0) continue;
            const double* yb = rec + (size_t)b * REC + 36;
            double Z[6][4];      // Sigma(a, b) Y_b
            for (int p = 0; p < 6; ++p) {
                const double* srow = Sig + (size_t)(oa + pmap(p)) * Pp + ob;
                for (int v = 0; v < r; ++v) {
                    double s = 0.0;
                    for (int q = 0; q < 6; ++q) s += srow[pmap(q)] * yb[q * 4 + v];
                    Z[p][v] = s;
                }
            }
            for (int u = 0; u < r; ++u)
                for (int v = 0; v < r; ++v) {
                    double s = 0.0;
                    for (int p = 0; p < 6; ++p) s += ya[p * 4 + u] * Z[p][v];
                    M[u][v] += s;
                }
        }
    }
    const double* lr = lmrec + (size_t)l * LMREC;
    double Sr[4][4], T1[4][4];
    for (int u = 0; u < r; ++u)      // T1 = M Lr^-1
        for (int v = 0; v < r; ++v) { double s = 0.0; for (int q = v; q < r; ++q) s += M[u][q] * lr[q * 4 + v]; T1[u][v] = s; }
    for (int u = 0; u < r; ++u)      // Sr = Lr^-T T1
        for (int v = 0; v < r; ++v) { double s = 0.0; for (int q = u; q < r; ++q) s += lr[q * 4 + u] * T1[q][v]; Sr[u][v] = s; }
    double BS[6][4];
    for (int a = 0; a < nd; ++a)
        for (int v = 0; v < r; ++v) { double s = 0.0; for (int u = 0; u < r; ++u) s += lr[16 + a * 4 + u] * Sr[u][v]; BS[a][v] = s; }
    for (int a = 0; a < nd; ++a)      // (mirrored: exactly symmetric)
        for (int b = 0; b <= a; ++b) { double s = 0.0; for (int v = 0; v < r; ++v) s += BS[a][v] * lr[16 + b * 4 + v]; o[a * nd + b] = s; o[b * nd + a] = s; }
}

// ---- 6. keyframe and pair blocks in slot order -----------------------------------------------------------------------------
CDEV int kf_dim(const DevBuf& d, int k, int r) {
    const int o = r < 9 ? d.kf_off_pvr[k] : d.kf_off_bias[k];
    return o < 0 ? -1 : o + (r < 9 ? r : r - 9);
}
__global__ void k_cov_gather(DevBuf d, const double* __restrict__ Sig, int Pp, const int32_t* __restrict__ pairs, int npairs, int want_kf,
                             const int* __restrict__ fail, double* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) out[0] = (double)*fail;
    const size_t nkf = want_kf ? (size_t)d.K * 225 : 0, tot = nkf + (size_t)npairs * 225;
    if (t >= tot) return;
    int ki, kj, rc;
    if (t < nkf) { ki = kj = (int)(t / 225); rc = (int)(t % 225); }
    else { const size_t u = t - nkf; const int q = (int)(u / 225); ki = pairs[2 * q]; kj = pairs[2 * q + 1]; rc = (int)(u % 225); }
    const int a = kf_dim(d, ki, rc / 15), b = kf_dim(d, kj, rc % 15);
    out[1 + t] = (a < 0 || b < 0) ? 0.0 : Sig[(size_t)a * Pp + b];
}

}  // namespace

int cov_run(plba_problem* p, plba_marginals* m) {
    const DevBuf& d = p->dv;
    hipStream_t s = p->stream;
    const int K = p->win.K, Np = p->win.Np, Nl = p->win.Nl, L = p->L, E = p->E, P = p->P;
    const bool want_kf = m->want & 1, want_pair = (m->want & 2) && m->n_pairs > 0, want_pt = m->want & 4, want_ln = m->want & 8;
    const int npairs = want_pair ? m->n_pairs : 0;
    const int Pp = dense_ppad(P), T = Pp / CB;      // (the dense factorisation's padding; ld = Pp)
    // host: the pose blocks the landmarks couple, and their observation pairs in a fixed order (landmark, then observation order)
    std::map<int64_t, std::vector<int32_t>> bl;
    std::vector<std::pair<int, int>> ob;      // (edge, pose offset) of one landmark's observations from free keyframes
    for (int l = 0, e = 0; l < L; ++l) {
        ob.clear();
        const bool pt = l < Np;
        const int lm = pt ? l : l - Np;
        for (; e < E; ++e) {
            const bool ept = e < p->win.Ep;
            if (ept != pt || (ept ? p->win.po_pt[e] : p->win.lo_ln[e - p->win.Ep]) != lm) break;
            const int o = p->off_pvr[ept ? p->win.po_kf[e] : p->win.lo_kf[e - p->win.Ep]];
            if (o >= 0) ob.push_back({e, o});
        }
        const bool fixed = p->lm_fixed[l] != 0;
        for (auto& a : ob)
            for (auto& b : ob) {
                if (b.second > a.second || (fixed && a.first != b.first)) continue;
                auto& v = bl[((int64_t)a.second << 32) | (uint32_t)b.second];
                v.push_back(a.first); v.push_back(b.first);
            }
    }
    std::vector<int32_t> blk, ent;
    for (auto& kv : bl) {
        blk.push_back((int32_t)(kv.first >> 32)); blk.push_back((int32_t)(kv.first & 0xffffffff));
        blk.push_back((int32_t)(ent.size() / 2));
        ent.insert(ent.end(), kv.second.begin(), kv.second.end());
        blk.push_back((int32_t)(ent.size() / 2));
    }
    const int nblk = (int)(blk.size() / 4);
    const size_t n_out = 1 + (want_kf ? (size_t)K * 225 : 0) + (size_t)npairs * 225 + (size_t)Np * 9 + (size_t)Nl * 36 + (size_t)L;
    DArr<double> Hp, bp, ierr, ichi, perr, pdx, pchi, bpr, S, d0, Sig, rec, lmrec, out;
    DArr<Ctrl> ctrl;
    DArr<int32_t> dblk, dent, dpairs, stat, fail; DenseWork work;
    PLBA_HIPCK(p, Hp.alloc((size_t)p->Ppad * p->ld, false)); PLBA_HIPCK(p, bp.alloc(p->ld, false));
    PLBA_HIPCK(p, ierr.alloc((size_t)std::max(p->win.M, 1) * 16, false)); PLBA_HIPCK(p, ichi.alloc((size_t)std::max(p->win.M, 1) * 4, false));
    PLBA_HIPCK(p, perr.alloc(std::max(p->pr_n, 1), false)); PLBA_HIPCK(p, pdx.alloc(std::max(p->pr_n, 1), false));
    PLBA_HIPCK(p, pchi.alloc(4, false)); PLBA_HIPCK(p, bpr.alloc(p->ld, false));
    // the dense factorisation's buffers, as plba_dense_solve sizes them, the explicit inverse at full size whatever path the problem's own
    // solve takes (chain / band / twin problems keep none, or one of the compact system only)
    const DenseCounts wn = dense_counts(Pp, Pp); const size_t sysn = wn.sys_len;
    PLBA_HIPCK(p, S.alloc(sysn, false)); PLBA_HIPCK(p, work.alloc(Pp, Pp, true, false)); PLBA_HIPCK(p, ctrl.alloc(1, false));      // (cleared below, on the call's stream)
    PLBA_HIPCK(p, d0.alloc(Pp, false)); PLBA_HIPCK(p, Sig.alloc((size_t)Pp * Pp, false));
    PLBA_HIPCK(p, rec.alloc((size_t)std::max(E, 1) * REC, false)); PLBA_HIPCK(p, lmrec.alloc((size_t)std::max(L, 1) * LMREC, false));
    PLBA_HIPCK(p, stat.alloc(std::max(L, 1), false)); PLBA_HIPCK(p, fail.alloc(1, false)); PLBA_HIPCK(p, out.alloc(n_out, false));
    PLBA_HIPCK(p, dblk.alloc(std::max(nblk, 1) * 4, false)); PLBA_HIPCK(p, dent.alloc(std::max(ent.size(), (size_t)2), false));
    PLBA_HIPCK(p, dpairs.alloc(std::max(npairs, 1) * 2, false));
    if (nblk) PLBA_HIPCK(p, hipMemcpyAsync(dblk.p, blk.data(), blk.size() * 4, hipMemcpyHostToDevice, s));
    if (!ent.empty()) PLBA_HIPCK(p, hipMemcpyAsync(dent.p, ent.data(), ent.size() * 4, hipMemcpyHostToDevice, s));
    if (npairs) PLBA_HIPCK(p, hipMemcpyAsync(dpairs.p, m->pairs, (size_t)npairs * 8, hipMemcpyHostToDevice, s));
    PLBA_HIPCK(p, hipMemsetAsync(fail.p, 0xff, 4, s));
    PLBA_HIPCK(p, hipMemsetAsync(Hp.p, 0, (size_t)p->Ppad * p->ld * 8, s));
    PLBA_HIPCK(p, hipMemsetAsync(bp.p, 0, (size_t)p->ld * 8, s));
    PLBA_HIPCK(p, hipMemsetAsync(S.p, 0, sysn * 8, s)); PLBA_HIPCK(p, hipMemsetAsync(work.Lfac.p, 0, sysn * 8, s));
    PLBA_HIPCK(p, hipMemsetAsync(work.Ninv.p, 0, wn.ninv * 8, s)); PLBA_HIPCK(p, hipMemsetAsync(work.Linv.p, 0, wn.Linv * 8, s));
    PLBA_HIPCK(p, hipMemsetAsync(work.LT32.p, 0, wn.LT32 * 8, s)); PLBA_HIPCK(p, hipMemsetAsync(work.rd32.p, 0, wn.rd32 * 8, s));
    PLBA_HIPCK(p, hipMemsetAsync(work.flow_flags.p, 0, wn.flow_flags * 4, s)); PLBA_HIPCK(p, hipMemsetAsync(work.chol_flags.p, 0, wn.chol_flags * 4, s));
    PLBA_HIPCK(p, hipMemsetAsync(ctrl.p, 0, sizeof(Ctrl), s));
    PLBA_HIPCK(p, hipMemsetAsync(&ctrl.p->solver_ok, 1, 1, s));      // solver_ok = 1 (the low byte of a zeroed int)
    // 1. IMU / prior edges at the current estimate into the scratch accumulator (the problem's own accumulators stay as they are)
    DevBuf dc = d;
    dc.Himu = Hp.p; dc.bimu = bp.p; dc.imu_err = ierr.p; dc.imu_chi = ichi.p;
    dc.pr_err = perr.p; dc.pr_dx = pdx.p; dc.pr_chi = pchi.p; dc.bprior = bpr.p;
    launch_pose_edges(dc, p->cur, true, p->rob, true, s);
    if (P) hipLaunchKernelGGL(k_cov_init, dim3((unsigned)(((size_t)Pp * Pp + 255) / 256)), dim3(256), 0, s, Hp.p, d.Hconst, P, p->ld, S.p, Pp, d0.p);
    else hipLaunchKernelGGL(k_cov_init, dim3((unsigned)(((size_t)Pp * Pp + 255) / 256)), dim3(256), 0, s, Hp.p, Hp.p, 0, p->ld, S.p, Pp, d0.p);
    // 2. landmarks, 3. their Schur terms
    if (L) hipLaunchKernelGGL(k_cov_lm, dim3((L + 63) / 64), dim3(64), 0, s, dc, p->cur, p->rob, rec.p, lmrec.p, stat.p);
    if (nblk) hipLaunchKernelGGL(k_cov_pairs, dim3(nblk), dim3(64), 0, s, dblk.p, dent.p, rec.p, S.p, Pp, d0.p);
    // 4. S = L L^T and N = L^-T on the matrix cores (launch_cholesky with the identity rows), N's last block column, the pivot test,
    //    Sigma_pp = N N^T
    const bool dump = (p->opt.diag & PLBA_DIAG_COV_DUMP) != 0;      // host copies for plba_debug_get("cov_S" / "cov_Sigma"): read only, the launches are the same
    auto keep = [&](const double* dev, std::vector<double>& dst) -> hipError_t {
        std::vector<double> h((size_t)Pp * Pp);
        const hipError_t e = plba_d2h(p, h.data(), dev, h.size() * 8);
        dst.resize((size_t)P * P);
        for (int r = 0; r < P; ++r) memcpy(dst.data() + (size_t)r * P, h.data() + (size_t)r * Pp, (size_t)P * 8);
        return e;
    };
    if (dump) PLBA_HIPCK(p, keep(S.p, p->cov_dbg_S));
    DevBuf dd; memset(&dd, 0, sizeof dd);
    dd.P = P; dd.Ppad = Pp; dd.ld = Pp; dd.sys = S.p; dd.ctrl = ctrl.p;
    work.bind(dd, p->opt); dd.fb = 32; dd.flow = 0; dd.wide = 0;      // always the multi-launch factorisation in 32-column steps, whatever the problem's options say
    launch_cholesky(dd, true, 1, s);
    hipLaunchKernelGGL(k_cov_nlast, dim3((unsigned)(((size_t)Pp * CB + 255) / 256)), dim3(256), 0, s, dd);
    hipLaunchKernelGGL(k_cov_pivots, dim3(1), dim3(256), 0, s, dd, d0.p, fail.p);
    hipLaunchKernelGGL(k_cov_syrk, dim3(T, T), dim3(256), 0, s, work.Ninv.p, Pp, Pp, Sig.p);
    if (dump) PLBA_HIPCK(p, keep(Sig.p, p->cov_dbg_Sigma));
    // 5. landmarks, 6. keyframe / pair blocks
    double* o_pt = out.p + n_out - L - (size_t)Nl * 36 - (size_t)Np * 9;
    double* o_ln = o_pt + (size_t)Np * 9;
    double* o_st = o_ln + (size_t)Nl * 36;
    if (L) hipLaunchKernelGGL(k_cov_landmark, dim3((L + 63) / 64), dim3(64), 0, s, dc, rec.p, lmrec.p, stat.p, Sig.p, Pp, o_pt, o_ln, o_st);
    const size_t ng = std::max((size_t)1, (want_kf ? (size_t)K * 225 : 0) + (size_t)npairs * 225);
    hipLaunchKernelGGL(k_cov_gather, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, dc, Sig.p, Pp, dpairs.p, npairs, want_kf ? 1 : 0, fail.p, out.p);
    PLBA_HIPCK(p, hipGetLastError());
    std::vector<double> h(n_out);
    PLBA_HIPCK(p, plba_d2h(p, h.data(), out.p, n_out * 8));      // the call's one wait
    const int fcol = (int)h[0];
    if (fcol >= 0) {
        int kf = -1;
        for (int k = 0; k < K && kf < 0; ++k) {
            const int op = p->off_pvr[k], ob2 = p->off_bias[k];
            if ((op >= 0 && fcol >= op && fcol < op + 9) || (ob2 >= 0 && fcol >= ob2 && fcol < ob2 + 6)) kf = k;
        }
        PLBA_FAIL(p, PLBA_ERR_NUMERIC, "plba_compute_marginals: the pose system is not positive definite (pivot of dimension %d, keyframe slot %d)", fcol, kf);
    }
    const double* src = h.data() + 1;
    if (want_kf) { memcpy(m->kf_cov, src, (size_t)K * 225 * 8); src += (size_t)K * 225; }
    if (npairs) memcpy(m->pair_cov, src, (size_t)npairs * 225 * 8);
    const double* hp = h.data() + n_out - L - (size_t)Nl * 36 - (size_t)Np * 9;
    const double* hl = hp + (size_t)Np * 9;
    const double* hs = hl + (size_t)Nl * 36;
    int nx_pt = 0, nx_ln = 0;
    for (int l = 0; l < L; ++l) { const int st = (int)hs[l]; if (st >= 2) ++(l < Np ? nx_pt : nx_ln); }
    if (want_pt) {
        if (Np) memcpy(m->pt_cov, hp, (size_t)Np * 9 * 8);
        if (m->pt_status) for (int l = 0; l < Np; ++l) m->pt_status[l] = (uint8_t)hs[l];
    }
    if (want_ln) {
        if (Nl) memcpy(m->ln_cov, hl, (size_t)Nl * 36 * 8);
        if (m->ln_status) for (int l = 0; l < Nl; ++l) m->ln_status[l] = (uint8_t)hs[Np + l];
    }
    m->n_excluded[0] = nx_pt; m->n_excluded[1] = nx_ln;
    return PLBA_OK;
}

}  // namespace plba
