// plba_pgo_cov.h — the host side of plba_pose_graph_marginals: where the entries of H^-1 that the selected inversion
// leaves in the fronts of a PgoSparsePlan (plba_pgo_sparse.h) lie, the checks of every index the kernels of plba_pgo_cov.hip form, and
// a plain C++ walk of the whole computation in any number type.  Standard library only: the plan type is a template parameter, so the
// stand-alone check (plba_pgo_cov_hostcheck.cpp) and the library share this text.
//
// After the factorisation front f holds L11 | L21 in its np pivot columns (column-major m x m, lower triangle) and a consumed F22.
// Takahashi's recurrence runs DOWN the tree and turns the same storage into Z = H^-1 on the pattern of L:
//   gather      Z22(f)[a, b] = Z(parent)[umap a, umap b]                              (the parent is complete: it ran a level earlier)
//   per pivot vertex j, last to first, S = every row of the front behind j:
//       G    = L_Sj L_jj^-1
//       Z_Sj = - Z_SS G                 written over L_Sj
//       Z_jj = L_jj^-T L_jj^-1 - G^T Z_Sj      (lower triangle) written over L_jj
// The block of H^-1 of two vertices lies in the front where the EARLIER eliminated of the two is a pivot, at (row position of the later
// one, pivot position of the earlier one) — if the later one is a row of that front at all; otherwise the block is outside the pattern.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace plba {

struct PgoCovPlace { int32_t front, rpos, cpos, transposed; };      // positions in vertices; front < 0: outside the pattern

struct PgoCovPlan {
    std::vector<int32_t> v_front, v_pos, v_elim;      // per free rank: its front, its pivot position there, its elimination position
    std::vector<int32_t> parent, level;               // per front
    std::vector<long long> g_off;                     // per front: its G scratch (6 m doubles)
    long long gsize = 0;
};

// what the two kernels read besides the solver's own PgoSparseDev (device pointers)
struct PgoCovDev {
    const int32_t* parent;       // per front
    const long long* g_off;      // per front: its part of G
    double* G;                   // G = L_Sj L_jj^-1 of the pivot vertex in work, |S| x 6 row-major
    int n_items;                 // requested blocks: the vertices (if wanted), then the pairs
    const int32_t* place;        // n_items x 4: a PgoCovPlace each (status 0 only)
    const uint8_t* status;       // n_items: 0 computed, 1 zeros, 2 / 3 NaN
    double* out;                 // n_items x 36
};
#ifdef __HIPCC__
struct PgoSparseDev;
struct PgoSparsePlan;
void pgo_cov_launch(const PgoSparseDev& d, const PgoCovDev& c, const PgoSparsePlan& pl, hipStream_t s);      // after the factorisation
#endif

// false: the plan is not one pgo_sparse_analyse made
template <class Plan>
inline bool pgo_cov_prepare(const Plan& pl, PgoCovPlan& cp) {
    cp = PgoCovPlan();
    const int F = pl.nfront, n = pl.n;
    cp.v_front.assign(n, -1); cp.v_pos.assign(n, -1); cp.v_elim.assign(n, -1);
    cp.parent.assign(F, -1); cp.level.assign(F, -1); cp.g_off.assign(F, 0);
    int q = 0;
    for (int f = 0; f < F; ++f) {
        const int m = pl.f_m[f], np = pl.f_np[f];
        if (m <= 0 || np <= 0 || np > m || m % 6 || np % 6) return false;
        for (int a = 0; a < np / 6; ++a) {
            const int v = pl.rows[pl.f_row0[f] + a];
            if (v < 0 || v >= n || cp.v_front[v] >= 0) return false;
            cp.v_front[v] = f; cp.v_pos[v] = a; cp.v_elim[v] = q++;
        }
        for (int e = pl.ch_start[f]; e < pl.ch_start[f + 1]; ++e) {
            const int c = pl.ch[e];
            if (c < 0 || c >= f || cp.parent[c] >= 0) return false;
            cp.parent[c] = f;
        }
        cp.g_off[f] = cp.gsize;
        cp.gsize += 6LL * m;
    }
    if (q != n) return false;
    for (int l = 0; l < pl.nlev; ++l)
        for (int e = pl.lv_start[l]; e < pl.lv_start[l + 1]; ++e) {
            const int f = pl.lv[e];
            if (f < 0 || f >= F || cp.level[f] >= 0) return false;
            cp.level[f] = l;
        }
    for (int f = 0; f < F; ++f) if (cp.level[f] < 0) return false;
    return true;
}

// the place of Cov(x_a, x_b), a and b free ranks
template <class Plan>
inline PgoCovPlace pgo_cov_locate(const Plan& pl, const PgoCovPlan& cp, int a, int b) {
    const bool a_first = cp.v_elim[a] <= cp.v_elim[b];
    const int e = a_first ? a : b, l = a_first ? b : a, f = cp.v_front[e];
    PgoCovPlace out{-1, 0, 0, 0};
    const int32_t* rw = pl.rows.data() + pl.f_row0[f];
    const int nr = pl.f_m[f] / 6, npv = pl.f_np[f] / 6;
    int q = -1;
    if (cp.v_front[l] == f) q = cp.v_pos[l];
    else {      // the update rows ascend in elimination position
        int lo = npv, hi = nr;
        while (lo < hi) { const int mid = (lo + hi) / 2; if (cp.v_elim[rw[mid]] < cp.v_elim[l]) lo = mid + 1; else hi = mid; }
        if (lo < nr && rw[lo] == l) q = lo;
    }
    if (q < 0) return out;
    out.front = f; out.rpos = q; out.cpos = cp.v_pos[e]; out.transposed = (a == e && a != b) ? 1 : 0;
    return out;
}

// every index k_sps_selinv and k_sps_covout form, before anything is launched; ranks: the two free ranks of each place
template <class Plan>
inline bool pgo_cov_check(const Plan& pl, const PgoCovPlan& cp, const std::vector<PgoCovPlace>& places, const std::vector<int32_t>& ranks) {
    const int F = pl.nfront;
    if ((int)cp.parent.size() != F || ranks.size() != 2 * places.size()) return false;
    for (int f = 0; f < F; ++f) {
        const long long m = pl.f_m[f];
        const int np = pl.f_np[f], pr = cp.parent[f];
        if (pl.f_off[f] < 0 || pl.f_off[f] + m * m > pl.fsize) return false;
        if (cp.g_off[f] < 0 || cp.g_off[f] + 6 * m > cp.gsize) return false;
        if (m > np && pr < 0) return false;
        if (pr >= 0 && cp.level[pr] <= cp.level[f]) return false;      // the gather reads a front that an earlier launch completed
        for (int a = np / 6; a < m / 6; ++a) {
            const int t = pl.umap[pl.f_row0[f] + a];
            if (t < 0 || 6 * t + 5 >= pl.f_m[pr] || pl.rows[pl.f_row0[pr] + t] != pl.rows[pl.f_row0[f] + a]) return false;
            if (a > np / 6 && t <= pl.umap[pl.f_row0[f] + a - 1]) return false;      // increasing: lower maps to lower
        }
    }
    for (size_t k = 0; k < places.size(); ++k) {
        const PgoCovPlace& c = places[k];
        if (c.front < 0) continue;
        if (c.front >= F) return false;
        const int nr = pl.f_m[c.front] / 6, npv = pl.f_np[c.front] / 6;
        if (c.cpos < 0 || c.cpos >= npv || c.rpos < c.cpos || c.rpos >= nr) return false;
        const int rv = pl.rows[pl.f_row0[c.front] + c.rpos], cv = pl.rows[pl.f_row0[c.front] + c.cpos];
        const int i = ranks[2 * k], j = ranks[2 * k + 1];
        if (!(c.transposed ? (rv == j && cv == i) : (rv == i && cv == j))) return false;
    }
    return true;
}

// ---- the whole computation in plain C++ (T: long double in the stand-alone check) ----------------------------------------------------
// Fm: pl.fsize entries, the layout of the device's arena.  Returns -1, or the first front whose factorisation met a pivot not > 0.
template <class T, class Plan>
inline int pgo_cov_walk(const Plan& pl, const PgoCovPlan& cp, const std::vector<T>& Hblk, std::vector<T>& Fm) {
    Fm.assign((size_t)pl.fsize, T(0));
    auto at = [&](int f, int r, int c) -> T& { return Fm[(size_t)(pl.f_off[f] + (long long)c * pl.f_m[f] + r)]; };
    for (int f = 0; f < pl.nfront; ++f) {      // assemble, extend-add, partial Cholesky: up the tree (children have lower numbers)
        const int m = pl.f_m[f], np = pl.f_np[f];
        for (int e = pl.as_start[f]; e < pl.as_start[f + 1]; ++e) {
            const int k = pl.as[3 * e], a = pl.as[3 * e + 1], b = pl.as[3 * e + 2];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) {
                    if (a == b && i < j) continue;
                    int r = 6 * a + i, c = 6 * b + j;
                    if (r < c) std::swap(r, c);
                    at(f, r, c) = Hblk[(size_t)36 * k + 6 * i + j];
                }
        }
        for (int q = pl.ch_start[f]; q < pl.ch_start[f + 1]; ++q) {
            const int c = pl.ch[q], mc = pl.f_m[c], npc = pl.f_np[c];
            const int32_t* um = pl.umap.data() + pl.f_row0[c] + npc / 6;
            for (int a = 0; a < mc - npc; ++a)
                for (int b = 0; b <= a; ++b) at(f, 6 * um[a / 6] + a % 6, 6 * um[b / 6] + b % 6) += at(c, npc + a, npc + b);
        }
        for (int c = 0; c < np; ++c) {
            T d = at(f, c, c);
            for (int k = 0; k < c; ++k) d -= at(f, c, k) * at(f, c, k);
            if (!(d > T(0)) || !std::isfinite((double)d)) return f;
            const T l = std::sqrt(d);
            at(f, c, c) = l;
            for (int r = c + 1; r < m; ++r) {
                T v = at(f, r, c);
                for (int k = 0; k < c; ++k) v -= at(f, r, k) * at(f, c, k);
                at(f, r, c) = v / l;
            }
        }
        for (int c = np; c < m; ++c)
            for (int r = c; r < m; ++r) {
                T v = at(f, r, c);
                for (int k = 0; k < np; ++k) v -= at(f, r, k) * at(f, c, k);
                at(f, r, c) = v;
            }
    }
    std::vector<T> G, W(36), Zj;
    for (int f = pl.nfront - 1; f >= 0; --f) {      // selected inversion: down the tree
        const int m = pl.f_m[f], np = pl.f_np[f], pr = cp.parent[f];
        const int32_t* um = pl.umap.data() + pl.f_row0[f] + np / 6;
        for (int a = 0; a < m - np; ++a)
            for (int b = 0; b <= a; ++b) at(f, np + a, np + b) = at(pr, 6 * um[a / 6] + a % 6, 6 * um[b / 6] + b % 6);
        auto Z = [&](int r, int c) -> T { return r >= c ? at(f, r, c) : at(f, c, r); };
        for (int j0 = np - 6; j0 >= 0; j0 -= 6) {
            const int s0 = j0 + 6, ns = m - s0;
            for (int c = 0; c < 6; ++c)      // W = L_jj^-1 (lower)
                for (int r = 0; r < 6; ++r) {
                    if (r < c) { W[r * 6 + c] = T(0); continue; }
                    T v = r == c ? T(1) : T(0);
                    for (int k = c; k < r; ++k) v -= at(f, j0 + r, j0 + k) * W[k * 6 + c];
                    W[r * 6 + c] = v / at(f, j0 + r, j0 + r);
                }
            G.assign((size_t)6 * ns, T(0)); Zj.assign((size_t)6 * ns, T(0));
            for (int i = 0; i < ns; ++i)
                for (int c = 0; c < 6; ++c) { T v = T(0); for (int k = c; k < 6; ++k) v += at(f, s0 + i, j0 + k) * W[k * 6 + c]; G[(size_t)i * 6 + c] = v; }
            for (int i = 0; i < ns; ++i)
                for (int c = 0; c < 6; ++c) { T v = T(0); for (int k = 0; k < ns; ++k) v += Z(s0 + i, s0 + k) * G[(size_t)k * 6 + c]; Zj[(size_t)i * 6 + c] = -v; }
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b <= a; ++b) {
                    T v = T(0);
                    for (int k = a; k < 6; ++k) v += W[k * 6 + a] * W[k * 6 + b];
                    for (int k = 0; k < ns; ++k) v -= G[(size_t)k * 6 + a] * Zj[(size_t)k * 6 + b];
                    at(f, j0 + a, j0 + b) = v;
                }
            for (int i = 0; i < ns; ++i) for (int c = 0; c < 6; ++c) at(f, s0 + i, j0 + c) = Zj[(size_t)i * 6 + c];
        }
    }
    return -1;
}

// entry (a, b) of the 6 x 6 block Cov(x_i, x_j) at a place, from an arena laid out as the device's
template <class T, class Plan>
inline T pgo_cov_entry(const Plan& pl, const std::vector<T>& Fm, const PgoCovPlace& c, int a, int b) {
    if (c.transposed) std::swap(a, b);
    int r = 6 * c.rpos + a, q = 6 * c.cpos + b;
    if (r < q) std::swap(r, q);      // a diagonal block: one triangle is stored
    return Fm[(size_t)(pl.f_off[c.front] + (long long)q * pl.f_m[c.front] + r)];
}

}  // namespace plba
