// plba_pgo_sparse.h — the sparse (multifrontal) solve of plba_optimize_pose_graph, options.pgo_solver = 1.
//
// Host analysis, once per call (the structure is fixed across trials), on 6 x 6 blocks of the free vertices:
//   ordering   nested dissection of the free-vertex adjacency: every connected component on its own; a component of more than
//              SP_LEAF vertices is bisected by the middle level of a BFS level structure rooted at a pseudo-peripheral vertex (that
//              level is a separator front, the rest is dissected again below it); smaller components, and components whose level
//              structure has fewer than three levels (nothing to bisect), are one front.  Ties go to the lower vertex index.
//   fronts     post-ordered (children before their parent, children in creation order); a front's rows are its pivot vertices
//              (ascending) and then its update vertices (ascending elimination position): the original neighbours of its pivots and
//              its children's update vertices that are eliminated after it
//   schedule   level 0 = fronts without children, a parent one level above its highest child
// Numeric work (plba_pgo_sparse.hip), one STEP = one LM trial, in place of k_pgo_fill + launch_cholesky + launch_trsv_back:
//   k_sps_assemble   every front: zero, its Hblk blocks (+ lambda on the diagonal) and b                workgroup per front
//   k_sps_factor     per level, bottom-up: extend-add of the children (fixed order), partial Cholesky of the
//                    pivot columns with the right-hand side carried along, F22 - L21 L21^T                workgroup per front
//   k_sps_back       per level, top-down: L11^T x1 = y1 - L21^T x2 with x2 gathered from the ancestors      workgroup per front
// Front f keeps its m x m frontal matrix column-major (lower triangle used) at F + f_off[f] and its right-hand side at R + f_roff[f];
// nothing of size n x n exists on either side.
// Standard library only (plba_pgo_cov_hostcheck.cpp builds over it with a plain C++ compiler); the device side, which plba_lba_visual
// (solver = 1) and plba_pose_graph_marginals use as well, is plba_pgo_sparse_dev.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace plba {

constexpr int SP_LEAF = 16;      // vertices of a nested-dissection leaf

struct PgoSparsePlan {
    int n = 0, nfront = 0, nlev = 0, max_m = 0;
    long long nnz_blk = 0;                      // nonzero 6 x 6 blocks of L (lower, diagonal blocks included)
    std::vector<int32_t> f_m, f_np;             // per front: dimension, pivot dimension (6 x vertices)
    std::vector<long long> f_off, f_roff;       // offsets of the frontal matrix and of the right-hand side
    std::vector<int32_t> f_row0, rows, umap;    // rows (free ranks) of front f at rows[f_row0[f] ..]; umap: an update row's vertex position in the parent
    std::vector<int32_t> ch_start, ch;          // children
    std::vector<int32_t> as_start, as;          // per front: (block id, row-vertex position, column-vertex position) of the Hblk blocks it assembles
    std::vector<int32_t> lv_start, lv;          // fronts of each level
    long long fsize = 0, rsize = 0;
};

// the record every caller of the solver keeps for plba_debug_get ("pgo_sparse", "lba_sparse", "pgo_cov"; include/plba.h):
// 1, n, fronts, levels, nonzero blocks of L, largest front, device bytes of the call's buffers, ms of the host analysis
inline void pgo_sparse_record(double rec[8], int n, const PgoSparsePlan& pl, size_t bytes, double ms) {
    rec[0] = 1.0; rec[1] = n; rec[2] = pl.nfront; rec[3] = pl.nlev; rec[4] = (double)pl.nnz_blk; rec[5] = pl.max_m; rec[6] = (double)bytes; rec[7] = ms;
}

// blk_row / blk_col: the free ranks of every block of H (row >= column); diagonal blocks exist for every free rank.
// false: the plan failed its own index checks (every index the kernels form is checked here, before anything is launched)
inline bool pgo_sparse_analyse(int n, const std::vector<int32_t>& blk_row, const std::vector<int32_t>& blk_col, PgoSparsePlan& pl) {
    pl = PgoSparsePlan();
    pl.n = n;
    const int nblk = (int)blk_row.size();
    // adjacency (CSR, ascending) and the blocks incident to each vertex
    std::vector<int32_t> a_start(n + 1, 0), adj, i_start(n + 1, 0), inc;
    for (int k = 0; k < nblk; ++k) {
        ++i_start[blk_row[k] + 1];
        if (blk_row[k] != blk_col[k]) { ++a_start[blk_row[k] + 1]; ++a_start[blk_col[k] + 1]; ++i_start[blk_col[k] + 1]; }
    }
    for (int v = 0; v < n; ++v) { a_start[v + 1] += a_start[v]; i_start[v + 1] += i_start[v]; }
    adj.resize(a_start[n]); inc.resize(i_start[n]);
    {
        std::vector<int32_t> ca(a_start.begin(), a_start.end() - 1), ci(i_start.begin(), i_start.end() - 1);
        for (int k = 0; k < nblk; ++k) {
            const int r = blk_row[k], c = blk_col[k];
            inc[ci[r]++] = k;
            if (r != c) { adj[ca[r]++] = c; adj[ca[c]++] = r; inc[ci[c]++] = k; }
        }
        for (int v = 0; v < n; ++v) std::sort(adj.begin() + a_start[v], adj.begin() + a_start[v + 1]);
    }

    // ---- nested dissection --------------------------------------------------------------------------------------------------------
    std::vector<std::vector<int32_t>> fpiv;      // pivots of each front, in creation order
    std::vector<int32_t> fpar;
    std::vector<int32_t> stamp(n, -1), lev(n, -1);
    int cur = 0;
    // BFS level structure from r over the vertices that carry stamp == tag (lev[] marks the reached ones)
    auto levels = [&](int r, int tag, std::vector<std::vector<int32_t>>& L) {
        L.clear();
        std::vector<int32_t> q{r};
        lev[r] = tag;
        while (!q.empty()) {
            L.push_back(q);
            std::vector<int32_t> nx;
            for (int32_t v : q)
                for (int e = a_start[v]; e < a_start[v + 1]; ++e) { const int u = adj[e]; if (stamp[u] == tag && lev[u] != tag) { lev[u] = tag; nx.push_back(u); } }
            std::sort(nx.begin(), nx.end());
            q.swap(nx);
        }
    };
    struct Work { std::vector<int32_t> set; int parent; };
    std::vector<Work> stack;
    { std::vector<int32_t> all(n); std::iota(all.begin(), all.end(), 0); stack.push_back({std::move(all), -1}); }
    std::vector<std::vector<int32_t>> L;
    while (!stack.empty()) {
        Work w = std::move(stack.back());
        stack.pop_back();
        // connected components of w.set, each from its lowest vertex
        const int tset = cur++;
        for (int32_t v : w.set) stamp[v] = tset;
        std::vector<std::vector<int32_t>> comps;
        for (int32_t s : w.set) {
            if (stamp[s] != tset) continue;
            std::vector<int32_t> c{s};
            stamp[s] = -2 - tset;      // visited
            for (size_t h = 0; h < c.size(); ++h)
                for (int e = a_start[c[h]]; e < a_start[c[h] + 1]; ++e) { const int u = adj[e]; if (stamp[u] == tset) { stamp[u] = -2 - tset; c.push_back(u); } }
            std::sort(c.begin(), c.end());
            comps.push_back(std::move(c));
        }
        for (auto& c : comps) {
            const int tag = cur++;
            for (int32_t v : c) stamp[v] = tag;
            if ((int)c.size() <= SP_LEAF) { fpiv.push_back(c); fpar.push_back(w.parent); continue; }
            // pseudo-peripheral vertex (George & Liu): from the lowest vertex, move to the last level's vertex of least degree while
            // the eccentricity grows
            int r = c[0];
            levels(r, tag, L);
            for (int it = 0; it < 8; ++it) {
                int best = -1, bd = 0;
                for (int32_t v : L.back()) { const int dg = a_start[v + 1] - a_start[v]; if (best < 0 || dg < bd) { best = v; bd = dg; } }
                const size_t ecc = L.size();
                for (int32_t v : c) lev[v] = -1;
                std::vector<std::vector<int32_t>> L2;
                levels(best, tag, L2);
                if (L2.size() <= ecc) break;
                r = best; L.swap(L2);
            }
            for (int32_t v : c) lev[v] = -1;
            if (L.size() < 3) { fpiv.push_back(c); fpar.push_back(w.parent); continue; }
            // the separator: the level where half the component is reached, kept off both ends
            size_t s = 0, acc = 0;
            for (; s < L.size(); ++s) { acc += L[s].size(); if (2 * acc >= c.size()) break; }
            s = std::min(std::max(s, (size_t)1), L.size() - 2);
            const int id = (int)fpiv.size();
            fpiv.push_back(L[s]); fpar.push_back(w.parent);
            std::vector<int32_t> rest;
            rest.reserve(c.size() - L[s].size());
            for (size_t q = 0; q < L.size(); ++q) if (q != s) rest.insert(rest.end(), L[q].begin(), L[q].end());
            std::sort(rest.begin(), rest.end());
            stack.push_back({std::move(rest), id});
        }
    }

    // ---- post-order, elimination positions ---------------------------------------------------------------------------------------
    const int F = (int)fpiv.size();
    std::vector<std::vector<int32_t>> kids(F);
    std::vector<int32_t> roots;
    for (int f = 0; f < F; ++f) (fpar[f] < 0 ? roots : kids[fpar[f]]).push_back(f);
    std::vector<int32_t> po, newid(F);
    po.reserve(F);
    {
        std::vector<std::pair<int32_t, size_t>> st;
        for (int32_t r : roots) {
            st.push_back({r, 0});
            while (!st.empty()) {
                auto& t = st.back();
                if (t.second < kids[t.first].size()) { const int32_t k = kids[t.first][t.second++]; st.push_back({k, 0}); }
                else { po.push_back(t.first); st.pop_back(); }
            }
        }
    }
    for (int i = 0; i < F; ++i) newid[po[i]] = i;
    std::vector<int32_t> pos(n), vfront(n), last(F);
    {
        int q = 0;
        for (int i = 0; i < F; ++i) { for (int32_t v : fpiv[po[i]]) { pos[v] = q++; vfront[v] = i; } last[i] = q - 1; }
    }

    // ---- symbolic factorisation --------------------------------------------------------------------------------------------------
    pl.nfront = F;
    pl.f_m.resize(F); pl.f_np.resize(F); pl.f_off.resize(F); pl.f_roff.resize(F); pl.f_row0.resize(F + 1);
    pl.ch_start.assign(F + 1, 0); pl.as_start.assign(F + 1, 0);
    std::vector<int32_t> par(F, -1), level(F, 0), loc(n, -1), mark(n, -1);
    std::vector<std::vector<int32_t>> upd(F);
    for (int i = 0; i < F; ++i) {
        const int o = po[i];
        par[i] = fpar[o] < 0 ? -1 : newid[fpar[o]];
        for (int32_t k : kids[o]) { pl.ch.push_back(newid[k]); level[i] = std::max(level[i], level[newid[k]] + 1); }
        pl.ch_start[i + 1] = (int32_t)pl.ch.size();
        std::vector<int32_t>& u = upd[i];
        for (int32_t v : fpiv[o])
            for (int e = a_start[v]; e < a_start[v + 1]; ++e) { const int w = adj[e]; if (pos[w] > last[i] && mark[w] != i) { mark[w] = i; u.push_back(w); } }
        for (int32_t k : kids[o])
            for (int32_t w : upd[newid[k]]) if (pos[w] > last[i] && mark[w] != i) { mark[w] = i; u.push_back(w); }
        std::sort(u.begin(), u.end(), [&](int32_t a, int32_t b) { return pos[a] < pos[b]; });
        const int nr = (int)(fpiv[o].size() + u.size());
        pl.f_row0[i] = (int32_t)pl.rows.size();
        pl.rows.insert(pl.rows.end(), fpiv[o].begin(), fpiv[o].end());
        pl.rows.insert(pl.rows.end(), u.begin(), u.end());
        pl.umap.resize(pl.rows.size(), -1);
        for (int q = 0; q < nr; ++q) loc[pl.rows[pl.f_row0[i] + q]] = q;
        for (int32_t k : kids[o]) {      // the children's update rows in this front
            const int c = newid[k], np_c = pl.f_np[c] / 6;
            for (size_t q = 0; q < upd[c].size(); ++q) pl.umap[pl.f_row0[c] + np_c + q] = loc[upd[c][q]];
        }
        for (int32_t v : fpiv[o])      // the blocks whose earlier vertex is a pivot here
            for (int e = i_start[v]; e < i_start[v + 1]; ++e) {
                const int k = inc[e], other = blk_row[k] == v ? blk_col[k] : blk_row[k];
                if (other != v && pos[other] < pos[v]) continue;
                pl.as.push_back(k); pl.as.push_back(loc[blk_row[k]]); pl.as.push_back(loc[blk_col[k]]);
            }
        pl.as_start[i + 1] = (int32_t)(pl.as.size() / 3);
        const int m = 6 * nr, np = 6 * (int)fpiv[o].size();
        pl.f_m[i] = m; pl.f_np[i] = np;
        pl.f_off[i] = pl.fsize; pl.f_roff[i] = pl.rsize;
        pl.fsize += (long long)m * m; pl.rsize += m;
        pl.max_m = std::max(pl.max_m, m);
        const long long p = (long long)fpiv[o].size();
        pl.nnz_blk += p * (p + 1) / 2 + p * (long long)u.size();
    }
    pl.f_row0[F] = (int32_t)pl.rows.size();
    pl.nlev = F ? *std::max_element(level.begin(), level.end()) + 1 : 0;
    pl.lv_start.assign(pl.nlev + 1, 0);
    for (int i = 0; i < F; ++i) ++pl.lv_start[level[i] + 1];
    for (int l = 0; l < pl.nlev; ++l) pl.lv_start[l + 1] += pl.lv_start[l];
    pl.lv.resize(F);
    { std::vector<int32_t> c(pl.lv_start.begin(), pl.lv_start.end() - 1); for (int i = 0; i < F; ++i) pl.lv[c[level[i]]++] = i; }
    // checks: every free vertex a pivot once; a child's update rows are rows of its parent at the mapped position, in increasing order;
    // the assembled blocks lie in their front
    std::vector<int32_t> seen(n, 0);
    for (int i = 0; i < F; ++i) {
        const int nr = pl.f_m[i] / 6, npv = pl.f_np[i] / 6;
        for (int q = 0; q < npv; ++q) { const int v = pl.rows[pl.f_row0[i] + q]; if (v < 0 || v >= n || seen[v]++) return false; }
        if (nr > npv && par[i] < 0) return false;
        for (int q = npv; q < nr; ++q) {
            const int v = pl.rows[pl.f_row0[i] + q], t = pl.umap[pl.f_row0[i] + q], pr = par[i];
            if (v < 0 || v >= n || t < 0 || t >= pl.f_m[pr] / 6 || pl.rows[pl.f_row0[pr] + t] != v) return false;
            if (q > npv && t <= pl.umap[pl.f_row0[i] + q - 1]) return false;
        }
        for (int e = pl.as_start[i]; e < pl.as_start[i + 1]; ++e) {
            const int k = pl.as[3 * e], a = pl.as[3 * e + 1], c = pl.as[3 * e + 2];
            if (k < 0 || k >= nblk || a < 0 || a >= nr || c < 0 || c >= nr || pl.rows[pl.f_row0[i] + a] != blk_row[k] || pl.rows[pl.f_row0[i] + c] != blk_col[k]) return false;
        }
    }
    for (int v = 0; v < n; ++v) if (seen[v] != 1) return false;
    if (pl.as_start[F] != nblk) return false;
    for (int i = 0; i < F; ++i) for (int q = pl.ch_start[i]; q < pl.ch_start[i + 1]; ++q) if (par[pl.ch[q]] != i || pl.ch[q] >= i) return false;
    return true;
}

}  // namespace plba
