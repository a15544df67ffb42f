// plba_pgo_cov_hostcheck.cpp — a stand-alone program over plba_pgo_cov.h, the host side of plba_pose_graph_marginals: built with the
// address and undefined-behaviour sanitizers and run directly by tests/test_pgo_cov_cpu.py.  On a family of graphs (free ranks and
// their 6 x 6 blocks, as plba_pgo.hip builds them) it runs pgo_sparse_analyse and then checks
//   - every located place against a brute-force search of the fronts' rows; every edge and every (i, i) inside the pattern;
//   - pgo_cov_check on the located places;
//   - the long double walk (assemble, factor up the tree, selected inversion down it, locate) on diagonally dominant random blocks
//     (kappa <= 10) against a dense long double inverse (Cholesky and column solves inside the envelope), on every selected block
//     inside the pattern: the largest entry-wise difference of a block over the block's own largest entry, at most 1e-12.
// Prints "ok <graph>" per graph; any failure prints what differed and makes the exit status 1.
#include <cstdio>
#include <random>
#include <string>
#include <utility>

#include "plba_pgo_sparse.h"
#include "plba_pgo_cov.h"

using namespace plba;
typedef long double LDb;
typedef std::vector<std::pair<int, int>> Edges;

static int g_bad = 0;
static void fail(const std::string& name, const char* what, long a = 0, long b = 0) { printf("FAIL %s: %s (%ld, %ld)\n", name.c_str(), what, a, b); ++g_bad; }

static void run(const std::string& name, int n, Edges edges, bool all_pairs) {
    const int bad0 = g_bad;
    for (auto& e : edges) if (e.first < e.second) std::swap(e.first, e.second);      // row >= column
    for (int v = 0; v < n; ++v) edges.push_back({v, v});
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int32_t> br, bc;
    for (auto& e : edges) { br.push_back(e.first); bc.push_back(e.second); }
    const int nblk = (int)br.size();
    PgoSparsePlan pl;
    PgoCovPlan cp;
    if (!pgo_sparse_analyse(n, br, bc, pl)) return fail(name, "analyse");
    if (!pgo_cov_prepare(pl, cp)) return fail(name, "prepare");

    // the selection: every edge in both orientations, every (i, i), and pairs no edge joins
    Edges sel;
    for (auto& e : edges) { sel.push_back(e); if (e.first != e.second) sel.push_back({e.second, e.first}); }
    const size_t n_edge_sel = sel.size();
    if (all_pairs) { for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) sel.push_back({i, j}); }
    else {
        std::mt19937 rng(12345);
        sel.push_back({0, n - 1}); sel.push_back({n - 1, 0});
        for (int k = 0; k < 400; ++k) sel.push_back({(int)(rng() % n), (int)(rng() % n)});
    }
    std::vector<PgoCovPlace> places;
    std::vector<int32_t> ranks;
    for (size_t k = 0; k < sel.size(); ++k) {
        const int i = sel[k].first, j = sel[k].second;
        const PgoCovPlace c = pgo_cov_locate(pl, cp, i, j);
        places.push_back(c); ranks.push_back(i); ranks.push_back(j);
        // brute force: the front where the earlier eliminated of the two is a pivot, every row of it
        const int e = cp.v_elim[i] <= cp.v_elim[j] ? i : j, l = e == i ? j : i;
        PgoCovPlace want{-1, 0, 0, 0};
        for (int f = 0; f < pl.nfront && want.front < 0; ++f)
            for (int a = 0; a < pl.f_np[f] / 6 && want.front < 0; ++a) {
                if (pl.rows[pl.f_row0[f] + a] != e) continue;
                for (int q = 0; q < pl.f_m[f] / 6; ++q)
                    if (pl.rows[pl.f_row0[f] + q] == l) { want = PgoCovPlace{f, q, a, (i == e && i != j) ? 1 : 0}; break; }
            }
        if (want.front != c.front || (c.front >= 0 && (want.rpos != c.rpos || want.cpos != c.cpos || want.transposed != c.transposed))) fail(name, "place differs from the brute-force search", i, j);
        if (k < n_edge_sel && c.front < 0) fail(name, "an edge or (i, i) outside the pattern", i, j);
    }
    if (!pgo_cov_check(pl, cp, places, ranks)) fail(name, "pgo_cov_check");

    // ---- numbers: diagonally dominant random blocks, the walk against a dense inverse ---------------------------------------------
    const int N = 6 * n;
    std::mt19937_64 rng(777 + n);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<LDb> A((size_t)N * N, 0.0L), H((size_t)36 * nblk);
    for (int k = 0; k < nblk; ++k)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                if (br[k] == bc[k] && j >= i) continue;
                const LDb v = U(rng);
                A[(size_t)(6 * br[k] + i) * N + 6 * bc[k] + j] = v; A[(size_t)(6 * bc[k] + j) * N + 6 * br[k] + i] = v;
            }
    for (int r = 0; r < N; ++r) { LDb s = 0; for (int c = 0; c < N; ++c) if (c != r) s += std::fabs(A[(size_t)r * N + c]); A[(size_t)r * N + r] = 1.5L * s + 1.0L; }      // kappa <= 5
    for (int k = 0; k < nblk; ++k) for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) H[(size_t)36 * k + 6 * i + j] = A[(size_t)(6 * br[k] + i) * N + 6 * bc[k] + j];
    std::vector<LDb> Fm;
    if (pgo_cov_walk<LDb>(pl, cp, H, Fm) != -1) return fail(name, "the walk met a bad pivot");
    // dense Cholesky inside the envelope, then the columns the selection needs
    std::vector<int> first(N);
    for (int r = 0; r < N; ++r) { int c = 0; while (A[(size_t)r * N + c] == 0.0L) ++c; first[r] = c; }
    std::vector<LDb> L((size_t)N * N, 0.0L);
    for (int r = 0; r < N; ++r)
        for (int c = first[r]; c <= r; ++c) {
            LDb v = A[(size_t)r * N + c];
            for (int k = std::max(first[r], first[c]); k < c; ++k) v -= L[(size_t)r * N + k] * L[(size_t)c * N + k];
            L[(size_t)r * N + c] = r == c ? std::sqrt(v) : v / L[(size_t)c * N + c];
        }
    std::vector<char> need(n, 0);
    for (size_t k = 0; k < sel.size(); ++k) if (places[k].front >= 0) need[sel[k].second] = 1;
    std::vector<LDb> col((size_t)N * 6), inv_cols((size_t)n * N * 6, 0.0L);      // column vertex j: N x 6 at inv_cols + j N 6
    LDb worst = 0;
    for (int j = 0; j < n; ++j) {
        if (!need[j]) continue;
        for (int b = 0; b < 6; ++b) {
            LDb* x = &col[(size_t)b * N];
            // both solves inside the envelope: forward from the unit entry's row, backward column by column
            for (int r = 0; r < 6 * j + b; ++r) x[r] = 0.0L;
            for (int r = 6 * j + b; r < N; ++r) { LDb v = r == 6 * j + b ? 1.0L : 0.0L; for (int k = std::max(first[r], 6 * j + b); k < r; ++k) v -= L[(size_t)r * N + k] * x[k]; x[r] = v / L[(size_t)r * N + r]; }
            for (int r = N - 1; r >= 0; --r) { x[r] /= L[(size_t)r * N + r]; for (int k = first[r]; k < r; ++k) x[k] -= L[(size_t)r * N + k] * x[r]; }
            for (int r = 0; r < N; ++r) inv_cols[((size_t)j * N + r) * 6 + b] = x[r];
        }
    }
    for (size_t k = 0; k < sel.size(); ++k) {
        if (places[k].front < 0) continue;
        const int i = sel[k].first, j = sel[k].second;
        LDb scale = 0, err = 0;
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) scale = std::max(scale, std::fabs(inv_cols[((size_t)j * N + 6 * i + a) * 6 + b]));
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) err = std::max(err, std::fabs(pgo_cov_entry<LDb>(pl, Fm, places[k], a, b) - inv_cols[((size_t)j * N + 6 * i + a) * 6 + b]));
        worst = std::max(worst, err / scale);      // relative to the block's own largest entry
    }
    if (!(worst <= 1e-12L)) fail(name, "the walk differs from the dense inverse (1e-18 units)", (long)(worst * 1e18L));
    printf("%s %s: n %d fronts %d levels %d max_m %d  selected %zu  walk-vs-dense %.2Le\n", g_bad != bad0 ? "failed" : "checked", name.c_str(), n, pl.nfront, pl.nlev, pl.max_m, sel.size(), worst);
    if (g_bad == bad0) printf("ok %s\n", name.c_str());
}

static Edges chain(int n) { Edges e; for (int i = 0; i + 1 < n; ++i) e.push_back({i, i + 1}); return e; }
static Edges clique(int n) { Edges e; for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) e.push_back({i, j}); return e; }

int main() {
    for (int n : {1, 2, 16, 17, 40}) run("chain" + std::to_string(n), n, chain(n), true);
    { Edges e; for (int i = 1; i < 40; ++i) e.push_back({0, i}); run("star", 40, e, true); }
    { Edges e; e.push_back({2, 3}); run("fixed_hub", 40, e, true); }      // (the hub is fixed: its leaves are isolated free vertices)
    {
        Edges e;
        for (int i = 0; i < 23; ++i) e.push_back({i, i + 1});
        for (int i = 0; i < 21; i += 3) e.push_back({i, i + 2});
        for (int i = 24; i < 48; ++i) e.push_back({i, i + 1});
        for (int i = 24; i < 45; i += 4) e.push_back({i, i + 3});
        run("two_components", 49, e, true);
    }
    for (int n : {3, 4, 6, 9}) run("clique" + std::to_string(n), n, clique(n), true);
    {
        const int n = 300;
        Edges e = chain(n);
        for (int i = 0; i < n; ++i) for (int j = i + 2; j < std::min(n, i + 9); ++j) if ((i + j) % 2 == 0) e.push_back({i, j});
        e.push_back({3, n - 5}); e.push_back({17, n - 1}); e.push_back({28, n - 20});
        run("band300", n, e, false);
    }
    return g_bad ? 1 : 0;
}
