// plba_lba_sparse_hostcheck.cpp — a stand-alone program over plba_lba_sparse.h, the block list of the reduced camera matrix that
// plba_lba_visual builds for its sparse solve (plba_lba_options.solver = 1).  Built with a plain C++ compiler under the address and
// undefined-behaviour sanitizers and run directly by tests/test_lba_sparse_cpu.py.  Every list is compared, element by element, with a
// brute-force enumeration: for every keyframe pair la <= lb in ascending order, every landmark, every ordered pair of its observations;
// lba_for_pairs, which both solvers' lists are built from, is run on its own as well.
// Prints one line per window, `ok <window>`, and exits 0; the first failed check prints its text and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plba_lba_sparse.h"

using namespace plba;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Win {
    int K = 0, n_fixed = 0;
    std::vector<std::vector<int>> tracks;      // keyframes of each landmark (a keyframe may repeat)
};

static void check(const char* name, const Win& w) {
    std::vector<int32_t> kf_loc(w.K), lm_start{0}, obs_kf;
    for (int k = 0; k < w.K; ++k) kf_loc[k] = k < w.n_fixed ? -1 : k - w.n_fixed;
    for (const auto& t : w.tracks) { for (int k : t) { CHECK(k >= 0 && k < w.K); obs_kf.push_back(k); } lm_start.push_back((int32_t)obs_kf.size()); }
    const int Nkf = w.K - w.n_fixed, L = (int)w.tracks.size();
    LbaBlockList bl;
    CHECK(lba_block_list(Nkf, L, lm_start.data(), obs_kf.data(), kf_loc.data(), bl));
    // brute force
    std::vector<int32_t> row, col, start, ent;
    for (int la = 0; la < Nkf; ++la)
        for (int lb = la; lb < Nkf; ++lb) {
            const size_t before = ent.size();
            for (int l = 0; l < L; ++l)
                for (int ea = lm_start[l]; ea < lm_start[l + 1]; ++ea)
                    for (int eb = lm_start[l]; eb < lm_start[l + 1]; ++eb)
                        if (kf_loc[obs_kf[ea]] == la && kf_loc[obs_kf[eb]] == lb) { ent.push_back(ea); ent.push_back(eb); }
            if (la == lb || ent.size() > before) { row.push_back(lb); col.push_back(la); start.push_back((int32_t)(before / 2)); }
        }
    start.push_back((int32_t)(ent.size() / 2));
    CHECK(bl.nent == (int64_t)(ent.size() / 2));
    CHECK(bl.blk_row == row);
    CHECK(bl.blk_col == col);
    CHECK(bl.blk_start == start);
    CHECK(bl.pair_ent == ent);
    // the shared enumerator on its own, as the dense solver's list takes it: the same entries, ea ascending and eb ascending within it
    int64_t seen = 0;
    int pea = -1, peb = -1;
    lba_for_pairs(L, lm_start.data(), obs_kf.data(), kf_loc.data(), [&](int la, int lb, int ea, int eb) {
        CHECK(la >= 0 && la <= lb && kf_loc[obs_kf[ea]] == la && kf_loc[obs_kf[eb]] == lb);
        CHECK(ea > pea || (ea == pea && eb > peb));
        pea = ea; peb = eb; ++seen;
    });
    CHECK(seen == bl.nent);
    // what the analysis and the kernels rely on: a diagonal block per keyframe, row >= column, no block twice, entries of the block's keyframes
    std::vector<int> diag(Nkf, 0);
    for (size_t k = 0; k < bl.blk_row.size(); ++k) {
        CHECK(bl.blk_row[k] >= bl.blk_col[k] && bl.blk_col[k] >= 0 && bl.blk_row[k] < Nkf);
        if (bl.blk_row[k] == bl.blk_col[k]) ++diag[bl.blk_row[k]];
        if (k) CHECK(bl.blk_col[k] > bl.blk_col[k - 1] || (bl.blk_col[k] == bl.blk_col[k - 1] && bl.blk_row[k] > bl.blk_row[k - 1]));
        CHECK(bl.blk_start[k] <= bl.blk_start[k + 1]);
        for (int t = bl.blk_start[k]; t < bl.blk_start[k + 1]; ++t)
            CHECK(kf_loc[obs_kf[bl.pair_ent[2 * t]]] == bl.blk_col[k] && kf_loc[obs_kf[bl.pair_ent[2 * t + 1]]] == bl.blk_row[k]);
    }
    for (int i = 0; i < Nkf; ++i) CHECK(diag[i] == 1);
    printf("ok %s\n", name);
}

// n_local keyframes behind 2 fixed ones; `per` landmarks first seen in every keyframe, each over `len` consecutive keyframes
static Win band(int n_local, int len, int per) {
    Win w; w.K = n_local + 2; w.n_fixed = 2;
    for (int k = 0; k < w.K; ++k)
        for (int i = 0; i < per; ++i) {
            std::vector<int> t;
            for (int q = k; q < k + len && q < w.K; ++q) t.push_back(q);
            if (t.size() >= 2) w.tracks.push_back(t);
        }
    return w;
}

int main() {
    check("band12", band(12, 4, 3));
    check("band17", band(17, 4, 3));
    check("band40", band(40, 4, 2));
    { Win w = band(40, 4, 2); for (int i = 0; i < 3; ++i) w.tracks.push_back({6, 7, 33, 34}); check("revisit40", w); }
    { Win w; w.K = 22; w.n_fixed = 2; std::vector<int> all; for (int k = 0; k < 22; ++k) all.push_back(k); for (int i = 0; i < 5; ++i) w.tracks.push_back(all); check("full20", w); }
    {   // two trajectories that share no landmark
        Win w; w.K = 26; w.n_fixed = 2;
        for (int h = 0; h < 2; ++h)
            for (int k = 0; k < 12; ++k)
                for (int i = 0; i < 2; ++i) { std::vector<int> t{h}; for (int q = k; q < k + 3 && q < 12; ++q) t.push_back(2 + 12 * h + q); w.tracks.push_back(t); }
        check("components", w);
    }
    { Win w = band(12, 4, 2); w.K += 1; for (int i = 0; i < 4; ++i) w.tracks.push_back({0, 1, 14}); check("lonely", w); }      // keyframe 14: landmarks otherwise seen from fixed keyframes only
    { Win w = band(5, 3, 2); w.tracks.push_back({2, 3, 3, 4}); check("duplicate", w); }      // a landmark seen twice from one keyframe
    { Win w = band(5, 3, 2); w.K += 1; check("unobserved", w); }      // the last keyframe observes nothing: an empty diagonal block
    { Win w; w.K = 3; w.n_fixed = 3; w.tracks.push_back({0, 1, 2}); check("all_fixed", w); }
    { Win w; w.K = 3; w.n_fixed = 1; check("no_landmark", w); }
    return 0;
}
