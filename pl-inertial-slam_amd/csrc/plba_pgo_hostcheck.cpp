// plba_pgo_hostcheck.cpp — the per-thread arithmetic of the pose-graph kernels (plba_pgo_dev.h) run on the CPU, for
// tests/test_pgo_exact_cpu.py: one linearisation of a graph (what k_pgo_edges<true> and k_pgo_sum compute), one update of the free
// vertices by a given step (k_pgo_update) and the errors at the updated poses (k_pgo_edges<false>).  Test plumbing with its own main:
// the product only ever runs these functions inside the kernels.
//
//   plba_pgo_hostcheck <in> <out>
// in : int32 nv ne n nblk nsrc cnt0 | X nv x 12 | ei ne | ej ne | meas ne x 12 | info ne x 36 | free_v n | blk_start nblk + 1 |
//      blk_src nsrc | blk_diag nblk | blk_row nblk | x 6 n               (ints int32, the rest double; cnt0: every oplus counter's start)
// out: erec ne x 120 | echi ne | Hblk nblk x 36 | b 6 n | X' nv x 12 | echi' ne | cnt nv (int32)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>      // __forceinline__ of PLBA_HD under hipcc

#include "plba_pgo_dev.h"

using namespace plba;
using namespace plba::pgo_dev;

namespace {
template <typename T> std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "plba_pgo_hostcheck: short input\n"); exit(2); }
    return v;
}
template <typename T> void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "plba_pgo_hostcheck: short output\n"); exit(2); }
}
void need(bool ok, const char* what) { if (!ok) { fprintf(stderr, "plba_pgo_hostcheck: %s\n", what); exit(2); } }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the input");
    const std::vector<int32_t> hd = rd<int32_t>(f, 6);
    const int nv = hd[0], ne = hd[1], n = hd[2], nblk = hd[3], nsrc = hd[4], cnt0 = hd[5];
    need(nv > 0 && ne >= 0 && n >= 0 && n <= nv && nblk >= 0 && nsrc >= 0, "bad header");
    std::vector<double> X = rd<double>(f, (size_t)12 * nv);
    const std::vector<int32_t> ei = rd<int32_t>(f, ne), ej = rd<int32_t>(f, ne);
    const std::vector<double> meas = rd<double>(f, (size_t)12 * ne), info = rd<double>(f, (size_t)36 * ne);
    const std::vector<int32_t> free_v = rd<int32_t>(f, n), blk_start = rd<int32_t>(f, (size_t)nblk + 1), blk_src = rd<int32_t>(f, nsrc),
                               blk_diag = rd<int32_t>(f, nblk), blk_row = rd<int32_t>(f, nblk);
    const std::vector<double> x = rd<double>(f, (size_t)6 * n);
    fclose(f);
    for (int k = 0; k < ne; ++k) need(ei[k] >= 0 && ei[k] < nv && ej[k] >= 0 && ej[k] < nv, "edge out of range");
    for (int k = 0; k < n; ++k) need(free_v[k] >= 0 && free_v[k] < nv, "free vertex out of range");
    for (int q = 0; q < nblk; ++q) need(blk_start[q] >= 0 && blk_start[q] <= blk_start[q + 1] && blk_start[q + 1] <= nsrc && blk_row[q] >= 0 && blk_row[q] < n, "block list out of range");
    for (int s = 0; s < nsrc; ++s) need(blk_src[s] >= 0 && (blk_src[s] >> 2) < ne, "source out of range");

    // the inverse measurements (pgo_stage_edges), then k_pgo_edges<true>: one record per edge
    std::vector<double> Zi((size_t)12 * ne), erec((size_t)PGO_REC * ne), echi(ne), echi2(ne);
    for (int k = 0; k < ne; ++k) iso_store(iso_inv(iso_load(&meas[(size_t)12 * k])), &Zi[(size_t)12 * k]);
    for (int k = 0; k < ne; ++k)
        pgo_edge_eval<true>(iso_load(&X[(size_t)12 * ei[k]]), iso_load(&X[(size_t)12 * ej[k]]), iso_load(&Zi[(size_t)12 * k]), &info[(size_t)36 * k], &echi[k], &erec[(size_t)PGO_REC * k]);
    // k_pgo_sum: every block's sources in the order of the list
    std::vector<double> Hblk((size_t)36 * nblk, 0.0), b((size_t)6 * n, 0.0);
    for (int q = 0; q < nblk; ++q)
        for (int l = 0; l < 42; ++l) {
            if (l >= 36 && !blk_diag[q]) continue;
            const int r = (l < 36) ? l / 6 : l - 36, c = l % 6;
            double acc = 0.0;
            for (int s = blk_start[q]; s < blk_start[q + 1]; ++s) {
                const int src = blk_src[s], k = src >> 2, slot = src & 3;
                const double* rec = &erec[(size_t)PGO_REC * k];
                if (l >= 36) acc -= rec[(slot == 0 ? 108 : 114) + r];
                else acc += pgo_block_term(rec, slot, r, c);
            }
            if (l < 36) Hblk[(size_t)36 * q + l] = acc;
            else b[(size_t)6 * blk_row[q] + r] = acc;
        }
    // k_pgo_update, then k_pgo_edges<false> at the updated poses
    std::vector<int32_t> cnt(nv, cnt0);
    for (int k = 0; k < n; ++k) { int c = cnt[free_v[k]]; pgo_vertex_oplus(&X[(size_t)12 * free_v[k]], &x[(size_t)6 * k], &c); cnt[free_v[k]] = c; }
    for (int k = 0; k < ne; ++k)
        pgo_edge_eval<false>(iso_load(&X[(size_t)12 * ei[k]]), iso_load(&X[(size_t)12 * ej[k]]), iso_load(&Zi[(size_t)12 * k]), &info[(size_t)36 * k], &echi2[k], nullptr);

    f = fopen(argv[2], "wb");
    need(f != nullptr, "cannot open the output");
    wr(f, erec); wr(f, echi); wr(f, Hblk); wr(f, b); wr(f, X); wr(f, echi2); wr(f, cnt);
    fclose(f);
    return 0;
}
