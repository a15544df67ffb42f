// Stand-alone host program around plba_covis_dev.h and include/plba_g2o/covis.h, used by tests/test_covis_cpu.py and
// tools/time_covis.py: it runs the shared header's text on the CPU.  Not linked into libplba_hip.so, never used by the product path.
//
//   plba_covis_hostcheck IN OUT
// IN:  int32 [K, Np, Nl, has_live, n_rows, min_count, idx, nv, n_loop, min_lm_ess_graph, min_lm_cov_graph, min_kf_local_map, kf]; uint8
//      live[K] (with has_live); int32 pt_start[Np + 1], pt_kf, ln_start[Nl + 1], ln_kf; int32 rows[n_rows]; double pose12[12 nv]; int32
//      loop_ij[2 n_loop]; double loop_meas12[12 n_loop].
// OUT: int32 row_start[n_rows + 1], col, cnt (plba_covis_rows); int32 cov[idx] (plba_covis_column); int32 ne, ei[ne], ej[ne], double
//      meas12[12 ne] (plba_covis_pose_graph); uint8 kf_local[K], pt_local[Np], ln_local[Nl], int32 counts3 (plba_covis_local_map of kf).
//      Exit code 3: the map or a query is refused.
//   plba_covis_hostcheck IN - REPS    timing: prints the best milliseconds of REPS repetitions of set, rows, pose_graph, column,
//      local_map, in that order, and writes nothing.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plba_g2o/covis.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s IN OUT | IN - REPS\n", argv[0]); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd, ps, pk, ls, lk, rows, loop_ij;
    std::vector<uint8_t> live;
    std::vector<double> pose, loop_meas;
    bool ok = rd(f, hd, 13);
    ok = ok && hd[0] >= 0 && hd[1] >= 0 && hd[2] >= 0 && hd[4] >= 0 && hd[6] >= 0 && hd[7] >= 0 && hd[8] >= 0;
    const int K = ok ? hd[0] : 0, Np = ok ? hd[1] : 0, Nl = ok ? hd[2] : 0, n_rows = ok ? hd[4] : 0, idx = ok ? hd[6] : 0, nv = ok ? hd[7] : 0, n_loop = ok ? hd[8] : 0;
    if (ok && hd[3]) ok = rd(f, live, (size_t)K);
    ok = ok && rd(f, ps, (size_t)Np + 1) && ps[(size_t)Np] >= 0 && rd(f, pk, (size_t)ps[(size_t)Np]);
    ok = ok && rd(f, ls, (size_t)Nl + 1) && ls[(size_t)Nl] >= 0 && rd(f, lk, (size_t)ls[(size_t)Nl]);
    ok = ok && rd(f, rows, (size_t)n_rows) && rd(f, pose, 12 * (size_t)nv) && rd(f, loop_ij, 2 * (size_t)n_loop) && rd(f, loop_meas, 12 * (size_t)n_loop);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: malformed input\n", argv[1]); return 2; }
    plba_g2o::CovisOptions o;
    o.min_lm_ess_graph = hd[9]; o.min_lm_cov_graph = hd[10]; o.min_kf_local_map = hd[11];
    const int min_count = hd[5], kf = hd[12];
    plba_g2o::CovisMap m;
    std::vector<int32_t> row_start, col, cnt, cov, ei, ej;
    std::vector<double> meas;
    std::vector<uint8_t> kl, pl, ll;
    int32_t c3[3] = {0, 0, 0};
    auto set = [&] { return m.set(K, live.empty() ? nullptr : live.data(), Np, ps.data(), pk.data(), Nl, ls.data(), lk.data()); };
    auto rows_ok = [&] {
        for (int r : rows) if (r < 0 || r >= K) return false;
        return idx < K;
    };
    if (!set()) { fprintf(stderr, "refused: %s\n", m.error().c_str()); return 3; }
    if (!rows_ok()) { fprintf(stderr, "refused: a requested keyframe is out of range\n"); return 3; }
    if (reps > 0) {
        auto best = [&](auto fn) {
            double b = 1e300;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                fn();
                b = std::min(b, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            return b;
        };
        const double t_set = best([&] { set(); });
        const double t_rows = best([&] { m.rows(n_rows, rows.data(), min_count, row_start, col, cnt); });
        const double t_pg = best([&] { m.pose_graph(o, nv, pose.data(), n_loop, loop_ij.data(), loop_meas.data(), ei, ej, meas); });
        const double t_col = best([&] { m.column(idx, cov); });
        const double t_lm = best([&] { m.local_map(o, kf, kl, pl, ll, c3); });
        printf("%.6f %.6f %.6f %.6f %.6f\n", t_set, t_rows, t_pg, t_col, t_lm);
        return 0;
    }
    m.rows(n_rows, rows.data(), min_count, row_start, col, cnt);
    m.column(idx, cov);
    if (!m.pose_graph(o, nv, pose.data(), n_loop, loop_ij.data(), loop_meas.data(), ei, ej, meas) || !m.local_map(o, kf, kl, pl, ll, c3)) {
        fprintf(stderr, "refused: a query\n");
        return 3;
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    const std::vector<int32_t> ne(1, (int32_t)ei.size()), counts(c3, c3 + 3);
    ok = wr(g, row_start) && wr(g, col) && wr(g, cnt) && wr(g, cov) && wr(g, ne) && wr(g, ei) && wr(g, ej) && wr(g, meas) && wr(g, kl) && wr(g, pl) && wr(g, ll) && wr(g, counts);
    ok = (fclose(g) == 0) && ok;
    return ok ? 0 : 2;
}
