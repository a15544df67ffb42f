// Stand-alone host program around plba_match_dev.h, used by tests/test_match_cpu.py and tools/time_match.py: it runs the shared header's
// text on the CPU in the kernels' tile order, or the plain-C++ drop-in of include/plba_g2o/match.h.  Not linked into libplba_hip.so,
// never used by the product path.
//
//   plba_match_hostcheck match IN OUT MODE [REPS]      MODE 0: match::match_problem per problem, with nn3; MODE 1: plba_g2o::match
// IN:  int32 [B, best_lr, has_nnr_b], float nnr, int32 a_start[B + 1], b_start[B + 1], uint8 desc1 (32 a row), desc2, float nnr_b[B] if has_nnr_b.
// OUT: int32 matches_12[a_start[B]], n_matches[B], nn3[3 a_start[B]] (MODE 1: -2 throughout, it has no such output).
//   plba_match_hostcheck loop IN OUT [REPS]            plba_g2o::is_loop_closure per candidate
// IN:  int32 [B, best_lr, use_points, use_lines], float [nnr_pt, nnr_ln], double [lc_inlier_ratio, fx, fy, cx, cy], int32 pa_start, pb_start,
//      la_start, lb_start (B + 1 each), then uint8 descPA, double P3A, uint8 descPB, double uvB, uint8 descLA, double sPeP6A, uint8 descLB, double l3B.
// OUT: per candidate int32 [common_pt, common_ls, ratio_ok, returned] and double [inl_ratio_pt, inl_ratio_ls, pose_inc as the call left it (6),
//      the report's pose_inc (6), T_inc (16), e]; then int32 pt_match, ln_match; then uint8 masks (points, lines): 1 where a matched pair is
//      still in the compacted lists of a candidate that returned true.
// REPS > 1 repeats the batch and prints the milliseconds per batch.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plba_g2o/match.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
static bool starts_ok(const std::vector<int32_t>& s) {
    if (s.empty() || s[0] != 0) return false;
    for (size_t i = 1; i < s.size(); ++i) if (s[i] < s[i - 1]) return false;
    return true;
}

static int run_match(const char* in, const char* out, int mode, int reps) {
    namespace mt = plba::match;
    FILE* f = fopen(in, "rb");
    if (!f) { perror(in); return 2; }
    std::vector<int32_t> hd, as, bs;
    std::vector<float> nnr, nnr_b;
    std::vector<uint8_t> dA, dB;
    bool ok = rd(f, hd, 3) && rd(f, nnr, 1);
    const int B = ok ? hd[0] : 0;
    ok = ok && B >= 1 && rd(f, as, (size_t)B + 1) && rd(f, bs, (size_t)B + 1) && starts_ok(as) && starts_ok(bs);
    const size_t NA = ok ? (size_t)as[B] : 0, NB = ok ? (size_t)bs[B] : 0;
    ok = ok && rd(f, dA, 32 * NA) && rd(f, dB, 32 * NB) && rd(f, nnr_b, hd[2] ? (size_t)B : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", in); return 2; }
    std::vector<int32_t> m(NA, -1), cnt((size_t)B, 0), nn3(3 * NA, -2);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; ++rep)
        for (int b = 0; b < B; ++b) {
            const int n1 = as[b + 1] - as[b], n2 = bs[b + 1] - bs[b];
            const float r = hd[2] ? nnr_b[b] : nnr[0];
            const uint8_t *d1 = dA.data() + 32 * (size_t)as[b], *d2 = dB.data() + 32 * (size_t)bs[b];
            if (mode == 0) {
                std::vector<int32_t> nn21(3 * (size_t)n2 + 3, -1);
                // an empty side: no search runs and every triple is -1, as the finishing launch writes them
                if (n2 == 0) for (int i = 0; i < 3 * n1; ++i) nn3[3 * (size_t)as[b] + i] = -1;
                cnt[b] = (n1 == 0 || n2 == 0) ? 0 : mt::match_problem(d1, n1, d2, n2, r, hd[1] ? mt::BEST_LR : 0, m.data() + as[b], nn3.data() + 3 * (size_t)as[b], nn21.data());
                if (n2 == 0) for (int i = 0; i < n1; ++i) m[(size_t)as[b] + i] = -1;
            } else {
                std::vector<int> m12;
                cnt[b] = plba_g2o::match(d1, n1, d2, n2, r, m12, hd[1] != 0);
                for (int i = 0; i < n1; ++i) m[(size_t)as[b] + i] = m12[(size_t)i];
            }
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    if (reps > 1) printf("%.6f\n", ms);
    f = fopen(out, "wb");
    if (!f) { perror(out); return 2; }
    ok = wr(f, m) && wr(f, cnt) && wr(f, nn3);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}

static int run_loop(const char* in, const char* out, int reps) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror(in); return 2; }
    std::vector<int32_t> hd, pa, pb, la, lb;
    std::vector<float> nnr;
    std::vector<double> par, P3, uv, pq, l3;
    std::vector<uint8_t> dPA, dPB, dLA, dLB;
    bool ok = rd(f, hd, 4) && rd(f, nnr, 2) && rd(f, par, 5);
    const int B = ok ? hd[0] : 0;
    ok = ok && B >= 1 && rd(f, pa, (size_t)B + 1) && rd(f, pb, (size_t)B + 1) && rd(f, la, (size_t)B + 1) && rd(f, lb, (size_t)B + 1) && starts_ok(pa) &&
         starts_ok(pb) && starts_ok(la) && starts_ok(lb);
    const size_t NpA = ok ? (size_t)pa[B] : 0, NpB = ok ? (size_t)pb[B] : 0, NlA = ok ? (size_t)la[B] : 0, NlB = ok ? (size_t)lb[B] : 0;
    ok = ok && rd(f, dPA, 32 * NpA) && rd(f, P3, 3 * NpA) && rd(f, dPB, 32 * NpB) && rd(f, uv, 2 * NpB) && rd(f, dLA, 32 * NlA) && rd(f, pq, 6 * NlA) &&
         rd(f, dLB, 32 * NlB) && rd(f, l3, 3 * NlB);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", in); return 2; }
    plba_g2o::LoopConfig cfg;
    cfg.best_lr = hd[1] != 0; cfg.has_points = hd[2] != 0; cfg.has_lines = hd[3] != 0; cfg.min_ratio_12p = nnr[0]; cfg.min_ratio_12l = nnr[1];
    cfg.lc_inlier_ratio = par[0]; cfg.relpose.fx = par[1]; cfg.relpose.fy = par[2]; cfg.relpose.cx = par[3]; cfg.relpose.cy = par[4];
    std::vector<int32_t> oi(4 * (size_t)B), mp(NpA, -1), ml(NlA, -1);
    std::vector<double> od(31 * (size_t)B, 0.0);
    std::vector<uint8_t> ip(NpA, 0), il(NlA, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; ++rep)
        for (int b = 0; b < B; ++b) {
            plba_g2o::KeyFrameFeatures k0, k1;
            k0.n_pt = pa[b + 1] - pa[b]; k0.n_ls = la[b + 1] - la[b]; k1.n_pt = pb[b + 1] - pb[b]; k1.n_ls = lb[b + 1] - lb[b];
            k0.pdesc = dPA.data() + 32 * (size_t)pa[b]; k0.P3 = P3.data() + 3 * (size_t)pa[b]; k0.ldesc = dLA.data() + 32 * (size_t)la[b]; k0.sPeP6 = pq.data() + 6 * (size_t)la[b];
            k1.pdesc = dPB.data() + 32 * (size_t)pb[b]; k1.uv = uv.data() + 2 * (size_t)pb[b]; k1.ldesc = dLB.data() + 32 * (size_t)lb[b]; k1.l3 = l3.data() + 3 * (size_t)lb[b];
            std::vector<plba_g2o::Vector4i> pi, li;
            std::vector<plba_g2o::PointFeature> pts;
            std::vector<plba_g2o::LineFeature> lns;
            double pose[6] = {0, 0, 0, 0, 0, 0};
            plba_g2o::LoopReport r;
            const bool ret = plba_g2o::is_loop_closure(k0, k1, pose, pi, li, pts, lns, cfg, &r);
            int32_t* q = &oi[4 * (size_t)b];
            q[0] = r.common_pt; q[1] = r.common_ls; q[2] = r.ratio_ok; q[3] = ret ? 1 : 0;
            double* o = &od[31 * (size_t)b];
            o[0] = r.inl_ratio_pt; o[1] = r.inl_ratio_ls;
            memcpy(o + 2, pose, 48);
            if (r.ratio_ok) { memcpy(o + 8, r.relpose.pose_inc, 48); memcpy(o + 14, r.relpose.T_inc, 128); o[30] = r.relpose.e; }
            for (int i = 0; i < k0.n_pt; ++i) { mp[(size_t)pa[b] + i] = r.pt_match[(size_t)i]; ip[(size_t)pa[b] + i] = 0; }
            for (int i = 0; i < k0.n_ls; ++i) { ml[(size_t)la[b] + i] = r.ln_match[(size_t)i]; il[(size_t)la[b] + i] = 0; }
            if (ret) {
                for (const auto& v : pi) ip[(size_t)pa[b] + (size_t)v[1]] = 1;
                for (const auto& v : li) il[(size_t)la[b] + (size_t)v[1]] = 1;
            }
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    if (reps > 1) printf("%.6f\n", ms);
    f = fopen(out, "wb");
    if (!f) { perror(out); return 2; }
    ok = wr(f, oi) && wr(f, od) && wr(f, mp) && wr(f, ml) && wr(f, ip) && wr(f, il);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc >= 5 && !strcmp(argv[1], "match")) {
        const int mode = atoi(argv[4]), reps = argc > 5 ? atoi(argv[5]) : 1;
        if ((mode != 0 && mode != 1) || reps < 1) { fprintf(stderr, "MODE is 0 or 1, REPS >= 1\n"); return 2; }
        return run_match(argv[2], argv[3], mode, reps);
    }
    if (argc >= 4 && !strcmp(argv[1], "loop")) {
        const int reps = argc > 4 ? atoi(argv[4]) : 1;
        if (reps < 1) { fprintf(stderr, "REPS >= 1\n"); return 2; }
        return run_loop(argv[2], argv[3], reps);
    }
    fprintf(stderr, "usage: %s match IN OUT MODE [REPS] | loop IN OUT [REPS]\n", argv[0]);
    return 2;
}
