// Stand-alone host program around plba_bow_dev.h and include/plba_g2o/bow.h, used by tests/test_bow_cpu.py and tools/time_bow.py: it
// runs the shared header's text on the CPU in the kernels' orders of summation, one keyframe after the other.  Not linked into
// libplba_hip.so, never used by the product path.
//
//   plba_bow_hostcheck IN OUT
// IN:  int32 [mode, weighting_p, weighting_l, n_nodes_p, n_nodes_l, n_kf, has_cov, topk, lc_kf_dist, lc_kf_max_dist, lc_nkf_closest,
//      min_lm_cov_graph, min_kf_local_map, n_removed]; per vocabulary (points, lines; absent when its n_nodes is 0): int32 parent[n], uint8
//      desc[32 n], double weight[n], int32 word_id[n]; int32 pt_start[n_kf + 1], ln_start[n_kf + 1]; uint8 pdesc, double pl (2 a row),
//      uint8 ldesc, double spl_epl (4 a row); int32 removed[2 n_removed]: pairs (a, kf), keyframe kf dies once a keyframes are in; with
//      has_cov int32 cov, keyframe idx's idx entries one after the other.
// OUT: double score_p, score_l, score (rows of idx + 1), float conf; with has_cov int32 cand_i[n_kf x 20] (is_candidate, kf_prev, n_closest,
//      n_eligible, topk) and double cand_d[n_kf x 18] (best_score, lc_min_score, topk_score); int32 pt_word, ln_word; int32 pt_nnz[n_kf],
//      ln_nnz[n_kf]; int32 pt_id, double pt_val, int32 ln_id, double ln_val (a row per descriptor, a keyframe's vector at its first row, -2 / 0
//      behind it).
//   plba_bow_hostcheck IN - REPS [STORED]    timing: the keyframes before the last are only transformed, the database is STORED of those
//      vectors, taken round and round (default: each once), and the LAST keyframe's insertion against it (transform, scores, decision on a zero covisibility column) is
//      repeated REPS times; prints the milliseconds per repetition and writes nothing.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plba_g2o/bow.h"

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

struct VocIn {
    std::vector<int32_t> parent, word;
    std::vector<uint8_t> desc;
    std::vector<double> weight;
};

int main(int argc, char** argv) {
    namespace bw = plba::bow;
    if (argc < 3) { fprintf(stderr, "usage: %s IN OUT | IN - REPS [STORED]\n", argv[0]); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 1, n_stored = argc > 4 ? atoi(argv[4]) : -1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd, ps, ls, removed, cov;
    std::vector<uint8_t> pdesc, ldesc;
    std::vector<double> pl, se;
    VocIn vin[2];
    bool ok = rd(f, hd, 14);
    const int mode = ok ? hd[0] : 0, n_kf = ok ? hd[5] : 0, has_cov = ok ? hd[6] : 0, n_removed = ok ? hd[13] : 0;
    ok = ok && mode >= 0 && mode <= 2 && n_kf >= 1 && n_removed >= 0 && hd[3] >= 0 && hd[4] >= 0 && hd[7] >= 0 && hd[7] <= bw::TOPK_MAX;
    for (int k = 0; ok && k < 2; ++k) {
        const size_t n = (size_t)hd[3 + k];
        ok = rd(f, vin[k].parent, n) && rd(f, vin[k].desc, 32 * n) && rd(f, vin[k].weight, n) && rd(f, vin[k].word, n);
    }
    ok = ok && rd(f, ps, (size_t)n_kf + 1) && rd(f, ls, (size_t)n_kf + 1) && starts_ok(ps) && starts_ok(ls);
    const size_t Np = ok ? (size_t)ps[n_kf] : 0, Nl = ok ? (size_t)ls[n_kf] : 0;
    ok = ok && rd(f, pdesc, 32 * Np) && rd(f, pl, 2 * Np) && rd(f, ldesc, 32 * Nl) && rd(f, se, 4 * Nl) && rd(f, removed, 2 * (size_t)n_removed);
    const size_t C = (size_t)n_kf * ((size_t)n_kf - 1) / 2, R = C + (size_t)n_kf;
    ok = ok && rd(f, cov, has_cov ? C : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", argv[1]); return 2; }
    plba_g2o::Vocabulary voc[2];
    for (int k = 0; k < 2; ++k)
        if (hd[3 + k] && !voc[k].set(hd[1 + k], hd[3 + k], vin[k].parent.data(), vin[k].desc.data(), vin[k].weight.data(), vin[k].word.data())) {
            fprintf(stderr, "vocabulary %d: %s\n", k, voc[k].error().c_str());
            return 3;
        }
    if ((mode != bw::MODE_LINES && voc[0].empty()) || (mode != bw::MODE_POINTS && voc[1].empty())) { fprintf(stderr, "no vocabulary for a kind the mode uses\n"); return 3; }
    plba_g2o::LoopCandidateConfig cfg;
    cfg.topk = hd[7]; cfg.lc_kf_dist = hd[8]; cfg.lc_kf_max_dist = hd[9]; cfg.lc_nkf_closest = hd[10]; cfg.min_lm_cov_graph = hd[11]; cfg.min_kf_local_map = hd[12];

    if (reps > 1) {      // timing
        std::vector<plba_g2o::BowStored> pool, stored;
        auto frame = [&](int idx) {
            plba_g2o::BowKeyFrame kf;
            kf.n_pt = ps[idx + 1] - ps[idx]; kf.n_ls = ls[idx + 1] - ls[idx];
            kf.pdesc = pdesc.data() + 32 * (size_t)ps[idx]; kf.pl = pl.data() + 2 * (size_t)ps[idx];
            kf.ldesc = ldesc.data() + 32 * (size_t)ls[idx]; kf.spl_epl = se.data() + 4 * (size_t)ls[idx];
            return kf;
        };
        for (int idx = 0; idx + 1 < n_kf; ++idx) {
            plba_g2o::BowStored st;
            const plba_g2o::BowKeyFrame kf = frame(idx);
            if (mode != bw::MODE_LINES) voc[0].transform(kf.pdesc, kf.n_pt, st.p);
            if (mode != bw::MODE_POINTS) voc[1].transform(kf.ldesc, kf.n_ls, st.l);
            pool.push_back(st);
        }
        const size_t want = n_stored >= 0 && !pool.empty() ? (size_t)n_stored : pool.size();
        for (size_t i = 0; i < want; ++i) stored.push_back(pool[i % pool.size()]);
        const std::vector<int32_t> zcov(stored.size(), 0);
        const std::vector<uint8_t> all_live(stored.size(), 1);
        const plba_g2o::BowKeyFrame kf = frame(n_kf - 1);
        plba_g2o::BowStored mine;
        plba_g2o::BowColumn col;
        int prev = -1, found = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int rep = 0; rep < reps; ++rep) {
            plba_g2o::insert_kf_bow_vector(mode, voc[0], voc[1], kf, stored, mine, col);
            found += plba_g2o::look_for_loop_candidates(col.conf.data(), zcov.data(), all_live.data(), (int)stored.size(), prev, cfg) ? 1 : 0;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
        printf("%.6f %d %zu\n", ms, found, stored.size());
        return 0;
    }
    std::vector<double> o_sp, o_sl, o_s, cand_d;
    std::vector<float> o_cf;
    std::vector<int32_t> cand_i, pt_word(Np, -1), ln_word(Nl, -1), pt_nnz((size_t)n_kf, 0), ln_nnz((size_t)n_kf, 0), pt_id(Np, -2), ln_id(Nl, -2);
    std::vector<double> pt_val(Np, 0.0), ln_val(Nl, 0.0);
    o_sp.reserve(R); o_sl.reserve(R); o_s.reserve(R); o_cf.reserve(R);
    std::vector<plba_g2o::BowStored> stored;
    std::vector<uint8_t> live;
    size_t cov_at = 0;
    for (int idx = 0; idx < n_kf; ++idx) {
        for (int r = 0; r < n_removed; ++r)
            if (removed[2 * (size_t)r] == idx && removed[2 * (size_t)r + 1] >= 0 && removed[2 * (size_t)r + 1] < idx) {
                stored[(size_t)removed[2 * (size_t)r + 1]].live = false; live[(size_t)removed[2 * (size_t)r + 1]] = 0;
            }
        plba_g2o::BowKeyFrame kf;
        kf.n_pt = ps[idx + 1] - ps[idx]; kf.n_ls = ls[idx + 1] - ls[idx];
        kf.pdesc = pdesc.data() + 32 * (size_t)ps[idx]; kf.pl = pl.data() + 2 * (size_t)ps[idx];
        kf.ldesc = ldesc.data() + 32 * (size_t)ls[idx]; kf.spl_epl = se.data() + 4 * (size_t)ls[idx];
        plba_g2o::BowStored mine;
        plba_g2o::BowColumn col;
        plba_g2o::LoopCandidate cand;
        plba_g2o::insert_kf_bow_vector(mode, voc[0], voc[1], kf, stored, mine, col);
        if (has_cov) {
            int prev = -1;
            plba_g2o::look_for_loop_candidates(col.conf.data(), cov.data() + cov_at, live.data(), idx, prev, cfg, &cand);
        }
        o_sp.insert(o_sp.end(), col.score_p.begin(), col.score_p.end()); o_sl.insert(o_sl.end(), col.score_l.begin(), col.score_l.end());
        o_s.insert(o_s.end(), col.score.begin(), col.score.end()); o_cf.insert(o_cf.end(), col.conf.begin(), col.conf.end());
        if (has_cov) {
            cand_i.push_back(cand.is_candidate); cand_i.push_back(cand.kf_prev); cand_i.push_back(cand.n_closest); cand_i.push_back(cand.n_eligible);
            cand_d.push_back(cand.best_score); cand_d.push_back(cand.lc_min_score);
            for (int k = 0; k < bw::TOPK_MAX; ++k) { cand_i.push_back(cand.topk[k]); cand_d.push_back(cand.topk_score[k]); }
            cov_at += (size_t)idx;
        }
        // the words again, for the output (the column's call does not return them)
        std::vector<int32_t> w;
        plba_g2o::BowVector v;
        if (mode != bw::MODE_LINES) {
            voc[0].transform(kf.pdesc, kf.n_pt, v, &w);
            for (int i = 0; i < kf.n_pt; ++i) pt_word[(size_t)ps[idx] + i] = w[(size_t)i];
            pt_nnz[(size_t)idx] = (int32_t)v.id.size();
            for (size_t e = 0; e < v.id.size(); ++e) { pt_id[(size_t)ps[idx] + e] = v.id[e]; pt_val[(size_t)ps[idx] + e] = v.val[e]; }
        }
        if (mode != bw::MODE_POINTS) {
            voc[1].transform(kf.ldesc, kf.n_ls, v, &w);
            for (int i = 0; i < kf.n_ls; ++i) ln_word[(size_t)ls[idx] + i] = w[(size_t)i];
            ln_nnz[(size_t)idx] = (int32_t)v.id.size();
            for (size_t e = 0; e < v.id.size(); ++e) { ln_id[(size_t)ls[idx] + e] = v.id[e]; ln_val[(size_t)ls[idx] + e] = v.val[e]; }
        }
        stored.push_back(mine); live.push_back(1);
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    ok = wr(g, o_sp) && wr(g, o_sl) && wr(g, o_s) && wr(g, o_cf) && wr(g, cand_i) && wr(g, cand_d) && wr(g, pt_word) && wr(g, ln_word) && wr(g, pt_nnz) &&
         wr(g, ln_nnz) && wr(g, pt_id) && wr(g, pt_val) && wr(g, ln_id) && wr(g, ln_val);
    ok = (fclose(g) == 0) && ok;
    return ok ? 0 : 2;
}
