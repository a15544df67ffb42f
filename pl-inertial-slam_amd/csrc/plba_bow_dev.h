// plba_bow_dev.h — the arithmetic of place recognition (plba_bow_*, include/plba.h), shared by the kernels (plba_bow.hip), the host
// check (plba_bow_hostcheck.cpp) and the plain-C++ drop-in (include/plba_g2o/bow.h).
//
// DBoW2's vocabulary-tree descent (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1198-1239), the bag-of-words vector
// (:1046-1102, src/DBoW2/BowVector.cpp:34-84), the L1 score (src/DBoW2/ScoringObject.cpp:23-68), the three insertKFBowVector* scores
// (src/mapHandler.cpp:3116-3237) and lookForLoopCandidates (:3239-3299).  Orders of summation, the same on the device and here:
//  - a word's value: its weight added once per occurrence (addWeight), in a chain;
//  - the L1 norm: the values in ascending word id, in a chain;
//  - a score, a mean and a sum of squares: LANE-TREE order over the J terms t_0 .. t_{J-1} (for a score: one term per entry of the
//    STORED vector, 0 where the query lacks the word): 64 partial sums, partial l the chain t_l + t_{l+64} + ..., then five pairwise
//    rounds p_l <- p_l + p_{l xor o}, o = 32, 16, 8, 4, 2, 1.  It depends on J alone, not on the batch or the database size.
// No product is contracted with a sum (fp contract off), so the host compiler's code rounds as the device's does.
#pragma once
#include <cmath>
#include <cstdint>

#include "plba_match_dev.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace plba {
namespace bow {

constexpr int MAX_DESC = 8192;          // descriptors of one kind in one keyframe
constexpr int LANES = 64;
constexpr int STOPPED = 0x7fffffff;     // sort key of a descriptor whose word is stopped (weight not > 0): behind every word id
constexpr int TOPK_MAX = 16;
constexpr int TF_IDF = 0, TF = 1, IDF = 2, BINARY = 3;            // WeightingType
constexpr int MODE_COMBINED = 0, MODE_POINTS = 1, MODE_LINES = 2;

MT_HD bool accumulates(int weighting) { return weighting == TF_IDF || weighting == TF; }      // addWeight; otherwise addIfNotExist

// ScoringObject.cpp:41: one common word's term; the score is -sum / 2 (:63)
MT_HD double l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
MT_HD double l1_finish(double sum) { return -sum / 2.0; }

// mapHandler.cpp:3224-3226, literally: an empty kind gives NaN through 0 / 0 and through vector_stdv's 1.0 / 0 * 0
MT_HD double combined_score(double score_p, double score_l, int n_pt, int n_ls, double std_pt, double std_ls) {
    const double std_pl = std_ls + std_pt;
    const int n_pl = n_pt + n_ls;
    double score = 0.0;
    score += (score_p * n_pt + score_l * n_ls) / n_pl;
    score += (score_p * std_pt + score_l * std_ls) / std_pl;
    return score;
}
MT_HD double mode_score(int mode, double score_p, double score_l, int n_pt, int n_ls, double std_pt, double std_ls) {
    if (mode == MODE_POINTS) return score_p;
    if (mode == MODE_LINES) return score_l;
    return combined_score(score_p, score_l, n_pt, n_ls, std_pt, std_ls);
}
// stvo-pl/src/auxiliar.cpp:504-513 from the two sums: sqrt(1.0 / n * e)
MT_HD double stdv_finish(int n, double e) { return sqrt(1.0 / (double)n * e); }

// the entry of the sorted ids that equals key, or -1
template <class IdPtr>
MT_HD int find_word(IdPtr ids, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && ids[lo] == key) ? lo : -1;
}

// lookForLoopCandidates' predicates (:3246-3248, :3266)
MT_HD bool eligible(int i, int idx, int lc_kf_dist, bool live) { return live && i < idx - lc_kf_dist; }
MT_HD bool in_min_scan(int cov_i, int i, int idx, int min_lm_cov_graph, int min_kf_local_map) {
    return cov_i >= min_lm_cov_graph || idx - i <= min_kf_local_map + 3;
}
// where row b of a call's score outputs begins: rows of n0 + b' + 1 entries; and of its covisibility columns: rows of n0 + b'
MT_HD size_t score_row(int b, int n0) { return (size_t)b * ((size_t)n0 + 1) + (size_t)b * (size_t)(b > 0 ? b - 1 : 0) / 2; }
MT_HD size_t cov_row(int b, int n0) { return (size_t)b * (size_t)n0 + (size_t)b * (size_t)(b > 0 ? b - 1 : 0) / 2; }

}  // namespace bow
}  // namespace plba

// ---- host only (plain inline functions: the device pass parses them and emits nothing) ------------------------------------------------
#include <algorithm>
#include <string>
#include <vector>

namespace plba {
namespace bow {

// ---- the vocabulary's plan: a pure host function ---------------------------------------------------------------------------------------
// The nodes are laid out again breadth first, so that a node's children are contiguous and in load()'s order (ascending node index,
// TemplatedVocabulary.h:1458-1471).  order[new] = old; child0 / nchild / word per NEW index; n_words = the largest word id + 1.
struct VocPlan {
    std::vector<int32_t> order, child0, nchild, word;
    int n_words = 0;
    std::string err;      // empty: the tree is well formed
};
inline VocPlan plan_vocabulary(int n_nodes, const int32_t* parent, const int32_t* word_id) {
    VocPlan pl;
    if (n_nodes < 2 || !parent || !word_id) { pl.err = "a vocabulary has a root and at least one word"; return pl; }
    std::vector<int32_t> cnt((size_t)n_nodes, 0), first((size_t)n_nodes + 1, 0), kids((size_t)n_nodes, 0);
    for (int i = 1; i < n_nodes; ++i) {
        if (parent[i] < 0 || parent[i] >= i) { pl.err = "parent[" + std::to_string(i) + "] is not a smaller node index"; return pl; }
        ++cnt[(size_t)parent[i]];
    }
    for (int i = 0; i < n_nodes; ++i) first[(size_t)i + 1] = first[(size_t)i] + cnt[(size_t)i];
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int i = 1; i < n_nodes; ++i) kids[(size_t)fill[(size_t)parent[i]]++] = i;      // ascending i within a parent
    pl.order.reserve((size_t)n_nodes); pl.order.push_back(0);
    pl.child0.assign((size_t)n_nodes, 0); pl.nchild.assign((size_t)n_nodes, 0); pl.word.assign((size_t)n_nodes, -1);
    for (size_t at = 0; at < pl.order.size(); ++at) {      // every node is reached: its parent has a smaller index
        const int old = pl.order[at];
        pl.child0[at] = (int32_t)pl.order.size(); pl.nchild[at] = cnt[(size_t)old];
        for (int c = first[(size_t)old]; c < first[(size_t)old + 1]; ++c) pl.order.push_back(kids[(size_t)c]);
    }
    std::vector<uint8_t> seen((size_t)n_nodes, 0);
    for (int at = 0; at < n_nodes; ++at) {
        const int old = pl.order[(size_t)at], w = word_id[old];
        if (pl.nchild[(size_t)at] > 0) continue;      // an inner node: its word id is not read
        if (w < 0) { pl.err = "leaf " + std::to_string(old) + " has no word id"; return pl; }
        if (w >= n_nodes) { pl.err = "word id " + std::to_string(w) + " is not below n_nodes"; return pl; }
        if (seen[(size_t)w]) { pl.err = "word id " + std::to_string(w) + " appears twice"; return pl; }
        seen[(size_t)w] = 1;
        pl.word[(size_t)at] = w;
        pl.n_words = std::max(pl.n_words, w + 1);
    }
    return pl;
}

// ---- the host's form of the launches, in the kernels' order ----------------------------------------------------------------------------
struct HostVoc {
    int weighting = TF_IDF, n_nodes = 0, n_words = 0;
    std::vector<uint8_t> desc;                      // 32 bytes per node, NEW order
    std::vector<int32_t> child0, nchild, word;
    std::vector<double> weight, word_weight;        // per node (NEW order); per word id
    std::string err;
    bool set(int weighting_, int n_nodes_, const int32_t* parent, const uint8_t* desc32, const double* w, const int32_t* word_id) {
        VocPlan pl = plan_vocabulary(n_nodes_, parent, word_id);
        err = pl.err;
        if (!err.empty()) return false;
        weighting = weighting_; n_nodes = n_nodes_; n_words = pl.n_words;
        desc.resize(32 * (size_t)n_nodes); weight.resize((size_t)n_nodes); word_weight.assign((size_t)n_words, 0.0);
        for (int at = 0; at < n_nodes; ++at) {
            __builtin_memcpy(&desc[32 * (size_t)at], desc32 + 32 * (size_t)pl.order[(size_t)at], 32);
            weight[(size_t)at] = w[pl.order[(size_t)at]];
            if (pl.word[(size_t)at] >= 0) word_weight[(size_t)pl.word[(size_t)at]] = weight[(size_t)at];
        }
        child0.swap(pl.child0); nchild.swap(pl.nchild); word.swap(pl.word);
        return true;
    }
};

inline match::Desc load32(const uint8_t* rows, int64_t i) {
    match::Desc d;
    __builtin_memcpy(d.w, rows + 32 * i, 32);
    return d;
}
// TemplatedVocabulary.h:1198-1239: the leaf (NEW index) a descriptor falls into
inline int descend(const HostVoc& v, const match::Desc& q) {
    int node = 0;
    while (v.nchild[(size_t)node] > 0) {
        const int c0 = v.child0[(size_t)node], nc = v.nchild[(size_t)node];
        int best = c0, bd = match::NONE;
        for (int c = 0; c < nc; ++c) {
            const int d = match::distance(q, load32(v.desc.data(), c0 + c));
            if (d < bd) { bd = d; best = c0 + c; }      // strict: the first of equal distances stays
        }
        node = best;
    }
    return node;
}
// words (n entries, -1: stopped) and the normalised vector (ids ascending) of n descriptors
inline void transform(const HostVoc& v, const uint8_t* desc32, int n, int32_t* words, std::vector<int32_t>& ids, std::vector<double>& vals) {
    std::vector<int32_t> keys((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int leaf = descend(v, load32(desc32, i));
        words[i] = v.weight[(size_t)leaf] > 0.0 ? v.word[(size_t)leaf] : -1;
        keys[(size_t)i] = words[i] >= 0 ? words[i] : STOPPED;
    }
    std::sort(keys.begin(), keys.end());
    ids.clear(); vals.clear();
    for (size_t i = 0; i < keys.size() && keys[i] != STOPPED;) {
        size_t e = i + 1;
        while (e < keys.size() && keys[e] == keys[i]) ++e;
        const double w = v.word_weight[(size_t)keys[i]];
        double val = w;
        if (accumulates(v.weighting)) for (size_t c = i + 1; c < e; ++c) val += w;
        ids.push_back(keys[i]); vals.push_back(val);
        i = e;
    }
    double norm = 0.0;
    for (double x : vals) norm += fabs(x);
    if (norm > 0.0) for (double& x : vals) x /= norm;
}

// the lane-tree sum of term(0) .. term(J - 1)
template <class F>
inline double lane_tree_sum(int J, F term) {
    double p[LANES];
    for (int l = 0; l < LANES; ++l) p[l] = 0.0;
    for (int j = 0; j < J; ++j) p[j % LANES] += term(j);
    for (int o = LANES / 2; o >= 1; o >>= 1) {
        double q[LANES];
        for (int l = 0; l < LANES; ++l) q[l] = p[l] + p[l ^ o];
        for (int l = 0; l < LANES; ++l) p[l] = q[l];
    }
    return p[0];
}
// L1Scoring::score of a query vector against a stored one
inline double score(const int32_t* q_id, const double* q_val, int nq, const int32_t* d_id, const double* d_val, int nd) {
    return l1_finish(lane_tree_sum(nd, [&](int j) {
        const int k = find_word(q_id, nq, d_id[j]);
        return k >= 0 ? l1_term(q_val[k], d_val[j]) : 0.0;
    }));
}
// vector_stdv of v[0], v[stride], ...
template <class F>
inline double stdv(int n, F at) {
    const double mean = lane_tree_sum(n, at) / (double)n;
    const double e = lane_tree_sum(n, [&](int j) { const double c = at(j) - mean; return c * c; });
    return stdv_finish(n, e);
}

struct DecideOptions { int topk = 8, lc_kf_dist = 50, lc_kf_max_dist = 50, lc_nkf_closest = 4, min_lm_cov_graph = 75, min_kf_local_map = 3; };
struct Candidate {
    int is_candidate = 0, kf_prev = -1, n_closest = 0, n_eligible = 0;
    double best_score = 0.0, lc_min_score = 1.0;
    int topk[TOPK_MAX];
    double topk_score[TOPK_MAX];
};
// lookForLoopCandidates on the float column col[0 .. idx) with the pinned order of the best entries (include/plba.h)
inline Candidate decide(const float* col, const int32_t* cov, const uint8_t* live, int idx, const DecideOptions& o) {
    Candidate c;
    for (int k = 0; k < TOPK_MAX; ++k) { c.topk[k] = -1; c.topk_score[k] = 0.0; }
    std::vector<int> el;
    for (int i = 0; i < idx; ++i) if (eligible(i, idx, o.lc_kf_dist, live[i] != 0)) el.push_back(i);
    c.n_eligible = (int)el.size();
    for (int i = 0; i < idx; ++i)
        if (in_min_scan(cov[i], i, idx, o.min_lm_cov_graph, o.min_kf_local_map)) {
            const double s = col[i];
            if (s < c.lc_min_score && s > 0.001) c.lc_min_score = s;
        }
    std::vector<uint8_t> taken(el.size(), 0);
    int idx_max = -1;
    const int rounds = std::max(o.topk, 1);
    for (int r = 0; r < rounds; ++r) {
        int best = -1;
        for (size_t e = 0; e < el.size(); ++e) {
            if (taken[e]) continue;
            if (best < 0 || col[el[e]] > col[el[(size_t)best]]) best = (int)e;
        }
        if (best < 0) break;
        taken[(size_t)best] = 1;
        if (r == 0) { idx_max = el[(size_t)best]; c.best_score = col[idx_max]; }
        if (r < o.topk) { c.topk[r] = el[(size_t)best]; c.topk_score[r] = col[el[(size_t)best]]; }
    }
    if (idx_max >= 0 && c.best_score >= c.lc_min_score) {
        for (int i : el)
            if (i != idx_max && std::abs(i - idx_max) <= o.lc_kf_max_dist && (double)col[i] >= c.lc_min_score * 0.8) ++c.n_closest;
    }
    if (c.n_eligible > o.lc_kf_max_dist && idx_max >= 0 && c.best_score >= c.lc_min_score && c.n_closest >= o.lc_nkf_closest) {
        c.is_candidate = 1; c.kf_prev = idx_max;
    }
    return c;
}

}  // namespace bow
}  // namespace plba
