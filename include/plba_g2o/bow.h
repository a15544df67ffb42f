// bow.h — place recognition for ONE keyframe in plain C++ on the host: DBoW2's vocabulary transform and L1 score
// (3rdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1046-1102, 1198-1239; src/DBoW2/BowVector.cpp:34-84; src/DBoW2/ScoringObject.cpp:
// 23-68), the three insertKFBowVector* scores (src/mapHandler.cpp:3116-3237) and lookForLoopCandidates (:3239-3299) over plain arrays:
// the drop-in for a caller without a device, and the CPU column of tools/time_bow.py.  The arithmetic and its orders of summation are
// the device's (pl-inertial-slam_amd/csrc/plba_bow_dev.h); plba_bow_insert_keyframes (include/plba.h) is the batched form and its
// comment states the semantics and the unpinned order of the best entries.  Standard library only; needs both include directories, as
// match.h does.  DBoW2's own class API takes cv::Mat; OpenCV is not available to this project, so there is no source-level DBoW2 facade.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "plba_bow_dev.h"

namespace plba_g2o {

struct BowVector {      // DBoW2::BowVector as two arrays: word ids ascending, L1-normalised values
    std::vector<int32_t> id;
    std::vector<double> val;
};

// TemplatedVocabulary<FORB::TDescriptor, FORB> built from the arrays plba_bow_set_vocabulary takes (only L1_NORM scoring)
class Vocabulary {
public:
    // false (and error() says why) for a malformed tree
    bool set(int weighting, int n_nodes, const int32_t* parent, const uint8_t* desc32, const double* weight, const int32_t* word_id) {
        return voc_.set(weighting, n_nodes, parent, desc32, weight, word_id);
    }
    const std::string& error() const { return voc_.err; }
    bool empty() const { return voc_.n_nodes == 0; }
    // transform(features, v): n rows of 32 bytes; words (optional): the word of every row, -1 when stopped
    void transform(const uint8_t* desc32, int n, BowVector& v, std::vector<int32_t>* words = nullptr) const {
        std::vector<int32_t> w((size_t)(n > 0 ? n : 0));
        plba::bow::transform(voc_, desc32, n > 0 ? n : 0, w.data(), v.id, v.val);
        if (words) words->swap(w);
    }
    double score(const BowVector& a, const BowVector& b) const {
        return plba::bow::score(a.id.data(), a.val.data(), (int)a.id.size(), b.id.data(), b.val.data(), (int)b.id.size());
    }

private:
    plba::bow::HostVoc voc_;
};

struct BowKeyFrame {      // what insertKFBowVector* reads of a keyframe
    int n_pt = 0, n_ls = 0;
    const uint8_t *pdesc = nullptr, *ldesc = nullptr;      // pdesc_l, ldesc_l: 32 bytes a row
    const double* pl = nullptr;                             // stereo_pt[i]->pl: 2 doubles a row
    const double* spl_epl = nullptr;                        // stereo_ls[i]->spl, epl: 4 doubles a row
};
struct BowStored {        // a keyframe of the map: null vectors are map_keyframes[i] == NULL
    bool live = true;
    BowVector p, l;
};
struct BowColumn {        // one column of conf_matrix: idx + 1 entries, the last one the self-score
    std::vector<double> score_p, score_l, score;
    std::vector<float> conf;
};

// insertKFBowVectorP / L / PL for one new keyframe with index stored.size(): fills its vectors into `mine` and its column
inline void insert_kf_bow_vector(int mode, const Vocabulary& voc_p, const Vocabulary& voc_l, const BowKeyFrame& kf, const std::vector<BowStored>& stored,
                                 BowStored& mine, BowColumn& col) {
    namespace bw = plba::bow;
    const bool use_p = mode != bw::MODE_LINES, use_l = mode != bw::MODE_POINTS;
    mine = BowStored();
    if (use_p) voc_p.transform(kf.pdesc, kf.n_pt, mine.p);
    if (use_l) voc_l.transform(kf.ldesc, kf.n_ls, mine.l);
    const int n_pt = use_p ? kf.n_pt : 0, n_ls = use_l ? kf.n_ls : 0;
    double std_pt = 0.0, std_ls = 0.0;
    if (mode == bw::MODE_COMBINED) {
        const double *pl = kf.pl, *se = kf.spl_epl;
        std_pt = bw::stdv(n_pt, [&](int j) { return pl[2 * (size_t)j]; }) + bw::stdv(n_pt, [&](int j) { return pl[2 * (size_t)j + 1]; });
        std_ls = bw::stdv(n_ls, [&](int j) { return (se[4 * (size_t)j] + se[4 * (size_t)j + 2]) * 0.5; }) +
                 bw::stdv(n_ls, [&](int j) { return (se[4 * (size_t)j + 1] + se[4 * (size_t)j + 3]) * 0.5; });
    }
    const size_t idx = stored.size();
    col.score_p.assign(idx + 1, 0.0); col.score_l.assign(idx + 1, 0.0); col.score.assign(idx + 1, 0.0); col.conf.assign(idx + 1, 0.0f);
    for (size_t i = 0; i <= idx; ++i) {
        const BowStored& o = i < idx ? stored[i] : mine;
        if (!o.live) continue;
        if (use_p) col.score_p[i] = voc_p.score(mine.p, o.p);
        if (use_l) col.score_l[i] = voc_l.score(mine.l, o.l);
        col.score[i] = bw::mode_score(mode, col.score_p[i], col.score_l[i], n_pt, n_ls, std_pt, std_ls);
        col.conf[i] = (float)col.score[i];
    }
}

using LoopCandidateConfig = plba::bow::DecideOptions;      // lc_kf_dist, lc_kf_max_dist, lc_nkf_closest, min_lm_cov_graph, min_kf_local_map, topk
using LoopCandidate = plba::bow::Candidate;

// lookForLoopCandidates on a host column: conf[i] = conf_matrix[i][idx], cov[i] = full_graph[i][idx], live[i] for i < idx
inline bool look_for_loop_candidates(const float* conf, const int32_t* cov, const uint8_t* live, int kf_curr_idx, int& kf_prev_idx,
                                     const LoopCandidateConfig& cfg = LoopCandidateConfig(), LoopCandidate* report = nullptr) {
    const LoopCandidate c = plba::bow::decide(conf, cov, live, kf_curr_idx, cfg);
    kf_prev_idx = c.kf_prev;
    if (report) *report = c;
    return c.is_candidate != 0;
}

}  // namespace plba_g2o
