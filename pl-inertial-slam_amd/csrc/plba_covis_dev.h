// plba_covis_dev.h — the arithmetic of the covisibility graph (plba_covis_*, include/plba.h), shared by the kernels (plba_covis.hip), the
// host check (plba_covis_hostcheck.cpp) and the plain-C++ drop-in (include/plba_g2o/covis.h).
//
// The definition (a decision of this project): for keyframes i != j
//     C[i][j] = sum over all landmarks l, points and lines together, of m_l(i) * m_l(j),
// m_l(k) the number of times k occurs in l's kf_obs_list; C[i][i] = 0; a dead keyframe's row and column are 0 (src/mapHandler.cpp:3033-3038).
// Nobody counts m: the keyframe -> landmark transpose lists a landmark once per OCCURRENCE of the keyframe, and every occurrence of i
// walks the landmark's whole list and adds one per entry j != i, which is m_l(i) * m_l(j) additions.  All of it is integer, so no order
// of summation shows.
//
// The predicates are the reference's text: the edge loop of loopClosureOptimizationCovGraphG2O (:4373-4393) and formLocalMap (:996-1002).
// The measurement Z = T_i^-1 T_j has T_i^-1 = [R_i^T, -R_i^T t_i] formed directly (inverse_se3); the reference's round trip through
// logmap_se3 / reverse_se3 / SE3Quat::exp is the identity in exact arithmetic and is not restated.  No product is contracted with a sum
// (fp contract off), so the host compiler's code rounds as the device's does.
#pragma once
#include <cstdint>

#include "plba_match_dev.h"      // MT_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace plba {
namespace covis {

// what ONE occurrence of keyframe i in the list kf[b .. e) adds to row i: one per entry j != i inside the column window [lo, hi);
// add(j - lo) is called once per such entry.  The caller's lanes stride the list (lane, lanes); the loop is bounded by the list.
template <class Add>
MT_HD void add_occurrence(const int32_t* kf, int b, int e, int lane, int lanes, int i, int lo, int hi, Add add) {
    for (int x = b + lane; x < e; x += lanes) {
        const int j = kf[x];
        if (j != i && j >= lo && j < hi) add(j - lo);
    }
}

// the entry C[i][j] from the raw sum of the lists: a dead keyframe's row and column are 0
MT_HD int count(int raw, bool live_i, bool live_j) { return (live_i && live_j) ? raw : 0; }

// an entry of a sparse row (plba_covis_rows): C >= max(1, min_count)
MT_HD bool row_entry(int c, int min_count) { return c >= (min_count > 1 ? min_count : 1); }

// :4377-4378 for j > i: both keyframes there, and enough shared landmarks for either graph or neighbours in the index.  A dead keyframe
// breaks the chain: neither (k - 1, k) nor (k, k + 1) is an edge and nothing bridges the gap, as in the text.
MT_HD bool edge(int c, int i, int j, bool live_i, bool live_j, int min_lm_ess_graph, int min_lm_cov_graph) {
    return live_i && live_j && (c >= min_lm_ess_graph || c >= min_lm_cov_graph || j - i == 1);
}

// :1000 with the row of kf (the text takes the newest keyframe's row whatever kf it was given) and a dead keyframe never local (the text
// dereferences it)
MT_HD bool local_keyframe(bool live_i, int c, int kf, int i, int min_lm_cov_graph, int min_kf_local_map) {
    const int gap = kf > i ? kf - i : i - kf;
    return live_i && (i == kf || c >= min_lm_cov_graph || gap <= min_kf_local_map);
}

// Z = T_i^-1 T_j in pose12's layout (R row-major, then t): the inverse first, then the product, each entry a chain over k = 0, 1, 2
MT_HD void relative_pose(const double* Ti, const double* Tj, double* Z) {
    double Rt[9], ti[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rt[3 * r + c] = Ti[3 * c + r];
    for (int r = 0; r < 3; ++r) ti[r] = -(Rt[3 * r] * Ti[9] + Rt[3 * r + 1] * Ti[10] + Rt[3 * r + 2] * Ti[11]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Z[3 * r + c] = Rt[3 * r] * Tj[c] + Rt[3 * r + 1] * Tj[3 + c] + Rt[3 * r + 2] * Tj[6 + c];
        Z[9 + r] = Rt[3 * r] * Tj[9] + Rt[3 * r + 1] * Tj[10] + Rt[3 * r + 2] * Tj[11] + ti[r];
    }
}

}  // namespace covis
}  // namespace plba
