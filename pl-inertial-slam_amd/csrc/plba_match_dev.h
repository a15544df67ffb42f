// plba_match_dev.h — the arithmetic of plba_match_descriptors and of the gate of plba_verify_loop_candidates (include/plba.h), shared by
// the kernels (plba_match.hip), the host check (plba_match_hostcheck.cpp) and the plain-C++ drop-in (include/plba_g2o/match.h).
//
// StVO::match / matchNNR (stvo-pl/src/matching.cpp:41-109) for ONE problem: the Hamming distance over 8 x 32-bit words, a 2-nearest-
// neighbour search that visits the train rows in ascending index and updates on a strict `<` (a tied distance keeps the LOWER train index
// first: OpenCV's brute-force k-NN as far as it is remembered; OpenCV is not available to this project, so the rule is unpinned, see
// DESIGN.md §9e), the ratio test in float and the mutual rule; and isLoopClosure's inlier-ratio gate (src/mapHandler.cpp:3382-3400).
// Everything is integer arithmetic but the one float product of the ratio test and the double quotients of the gate, which have no
// order of evaluation to depend on: device and host agree exactly.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MT_HD __host__ __device__ inline
#else
#define MT_HD inline
#endif

namespace plba {
namespace match {

constexpr int WORDS = 8;            // a descriptor: 32 bytes, read as 8 x 32-bit words (:97-98)
constexpr int QUERY_TILE = 64;      // query rows of one work item of the kernel: one per lane of a wave
constexpr int TRAIN_TILE = 128;     // train rows that pass through LDS at a time
constexpr int NONE = 257;           // a distance no pair has (the largest is 256): "no neighbour yet"
constexpr int BEST_LR = 1, SKIP = 2;      // per-problem flags: Config::bestLRMatches; the problem is not matched at all (all -1, count 0)

struct Desc { uint32_t w[WORDS]; };
struct NN2 { int i0, d0, d1; };     // the best train index, its distance and the second-best distance; NONE where there is none

MT_HD int popcount32(uint32_t v) { return __builtin_popcount(v); }      // one v_bcnt_u32_b32 on the device, as __popc is

// :93-109 (the bit trick there is a population count)
MT_HD int distance(const Desc& a, const Desc& b) {
    int d = 0;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) d += popcount32(a.w[i] ^ b.w[i]);
    return d;
}

MT_HD void nn_init(NN2& s) { s.i0 = -1; s.d0 = NONE; s.d1 = NONE; }
// the train rows arrive in ascending index, so the strict comparisons are the tie rule: the first of equal distances stays in front
MT_HD void nn_update(NN2& s, int d, int idx) {
    if (d < s.d0) { s.d1 = s.d0; s.d0 = d; s.i0 = idx; }
    else if (d < s.d1) s.d1 = d;
}
// what is stored per query row (and returned as nn3): -1 where there is no such neighbour
MT_HD void nn_store(const NN2& s, int32_t* out3) {
    out3[0] = s.i0; out3[1] = s.d0 == NONE ? -1 : s.d0; out3[2] = s.d1 == NONE ? -1 : s.d1;
}

// :54: DMatch::distance is a float, nnr is a float: one product rounded to float, then the comparison
MT_HD bool ratio_ok(int d0, int d1, float nnr) {
    const float prod = (float)d1 * nnr;
    return (float)d0 < prod;
}

// matches_12[i1] of match() (:63-91) from the two searches' stored triples.  nn_12: the triple of query row i1 of desc1; nn_21: the
// triples of ALL rows of desc2 (read at the matched row only).  A direction whose train set has fewer than two rows yields no match
// (the reference reads matches_[idx][1] out of bounds there).
MT_HD int resolve(const int32_t* nn_12, const int32_t* nn_21, int i1, int n1, int n2, float nnr, int best_lr) {
    if (n2 < 2 || !ratio_ok(nn_12[1], nn_12[2], nnr)) return -1;
    const int i2 = nn_12[0];
    if (best_lr) {
        if (n1 < 2) return -1;
        const int32_t* r = nn_21 + 3 * (int64_t)i2;
        if (!ratio_ok(r[1], r[2], nnr) || r[0] != i1) return -1;      // matches_21[i2] != i1 (:82)
    }
    return i2;
}

// isLoopClosure's gate (:3382-3400).  std::max(a, b) is (a < b) ? b : a: a NaN first operand (n0 = 0) stays, a NaN second one (n1 = 0,
// n0 > 0) is dropped and leaves 100 * 0 / n0 = 0; neither passes a finite threshold's strict `>` unless the threshold is negative.
MT_HD double inlier_ratio(int common, int n0, int n1) {
    const double a = 100.0 * common / (double)n0, b = 100.0 * common / (double)n1;
    return (a < b) ? b : a;
}
MT_HD int gate(double ratio_pt, double ratio_ls, int use_points, int use_lines, double lc_inlier_ratio) {
    if (use_points && use_lines) return (ratio_pt > lc_inlier_ratio && ratio_ls > lc_inlier_ratio) ? 1 : 0;
    if (use_points) return ratio_pt > lc_inlier_ratio ? 1 : 0;
    if (use_lines) return ratio_ls > lc_inlier_ratio ? 1 : 0;
    return 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host's form of the two launches, in the kernel's order: query tiles of QUERY_TILE rows, train tiles of TRAIN_TILE rows -------
inline Desc load_desc(const uint8_t* rows, int64_t i) {
    Desc d;
    __builtin_memcpy(d.w, rows + 32 * i, 32);
    return d;
}
// the search of one direction: nn3[3 * q] for every query row
inline void search(const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* nn3) {
    for (int q0 = 0; q0 < nq; q0 += QUERY_TILE)
        for (int l = 0; l < QUERY_TILE && q0 + l < nq; ++l) {
            const Desc q = load_desc(query, q0 + l);
            NN2 s;
            nn_init(s);
            for (int t0 = 0; t0 < nt; t0 += TRAIN_TILE)
                for (int r = 0; r < TRAIN_TILE && t0 + r < nt; ++r) nn_update(s, distance(q, load_desc(train, t0 + r)), t0 + r);
            nn_store(s, nn3 + 3 * (int64_t)(q0 + l));
        }
}
// one problem: matches_12 (n1 entries) and the count match() returns; nn_12 / nn_21: 3 * n1 / 3 * n2 ints of work space (nn_12 is nn3)
inline int match_problem(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr, int flags, int32_t* matches_12, int32_t* nn_12, int32_t* nn_21) {
    if (flags & SKIP) {
        for (int i = 0; i < n1; ++i) { matches_12[i] = -1; nn_12[3 * i] = nn_12[3 * i + 1] = nn_12[3 * i + 2] = -1; }
        return 0;
    }
    search(desc1, n1, desc2, n2, nn_12);
    if (flags & BEST_LR) search(desc2, n2, desc1, n1, nn_21);
    int count = 0;
    for (int i1 = 0; i1 < n1; ++i1) {
        matches_12[i1] = resolve(nn_12 + 3 * (int64_t)i1, nn_21, i1, n1, n2, nnr, flags & BEST_LR);
        count += matches_12[i1] >= 0 ? 1 : 0;
    }
    return count;
}
#endif

}  // namespace match
}  // namespace plba
