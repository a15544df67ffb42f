// plba_lba_sparse.h — the host side of plba_lba_visual's sparse reduced-camera solve, plba_lba_options.solver = 1: the
// block list of the reduced camera matrix S from the observation lists.  Standard library only (csrc/plba_lba_sparse_hostcheck.cpp
// compiles it with a plain C++ compiler).
//
// S has one 6 x 6 block per local keyframe on its diagonal and one block (lb, la), lb > la, per pair of local keyframes that observe a
// common landmark (the covisibility graph).  A Schur pair entry is a pair of observations (ea, eb) of ONE landmark from the local
// keyframes la <= lb (an observation with itself included; la == lb keeps every ordered pair), exactly what lba_for_pairs below
// enumerates for both solvers: landmark by landmark, ea ascending, eb ascending.  Here the entries are sorted by block with two stable
// counting passes (by lb, then by la), so that
//   blocks    come in ascending (la, lb): every keyframe's diagonal block first (it exists even without an entry: a keyframe that
//             observes nothing keeps its zero block, and the factorisation reports the zero pivot), then its blocks with lb > la;
//   entries   of one block keep the enumeration order above, the order in which the dense path's pair list holds them.
// Work and memory are O(entries + Nkf); nothing of size Nkf x Nkf exists.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace plba {

struct LbaBlockList {
    std::vector<int32_t> blk_row, blk_col;      // per block: lb, la (row >= column: what pgo_sparse_analyse takes)
    std::vector<int32_t> blk_start;             // nblk + 1: block k owns the entries blk_start[k] .. blk_start[k + 1]
    std::vector<int32_t> pair_ent;              // 2 x nent: (ea, eb), ea an observation of keyframe la, eb of lb
    int64_t nent = 0;
};

constexpr int64_t LBA_MAX_PAIR_ENT = INT32_MAX / 2;

// The Schur pair entries in enumeration order, fn(la, lb, ea, eb) for each: the one definition both solvers' lists are built from.
// lm_start (L + 1) / obs_kf: the landmark-major observation lists; kf_loc[k] = local index of keyframe k or < 0.
template <class Fn>
inline void lba_for_pairs(int L, const int32_t* lm_start, const int32_t* obs_kf, const int32_t* kf_loc, Fn&& fn) {
    for (int l = 0; l < L; ++l)
        for (int ea = lm_start[l]; ea < lm_start[l + 1]; ++ea) {
            const int la = kf_loc[obs_kf[ea]];
            if (la < 0) continue;
            for (int eb = lm_start[l]; eb < lm_start[l + 1]; ++eb) {
                const int lb = kf_loc[obs_kf[eb]];
                if (lb < la) continue;      // the (lb, la) block is the transpose; la == lb keeps every ordered pair (normally just the observation with itself)
                fn(la, lb, ea, eb);
            }
        }
}

// false: more than LBA_MAX_PAIR_ENT entries (nothing is built)
inline bool lba_block_list(int Nkf, int L, const int32_t* lm_start, const int32_t* obs_kf, const int32_t* kf_loc, LbaBlockList& out) {
    out = LbaBlockList();
    // pass 1: count by lb, place in enumeration order
    std::vector<int64_t> cb((size_t)Nkf + 1, 0), ca((size_t)Nkf + 1, 0);
    int64_t nent = 0;
    lba_for_pairs(L, lm_start, obs_kf, kf_loc, [&](int la, int lb, int, int) { ++cb[lb + 1]; ++ca[la + 1]; ++nent; });
    if (nent > LBA_MAX_PAIR_ENT) return false;
    for (int i = 0; i < Nkf; ++i) { cb[i + 1] += cb[i]; ca[i + 1] += ca[i]; }
    struct Ent { int32_t la, lb, ea, eb; };
    std::vector<Ent> by_b((size_t)nent);
    lba_for_pairs(L, lm_start, obs_kf, kf_loc, [&](int la, int lb, int ea, int eb) { by_b[(size_t)cb[lb]++] = Ent{la, lb, ea, eb}; });
    // pass 2: stable by la: ascending (la, lb), enumeration order within a block
    std::vector<Ent> s((size_t)nent);
    for (const Ent& e : by_b) s[(size_t)ca[e.la]++] = e;
    by_b = std::vector<Ent>();
    out.nent = nent;
    out.pair_ent.resize((size_t)2 * nent);
    size_t t = 0;
    for (int la = 0; la < Nkf; ++la) {
        out.blk_row.push_back(la); out.blk_col.push_back(la); out.blk_start.push_back((int32_t)t);      // the diagonal block, entries or not
        int cur = la;
        for (; t < (size_t)nent && s[t].la == la; ++t) {
            if (s[t].lb != cur) { cur = s[t].lb; out.blk_row.push_back(cur); out.blk_col.push_back(la); out.blk_start.push_back((int32_t)t); }
            out.pair_ent[2 * t] = s[t].ea; out.pair_ent[2 * t + 1] = s[t].eb;
        }
    }
    out.blk_start.push_back((int32_t)nent);
    return true;
}

}  // namespace plba
