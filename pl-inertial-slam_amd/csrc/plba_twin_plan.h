// plba_twin_plan.h — the plan of the multi-chain ("twin") form of the multi-launch factorisation (plba_dense.hip): a pure function
// of the system's tile count T (tiles of 32 columns) and its band hbt (sub-diagonal tiles).
//
// Standard library only (no HIP header: csrc/plba_twin_plan_hostcheck.cpp compiles it with a plain C++ compiler, and
// tests/test_twin_plan_cpu.py pins every table without a GPU).  prepare() uploads the tables; the segment-length choice asks
// twin_plan_launches() only.
//
// Natural layout of the band:
//   two chains :  C0 (n + 1 tiles) | S1 | C1 (n tiles, eliminated bottom-up)
//   four chains:  C0 (n + 1) | S1 | C1 (n) | S2 | C2 (n + 1) | S3 | C3 (n, bottom-up)
// separators >= hbt tiles wide (chains must not couple); C1 / C3 accumulate their separator updates in `alt` and are one tile
// shorter, so that the last step of C0 / C2 folds those in.  With four chains the separator region [S1 S2 S3] is itself
// block-tridiagonal and can be taken the same way once more (second stage, "nested"): S1 top-down and S3 bottom-up (one tile
// shorter, accumulating in `alt2`) towards S2.  The system is stored PERMUTED: the chains, then the separators (nested: S1 | S3
// turned around | S2); what no chain stage eliminates — from tile final0 on — is the final block, taken by ordinary steps.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace plba {

// one workgroup of a list-driven block step: block row / column, identity row (-1: a tile of the factorisation proper), flags,
// the pivot tile of the step this workgroup belongs to
struct TwinTile { int16_t r, c, aj, flags, k, pad; };
enum : int {
    TWIN_TO_ALT = 1,       // writes d.alt instead of d.sys
    TWIN_NO_LOOK = 2,      // no look-ahead on this tile
    TWIN_FIRST_COL = 4,    // c is the step's first trailing column (stores the finished panel block)
    TWIN_ADD_ALT = 8,      // add d.alt's tile to the old value first
    TWIN_PIVOT = 16,       // this (diagonal) tile is the next pivot: factor it here
    TWIN_ALT2 = 32,        // with TWIN_TO_ALT / TWIN_ADD_ALT: d.alt2 instead of d.alt (second stage of a nested plan)
};

// Tile counts of one variant (0: two chains, 1: four chains, 2: four chains nested).  sep0: first permuted tile of the separator
// region; final0: of the final block; stage1: launches of the first stage; launches: dependent launches up to the one that ends
// the factorisation.  !valid: T and hbt leave no room for the variant.
struct TwinLayout { bool valid; int nch, nC, w[3], stage1, sep0, lenA, lenB, final0, launches; };
inline TwinLayout twin_layout(int T, int hbt, int variant) {
    TwinLayout L = {};
    const int nch = variant == 0 ? 2 : 4, nsep = nch - 1;
    L.nch = nch;
    L.nC = (T - nsep * hbt - nch / 2) / nch;      // nch / 2 chains carry the extra tile
    if (L.nC < 1) return L;
    int left = T - nsep * hbt - nch / 2 - nch * L.nC;      // tiles that do not divide: widen the first separators
    for (int q = 0; q < nsep; ++q) { L.w[q] = hbt + (left > 0 ? 1 : 0); if (left > 0) --left; }
    L.stage1 = L.nC + 1; L.sep0 = nch * L.nC + nch / 2; L.final0 = L.sep0;
    if (variant == 2) {      // second stage: S1 (all of it) and the first lenB tiles of the turned-around S3; what is left of S3 joins S2 as the final block
        L.lenA = L.w[0]; L.lenB = std::min(L.w[2], L.lenA - 1);
        if (L.lenB < 1) return L;
        L.final0 = L.sep0 + L.lenA + L.lenB;
    }
    L.launches = L.stage1 + L.lenA + (T - L.final0 - 1);
    L.valid = true;
    return L;
}
// The variant with the fewest dependent launches (the first one on a tie), -1 where none beats the T - 1 of the plain factorisation.
inline int twin_best_variant(int T, int hbt, int& launches) {
    int best = -1;
    launches = T - 1;
    if (T < 8 || hbt < 1) return best;
    for (int variant = 0; variant < 3; ++variant) {
        const TwinLayout L = twin_layout(T, hbt, variant);
        if (L.valid && L.launches < launches) { launches = L.launches; best = variant; }
    }
    return best;
}
// Dependent launches of the factorisation of T tiles with band hbt, without building anything (the chain elimination's
// segment-length choice asks for every candidate): T where no plan is built.
inline int twin_plan_launches(int T, int hbt) {
    int launches;
    twin_best_variant(T, hbt, launches);
    return launches + 1;      // + the launch that ends the factorisation (k_chol32's last step)
}

struct TwinPlan {
    int T = 0, final0 = 0, sep0 = 0, nchains = 0, nlaunch = 0;      // nchains: of both stages; nlaunch: launches of the chain stages
    std::vector<int32_t> perm, xmap;      // 32 T: natural dense index -> permuted, and back
    std::vector<int32_t> fac;             // per NATURAL diagonal tile: -1, or the permuted tile it becomes as a chain's first tile (| 1 << 16: turned around)
    std::vector<TwinTile> list;           // all launches' tiles: launch t = [off[t], off[t + 1])
    std::vector<int32_t> off;
    std::vector<int32_t> cs_order;        // k_chain_schur: tile (ta << 16 | tb) of each workgroup
    double summary[5] = {0, 0, 0, 0, 0};  // first-stage chains, nested, up to three separator widths (debug_get "solver_plan")
};

// false (and pl untouched): no variant needs fewer launches than the plain factorisation
inline bool twin_plan_build(int T, int hbt, TwinPlan& pl) {
    struct Chain { int p0, len, alt /* 0 = writes sys, 1 = alt, 2 = alt2 */, stage; std::vector<int> later /* tiles it couples with beyond itself */, rows /* identity rows with support on its columns */; };
    int launches;
    const int variant = twin_best_variant(T, hbt, launches);
    if (variant < 0) return false;
    const TwinLayout L = twin_layout(T, hbt, variant);
    const bool nested = variant == 2;
    const int nch = L.nch, nsep = nch - 1, sep0 = L.sep0, final0 = L.final0;
    pl = TwinPlan();
    pl.T = T; pl.final0 = final0; pl.sep0 = sep0;
    pl.summary[0] = nch; pl.summary[1] = nested ? 1.0 : 0.0;
    for (int q = 0; q < nsep; ++q) pl.summary[2 + q] = L.w[q];
    // permuted positions: level-1 chains, then (nested) S1 | S3 reversed | S2, else the separators in natural order
    int sep_p0[3] = {sep0, sep0 + L.w[0], sep0 + L.w[0] + L.w[1]};
    if (nested) { sep_p0[2] = sep0 + L.w[0]; sep_p0[1] = sep_p0[2] + L.w[2]; }
    pl.perm.assign((size_t)32 * T, 0); pl.fac.assign(T, -1);
    auto map_range = [&](int nat0, int w, int p0, bool rev) {
        for (int j = 0; j < w; ++j)
            for (int e = 0; e < 32; ++e) pl.perm[(nat0 + j) * 32 + e] = rev ? (p0 + (w - 1 - j)) * 32 + (31 - e) : (p0 + j) * 32 + e;
    };
    std::vector<Chain> chains(nch);
    for (int c = 0, nat0 = 0, p0 = 0; c < nch; ++c) {
        Chain& ch = chains[c];
        const bool rev = c == nch - 1;
        ch.p0 = p0; ch.len = L.nC + ((c & 1) ? 0 : 1); ch.alt = c & 1; ch.stage = 0;
        map_range(nat0, ch.len, p0, rev);
        pl.fac[rev ? nat0 + ch.len - 1 : nat0] = p0 | (rev ? 1 << 16 : 0);
        nat0 += ch.len; p0 += ch.len;
        if (c < nsep) { map_range(nat0, L.w[c], sep_p0[c], nested && c == 2); nat0 += L.w[c]; }
        for (int q = std::max(c - 1, 0); q <= std::min(c, nsep - 1); ++q)      // its adjacent separators
            for (int j = 0; j < L.w[q]; ++j) ch.later.push_back(sep_p0[q] + j);
        std::sort(ch.later.begin(), ch.later.end());
    }
    if (nested) {
        Chain a, b;
        a.p0 = sep_p0[0]; a.len = L.lenA; a.alt = 0; a.stage = 1;
        b.p0 = sep_p0[2]; b.len = L.lenB; b.alt = 2; b.stage = 1;
        for (int t = final0; t < T; ++t) { a.later.push_back(t); b.later.push_back(t); }
        for (int t = 0; t < chains[2].p0; ++t) a.rows.push_back(t);      // C0, C1: rows with support on S1's columns
        for (int t = chains[2].p0; t < sep0; ++t) b.rows.push_back(t);   // C2, C3: on S3's
        chains.push_back(a); chains.push_back(b);
    }
    pl.nchains = (int)chains.size();
    pl.xmap.resize(pl.perm.size());
    for (size_t i = 0; i < pl.perm.size(); ++i) pl.xmap[pl.perm[i]] = (int32_t)i;
    pl.off.assign(1, 0);
    for (int stage = 0; stage < 2; ++stage) {
        int nl = 0;
        for (const Chain& ch : chains) if (ch.stage == stage) nl = std::max(nl, ch.len);
        const int asel = stage == 1 ? TWIN_ALT2 : 0;      // second stage accumulates in alt2
        for (int t = 0; t < nl; ++t) {
            int ci_stage = 0;
            for (const Chain& ch : chains) {
                if (ch.stage != stage) continue;
                const int cis = ci_stage++;
                if (t >= ch.len) continue;
                const int k = ch.p0 + t;
                const bool last = (t == ch.len - 1);
                std::vector<int> S;      // the step's trailing tiles: the rest of the chain, then what it couples with (ascending)
                for (int c = k + 1; c < ch.p0 + ch.len; ++c) S.push_back(c);
                S.insert(S.end(), ch.later.begin(), ch.later.end());
                auto in_later = [&](int x) { return std::binary_search(ch.later.begin(), ch.later.end(), x); };
                auto push = [&](int r, int c, int aj, int flags) { pl.list.push_back({(int16_t)r, (int16_t)c, (int16_t)aj, (int16_t)flags, (int16_t)k, 0}); };
                const bool fold = ch.alt == 0 && last;      // this step folds the accumulating chains' part of its later tiles in
                // the tile a folding step factors by look-ahead: the first tile of the next stage's first chain (or of the final
                // block), and — first stage of a nested plan — C2's last step factors the second-stage chain S3's first tile
                int look1 = -1;
                if (fold && cis == 0) look1 = stage == 0 && nested ? chains[nch].p0 : final0;
                else if (fold && stage == 0 && nested && cis == 2) look1 = chains[nch + 1].p0;
                for (size_t a2 = 0; a2 < S.size(); ++a2)
                    for (size_t b2 = 0; b2 <= a2; ++b2) {
                        const int r = S[a2], c = S[b2];
                        const bool ss = in_later(r) && in_later(c);
                        push(r, c, -1, ((ch.alt && ss) ? (TWIN_TO_ALT | asel) : 0) | ((last && r == k + 1) ? TWIN_NO_LOOK : 0) | (c == S[0] ? TWIN_FIRST_COL : 0) |
                                       ((fold && ss) ? (TWIN_ADD_ALT | asel) : 0) | ((fold && r == look1 && c == look1) ? TWIN_PIVOT : 0));
                    }
                if (fold && stage == 0 && cis == 0)      // separator cross blocks only an accumulating chain writes ((S2, S1) by C1): folded in here, with a zero panel
                    for (int c2 = 1; c2 + 1 < nch; ++c2) {
                        const Chain& oc = chains[c2];
                        if (oc.alt == 0) continue;
                        // oc.later = two separators' tiles: every (r, c) pair with r, c in DIFFERENT separators
                        for (int r : oc.later) for (int c : oc.later) {
                            if (r <= c) continue;
                            bool same = false;      // same separator <=> covered by a sys-writer's own list
                            for (int c3 = 0; c3 < nch; c3 += 2)
                                same |= std::binary_search(chains[c3].later.begin(), chains[c3].later.end(), r) && std::binary_search(chains[c3].later.begin(), chains[c3].later.end(), c);
                            if (!same) push(r, c, -1, TWIN_ADD_ALT);
                        }
                    }
                for (int c : S) push(T, c, -1, ((ch.alt && in_later(c)) ? (TWIN_TO_ALT | asel) : 0) | (c == S[0] ? TWIN_FIRST_COL : 0) | ((fold && in_later(c)) ? (TWIN_ADD_ALT | asel) : 0));
                for (int aj : ch.rows) for (int c : S) push(T, c, aj, c == S[0] ? TWIN_FIRST_COL : 0);
                for (int aj = ch.p0; aj < k; ++aj) for (int c : S) push(T, c, aj, c == S[0] ? TWIN_FIRST_COL : 0);
                // the identity row that STARTS at this step is initialised over every later tile of the system, not only the ones this
                // chain couples with: later stages read R(k, c) for all of them, and a block left untouched would hold the previous
                // solve's values
                bool first = true;
                for (int c = k + 1; c < T; ++c) {
                    if (c >= ch.p0 + ch.len && c < (stage == 0 ? sep0 : final0)) continue;
                    push(T, c, k, first ? TWIN_FIRST_COL : 0);
                    first = false;
                }
            }
            pl.off.push_back((int32_t)pl.list.size());
        }
        pl.nlaunch += nl;
    }
    // k_chain_schur's workgroup order: at 44 tiles the launch is two rounds of workgroups, and a chain's first tile — 6 us of
    // factorisation behind its own Schur update — must not start in the second one
    for (int t = 0; t < T; ++t) if (pl.fac[t] >= 0) pl.cs_order.push_back((t << 16) | t);
    for (int dist = 0; dist <= T; ++dist) for (int ta = dist; ta < T; ++ta) { if (dist == 0 && pl.fac[ta] >= 0) continue; pl.cs_order.push_back((ta << 16) | (ta - dist)); }
    for (int tb = 0; tb < T; ++tb) pl.cs_order.push_back((T << 16) | tb);
    return true;
}

}  // namespace plba
