// plba_window.h — the host copy of the uploaded window as ONE value, and the host half of plba_slide_window.
//
// Standard library only (no HIP header: csrc/plba_window_hostcheck.cpp compiles it with a plain C++ compiler, and
// tests/test_slide_plan_cpu.py runs the slide's planning on a machine without a GPU).  plba_problem holds two of these: `win`, the
// window the device image was (or will be) built from, and `win_next`, the storage plba_slide_window plans the next one into; the
// slide swaps them at its single commit point, after the last call that can fail.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plba.h"
#include "plba_math.h"

namespace plba {

inline bool all_finite(const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
    return true;
}

// What the plba_set_* entry points wrote (or a slide planned).  The carry_* flags say which arrays are STALE because the device holds
// the truth after a slide: kf0 (carry_kf), pts / lns (carry_pts / carry_lns), po_uv / po_w (carry_po), lo_l / lo_w (carry_lo) — they
// keep the right SIZE and the matching plba_set_* clears the flag.
struct Window {
    bool have_cam = false;
    double fx = 0, fy = 0, cx = 0, cy = 0, Rbc[9] = {}, Pbc[3] = {}, gw[3] = {0, 0, 0};
    int K = 0, Np = 0, Nl = 0, Ep = 0, El = 0, M = 0;
    std::vector<int32_t> vid_pvr, vid_bias;
    std::vector<double> kf0;              // K x 24 initial records
    std::vector<uint8_t> fix_pvr, fix_bias;
    std::vector<double> pts, lns;
    std::vector<uint8_t> pt_fixed, ln_fixed;
    std::vector<int32_t> po_pt, po_kf, lo_ln, lo_kf;
    std::vector<double> po_uv, po_w, lo_l, lo_w;
    std::vector<uint8_t> level;           // E (points then lines)
    std::vector<int32_t> imu_i, imu_j;
    std::vector<double> imu_pre, imu_ipvr, imu_ibias;
    bool carry_pts = false, carry_lns = false, carry_kf = false, carry_po = false, carry_lo = false;

    // back to a new Window's state; the vectors KEEP their capacity (a parked handle must not fault its pages in again)
    void clear() {
        have_cam = false;
        fx = fy = cx = cy = 0; for (double& v : Rbc) v = 0; for (double& v : Pbc) v = 0; for (double& v : gw) v = 0;
        K = Np = Nl = Ep = El = M = 0;
        vid_pvr.clear(); vid_bias.clear(); kf0.clear(); fix_pvr.clear(); fix_bias.clear();
        pts.clear(); lns.clear(); pt_fixed.clear(); ln_fixed.clear();
        po_pt.clear(); po_kf.clear(); lo_ln.clear(); lo_kf.clear(); po_uv.clear(); po_w.clear(); lo_l.clear(); lo_w.clear();
        level.clear(); imu_i.clear(); imu_j.clear(); imu_pre.clear(); imu_ipvr.clear(); imu_ibias.clear();
        carry_pts = carry_lns = carry_kf = carry_po = carry_lo = false;
    }
};

// What only the device stage of a slide needs.  A source index >= 0 names an entry of the OLD device array, -(1 + a) the a-th addition.
struct SlidePlan {
    int Npk = 0, Nlk = 0;                       // kept points / lines (the added ones follow them)
    std::vector<int32_t> pmap, lmap;            // old landmark -> new index, -1: leaves
    std::vector<int32_t> src_lm;                // [Np1 + Nl1] new landmark slot <- old slot (points, then Np0 + line) | addition (points, then Np_add + line)
    std::vector<int32_t> src_ob;                // [Ep1 + El1] new observation <- old observation of its kind | added observation of its kind
    std::vector<double> kf_add;                 // K_add x KF_STRIDE records
    std::vector<double> add_lm;                 // (Np_add + Nl_add) x 6
    std::vector<double> add_ob;                 // [uv (2 Ep_add) | w (Ep_add) | l (3 El_add) | w (El_add)]
    std::vector<uint8_t> pdrop, ldrop;          // scratch
};

#define PLBA_PLAN_FAIL(code, ...)                 \
    do {                                          \
        snprintf(err, errcap, __VA_ARGS__);       \
        return (code);                            \
    } while (0)

// The host half of plba_slide_window (include/plba.h): every check of the call, the keep / drop maps, the landmark-by-landmark merge of
// the observation lists, and the complete next window in `next`.  `cur` is const: a refused slide leaves the resident window as it was.
// `next` and `plan` are storage the caller keeps between slides (no fresh pages per call); after a refusal their contents are unspecified.
inline int slide_plan(const Window& cur, const plba_slide& s, Window& next, SlidePlan& plan, char* err, size_t errcap) {
    const int K0 = cur.K, Np0 = cur.Np, Nl0 = cur.Nl, Ep0 = cur.Ep, El0 = cur.El, M0 = cur.M, nd = s.n_drop;
    if (nd < 0 || nd >= K0 || s.K_add < 0 || s.M_add < 0 || s.Np_add < 0 || s.Nl_add < 0 || s.Ep_add < 0 || s.El_add < 0) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "plba_slide_window: counts out of range (n_drop %d of %d keyframes)", nd, K0);
    const int Kk = K0 - nd, K1 = Kk + s.K_add;      // kept keyframes, keyframes after the slide
    if (s.K_add && (!s.vid_pvr || !s.P3 || !s.V3 || !s.q_xyzw4)) return PLBA_ERR_INVALID;
    if ((s.M_add && (!s.imu_kf_i || !s.imu_kf_j || !s.preint142 || !s.info_pvr81 || !s.info_bias36)) || (s.Np_add && !s.xyz3) || (s.Nl_add && !s.sPeP6) ||
        (s.Ep_add && (!s.po_pt || !s.po_kf || !s.uv2)) || (s.El_add && (!s.lo_ln || !s.lo_kf || !s.l3))) return PLBA_ERR_INVALID;
    for (int k = 0; k < s.K_add; ++k) {
        const int prev = k ? s.vid_pvr[k - 1] : cur.vid_pvr[K0 - 1];
        if (s.vid_pvr[k] <= prev) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "keyframe vertex ids must be ascending");
    }
    if (!all_finite(s.P3, 3 * (size_t)s.K_add) || !all_finite(s.V3, 3 * (size_t)s.K_add) || !all_finite(s.q_xyzw4, 4 * (size_t)s.K_add)) PLBA_PLAN_FAIL(PLBA_ERR_NUMERIC, "non-finite keyframe state");
    if (!all_finite(s.xyz3, 3 * (size_t)s.Np_add) || !all_finite(s.sPeP6, 6 * (size_t)s.Nl_add) || !all_finite(s.uv2, 2 * (size_t)s.Ep_add) || !all_finite(s.l3, 3 * (size_t)s.El_add)) PLBA_PLAN_FAIL(PLBA_ERR_NUMERIC, "non-finite landmark or observation");
    if (!all_finite(s.preint142, 142 * (size_t)s.M_add) || !all_finite(s.info_pvr81, 81 * (size_t)s.M_add)) PLBA_PLAN_FAIL(PLBA_ERR_NUMERIC, "non-finite IMU edge");
    // ---- which landmarks stay -----------------------------------------------------------------------------------------------------
    std::vector<int32_t>& pmap = plan.pmap; std::vector<int32_t>& lmap = plan.lmap;
    pmap.resize(Np0); lmap.resize(Nl0);
    plan.pdrop.assign(Np0, 0); plan.ldrop.assign(Nl0, 0);
    if (s.drop_point) for (int i = 0; i < Np0; ++i) plan.pdrop[i] = s.drop_point[i] != 0;
    if (s.drop_line) for (int i = 0; i < Nl0; ++i) plan.ldrop[i] = s.drop_line[i] != 0;
    for (int e = 0; e < Ep0; ++e) if (cur.po_kf[e] < nd) plan.pdrop[cur.po_pt[e]] = 1;
    for (int e = 0; e < El0; ++e) if (cur.lo_kf[e] < nd) plan.ldrop[cur.lo_ln[e]] = 1;
    int Npk = 0, Nlk = 0;
    for (int i = 0; i < Np0; ++i) pmap[i] = plan.pdrop[i] ? -1 : Npk++;
    for (int i = 0; i < Nl0; ++i) lmap[i] = plan.ldrop[i] ? -1 : Nlk++;
    plan.Npk = Npk; plan.Nlk = Nlk;
    const int Np1 = Npk + s.Np_add, Nl1 = Nlk + s.Nl_add;
    // added observations: landmark index before the slide (must stay) or N_before + i; keyframes in the new numbering
    auto check_add = [&](int E, const int32_t* lm, const int32_t* kf, int N0, int Nadd, const std::vector<int32_t>& map, const char* what) -> int {
        for (int e = 0; e < E; ++e) {
            if (lm[e] < 0 || lm[e] >= N0 + Nadd) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added %s observation %d: landmark index %d out of range", what, e, lm[e]);
            if (lm[e] < N0 && map[lm[e]] < 0) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added %s observation %d: landmark %d leaves the window with this slide", what, e, lm[e]);
            if (kf[e] < 0 || kf[e] >= K1) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added %s observation %d: keyframe index %d out of range (new numbering, %d keyframes)", what, e, kf[e], K1);
            if (e && lm[e] < lm[e - 1]) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added %s observations must be sorted by landmark", what);
        }
        return PLBA_OK;
    };
    if (int rc = check_add(s.Ep_add, s.po_pt, s.po_kf, Np0, s.Np_add, pmap, "point")) return rc;
    if (int rc = check_add(s.El_add, s.lo_ln, s.lo_kf, Nl0, s.Nl_add, lmap, "line")) return rc;
    for (int m = 0; m < s.M_add; ++m) if (s.imu_kf_i[m] < 0 || s.imu_kf_i[m] >= K1 || s.imu_kf_j[m] < 0 || s.imu_kf_j[m] >= K1) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added imu edge %d: keyframe index (new numbering)", m);
    // ---- observations: compacted, shifted and merged landmark by landmark -----------------------------------------------------------
    // Only the integer lists — landmark and keyframe of every observation — are rebuilt on the host; `src` says where each new
    // observation's measurement and weight come from.  The old list is landmark-major and so is the added one: the merged list is the
    // old one with the dropped landmarks' stretches cut out and each added run spliced in behind its landmark's last old observation.
    // Between two splice points the old observations are copied in one tight loop (new landmark index through the map, keyframe index
    // shifted, source = old position); only a landmark that RECEIVES observations is checked for a keyframe seeing it twice (the old
    // ones were checked when they were uploaded).  Returns the merged count through `n_out`.
    auto merge = [&](int N0, int E0, int Eadd, const std::vector<int32_t>& map, int nkept, const std::vector<int32_t>& ob_lm, const std::vector<int32_t>& ob_kf,
                     const uint8_t* drop_obs, const int32_t* a_lm, const int32_t* a_kf, std::vector<int32_t>& out_lm, std::vector<int32_t>& out_kf, int32_t* osrc, size_t& n_out) -> int {
        out_lm.resize((size_t)E0 + Eadd); out_kf.resize((size_t)E0 + Eadd);
        int32_t* olm = out_lm.data(); int32_t* okf = out_kf.data();
        const int32_t* mp = map.data(); const int32_t* il = ob_lm.data(); const int32_t* ik = ob_kf.data();
        size_t n = 0;
        auto copy_old = [&](int e0, int e1) {      // old observations [e0, e1)
            if (!drop_obs) { for (int e = e0; e < e1; ++e) { const int nl = mp[il[e]]; olm[n] = nl; okf[n] = ik[e] - nd; osrc[n] = e; n += nl >= 0; } }
            else for (int e = e0; e < e1; ++e) { const int nl = mp[il[e]]; olm[n] = nl; okf[n] = ik[e] - nd; osrc[n] = e; n += (nl >= 0) & !drop_obs[e]; }
        };
        int e = 0, a = 0;
        while (a < Eadd) {
            const int l = a_lm[a];
            int a1 = a;
            while (a1 < Eadd && a_lm[a1] == l) ++a1;
            const int nl = l < N0 ? mp[l] : nkept + (l - N0);
            // old observations up to and including landmark l's (none for an added landmark: those come after every old one)
            const int e1 = l < N0 ? (int)(std::upper_bound(il + e, il + E0, l) - il) : E0;
            const size_t before = n;
            copy_old(e, e1);
            e = e1;
            size_t first = n;      // where landmark l's own (kept) observations start in the output
            while (first > before && olm[first - 1] == nl) --first;
            for (int q = a; q < a1; ++q) { olm[n] = nl; okf[n] = a_kf[q]; osrc[n] = -(1 + q); ++n; }
            for (size_t x = first; x < n; ++x) for (size_t y = std::max(x + 1, n - (size_t)(a1 - a)); y < n; ++y)
                if (okf[y] == okf[x]) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "landmark %d observed twice by keyframe %d", nl, okf[x]);
            a = a1;
        }
        copy_old(e, E0);
        out_lm.resize(n); out_kf.resize(n);
        n_out = n;
        return PLBA_OK;
    };
    // (one source list for both kinds, points first: a loop above writes one entry past what it keeps, so the list is sized for every
    // candidate and cut afterwards)
    plan.src_ob.resize(std::max<size_t>((size_t)Ep0 + s.Ep_add + (size_t)El0 + s.El_add, 1));
    size_t nEp = 0, nEl = 0;
    if (int rc = merge(Np0, Ep0, s.Ep_add, pmap, Npk, cur.po_pt, cur.po_kf, s.drop_point_obs, s.po_pt, s.po_kf, next.po_pt, next.po_kf, plan.src_ob.data(), nEp)) return rc;
    if (int rc = merge(Nl0, El0, s.El_add, lmap, Nlk, cur.lo_ln, cur.lo_kf, s.drop_line_obs, s.lo_ln, s.lo_kf, next.lo_ln, next.lo_kf, plan.src_ob.data() + nEp, nEl)) return rc;
    const int Ep1 = (int)nEp, El1 = (int)nEl;
    plan.src_ob.resize(std::max<size_t>(nEp + nEl, 1));
    for (int m = 0; m < s.M_add; ++m) {      // bias vertices of the added edges' keyframes (new numbering: kept ones shifted, added ones from the call)
        for (int kk : {s.imu_kf_i[m], s.imu_kf_j[m]}) {
            const int vb = kk < Kk ? cur.vid_bias[kk + nd] : (s.vid_bias ? s.vid_bias[kk - Kk] : -1);
            if (vb < 0) PLBA_PLAN_FAIL(PLBA_ERR_INVALID, "added imu edge %d: keyframe without bias vertex", m);
        }
    }
    // ==== every check has passed: the rest fills `next` and `plan` ====================================================================
    next.have_cam = cur.have_cam; next.fx = cur.fx; next.fy = cur.fy; next.cx = cur.cx; next.cy = cur.cy;
    memcpy(next.Rbc, cur.Rbc, sizeof next.Rbc); memcpy(next.Pbc, cur.Pbc, sizeof next.Pbc); memcpy(next.gw, cur.gw, sizeof next.gw);
    next.K = K1; next.Np = Np1; next.Nl = Nl1; next.Ep = Ep1; next.El = El1;
    // ---- keyframes: ids and flags of the kept ones shifted, the added ones behind them; their states reach the device from plan.kf_add ----
    next.vid_pvr.assign(cur.vid_pvr.begin() + nd, cur.vid_pvr.end()); next.vid_bias.assign(cur.vid_bias.begin() + nd, cur.vid_bias.end());
    next.fix_pvr.assign(cur.fix_pvr.begin() + nd, cur.fix_pvr.end()); next.fix_bias.assign(cur.fix_bias.begin() + nd, cur.fix_bias.end());
    next.vid_pvr.resize(K1); next.vid_bias.resize(K1, -1); next.fix_pvr.resize(K1, 0); next.fix_bias.resize(K1, 0);
    plan.kf_add.assign((size_t)std::max(s.K_add, 1) * KF_STRIDE, 0.0);
    for (int k = 0; k < s.K_add; ++k) {
        double* o = &plan.kf_add[(size_t)k * KF_STRIDE];
        memcpy(o, s.P3 + 3 * k, 24); memcpy(o + 3, s.V3 + 3 * k, 24); memcpy(o + 6, s.q_xyzw4 + 4 * k, 32);
        if (s.bg3) memcpy(o + 10, s.bg3 + 3 * k, 24);
        if (s.ba3) memcpy(o + 13, s.ba3 + 3 * k, 24);
        if (s.dbg3) memcpy(o + 16, s.dbg3 + 3 * k, 24);
        if (s.dba3) memcpy(o + 19, s.dba3 + 3 * k, 24);
        next.vid_pvr[Kk + k] = s.vid_pvr[k]; next.vid_bias[Kk + k] = s.vid_bias ? s.vid_bias[k] : -1;
    }
    if (s.fixed_pvr) for (int k = 0; k < K1; ++k) next.fix_pvr[k] = s.fixed_pvr[k];
    if (s.fixed_bias) for (int k = 0; k < K1; ++k) next.fix_bias[k] = s.fixed_bias[k];
    next.kf0.assign((size_t)K1 * KF_STRIDE, 0.0);      // (stale: carry_kf)
    // ---- landmarks: where each slot of the new array comes from, the packed additions, the fixed flags in the new numbering ---------
    {
        const int L1 = Np1 + Nl1;
        std::vector<int32_t>& src = plan.src_lm; src.assign(std::max(L1, 1), 0);
        for (int i = 0; i < Np0; ++i) if (pmap[i] >= 0) src[pmap[i]] = i;
        for (int i = 0; i < s.Np_add; ++i) src[Npk + i] = -(1 + i);
        for (int i = 0; i < Nl0; ++i) if (lmap[i] >= 0) src[Np1 + lmap[i]] = Np0 + i;
        for (int i = 0; i < s.Nl_add; ++i) src[Np1 + Nlk + i] = -(1 + s.Np_add + i);
        std::vector<double>& add = plan.add_lm; add.assign((size_t)std::max(s.Np_add + s.Nl_add, 1) * 6, 0.0);
        for (int i = 0; i < s.Np_add; ++i) memcpy(&add[(size_t)i * 6], s.xyz3 + 3 * (size_t)i, 24);
        for (int i = 0; i < s.Nl_add; ++i) memcpy(&add[(size_t)(s.Np_add + i) * 6], s.sPeP6 + 6 * (size_t)i, 48);
        next.pt_fixed.assign(Np1, 0); next.ln_fixed.assign(Nl1, 0);
        for (int i = 0; i < Np0; ++i) if (pmap[i] >= 0) next.pt_fixed[pmap[i]] = cur.pt_fixed[i];
        for (int i = 0; i < s.Np_add; ++i) next.pt_fixed[Npk + i] = s.point_fixed ? s.point_fixed[i] : 0;
        for (int i = 0; i < Nl0; ++i) if (lmap[i] >= 0) next.ln_fixed[lmap[i]] = cur.ln_fixed[i];
        for (int i = 0; i < s.Nl_add; ++i) next.ln_fixed[Nlk + i] = s.line_fixed ? s.line_fixed[i] : 0;
        next.pts.assign((size_t)Np1 * 3, 0.0); next.lns.assign((size_t)Nl1 * 6, 0.0);      // (stale: carry_pts / carry_lns)
    }
    // ---- measurements and weights: the packed additions; the host arrays only follow the new sizes (stale: carry_po / carry_lo — their
    // contents are whatever the storage held, no pass over them per slide) -----------------------------------------------------------------
    {
        std::vector<double>& add = plan.add_ob; add.resize(std::max<size_t>(3 * (size_t)s.Ep_add + 4 * (size_t)s.El_add, 1));
        double* a_uv = add.data(); double* a_wp = a_uv + 2 * (size_t)s.Ep_add; double* a_l = a_wp + s.Ep_add; double* a_wl = a_l + 3 * (size_t)s.El_add;
        if (s.Ep_add) memcpy(a_uv, s.uv2, 16 * (size_t)s.Ep_add);
        for (int e = 0; e < s.Ep_add; ++e) a_wp[e] = s.po_inv_sigma2 ? (double)(float)s.po_inv_sigma2[e] : 1.0;      // const float& invSigma2 (mapHandler.cpp:5340)
        if (s.El_add) memcpy(a_l, s.l3, 24 * (size_t)s.El_add);
        for (int e = 0; e < s.El_add; ++e) a_wl[e] = s.lo_inv_sigma2 ? (double)(float)s.lo_inv_sigma2[e] : 1.0;
        next.po_uv.resize(2 * (size_t)Ep1); next.po_w.resize(Ep1); next.lo_l.resize(3 * (size_t)El1); next.lo_w.resize(El1);
    }
    next.level.assign((size_t)Ep1 + El1, 0);      // a new graph: every edge at level 0
    // ---- IMU edges: those of the kept keyframes, shifted, then the added ones ---------------------------------------------------------
    next.imu_i.clear(); next.imu_j.clear(); next.imu_pre.clear(); next.imu_ipvr.clear(); next.imu_ibias.clear();
    for (int m = 0; m < M0; ++m) {
        if (cur.imu_i[m] < nd || cur.imu_j[m] < nd) continue;
        next.imu_i.push_back(cur.imu_i[m] - nd); next.imu_j.push_back(cur.imu_j[m] - nd);
        next.imu_pre.insert(next.imu_pre.end(), &cur.imu_pre[(size_t)m * 142], &cur.imu_pre[(size_t)m * 142] + 142);
        next.imu_ipvr.insert(next.imu_ipvr.end(), &cur.imu_ipvr[(size_t)m * 81], &cur.imu_ipvr[(size_t)m * 81] + 81);
        next.imu_ibias.insert(next.imu_ibias.end(), &cur.imu_ibias[(size_t)m * 36], &cur.imu_ibias[(size_t)m * 36] + 36);
    }
    for (int m = 0; m < s.M_add; ++m) {
        next.imu_i.push_back(s.imu_kf_i[m]); next.imu_j.push_back(s.imu_kf_j[m]);
        next.imu_pre.insert(next.imu_pre.end(), s.preint142 + (size_t)m * 142, s.preint142 + (size_t)m * 142 + 142);
        next.imu_ipvr.insert(next.imu_ipvr.end(), s.info_pvr81 + (size_t)m * 81, s.info_pvr81 + (size_t)m * 81 + 81);
        next.imu_ibias.insert(next.imu_ibias.end(), s.info_bias36 + (size_t)m * 36, s.info_bias36 + (size_t)m * 36 + 36);
    }
    next.M = (int)next.imu_i.size();
    next.carry_pts = next.carry_lns = next.carry_kf = next.carry_po = next.carry_lo = true;
    return PLBA_OK;
}
#undef PLBA_PLAN_FAIL

}  // namespace plba
