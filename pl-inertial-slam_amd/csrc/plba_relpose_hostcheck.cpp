// Stand-alone host program around plba_relpose_dev.h, used by tests/test_relpose_cpu.py and tools/time_relpose.py: it runs the device's
// arithmetic and reduction order on the CPU — 64 emulated lanes — or, with one lane, the plain-C++ drop-in of
// include/plba_g2o/relative_pose.h, through that header in both cases.  Not linked into libplba_hip.so, never used by the product path.
//
//   plba_relpose_hostcheck IN OUT LANES [REPS]
// IN:  int32 [B, protocol, max_iters, max_iters_ref, has_T0, has_masks], double [homog_th, chi2_th, lc_res, lc_unc, lc_inl, lc_trs, lc_rot,
//      fx, fy, cx, cy], int32 pt_start[B + 1], ln_start[B + 1], double P3, uv2, sPeP6, l3, T0 (B x 16 if has_T0), uint8 masks (points, lines).
// OUT: per candidate double [T_inc16, pose_inc6, H36, e, cov_eig6, t, r] and int32 [n_inliers, iters0, iters1, status, accepted, lc_res,
//      lc_unc, lc_inl, lc_trs, lc_rot, returned]; then the masks.  REPS > 1 repeats the batch and prints the milliseconds per batch.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plba_g2o/relative_pose.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s IN OUT LANES [REPS]\n", argv[0]); return 2; }
    const int lanes = atoi(argv[3]), reps = argc > 4 ? atoi(argv[4]) : 1;
    if (lanes < 1 || (lanes & (lanes - 1)) || reps < 1) { fprintf(stderr, "LANES must be a power of two, REPS >= 1\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd, ps, ls;
    std::vector<double> par, P, uv, pq, l3, T0;
    std::vector<uint8_t> pm, lm;
    bool ok = rd(f, hd, 6) && rd(f, par, 11);
    const int B = ok ? hd[0] : 0;
    ok = ok && B >= 1 && rd(f, ps, (size_t)B + 1) && rd(f, ls, (size_t)B + 1);
    const size_t Np = ok ? (size_t)ps[B] : 0, Nl = ok ? (size_t)ls[B] : 0;
    ok = ok && rd(f, P, 3 * Np) && rd(f, uv, 2 * Np) && rd(f, pq, 6 * Nl) && rd(f, l3, 3 * Nl) && rd(f, T0, hd[4] ? 16 * (size_t)B : 0);
    if (ok && hd[5]) ok = rd(f, pm, Np) && rd(f, lm, Nl);
    else { pm.assign(Np, 1); lm.assign(Nl, 1); }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", argv[1]); return 2; }
    plba_g2o::RelposeConfig cfg;
    cfg.max_iters = hd[2]; cfg.max_iters_ref = hd[3]; cfg.homog_th = par[0]; cfg.chi2_th = par[1];
    cfg.lc_res = par[2]; cfg.lc_unc = par[3]; cfg.lc_inl = par[4]; cfg.lc_trs = par[5]; cfg.lc_rot = par[6];
    cfg.fx = par[7]; cfg.fy = par[8]; cfg.cx = par[9]; cfg.cy = par[10];
    std::vector<double> od((size_t)B * 73);
    std::vector<int32_t> oi((size_t)B * 11);
    std::vector<uint8_t> pmo(Np), lmo(Nl);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; ++rep)
        for (int b = 0; b < B; ++b) {
            std::vector<plba_g2o::PointFeature> pts((size_t)(ps[b + 1] - ps[b]));
            std::vector<plba_g2o::LineFeature> lns((size_t)(ls[b + 1] - ls[b]));
            std::vector<plba_g2o::Vector4i> pi(pts.size()), li(lns.size());
            for (size_t i = 0; i < pts.size(); ++i) {
                const size_t k = (size_t)ps[b] + i;
                memcpy(pts[i].P, &P[3 * k], 24); memcpy(pts[i].pl_obs, &uv[2 * k], 16); pts[i].inlier = pm[k] != 0;
                pi[i] = {(int)i, (int)i, (int)i, (int)i};
            }
            for (size_t i = 0; i < lns.size(); ++i) {
                const size_t k = (size_t)ls[b] + i;
                memcpy(lns[i].sP, &pq[6 * k], 24); memcpy(lns[i].eP, &pq[6 * k + 3], 24); memcpy(lns[i].le_obs, &l3[3 * k], 24); lns[i].inlier = lm[k] != 0;
                li[i] = {(int)i, (int)i, (int)i, (int)i};
            }
            double pose[6] = {0, 0, 0, 0, 0, 0};
            plba_g2o::RelposeReport r;
            const double* t0p = hd[4] ? &T0[16 * (size_t)b] : nullptr;
            const bool ret = hd[1] == 0 ? plba_g2o::computeRelativePoseRobustGN(pts, lns, pi, li, pose, cfg, &r, t0p, lanes)
                                        : plba_g2o::computeRelativePoseGN(pts, lns, pi, li, pose, cfg, &r, t0p, lanes);
            double* o = &od[(size_t)b * 73];
            memcpy(o, r.T_inc, 128); memcpy(o + 16, r.pose_inc, 48); memcpy(o + 22, r.H, 288); o[58] = r.e; memcpy(o + 59, r.d.cov_eig, 48); o[65] = r.d.t; o[66] = r.d.r;
            memcpy(o + 67, pose, 48);
            int32_t* q = &oi[(size_t)b * 11];
            q[0] = r.n_inliers; q[1] = r.iters[0]; q[2] = r.iters[1]; q[3] = r.d.status; q[4] = r.d.accepted; q[5] = r.d.lc_res; q[6] = r.d.lc_unc;
            q[7] = r.d.lc_inl; q[8] = r.d.lc_trs; q[9] = r.d.lc_rot; q[10] = ret ? 1 : 0;
            // the masks: an accepted candidate's lists come back compacted (their indices say which features stayed), a refused one's in place
            for (size_t i = 0; i < (size_t)(ps[b + 1] - ps[b]); ++i) pmo[(size_t)ps[b] + i] = 0;
            for (size_t i = 0; i < (size_t)(ls[b + 1] - ls[b]); ++i) lmo[(size_t)ls[b] + i] = 0;
            if (ret) {
                for (const auto& v : pi) pmo[(size_t)ps[b] + (size_t)v[0]] = 1;
                for (const auto& v : li) lmo[(size_t)ls[b] + (size_t)v[0]] = 1;
            } else {
                for (size_t i = 0; i < pts.size(); ++i) pmo[(size_t)ps[b] + i] = pts[i].inlier ? 1 : 0;
                for (size_t i = 0; i < lns.size(); ++i) lmo[(size_t)ls[b] + i] = lns[i].inlier ? 1 : 0;
            }
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    if (reps > 1) printf("%.6f\n", ms);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = fwrite(od.data(), 8, od.size(), f) == od.size() && fwrite(oi.data(), 4, oi.size(), f) == oi.size();
    ok = ok && (Np == 0 || fwrite(pmo.data(), 1, Np, f) == Np) && (Nl == 0 || fwrite(lmo.data(), 1, Nl, f) == Nl);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}
