// Stand-alone host program around plba_vitrack_dev.h, used by tests/test_vitrack_cpu.py and tools/time_track_inertial.py: it runs the
// device's arithmetic and reduction order on the CPU — 64 emulated lanes — or, with one lane, the plain-C++ route of
// include/plba_g2o/track_inertial.h, through that header in both cases.  Not linked into libplba_hip.so, never used by the product path.
//
//   plba_vitrack_hostcheck IN OUT LANES [REPS]
// IN:  int32 [B, rounds, iters, max_trials, robust_rounds, has_masks], double [tau, user_lambda_init, huber_pt, huber_ln, huber_imu,
//      chi2_pt, chi2_ln, fx, fy, cx, cy, Rbc9, Pbc3, gw3], uint8 anchor_free[B], double state_i22, state_j22, preint142, info_pvr81,
//      info_bias36, prior_state22, prior_info225 (B rows each), int32 pt_start[B + 1], ln_start[B + 1], double Pw3, uv2, pt_inv_sigma2,
//      sPeP6, l3, ln_inv_sigma2, uint8 masks (points, lines; if has_masks).
// OUT: B plba_vitrack_result as they lie in memory; then the masks.  REPS > 1 repeats the batch and prints the ms per batch.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plba_g2o/track_inertial.h"

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
    std::vector<double> par, si, sj, pre, ip, ib, pst, pinfo, P, uv, wp, pq, l3, wl;
    std::vector<uint8_t> af, pm, lm;
    bool ok = rd(f, hd, 6) && rd(f, par, 26);
    const int B = ok ? hd[0] : 0;
    const size_t nb = (size_t)(B > 0 ? B : 0);
    ok = ok && B >= 1 && rd(f, af, nb) && rd(f, si, 22 * nb) && rd(f, sj, 22 * nb) && rd(f, pre, 142 * nb) && rd(f, ip, 81 * nb) && rd(f, ib, 36 * nb) &&
         rd(f, pst, 22 * nb) && rd(f, pinfo, 225 * nb) && rd(f, ps, nb + 1) && rd(f, ls, nb + 1);
    ok = ok && ps[0] == 0 && ls[0] == 0;
    for (int b = 0; ok && b < B; ++b) ok = ps[b + 1] >= ps[b] && ls[b + 1] >= ls[b];
    const size_t Np = ok ? (size_t)ps[B] : 0, Nl = ok ? (size_t)ls[B] : 0;
    ok = ok && rd(f, P, 3 * Np) && rd(f, uv, 2 * Np) && rd(f, wp, Np) && rd(f, pq, 6 * Nl) && rd(f, l3, 3 * Nl) && rd(f, wl, Nl);
    if (ok && hd[5]) ok = rd(f, pm, Np) && rd(f, lm, Nl);
    else { pm.assign(Np, 1); lm.assign(Nl, 1); }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", argv[1]); return 2; }
    plba_g2o::ViConfig cfg;
    cfg.rounds = hd[1]; cfg.iters = hd[2]; cfg.max_trials = hd[3]; cfg.robust_rounds = hd[4];
    cfg.tau = par[0]; cfg.user_lambda_init = par[1]; cfg.huber_pt = par[2]; cfg.huber_ln = par[3]; cfg.huber_imu = par[4]; cfg.chi2_pt = par[5]; cfg.chi2_ln = par[6];
    cfg.fx = par[7]; cfg.fy = par[8]; cfg.cx = par[9]; cfg.cy = par[10];
    memcpy(cfg.Rbc, &par[11], 72); memcpy(cfg.Pbc, &par[20], 24); memcpy(cfg.gw, &par[23], 24);
    if (cfg.rounds < 0 || cfg.rounds > 8 || cfg.iters < 0 || cfg.max_trials < 0) { fprintf(stderr, "%s: options out of range\n", argv[1]); return 2; }
    std::vector<plba_vitrack_result> out(nb);
    std::vector<uint8_t> pmo(Np), lmo(Nl);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; ++rep)
        for (int b = 0; b < B; ++b) {
            std::vector<plba_g2o::ViPoint> pts((size_t)(ps[b + 1] - ps[b]));
            std::vector<plba_g2o::ViLine> lns((size_t)(ls[b + 1] - ls[b]));
            for (size_t i = 0; i < pts.size(); ++i) {
                const size_t k = (size_t)ps[b] + i;
                memcpy(pts[i].Pw, &P[3 * k], 24); memcpy(pts[i].uv, &uv[2 * k], 16); pts[i].inv_sigma2 = wp[k]; pts[i].inlier = pm[k] != 0;
            }
            for (size_t i = 0; i < lns.size(); ++i) {
                const size_t k = (size_t)ls[b] + i;
                memcpy(lns[i].sP, &pq[6 * k], 24); memcpy(lns[i].eP, &pq[6 * k + 3], 24); memcpy(lns[i].l, &l3[3 * k], 24);
                lns[i].inv_sigma2 = wl[k]; lns[i].inlier = lm[k] != 0;
            }
            plba_g2o::ViFrame fr;
            const size_t k = (size_t)b;
            fr.anchor_free = af[k] != 0;
            memcpy(fr.state_i, &si[22 * k], 176); memcpy(fr.state_j, &sj[22 * k], 176); memcpy(fr.preint, &pre[142 * k], 1136);
            memcpy(fr.info_pvr, &ip[81 * k], 648); memcpy(fr.info_bias, &ib[36 * k], 288);
            memcpy(fr.prior_state, &pst[22 * k], 176); memcpy(fr.prior_info, &pinfo[225 * k], 1800);
            plba_g2o::trackInertial(fr, pts, lns, cfg, out[k], lanes);
            for (size_t i = 0; i < pts.size(); ++i) pmo[(size_t)ps[b] + i] = pts[i].inlier ? 1 : 0;
            for (size_t i = 0; i < lns.size(); ++i) lmo[(size_t)ls[b] + i] = lns[i].inlier ? 1 : 0;
        }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    if (reps > 1) printf("%.6f\n", ms);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = fwrite(out.data(), sizeof(plba_vitrack_result), nb, f) == nb;
    ok = ok && (Np == 0 || fwrite(pmo.data(), 1, Np, f) == Np) && (Nl == 0 || fwrite(lmo.data(), 1, Nl, f) == Nl);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}
