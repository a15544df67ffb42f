// Stand-alone host program around plba_track_dev.h, used by tests/test_track_cpu.py and tools/time_track.py: it runs the device's
// arithmetic and reduction order on the CPU — 64 emulated lanes — or, with one lane, the plain-C++ route of
// include/plba_g2o/track_pose.h, through that header in both cases.  Not linked into libplba_hip.so, never used by the product path.
//
//   plba_track_hostcheck IN OUT LANES [REPS]
//   plba_track_hostcheck select IN OUT LANES
// IN:  int32 [B, max_iters, max_iters_ref, min_features, has_T0, has_masks], double [homog_th, min_error, min_error_change, inlier_k,
//      fx, fy, cx, cy], int32 pt_start[B + 1], ln_start[B + 1], double P3, uv2, pt_sigma2, sPeP6, l3, spl_epl4, ln_sigma2, T0 (B x 16 if
//      has_T0), uint8 masks (points, lines).
// OUT: per problem double [DT16, T_opt16, H36, cov36, cov_eig6, err, pt_mean, pt_stdv, ln_mean, ln_stdv] and int32 [n_inliers_pt,
//      n_inliers_ln, iters0, iters1, iters2, path, status, good]; then the masks.  REPS > 1 repeats the batch and prints the ms per batch.
// select: IN = int32 [n, has_mask], double v[n], uint8 mask[n] (if has_mask); OUT = double [element k of the sorted (flagged) values, for
//      every k], through track::select with LANES lanes.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plba_g2o/track_pose.h"

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_select(const char* in, const char* out, int lanes) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror(in); return 2; }
    std::vector<int32_t> hd;
    std::vector<double> v;
    std::vector<uint8_t> m;
    bool ok = rd(f, hd, 2) && hd[0] >= 0 && rd(f, v, (size_t)hd[0]) && (!hd[1] || rd(f, m, (size_t)hd[0]));
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", in); return 2; }
    int cnt = 0;
    for (int i = 0; i < hd[0]; ++i) cnt += (!hd[1] || m[(size_t)i]) ? 1 : 0;
    std::vector<plba::relpose::Acc> acc((size_t)lanes);
    plba::track::HostWave w{lanes, acc.data()};
    std::vector<double> r((size_t)cnt);
    for (int k = 0; k < cnt; ++k) r[(size_t)k] = plba::track::select(w, v.data(), hd[1] ? m.data() : nullptr, hd[0], k);
    f = fopen(out, "wb");
    if (!f) { perror(out); return 2; }
    ok = cnt == 0 || fwrite(r.data(), 8, r.size(), f) == r.size();
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc >= 5 && !strcmp(argv[1], "select")) {
        const int lanes = atoi(argv[4]);
        if (lanes < 1 || (lanes & (lanes - 1))) { fprintf(stderr, "LANES must be a power of two\n"); return 2; }
        return run_select(argv[2], argv[3], lanes);
    }
    if (argc < 4) { fprintf(stderr, "usage: %s IN OUT LANES [REPS] | select IN OUT LANES\n", argv[0]); return 2; }
    const int lanes = atoi(argv[3]), reps = argc > 4 ? atoi(argv[4]) : 1;
    if (lanes < 1 || (lanes & (lanes - 1)) || reps < 1) { fprintf(stderr, "LANES must be a power of two, REPS >= 1\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> hd, ps, ls;
    std::vector<double> par, P, uv, s2p, pq, l3, se, s2l, T0;
    std::vector<uint8_t> pm, lm;
    bool ok = rd(f, hd, 6) && rd(f, par, 8);
    const int B = ok ? hd[0] : 0;
    ok = ok && B >= 1 && rd(f, ps, (size_t)B + 1) && rd(f, ls, (size_t)B + 1);
    const size_t Np = ok ? (size_t)ps[B] : 0, Nl = ok ? (size_t)ls[B] : 0;
    ok = ok && rd(f, P, 3 * Np) && rd(f, uv, 2 * Np) && rd(f, s2p, Np) && rd(f, pq, 6 * Nl) && rd(f, l3, 3 * Nl) && rd(f, se, 4 * Nl) && rd(f, s2l, Nl) &&
         rd(f, T0, hd[4] ? 16 * (size_t)B : 0);
    if (ok && hd[5]) ok = rd(f, pm, Np) && rd(f, lm, Nl);
    else { pm.assign(Np, 1); lm.assign(Nl, 1); }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", argv[1]); return 2; }
    plba_g2o::TrackConfig cfg;
    cfg.max_iters = hd[1]; cfg.max_iters_ref = hd[2]; cfg.min_features = hd[3];
    cfg.homog_th = par[0]; cfg.min_error = par[1]; cfg.min_error_change = par[2]; cfg.inlier_k = par[3];
    cfg.fx = par[4]; cfg.fy = par[5]; cfg.cx = par[6]; cfg.cy = par[7];
    std::vector<double> od((size_t)B * 115);
    std::vector<int32_t> oi((size_t)B * 8);
    std::vector<uint8_t> pmo(Np), lmo(Nl);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; ++rep)
        for (int b = 0; b < B; ++b) {
            std::vector<plba_g2o::TrackPoint> pts((size_t)(ps[b + 1] - ps[b]));
            std::vector<plba_g2o::TrackLine> lns((size_t)(ls[b + 1] - ls[b]));
            for (size_t i = 0; i < pts.size(); ++i) {
                const size_t k = (size_t)ps[b] + i;
                memcpy(pts[i].P, &P[3 * k], 24); memcpy(pts[i].pl_obs, &uv[2 * k], 16); pts[i].sigma2 = s2p[k]; pts[i].inlier = pm[k] != 0;
            }
            for (size_t i = 0; i < lns.size(); ++i) {
                const size_t k = (size_t)ls[b] + i;
                memcpy(lns[i].sP, &pq[6 * k], 24); memcpy(lns[i].eP, &pq[6 * k + 3], 24); memcpy(lns[i].le_obs, &l3[3 * k], 24);
                memcpy(lns[i].spl, &se[4 * k], 16); memcpy(lns[i].epl, &se[4 * k + 2], 16); lns[i].sigma2 = s2l[k]; lns[i].inlier = lm[k] != 0;
            }
            plba_g2o::TrackReport r;
            plba_g2o::trackPose(pts, lns, cfg, hd[4] ? &T0[16 * (size_t)b] : nullptr, r, lanes);
            double* o = &od[(size_t)b * 115];
            memcpy(o, r.DT, 128); memcpy(o + 16, r.T_opt, 128); memcpy(o + 32, r.H, 288); memcpy(o + 68, r.cov, 288); memcpy(o + 104, r.cov_eig, 48);
            o[110] = r.err; o[111] = r.pt_mean; o[112] = r.pt_stdv; o[113] = r.ln_mean; o[114] = r.ln_stdv;
            int32_t* q = &oi[(size_t)b * 8];
            q[0] = r.n_inliers_pt; q[1] = r.n_inliers_ln; q[2] = r.iters[0]; q[3] = r.iters[1]; q[4] = r.iters[2]; q[5] = r.path; q[6] = r.status; q[7] = r.good;
            for (size_t i = 0; i < pts.size(); ++i) pmo[(size_t)ps[b] + i] = pts[i].inlier ? 1 : 0;
            for (size_t i = 0; i < lns.size(); ++i) lmo[(size_t)ls[b] + i] = lns[i].inlier ? 1 : 0;
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
