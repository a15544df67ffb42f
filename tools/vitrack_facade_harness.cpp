// The graph of plba_track_inertial (include/plba.h) built from the g2o facade's classes and run through SparseOptimizer::optimize, i.e.
// optimizeHost: VertexNavState x 2, EdgeNavState, EdgeNavStatePrior, EdgeNavStatePointXYZOnlyPose and EdgeNavStateLineOnlyPose, the
// rounds, the kernels and the gate written here as a call site would write them (levels, setRobustKernel).  A third statement of the
// protocol's control flow next to csrc/plba_vitrack_dev.h and tests/vitrack_ref.py; built by tests/test_vitrack_cpu.py with plain g++
// against libplba_hip.so (no device is touched: every edge is host-evaluated).  Not part of the product library.
//
//   vitrack_facade_harness IN OUT
// IN: the input file of csrc/plba_vitrack_hostcheck.cpp.  OUT: per problem double [state_i22, state_j22, chi2_initial, chi2_final] and
// int32 [iterations[8], trials, solver_failures]; then the masks (points, lines).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plba_g2o/g2otypes.h"

using namespace g2o;

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static NavState nav(const double* s22) {
    NavState ns;
    for (int i = 0; i < 22; ++i) ns.raw()[i] = s22[i];
    return ns;
}
template <class E>
static void set_kernel(E* e, double delta) {
    if (delta > 0.0) { auto* rk = new g2o::RobustKernelHuber; e->setRobustKernel(rk); rk->setDelta(delta); }
    else e->setRobustKernel(0);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
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
    const size_t Np = ok ? (size_t)ps[B] : 0, Nl = ok ? (size_t)ls[B] : 0;
    ok = ok && rd(f, P, 3 * Np) && rd(f, uv, 2 * Np) && rd(f, wp, Np) && rd(f, pq, 6 * Nl) && rd(f, l3, 3 * Nl) && rd(f, wl, Nl);
    if (ok && hd[5]) ok = rd(f, pm, Np) && rd(f, lm, Nl);
    else { pm.assign(Np, 1); lm.assign(Nl, 1); }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short or malformed input\n", argv[1]); return 2; }
    const int rounds = hd[1], iters = hd[2], max_trials = hd[3], robust_rounds = hd[4];
    const double lambda_init = par[1], huber_pt = par[2], huber_ln = par[3], huber_imu = par[4], chi2_pt = par[5], chi2_ln = par[6];
    Matrix3d Rbc;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rbc(i, j) = par[11 + i * 3 + j];
    const Vector3d Pbc(par[20], par[21], par[22]), gw(par[23], par[24], par[25]);
    std::vector<double> od(46 * nb);
    std::vector<int32_t> oi(10 * nb, 0);

    for (int b = 0; b < B; ++b) {
        g2o::SparseOptimizer optimizer;
        auto* lm_alg = new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<g2o::BlockSolverX>(g2o::make_unique<SlamLinearSolver>()));
        lm_alg->setUserLambdaInit(lambda_init);
        lm_alg->setMaxTrialsAfterFailure(max_trials);
        optimizer.setAlgorithm(lm_alg);
        auto* vi = new VertexNavState; vi->setId(0); vi->setEstimate(nav(&si[22 * (size_t)b])); vi->setFixed(!af[(size_t)b]); optimizer.addVertex(vi);
        auto* vj = new VertexNavState; vj->setId(1); vj->setEstimate(nav(&sj[22 * (size_t)b])); vj->setFixed(false); optimizer.addVertex(vj);
        auto* eimu = new EdgeNavState;
        eimu->setVertex(0, vi); eimu->setVertex(1, vj);
        IMUPreintegrator M; M.setPayload(&pre[142 * (size_t)b]);
        eimu->setMeasurement(M); eimu->SetParams(gw);
        std::vector<double> info(225, 0.0);
        for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) info[(size_t)r * 15 + c] = ip[81 * (size_t)b + r * 9 + c];
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) info[(size_t)(9 + r) * 15 + 9 + c] = ib[36 * (size_t)b + r * 6 + c];
        eimu->setInformationRowMajor(info);
        set_kernel(eimu, huber_imu);
        optimizer.addEdge(eimu);
        if (af[(size_t)b]) {
            auto* ep = new EdgeNavStatePrior;
            ep->setVertex(0, vi); ep->setMeasurement(nav(&pst[22 * (size_t)b]));
            ep->setInformationRowMajor(std::vector<double>(&pinfo[225 * (size_t)b], &pinfo[225 * (size_t)b] + 225));
            optimizer.addEdge(ep);
        }
        std::vector<EdgeNavStatePointXYZOnlyPose*> epts;
        std::vector<EdgeNavStateLineOnlyPose*> elns;
        for (int k = ps[b]; k < ps[b + 1]; ++k) {
            auto* e = new EdgeNavStatePointXYZOnlyPose;
            e->setVertex(0, vj); e->setMeasurement(Vector2d(uv[2 * (size_t)k], uv[2 * (size_t)k + 1]));
            e->setInformationRowMajor({wp[(size_t)k], 0.0, 0.0, wp[(size_t)k]});
            e->SetParams(par[7], par[8], par[9], par[10], Rbc, Pbc, Vector3d(P[3 * (size_t)k], P[3 * (size_t)k + 1], P[3 * (size_t)k + 2]));
            e->setLevel(pm[(size_t)k] ? 0 : 1);
            optimizer.addEdge(e); epts.push_back(e);
        }
        for (int k = ls[b]; k < ls[b + 1]; ++k) {
            auto* e = new EdgeNavStateLineOnlyPose;
            const double* q = &pq[6 * (size_t)k];
            e->setVertex(0, vj); e->setMeasurement(Vector3d(l3[3 * (size_t)k], l3[3 * (size_t)k + 1], l3[3 * (size_t)k + 2]));
            e->setInformationRowMajor({wl[(size_t)k], 0.0, 0.0, wl[(size_t)k]});
            e->SetParams(par[7], par[8], par[9], par[10], Rbc, Pbc, Vector3d(q[0], q[1], q[2]), Vector3d(q[3], q[4], q[5]));
            e->setLevel(lm[(size_t)k] ? 0 : 1);
            optimizer.addEdge(e); elns.push_back(e);
        }
        auto kernels = [&](bool on) {
            for (auto* e : epts) set_kernel(e, on ? huber_pt : 0.0);
            for (auto* e : elns) set_kernel(e, on ? huber_ln : 0.0);
        };
        double* o = &od[46 * (size_t)b];
        int32_t* q = &oi[10 * (size_t)b];
        optimizer.initializeOptimization(0);
        kernels(0 < robust_rounds);
        optimizer.computeActiveErrors();
        o[44] = optimizer.activeRobustChi2();
        for (int r = 0; r < rounds; ++r) {
            kernels(r < robust_rounds);
            optimizer.initializeOptimization(0);
            q[r] = optimizer.optimize(iters);
            q[8] += optimizer.lastStats().trials; q[9] += optimizer.lastStats().solver_failures;
            for (auto* e : epts) { e->computeError(); e->setLevel((e->chi2() > chi2_pt || !e->isDepthPositive()) ? 1 : 0); }
            for (auto* e : elns) { e->computeError(); e->setLevel((e->chi2() > chi2_ln || !e->isDepthPositive()) ? 1 : 0); }
        }
        kernels((rounds > 0 ? rounds - 1 : 0) < robust_rounds);
        optimizer.initializeOptimization(0);
        optimizer.computeActiveErrors();
        o[45] = optimizer.activeRobustChi2();
        for (int k = 0; k < 22; ++k) { o[k] = vi->estimate().raw()[k]; o[22 + k] = vj->estimate().raw()[k]; }
        for (size_t k = 0; k < epts.size(); ++k) pm[(size_t)ps[b] + k] = epts[k]->level() == 0 ? 1 : 0;
        for (size_t k = 0; k < elns.size(); ++k) lm[(size_t)ls[b] + k] = elns[k]->level() == 0 ? 1 : 0;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    ok = fwrite(od.data(), 8, od.size(), f) == od.size() && fwrite(oi.data(), 4, oi.size(), f) == oi.size();
    ok = ok && (Np == 0 || fwrite(pm.data(), 1, Np, f) == Np) && (Nl == 0 || fwrite(lm.data(), 1, Nl, f) == Nl);
    ok = (fclose(f) == 0) && ok;
    return ok ? 0 : 2;
}
