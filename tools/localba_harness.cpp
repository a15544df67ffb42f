// localba_harness.cpp — the reference's local-BA call site re-enacted against the g2o-compatible facade.
//
// Follows the PROTOCOL of MapHandler::localBundleAdjustmentWithImuAndMarg (src/mapHandler.cpp:5741-6254) — vertex ids,
// edge insertion order, Huber deltas, optimize(5) / gating / optimize(10), marginalization factor selection, write-back —
// on a window read from a flat binary file (written by tests/test_facade.py) instead of KeyFrame/MapPoint objects.
// It proves that code written against the reference's g2o API (IMU/g2otypes.h, IMU/marginalization.h) runs on the HIP
// path unchanged in shape.  Usage: localba_harness <window.bin> <result.bin>
//
// The same translation unit also holds the OTHER g2o users of src/mapHandler.cpp, in the shape of their call sites and
// compiled against the header set include/mapHandler.h:35-45 pulls (slam3d, cholmod / dense / structure_only solvers,
// types_six_dof_expmap), so that "mapHandler.cpp compiles against include/" is checked on everything it uses from g2o:
//   localba_harness nomarg  <window.bin> <result.bin>   MapHandler::localBundleAdjustmentWithImu (USE_MARG off, :5086-5739)
//   localba_harness gyrbias <in.bin> <out.bin>          MapHandler::IMUInitEstBg (:4989-5036)
//   localba_harness pgo     <in.bin> <out.bin>          MapHandler::loopClosureOptimizationCovGraphG2O (:4299-4528), g2o part
//   localba_harness lba     <in.bin> <out.bin>          MapHandler::localBundleAdjustment + levMarquardtOptimizationLBA (:1329-2098): the
//                                                       pre-init visual-only path, which does not use g2o at all: its list building on
//                                                       map-shaped objects, then the optimiser's body as one plba_lba_visual call
//   localba_harness track   <in.bin> <out.bin>          MapHandler::lookForCommonMatches' pose refinement (:819-859) for B keyframe pairs:
//                                                       the matched lists, StereoFrameHandler::optimizePose as one plba_track_pose call,
//                                                       the inlier ratios and kf1->T_kf_w
#include "plba_g2o/vio_init.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <g2o/core/block_solver.h>
#include <g2o/core/optimization_algorithm_levenberg.h>
#include <g2o/core/robust_kernel_impl.h>
#include <g2o/core/sparse_optimizer.h>
#include <g2o/solvers/eigen/linear_solver_eigen.h>
// the rest of what include/mapHandler.h:35-45 includes from g2o
#include <g2o/types/slam3d/vertex_se3.h>
#include <g2o/types/slam3d/edge_se3.h>
#include <g2o/core/solver.h>
#include <g2o/core/robust_kernel.h>
#include <g2o/solvers/cholmod/linear_solver_cholmod.h>
#include <g2o/solvers/dense/linear_solver_dense.h>
#include <g2o/solvers/structure_only/structure_only_solver.h>
#include <g2o/types/sba/types_six_dof_expmap.h>
#include "plba_g2o/g2otypes.h"

#include <chrono>
#include <cstring>
#include <map>
#include <string>
typedef Eigen::Matrix<double, 6, 6> Matrix6d;

template <typename T> static std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }
template <typename T> static void wr(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// ---- MapHandler::localBundleAdjustment (src/mapHandler.cpp:1329-1439) + levMarquardtOptimizationLBA (:1441-2098) ----------------------
// Map-shaped objects with the members the two functions touch.  localBundleAdjustment's list building is re-enacted as written
// (local keyframes first, then per landmark its observations with the local index or -1); the optimiser keeps its signature and
// its write-back, its body is the flattening of INTEGRATION.md plus one call.
#include "plba.h"
#include <array>
namespace lba_map {
typedef std::array<int, 6> Vector6i;
struct KeyFrame { int kf_idx; Matrix4d T_kf_w; bool local; };
struct MapPoint { int idx; Vector3d point3D; std::vector<Eigen::Vector2d> obs_list; std::vector<int> kf_obs_list; bool inlier = true; };
struct MapLine { int idx; Eigen::Matrix<double, 6, 1> line3D; std::vector<Vector3d> obs_list; std::vector<int> kf_obs_list; bool inlier = true; };
struct MapHandler {
    std::vector<KeyFrame*> map_keyframes;
    std::vector<MapPoint*> map_points;
    std::vector<MapLine*> map_lines;
    double fx, fy, cx, cy;
    plba_problem* problem = nullptr;
    plba_lba_stats last;

    int levMarquardtOptimizationLBA(std::vector<double> X_aux, std::vector<int> kf_list, std::vector<int> pt_list, std::vector<int> ls_list,
                                    std::vector<Vector6i> pt_obs_list, std::vector<Vector6i> ls_obs_list) {
        // keyframes appearing in the observations -> compact index; kf_loc = position in kf_list or -1 (obs(4) of the reference)
        std::map<int, int> kfi; std::vector<double> T16; std::vector<int32_t> kf_loc;
        auto kf_of = [&](const Vector6i& o) {
            auto it = kfi.find(o[3]); if (it != kfi.end()) return it->second;
            const Matrix4d& T = map_keyframes[o[3]]->T_kf_w;
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T16.push_back(T(r, c));
            kf_loc.push_back(o[4]);
            return kfi[o[3]] = (int)kf_loc.size() - 1; };
        std::vector<int32_t> ppt, pkf, lln, lkf; std::vector<double> uv, l3;
        for (auto& o : pt_obs_list) { ppt.push_back(o[1]); pkf.push_back(kf_of(o)); const auto& z = map_points[o[0]]->obs_list[o[2]]; uv.push_back(z(0)); uv.push_back(z(1)); }
        for (auto& o : ls_obs_list) { lln.push_back(o[1]); lkf.push_back(kf_of(o)); const auto& z = map_lines[o[0]]->obs_list[o[2]]; l3.push_back(z(0)); l3.push_back(z(1)); l3.push_back(z(2)); }
        const int Nkf = kf_list.size(), Np = pt_list.size(), Nl = ls_list.size();
        double *xyz = X_aux.data() + 6 * Nkf, *pq = xyz + 3 * Np;            // the landmark part of X_aux is already the layout plba wants
        plba_lba_options o; plba_lba_default_options(&o);
        std::vector<double> Tout(T16.size()); std::vector<uint8_t> pm(Np + 1), lm(Nl + 1);
        const int rc = plba_lba_visual(problem, &o, (int)kf_loc.size(), T16.data(), kf_loc.data(), Np, xyz, Nl, pq,
                                       (int)ppt.size(), ppt.data(), pkf.data(), uv.data(), (int)lln.size(), lln.data(), lkf.data(), l3.data(),
                                       fx, fy, cx, cy, Tout.data(), pm.data(), lm.data(), &last);
        if (rc != PLBA_OK) { fprintf(stderr, "plba_lba_visual: %s\n", plba_last_error(problem)); return -1; }
        // write-back as :1925-1970
        for (int i = 0; i < Nkf; ++i) {
            const int ci = kfi.at(kf_list[i]);
            Matrix4d T; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = Tout[16 * ci + 4 * r + c];
            map_keyframes[kf_list[i]]->T_kf_w = T;
        }
        for (int i = 0; i < Np; ++i) { MapPoint* mp = map_points[pt_list[i]]; if (pm[i]) mp->inlier = false; for (int c = 0; c < 3; ++c) mp->point3D(c) = xyz[3 * i + c]; }
        for (int i = 0; i < Nl; ++i) { MapLine* ml = map_lines[ls_list[i]]; if (lm[i]) ml->inlier = false; for (int c = 0; c < 6; ++c) ml->line3D(c) = pq[6 * i + c]; }
        return last.iterations;
    }

    void localBundleAdjustment() {      // :1329-1439, list building
        std::vector<double> X_aux;
        std::vector<int> kf_list;
        for (KeyFrame* kf : map_keyframes) if (kf && kf->local) kf_list.push_back(kf->kf_idx);
        // x_kf_w of the local keyframes heads X_aux in the reference; plba_lba_visual takes logmap_se3(T_kf_w) itself: zeros keep the layout
        X_aux.assign(6 * kf_list.size(), 0.0);
        std::vector<Vector6i> pt_obs_list, ls_obs_list; std::vector<int> pt_list, ls_list;
        auto local_of = [&](int kf) { for (size_t j = 0; j < kf_list.size(); ++j) if (kf_list[j] == kf) return (int)j; return -1; };
        int lm_local_idx = 0;
        for (MapPoint* mp : map_points) {
            if (!mp) continue;
            for (int c = 0; c < 3; ++c) X_aux.push_back(mp->point3D(c));
            for (size_t i = 0; i < mp->obs_list.size(); ++i) pt_obs_list.push_back({mp->idx, lm_local_idx, (int)i, mp->kf_obs_list[i], local_of(mp->kf_obs_list[i]), 1});
            ++lm_local_idx; pt_list.push_back(mp->idx);
        }
        lm_local_idx = 0;
        for (MapLine* ml : map_lines) {
            if (!ml) continue;
            for (int c = 0; c < 6; ++c) X_aux.push_back(ml->line3D(c));
            for (size_t i = 0; i < ml->obs_list.size(); ++i) ls_obs_list.push_back({ml->idx, lm_local_idx, (int)i, ml->kf_obs_list[i], local_of(ml->kf_obs_list[i]), 1});
            ++lm_local_idx; ls_list.push_back(ml->idx);
        }
        levMarquardtOptimizationLBA(X_aux, kf_list, pt_list, ls_list, pt_obs_list, ls_obs_list);
    }
};
}  // namespace lba_map

static int visual_lba(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("in"); return 2; }
    auto hdr = rd<int32_t>(f, 5);
    const int K = hdr[0], Np = hdr[1], Nl = hdr[2], Ep = hdr[3], El = hdr[4];
    auto cam = rd<double>(f, 4); auto T = rd<double>(f, 16 * (size_t)K); auto loc = rd<int32_t>(f, K);
    auto xyz = rd<double>(f, 3 * (size_t)Np), pq = rd<double>(f, 6 * (size_t)Nl);
    auto po_pt = rd<int32_t>(f, Ep), po_kf = rd<int32_t>(f, Ep); auto uv = rd<double>(f, 2 * (size_t)Ep);
    auto lo_ln = rd<int32_t>(f, El), lo_kf = rd<int32_t>(f, El); auto l3 = rd<double>(f, 3 * (size_t)El);
    fclose(f);
    lba_map::MapHandler mh; mh.fx = cam[0]; mh.fy = cam[1]; mh.cx = cam[2]; mh.cy = cam[3];
    // local keyframes must enumerate in kf_loc order: the window generator numbers them ascending with the keyframe index
    for (int k = 0; k < K; ++k) { auto* kf = new lba_map::KeyFrame; kf->kf_idx = k; kf->local = loc[k] >= 0; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) kf->T_kf_w(r, c) = T[16 * k + 4 * r + c]; mh.map_keyframes.push_back(kf); }
    for (int i = 0; i < Np; ++i) { auto* mp = new lba_map::MapPoint; mp->idx = i; mp->point3D = Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]); mh.map_points.push_back(mp); }
    for (int e = 0; e < Ep; ++e) { auto* mp = mh.map_points[po_pt[e]]; Eigen::Vector2d z; z(0) = uv[2 * e]; z(1) = uv[2 * e + 1]; mp->obs_list.push_back(z); mp->kf_obs_list.push_back(po_kf[e]); }
    for (int i = 0; i < Nl; ++i) { auto* ml = new lba_map::MapLine; ml->idx = i; for (int c = 0; c < 6; ++c) ml->line3D(c) = pq[6 * i + c]; mh.map_lines.push_back(ml); }
    for (int e = 0; e < El; ++e) { auto* ml = mh.map_lines[lo_ln[e]]; ml->obs_list.push_back(Vector3d(l3[3 * e], l3[3 * e + 1], l3[3 * e + 2])); ml->kf_obs_list.push_back(lo_kf[e]); }
    plba_options po; plba_default_options(&po);
    if (plba_create(&po, &mh.problem) != PLBA_OK) { fprintf(stderr, "plba_create failed\n"); return 3; }
    mh.localBundleAdjustment();
    FILE* g = fopen(out, "wb");
    if (!g) { perror("out"); return 2; }
    std::vector<double> oT, oX, oL; std::vector<int32_t> flags;
    for (auto* kf : mh.map_keyframes) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) oT.push_back(kf->T_kf_w(r, c));
    for (auto* mp : mh.map_points) { for (int c = 0; c < 3; ++c) oX.push_back(mp->point3D(c)); flags.push_back(mp->inlier ? 1 : 0); }
    for (auto* ml : mh.map_lines) { for (int c = 0; c < 6; ++c) oL.push_back(ml->line3D(c)); flags.push_back(ml->inlier ? 1 : 0); }
    std::vector<int32_t> h2 = {mh.last.iterations, mh.last.updates};
    wr(g, h2); wr(g, oT); wr(g, oX); wr(g, oL); wr(g, flags);
    fclose(g);
    plba_destroy(mh.problem);
    return 0;
}

// ---- MapHandler::IMUInitEstBg (src/mapHandler.cpp:4989-5036): one VertexGyrBias, one EdgeGyrBias per keyframe pair ------------
static int imu_init_est_bg(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("in"); return 2; }
    auto hdr = rd<int32_t>(f, 2);
    const int M = hdr[0], iters = hdr[1];
    auto dR = rd<double>(f, 9 * (size_t)M), JRg = rd<double>(f, 9 * (size_t)M), Ri = rd<double>(f, 9 * (size_t)M), Rj = rd<double>(f, 9 * (size_t)M), info = rd<double>(f, 9 * (size_t)M);
    fclose(f);
    auto m3 = [](const double* p) { Matrix3d m; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m(i, j) = p[i * 3 + j]; return m; };

    g2o::SparseOptimizer optimizer;
    auto linearSolver = g2o::make_unique<SlamLinearSolver>();
    linearSolver->setBlockOrdering(false);
    auto blockSolver = g2o::make_unique<g2o::BlockSolverX>(std::move(linearSolver));
    g2o::OptimizationAlgorithm* algorithm = new g2o::OptimizationAlgorithmLevenberg(std::move(blockSolver));
    optimizer.setAlgorithm(algorithm);
    g2o::VertexGyrBias* vBiasg = new g2o::VertexGyrBias();
    vBiasg->setEstimate(Eigen::Vector3d::Zero());
    vBiasg->setId(0);
    optimizer.addVertex(vBiasg);
    for (int m = 0; m < M; ++m) {
        g2o::EdgeGyrBias* eBiasg = new g2o::EdgeGyrBias();
        eBiasg->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(0)));
        eBiasg->dRbij = m3(&dR[9 * (size_t)m]);
        eBiasg->J_dR_bg = m3(&JRg[9 * (size_t)m]);
        eBiasg->Rwbi = m3(&Ri[9 * (size_t)m]);
        eBiasg->Rwbj = m3(&Rj[9 * (size_t)m]);
        eBiasg->setInformation(m3(&info[9 * (size_t)m]));          // getCovPVPhi().bottomRightCorner(3,3).inverse(), formed by the caller
        optimizer.addEdge(eBiasg);
    }
    optimizer.initializeOptimization();
    const int done = optimizer.optimize(iters);                    // the reference: 1 ("actually a linear estimator")
    g2o::VertexGyrBias* vBgEst = static_cast<g2o::VertexGyrBias*>(optimizer.vertex(0));
    const Vector3d bg = vBgEst->estimate();
    FILE* o = fopen(out, "wb");
    if (!o) { perror("out"); return 2; }
    wr(o, std::vector<double>{bg[0], bg[1], bg[2], optimizer.lastStats().chi2_initial, optimizer.lastStats().chi2_final, (double)done});
    fclose(o);
    printf("imu_init_est_bg: %d edges, bg = (%.6e, %.6e, %.6e)\n", M, bg[0], bg[1], bg[2]);
    return 0;
}

// ---- g2o part of MapHandler::loopClosureOptimizationCovGraphG2O (src/mapHandler.cpp:4299-4528) -------------------------------------
// vertices: id, fixed flag, se3 6-vector x with estimate SE3Quat::exp(x); kf2kf edges with setInformation, loop-closure edges
// with `information() = ...`; computeInitialGuess / computeActiveErrors / optimize(maxItersPGO); poses back as SE3Quat::log().
static int pose_graph(const char* in, const char* out, bool ess_graph = false) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("in"); return 2; }
    auto hdr = rd<int32_t>(f, 5);
    const int nv = hdr[0], ne = hdr[1], nlc = hdr[2], iters = hdr[3], init_guess = hdr[4];
    auto vid = rd<int32_t>(f, nv), vfix = rd<int32_t>(f, nv); auto vx = rd<double>(f, 6 * (size_t)nv);
    auto ei = rd<int32_t>(f, ne + nlc), ej = rd<int32_t>(f, ne + nlc); auto ex = rd<double>(f, 6 * (size_t)(ne + nlc));
    fclose(f);
    auto v6 = [](const double* p) { Vector6d x; for (int i = 0; i < 6; ++i) x[i] = p[i]; return x; };

    typedef g2o::BlockSolver<g2o::BlockSolverTraits<6, 3>> BlockSolverType;
    typedef g2o::LinearSolverCholmod<BlockSolverType::PoseMatrixType> LinearSolverType;
    auto solver = new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<BlockSolverType>(g2o::make_unique<LinearSolverType>()));
    g2o::SparseOptimizer optimizer;
    optimizer.setVerbose(false);
    solver->setUserLambdaInit(1e-10);
    optimizer.setAlgorithm(solver);
    for (int i = 0; i < nv; ++i) {
        g2o::VertexSE3* v_se3 = new g2o::VertexSE3();
        v_se3->setId(vid[i]);
        v_se3->setMarginalized(false);
        v_se3->setEstimate(g2o::SE3Quat::exp(v6(&vx[6 * (size_t)i])));
        if (vfix[i]) v_se3->setFixed(true);
        optimizer.addVertex(v_se3);
    }
    for (int k = 0; k < ne + nlc; ++k) {
        g2o::EdgeSE3* e_se3 = new g2o::EdgeSE3();
        e_se3->setVertex(0, optimizer.vertex(ei[k]));
        e_se3->setVertex(1, optimizer.vertex(ej[k]));
        e_se3->setMeasurement(g2o::SE3Quat::exp(v6(&ex[6 * (size_t)k])));
        if (k < ne) e_se3->setInformation(Matrix6d::Identity());
        else e_se3->information() = Matrix6d::Identity();           // the loop-closure edges' spelling (:4406)
        optimizer.addEdge(e_se3);
    }
    optimizer.initializeOptimization();
    if (init_guess || ess_graph) optimizer.computeInitialGuess();      // loopClosureOptimizationEssGraphG2O calls it unconditionally (:4163)
    optimizer.computeActiveErrors();
    const double chi0 = optimizer.activeChi2();
    const int done = optimizer.optimize(iters);
    std::vector<double> res;
    for (int i = 0; i < nv; ++i) {
        g2o::VertexSE3* v_se3 = static_cast<g2o::VertexSE3*>(optimizer.vertex(vid[i]));
        g2o::SE3Quat Tiw_corr = v_se3->estimateAsSE3Quat();
        const Vector6d x = Tiw_corr.log();
        for (int c = 0; c < 6; ++c) res.push_back(x[c]);
    }
    res.push_back(chi0); res.push_back(optimizer.lastStats().chi2_final); res.push_back((double)done); res.push_back((double)optimizer.lastStats().trials);
    res.push_back((double)optimizer.deviceSolves());
    FILE* o = fopen(out, "wb");
    if (!o) { perror("out"); return 2; }
    wr(o, res);
    fclose(o);
    printf("pose_graph: %d vertices, %d + %d edges, chi2 %.6e -> %.6e in %d iterations\n", nv, ne, nlc, chi0, optimizer.lastStats().chi2_final, done);
    return 0;
}

static int local_ba_with_imu(const char* in, const char* out);
static int structure_only(const char* in, const char* out, bool bad_vertex);
static int local_ba_with_imu_and_marg(const char* in, const char* out, double* laps);
// `scrambled`: the same graph as the default mode, built in an order the call site does not use — landmark vertices in DESCENDING id
// order, every edge after every vertex and the edges of the landmarks in that descending order too, one measurement set again after
// addEdge: the facade must fall back from its insertion-time arrays to the objects and sort the observations itself
static bool g_scrambled = false;
static bool g_late_estimates = false;      // landmark vertices are inserted with a placeholder estimate; the real one is set after every edge is in

// ---- MapHandler::tryVioInit, the steps between its g2o graphs (src/mapHandler.cpp:4853-4980) ---------------------------------------
// in: N | dt (N-1) | dP, dV (3 (N-1)) | JPa, JVa (9 (N-1)) | Rc (9 N), pc (3 N) | Rb (9 N), pb (3 N) | Rcb 9, pcb 3
static int vio_init(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("in"); return 2; }
    const int N = rd<int32_t>(f, 1)[0];
    auto dt = rd<double>(f, N - 1); auto dP = rd<double>(f, 3 * (size_t)(N - 1)); auto dV = rd<double>(f, 3 * (size_t)(N - 1));
    auto JPa = rd<double>(f, 9 * (size_t)(N - 1)); auto JVa = rd<double>(f, 9 * (size_t)(N - 1));
    auto Rc = rd<double>(f, 9 * (size_t)N); auto pc = rd<double>(f, 3 * (size_t)N); auto Rb = rd<double>(f, 9 * (size_t)N); auto pb = rd<double>(f, 3 * (size_t)N);
    auto Rcb = rd<double>(f, 9); auto pcb = rd<double>(f, 3);
    fclose(f);
    if (N < 10) { fprintf(stderr, "tryVioInit needs 10 keyframes (:4834)\n"); return 2; }
    double gpre[3], g0[3], ba[3];
    std::vector<double> V(3 * (size_t)N);
    plba_vio::gravity(N, dt.data(), dP.data(), dV.data(), Rc.data(), pc.data(), Rcb.data(), pcb.data(), gpre, g0);
    plba_vio::acc_bias(N, dt.data(), dP.data(), dV.data(), JPa.data(), JVa.data(), Rc.data(), pc.data(), Rcb.data(), pcb.data(), g0, ba);
    plba_vio::velocities(N, dt.data(), dP.data(), dV.data(), Rb.data(), pb.data(), g0, V.data());
    std::vector<double> res(gpre, gpre + 3);
    res.insert(res.end(), g0, g0 + 3); res.insert(res.end(), ba, ba + 3); res.insert(res.end(), V.begin(), V.end());
    FILE* o = fopen(out, "wb");
    if (!o) { perror("out"); return 2; }
    wr(o, res);
    fclose(o);
    printf("vio_init: g0 = (%.4f, %.4f, %.4f), ba = (%.4e, %.4e, %.4e)\n", g0[0], g0[1], g0[2], ba[0], ba[1], ba[2]);
    return 0;
}

static int relpose(const char* in, const char* out);
static int track(const char* in, const char* out);
int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "gyrbias")) return imu_init_est_bg(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "pgo")) return pose_graph(argv[2], argv[3]);
    // MapHandler::loopClosureOptimizationEssGraphG2O (src/mapHandler.cpp:4068-4297): the same g2o calls as the covisibility-graph
    // version over the essential graph — every keyframe from the first loop keyframe on (several of them fixed: the loop ends), spanning
    // tree + strong covisibility + loop edges, computeInitialGuess before optimize.  Its size is what sends the reduced system to the
    // device (more than 384 dims).
    if (argc >= 4 && !strcmp(argv[1], "essgraph")) return pose_graph(argv[2], argv[3], true);
    if (argc >= 4 && !strcmp(argv[1], "vioinit")) return vio_init(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "nomarg")) return local_ba_with_imu(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "late")) { g_late_estimates = true; return local_ba_with_imu_and_marg(argv[2], argv[3], nullptr); }
    if (argc >= 4 && !strcmp(argv[1], "scrambled")) { g_scrambled = true; return local_ba_with_imu_and_marg(argv[2], argv[3], nullptr); }
    if (argc >= 4 && !strcmp(argv[1], "lba")) return visual_lba(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "relpose")) return relpose(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "track")) return track(argv[2], argv[3]);
    if (argc >= 4 && !strcmp(argv[1], "structonly")) return structure_only(argv[2], argv[3], false);
    if (argc >= 4 && !strcmp(argv[1], "structonly_bad")) return structure_only(argv[2], argv[3], true);
    // `time window.bin reps`: one localBundleAdjustmentWithImuAndMarg-shaped call through Boundary 1, `reps` times on fresh optimizers, lap by lap
    // (VERDICT r04 item 1b): graph construction | optimize(5) + gating loop + optimize(10) | marginalization | write-back | optimizer teardown.
    if (argc >= 4 && !strcmp(argv[1], "time")) {
        const int reps = std::max(1, atoi(argv[3]));
        double best[9] = {1e300, 1e300, 1e300, 1e300, 1e300, 1e300, 1e300, 1e300, 1e300};
        for (int r = 0; r < reps; ++r) {
            double laps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int rc = local_ba_with_imu_and_marg(argv[2], nullptr, laps);
            if (rc) return rc;
            if (r == 0 && reps > 1) continue;      // (the first call pays for module load and first-touch allocations)
            double tot = 0.0;
            for (int i = 0; i < 7; ++i) tot += laps[i];
            if (tot < best[7]) { for (int i = 0; i < 7; ++i) best[i] = laps[i]; best[7] = tot; best[8] = laps[7]; }
        }
        // facade_ba_call_ms: what end_to_end_ba_call_ms covers through the C ABI (upload + 5 + gating + 10 iterations + write-back); the call
        // site's own loops over its edge objects (gating: chi2() / isDepthPositive() / setLevel / setRobustKernel(0) per edge) are inside it
        printf("{\"facade_graph_construction_ms\": %.4f, \"facade_optimize5_ms\": %.4f, \"facade_gating_loop_ms\": %.4f, \"facade_optimize10_ms\": %.4f, "
               "\"facade_marginalize_ms\": %.4f, \"facade_write_back_ms\": %.4f, \"facade_teardown_ms\": %.4f, \"facade_ba_call_ms\": %.4f, "
               "\"facade_ba_call_with_graph_construction_ms\": %.4f, \"facade_optimize5_inside_plba_optimize_ms\": %.4f, \"reps\": %d}\n",
               best[0], best[1], best[2], best[3], best[4], best[5], best[6], best[1] + best[2] + best[3] + best[5],
               best[0] + best[1] + best[2] + best[3] + best[5] + best[6], best[8], reps);
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: %s [nomarg|gyrbias|pgo|time] window.bin result.bin\n", argv[0]); return 2; }
    return local_ba_with_imu_and_marg(argv[1], argv[2], nullptr);
}

// ---- MapHandler::localBundleAdjustmentWithImuAndMarg (src/mapHandler.cpp:5741-6254) ---------------------------------------------------
// laps (optional, ms): [0] graph construction, [1] optimize(5), [2] the gating loop, [3] optimize(10), [4] marginalization, [5] write-back, [6] teardown, [7] plba_optimize(5)'s own ms_total
static int local_ba_with_imu_and_marg(const char* in, const char* out, double* laps) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("window"); return 2; }
    auto hdr = rd<int32_t>(f, 8);
    const int K = hdr[0], Np = hdr[1], Nl = hdr[2], Ep = hdr[3], El = hdr[4], M = hdr[5], do_marg = hdr[6], max_kf_in_window = hdr[7];
    auto cam = rd<double>(f, 4); auto Rbcv = rd<double>(f, 9); auto Pbcv = rd<double>(f, 3); auto gwv = rd<double>(f, 3); auto hub = rd<double>(f, 4);
    auto kf_idx = rd<int32_t>(f, K);
    auto P = rd<double>(f, 3 * K), V = rd<double>(f, 3 * K), q = rd<double>(f, 4 * K), bg = rd<double>(f, 3 * K), ba = rd<double>(f, 3 * K);
    auto pts = rd<double>(f, 3 * (size_t)Np), lns = rd<double>(f, 6 * (size_t)Nl);
    auto po_pt = rd<int32_t>(f, Ep), po_kf = rd<int32_t>(f, Ep); auto po_uv = rd<double>(f, 2 * (size_t)Ep), po_sig = rd<double>(f, Ep);
    auto lo_ln = rd<int32_t>(f, El), lo_kf = rd<int32_t>(f, El); auto lo_l = rd<double>(f, 3 * (size_t)El), lo_sig = rd<double>(f, El);
    auto pre = rd<double>(f, 142 * (size_t)M), ipvr = rd<double>(f, 81 * (size_t)M), ibias = rd<double>(f, 36 * (size_t)M);
    fclose(f);

    Matrix3d Rbc; Vector3d tbc, gw(gwv[0], gwv[1], gwv[2]);
    for (int i = 0; i < 3; ++i) { tbc(i) = Pbcv[i]; for (int j = 0; j < 3; ++j) Rbc(i, j) = Rbcv[i * 3 + j]; }
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    bool abortFlag = false;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(tnow() - t).count(); };
    auto t_lap = tnow();
    MarginalizationInfo* new_marg_info = new MarginalizationInfo();
    int gated_pt = 0, gated_ln = 0, maxKFid = 0, maxPointId = 0;
    double chi2_final = 0.0;
    std::vector<double> oP(3 * K), oV(3 * K), oq(4 * K), odbg(3 * K), odba(3 * K), opts(3 * (size_t)Np), olns(6 * (size_t)Nl);
    {      // (scope of the optimizer: its teardown — one delete per edge and vertex — is part of what a call costs the mapping thread)
    g2o::SparseOptimizer optimizer;
    auto linearSolver = g2o::make_unique<SlamLinearSolver>();
    auto blockSolver = g2o::make_unique<g2o::BlockSolverX>(std::move(linearSolver));
    g2o::OptimizationAlgorithm* algorithm = new g2o::OptimizationAlgorithmLevenberg(std::move(blockSolver));
    optimizer.setAlgorithm(algorithm);
    optimizer.setForceStopFlag(&abortFlag);

    for (int k = 0; k < K; ++k) {                                   // :5802-5830
        NavState ns;
        ns.Set_Pos(Vector3d(P[3 * k], P[3 * k + 1], P[3 * k + 2])); ns.Set_Vel(Vector3d(V[3 * k], V[3 * k + 1], V[3 * k + 2]));
        ns.Set_Rot(Sophus::SO3(Quaterniond(q[4 * k + 3], q[4 * k], q[4 * k + 1], q[4 * k + 2])));
        ns.Set_BiasGyr(Vector3d(bg[3 * k], bg[3 * k + 1], bg[3 * k + 2])); ns.Set_BiasAcc(Vector3d(ba[3 * k], ba[3 * k + 1], ba[3 * k + 2]));
        const int idKF = kf_idx[k] * 2;
        g2o::VertexNavStatePVR* vNSPVR = new g2o::VertexNavStatePVR();
        vNSPVR->setEstimate(ns); vNSPVR->setId(idKF); vNSPVR->setFixed(k == 0);
        optimizer.addVertex(vNSPVR);
        g2o::VertexNavStateBias* vNSBias = new g2o::VertexNavStateBias();
        vNSBias->setEstimate(ns); vNSBias->setId(idKF + 1); vNSBias->setFixed(k == 0);
        optimizer.addVertex(vNSBias);
        if (idKF + 1 > maxKFid) maxKFid = idKF + 1;
    }
    std::vector<g2o::EdgeNavStatePVR*> vpEdgesNavStatePVR;
    std::vector<g2o::EdgeNavStateBias*> vpEdgesNavStateBias;
    for (int m = 0; m < M; ++m) {                                   // :5842-5885 (edge m links window keyframes m, m+1)
        IMUPreintegrator imupre; imupre.setPayload(&pre[(size_t)m * 142]);
        g2o::EdgeNavStatePVR* epvr = new g2o::EdgeNavStatePVR();
        epvr->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[m])));
        epvr->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[m + 1])));
        epvr->setVertex(2, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[m] + 1)));
        epvr->setMeasurement(imupre);
        Matrix9d InvCovPVR; for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) InvCovPVR(i, j) = ipvr[(size_t)m * 81 + i * 9 + j];
        epvr->setInformation(InvCovPVR);
        epvr->SetParams(gw);
        g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; epvr->setRobustKernel(rk); rk->setDelta(hub[2]);
        optimizer.addEdge(epvr); vpEdgesNavStatePVR.push_back(epvr);
        g2o::EdgeNavStateBias* ebias = new g2o::EdgeNavStateBias();
        ebias->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[m] + 1)));
        ebias->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[m + 1] + 1)));
        ebias->setMeasurement(imupre);
        Eigen::Matrix<double, 6, 6> InvCovB; for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) InvCovB(i, j) = ibias[(size_t)m * 36 + i * 6 + j];
        ebias->setInformation(InvCovB);
        g2o::RobustKernelHuber* rkb = new g2o::RobustKernelHuber; ebias->setRobustKernel(rkb); rkb->setDelta(hub[3]);
        optimizer.addEdge(ebias); vpEdgesNavStateBias.push_back(ebias);
    }
    std::vector<g2o::EdgeNavStatePVRPointXYZ*> vpEdgesMono;
    std::vector<int> vpFirstObsKf;                                   // kf_obs_list[0] of the edge's map point
    int e = 0;
    maxPointId = maxKFid;
    std::vector<int> pt_e0(Np + 1, Ep), ln_e0(Nl + 1, El);      // first observation of every landmark (the lists are landmark-major)
    for (int q = Ep - 1; q >= 0; --q) pt_e0[po_pt[q]] = q;
    for (int q = El - 1; q >= 0; --q) ln_e0[lo_ln[q]] = q;
    if (g_scrambled) {      // every landmark vertex first, highest id first
        for (int l = Nl - 1; l >= 0; --l) {
            g2o::VertexLine* vLine = new g2o::VertexLine();
            Vector6d l6; for (int c = 0; c < 6; ++c) l6(c) = lns[6 * l + c];
            vLine->setEstimate(l6); vLine->setId(l + (Np + maxKFid + 1) + 1); vLine->setMarginalized(true);
            optimizer.addVertex(vLine);
        }
        for (int l = Np - 1; l >= 0; --l) {
            g2o::VertexLMPointXYZ* vPoint = new g2o::VertexLMPointXYZ();
            vPoint->setEstimate(Vector3d(pts[3 * l], pts[3 * l + 1], pts[3 * l + 2]));
            vPoint->setId(l + maxKFid + 1); vPoint->setFixed(false); vPoint->setMarginalized(true);
            optimizer.addVertex(vPoint);
        }
    }
    for (int lq = 0; lq < Np; ++lq) {                                  // :5897-5948
        const int l = g_scrambled ? Np - 1 - lq : lq;
        const int id = l + maxKFid + 1;
        if (!g_scrambled) {
            g2o::VertexLMPointXYZ* vPoint = new g2o::VertexLMPointXYZ();
            vPoint->setEstimate(g_late_estimates ? Vector3d(0, 0, 1) : Vector3d(pts[3 * l], pts[3 * l + 1], pts[3 * l + 2]));
            vPoint->setId(id); vPoint->setFixed(false); vPoint->setMarginalized(true);
            optimizer.addVertex(vPoint);
        }
        e = pt_e0[l];
        const int e0 = e;
        for (; e < Ep && po_pt[e] == l; ++e) {
            g2o::EdgeNavStatePVRPointXYZ* ed = new g2o::EdgeNavStatePVRPointXYZ();
            ed->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id)));
            ed->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[po_kf[e]])));
            ed->setMeasurement(Vector2d(po_uv[2 * e], po_uv[2 * e + 1]));
            const float invSigma2 = 1.0 / po_sig[e];
            ed->setInformation(Eigen::Matrix2d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[0]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed); vpEdgesMono.push_back(ed); vpFirstObsKf.push_back(kf_idx[po_kf[e0]]);
            if (g_scrambled && (e % 7) == 0) ed->setMeasurement(Vector2d(po_uv[2 * e], po_uv[2 * e + 1]));      // edited after insertion (same value)
        }
    }
    maxPointId = Np + maxKFid + 1;
    std::vector<g2o::EdgeNavStateLine*> vlEdgesMono;
    std::vector<int> vlFirstObsKf;
    e = 0;
    for (int lq = 0; lq < Nl; ++lq) {                                  // :5957-6004
        const int l = g_scrambled ? Nl - 1 - lq : lq;
        const int id = l + maxPointId + 1;
        if (!g_scrambled) {
            g2o::VertexLine* vLine = new g2o::VertexLine();
            Vector6d l6; for (int c = 0; c < 6; ++c) l6(c) = lns[6 * l + c];
            vLine->setEstimate(l6);
            vLine->setId(id); vLine->setMarginalized(true);
            optimizer.addVertex(vLine);
        }
        e = ln_e0[l];
        const int e0 = e;
        for (; e < El && lo_ln[e] == l; ++e) {
            g2o::EdgeNavStateLine* ed = new g2o::EdgeNavStateLine();
            ed->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id)));
            ed->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[lo_kf[e]])));
            ed->setMeasurement(Vector3d(lo_l[3 * e], lo_l[3 * e + 1], lo_l[3 * e + 2]));
            const float invSigma2 = 1.0 / lo_sig[e];
            ed->setInformation(Eigen::Matrix3d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[1]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed); vlEdgesMono.push_back(ed); vlFirstObsKf.push_back(kf_idx[lo_kf[e0]]);
        }
    }
    if (g_late_estimates) {      // g2o reads a vertex's estimate at optimize(): what is set after addVertex counts (the facade writes it through)
        for (int l = 0; l < Np; ++l) {
            g2o::VertexLMPointXYZ* v = dynamic_cast<g2o::VertexLMPointXYZ*>(optimizer.vertex(l + maxKFid + 1));
            v->setFixed(true);
            v->setEstimate(Vector3d(pts[3 * l], pts[3 * l + 1], pts[3 * l + 2]));
            v->setFixed(false);
        }
    }
    if (laps) { laps[0] = ms_since(t_lap); t_lap = tnow(); }
    optimizer.initializeOptimization();                              // :6038-6039
    optimizer.optimize(5);
    if (laps) { laps[1] = ms_since(t_lap); t_lap = tnow(); laps[7] = optimizer.lastStats().ms_total; }
    if (!abortFlag) {                                                // :6047-6069
        for (size_t i = 0; i < vpEdgesMono.size(); i++) {
            g2o::EdgeNavStatePVRPointXYZ* ed = vpEdgesMono[i];
            if (ed->chi2() > 5.991 || !ed->isDepthPositive()) { ed->setLevel(1); ++gated_pt; }
            ed->setRobustKernel(0);
        }
        for (size_t i = 0; i < vlEdgesMono.size(); i++) {
            g2o::EdgeNavStateLine* ed = vlEdgesMono[i];
            if (ed->chi2() > 5.991 || !ed->isDepthPositive()) { ed->setLevel(1); ++gated_ln; }
            ed->setRobustKernel(0);
        }
        if (laps) { laps[2] = ms_since(t_lap); t_lap = tnow(); }
        optimizer.initializeOptimization(0);
        optimizer.optimize(10);
    }
    chi2_final = optimizer.lastStats().chi2_final;
    if (laps) { laps[3] = ms_since(t_lap); t_lap = tnow(); }
    // ---- marginalization of the oldest keyframe (:6075-6199) -------------------------------------------------------
    const int NUM = 50;
    const int first_kf_idx = kf_idx[0];
    if (do_marg && K >= max_kf_in_window) {
        {
            std::vector<int> drop_set{0}; std::vector<double*> addr; std::vector<VectorXd> est;
            vpEdgesNavStatePVR[0]->GetJacAddr(addr); vpEdgesNavStatePVR[0]->GetEstData(est);
            new_marg_info->addResidualBlockInfo(new ResidualBlockInfo(dynamic_cast<g2o::OptimizableGraph::Edge*>(vpEdgesNavStatePVR[0]), drop_set, est, addr, "PVR"));
        }
        {
            std::vector<int> drop_set{0}; std::vector<double*> addr; std::vector<VectorXd> est;
            vpEdgesNavStateBias[0]->GetJacAddr(addr); vpEdgesNavStateBias[0]->GetEstData(est);
            new_marg_info->addResidualBlockInfo(new ResidualBlockInfo(dynamic_cast<g2o::OptimizableGraph::Edge*>(vpEdgesNavStateBias[0]), drop_set, est, addr, "BIAS"));
        }
        int num = 0;
        for (size_t i = 0; i < vpEdgesMono.size(); i++) {
            if (vpFirstObsKf[i] != first_kf_idx) continue;
            g2o::OptimizableGraph::Edge* edgePoint = dynamic_cast<g2o::OptimizableGraph::Edge*>(vpEdgesMono[i]);
            std::vector<int> drop_set{0}; std::vector<double*> addr; std::vector<VectorXd> est;
            if (edgePoint->vertex(1)->id() == 2 * first_kf_idx) drop_set.push_back(1);
            vpEdgesMono[i]->GetJacAddr(addr); vpEdgesMono[i]->GetEstData(est);
            new_marg_info->addResidualBlockInfo(new ResidualBlockInfo(edgePoint, drop_set, est, addr, "POINT"));
            if (++num > NUM) break;
        }
        num = 0;
        for (size_t i = 0; i < vlEdgesMono.size(); i++) {
            if (vlFirstObsKf[i] != first_kf_idx) continue;
            g2o::OptimizableGraph::Edge* edgeLine = dynamic_cast<g2o::OptimizableGraph::Edge*>(vlEdgesMono[i]);
            std::vector<int> drop_set{0}; std::vector<double*> addr; std::vector<VectorXd> est;
            if (edgeLine->vertex(1)->id() == 2 * first_kf_idx) drop_set.push_back(1);
            vlEdgesMono[i]->GetJacAddr(addr); vlEdgesMono[i]->GetEstData(est);
            new_marg_info->addResidualBlockInfo(new ResidualBlockInfo(edgeLine, drop_set, est, addr, "LINE"));
            if (++num > NUM) break;
        }
        new_marg_info->preMarginalize();
        new_marg_info->marginalizeWithoutThread();
    }
    if (laps) { laps[4] = ms_since(t_lap); t_lap = tnow(); }
    // ---- write-back (:6202-6239) -----------------------------------------------------------------------------------------
    for (int k = 0; k < K; ++k) {
        g2o::VertexNavStatePVR* vNSPVR = static_cast<g2o::VertexNavStatePVR*>(optimizer.vertex(2 * kf_idx[k]));
        g2o::VertexNavStateBias* vNSBias = static_cast<g2o::VertexNavStateBias*>(optimizer.vertex(2 * kf_idx[k] + 1));
        const NavState& a = vNSPVR->estimate(); const NavState& b = vNSBias->estimate();
        Vector3d p = a.Get_P(), v = a.Get_V(), g = b.Get_dBias_Gyr(), c = b.Get_dBias_Acc();
        Quaterniond qq = a.Get_R().unit_quaternion();
        for (int i = 0; i < 3; ++i) { oP[3 * k + i] = p(i); oV[3 * k + i] = v(i); odbg[3 * k + i] = g(i); odba[3 * k + i] = c(i); }
        oq[4 * k] = qq.x(); oq[4 * k + 1] = qq.y(); oq[4 * k + 2] = qq.z(); oq[4 * k + 3] = qq.w();
    }
    for (int l = 0; l < Np; ++l) { const Vector3d& p = static_cast<g2o::VertexLMPointXYZ*>(optimizer.vertex(l + maxKFid + 1))->estimate(); for (int i = 0; i < 3; ++i) opts[3 * l + i] = p(i); }
    for (int l = 0; l < Nl; ++l) { const Vector6d& p = static_cast<g2o::VertexLine*>(optimizer.vertex(l + maxPointId + 1))->estimate(); for (int i = 0; i < 6; ++i) olns[6 * l + i] = p(i); }
    if (laps) { laps[5] = ms_since(t_lap); t_lap = tnow(); }
    }
    if (laps) laps[6] = ms_since(t_lap);
    if (!out) { delete new_marg_info; return 0; }
    FILE* o = fopen(out, "wb");
    if (!o) { perror("result"); return 2; }
    std::vector<int32_t> oh{gated_pt, gated_ln, new_marg_info->n, new_marg_info->m, (int32_t)new_marg_info->keep_vertex_id.size()};
    wr(o, oh); wr(o, std::vector<double>{chi2_final});
    wr(o, oP); wr(o, oV); wr(o, oq); wr(o, odbg); wr(o, odba); wr(o, opts); wr(o, olns);
    std::vector<int32_t> kv(new_marg_info->keep_vertex_id.begin(), new_marg_info->keep_vertex_id.end()), ks(new_marg_info->keep_vertex_size.begin(), new_marg_info->keep_vertex_size.end()), ki(new_marg_info->keep_vertex_idx.begin(), new_marg_info->keep_vertex_idx.end());
    wr(o, kv); wr(o, ks); wr(o, ki);
    const int n = new_marg_info->n;
    std::vector<double> J0((size_t)n * n), r0(n);
    for (int c = 0; c < n; ++c) for (int r = 0; r < n; ++r) J0[(size_t)c * n + r] = new_marg_info->linearized_jacobians(r, c);
    for (int r = 0; r < n; ++r) r0[r] = new_marg_info->linearized_residuals(r);
    wr(o, J0); wr(o, r0);
    fclose(o);
    printf("localba_harness: gated %d+%d, chi2 %.6f, prior n=%d\n", gated_pt, gated_ln, chi2_final, n);
    return 0;
}


// ---- MapHandler::localBundleAdjustmentWithImu (USE_MARG off, src/mapHandler.cpp:5086-5739) --------------------------------------------
// Window file as above plus per-keyframe roles: 0 = sliding-window keyframe, 1 = fixed covisible keyframe outside the window (PVR
// vertex only, :5220-5231), 2 = RefKeyframe, the window's predecessor (fixed PVR + bias vertices, :5233-5240, source of the first
// IMU edge).  IMU edge m joins keyframes imu_i[m] -> imu_j[m].  After the two-stage solve the culling decision of :5541-5620.
static int local_ba_with_imu(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("window"); return 2; }
    auto hdr = rd<int32_t>(f, 8);
    const int K = hdr[0], Np = hdr[1], Nl = hdr[2], Ep = hdr[3], El = hdr[4], M = hdr[5];
    auto cam = rd<double>(f, 4); auto Rbcv = rd<double>(f, 9); auto Pbcv = rd<double>(f, 3); auto gwv = rd<double>(f, 3); auto hub = rd<double>(f, 4);
    auto kf_idx = rd<int32_t>(f, K);
    auto P = rd<double>(f, 3 * K), V = rd<double>(f, 3 * K), q = rd<double>(f, 4 * K), bg = rd<double>(f, 3 * K), ba = rd<double>(f, 3 * K);
    auto pts = rd<double>(f, 3 * (size_t)Np), lns = rd<double>(f, 6 * (size_t)Nl);
    auto po_pt = rd<int32_t>(f, Ep), po_kf = rd<int32_t>(f, Ep); auto po_uv = rd<double>(f, 2 * (size_t)Ep), po_sig = rd<double>(f, Ep);
    auto lo_ln = rd<int32_t>(f, El), lo_kf = rd<int32_t>(f, El); auto lo_l = rd<double>(f, 3 * (size_t)El), lo_sig = rd<double>(f, El);
    auto pre = rd<double>(f, 142 * (size_t)M), ipvr = rd<double>(f, 81 * (size_t)M), ibias = rd<double>(f, 36 * (size_t)M);
    auto role = rd<int32_t>(f, K); auto imu_i = rd<int32_t>(f, M), imu_j = rd<int32_t>(f, M);
    fclose(f);
    Matrix3d Rbc; Vector3d tbc, gw(gwv[0], gwv[1], gwv[2]);
    for (int i = 0; i < 3; ++i) { tbc(i) = Pbcv[i]; for (int j = 0; j < 3; ++j) Rbc(i, j) = Rbcv[i * 3 + j]; }
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    bool abortFlag = false;
    bool* mbaAbort = &abortFlag;
    auto nav = [&](int k) {
        NavState ns;
        ns.Set_Pos(Vector3d(P[3 * k], P[3 * k + 1], P[3 * k + 2])); ns.Set_Vel(Vector3d(V[3 * k], V[3 * k + 1], V[3 * k + 2]));
        ns.Set_Rot(Sophus::SO3(Quaterniond(q[4 * k + 3], q[4 * k], q[4 * k + 1], q[4 * k + 2])));
        ns.Set_BiasGyr(Vector3d(bg[3 * k], bg[3 * k + 1], bg[3 * k + 2])); ns.Set_BiasAcc(Vector3d(ba[3 * k], ba[3 * k + 1], ba[3 * k + 2]));
        return ns;
    };
    int first_window = -1, ref_kf = -1;
    for (int k = 0; k < K; ++k) { if (role[k] == 0 && first_window < 0) first_window = k; if (role[k] == 2) ref_kf = k; }
    const bool firstFix = ref_kf < 0;                                // :5157-5166

    g2o::SparseOptimizer optimizer;
    auto linearSolver = g2o::make_unique<SlamLinearSolver>();
    auto blockSolver = g2o::make_unique<g2o::BlockSolverX>(std::move(linearSolver));
    g2o::OptimizationAlgorithm* algorithm = new g2o::OptimizationAlgorithmLevenberg(std::move(blockSolver));
    optimizer.setAlgorithm(algorithm);
    if (mbaAbort) optimizer.setForceStopFlag(mbaAbort);
    int maxKFid = 0;
    for (int k = 0; k < K; ++k) {                                    // sliding-window keyframe vertices (:5190-5218)
        if (role[k] != 0) continue;
        const int idKF = kf_idx[k] * 2;
        g2o::VertexNavStatePVR* vNSPVR = new g2o::VertexNavStatePVR();
        vNSPVR->setEstimate(nav(k)); vNSPVR->setId(idKF); vNSPVR->setFixed(false);
        if (k == first_window && firstFix) vNSPVR->setFixed(true);
        optimizer.addVertex(vNSPVR);
        g2o::VertexNavStateBias* vNSBias = new g2o::VertexNavStateBias();
        vNSBias->setEstimate(nav(k)); vNSBias->setId(idKF + 1); vNSBias->setFixed(false);
        if (k == first_window && firstFix) vNSBias->setFixed(true);
        optimizer.addVertex(vNSBias);
        if (idKF + 1 > maxKFid) maxKFid = idKF + 1;
    }
    for (int k = 0; k < K; ++k) {                                    // fixed keyframes (:5220-5243)
        if (role[k] == 0) continue;
        const int idKF = kf_idx[k] * 2;
        g2o::VertexNavStatePVR* vNSPVR = new g2o::VertexNavStatePVR();
        vNSPVR->setEstimate(nav(k)); vNSPVR->setId(idKF); vNSPVR->setFixed(true);
        optimizer.addVertex(vNSPVR);
        if (role[k] == 2) {
            g2o::VertexNavStateBias* vNSBias = new g2o::VertexNavStateBias();
            vNSBias->setEstimate(nav(k)); vNSBias->setId(idKF + 1); vNSBias->setFixed(true);
            optimizer.addVertex(vNSBias);
        }
        if (idKF + 1 > maxKFid) maxKFid = idKF + 1;
    }
    for (int m = 0; m < M; ++m) {                                    // :5253-5293
        IMUPreintegrator imupre; imupre.setPayload(&pre[(size_t)m * 142]);
        const int k0 = imu_i[m], k1 = imu_j[m];
        g2o::EdgeNavStatePVR* epvr = new g2o::EdgeNavStatePVR();
        epvr->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[k0])));
        epvr->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[k1])));
        epvr->setVertex(2, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[k0] + 1)));
        epvr->setMeasurement(imupre);
        Matrix9d InvCovPVR; for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) InvCovPVR(i, j) = ipvr[(size_t)m * 81 + i * 9 + j];
        epvr->setInformation(InvCovPVR);
        epvr->SetParams(gw);
        g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; epvr->setRobustKernel(rk); rk->setDelta(hub[2]);
        optimizer.addEdge(epvr);
        g2o::EdgeNavStateBias* ebias = new g2o::EdgeNavStateBias();
        ebias->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[k0] + 1)));
        ebias->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[k1] + 1)));
        ebias->setMeasurement(imupre);
        Matrix6d InvCovB; for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) InvCovB(i, j) = ibias[(size_t)m * 36 + i * 6 + j];
        ebias->setInformation(InvCovB);
        g2o::RobustKernelHuber* rkb = new g2o::RobustKernelHuber; ebias->setRobustKernel(rkb); rkb->setDelta(hub[3]);
        optimizer.addEdge(ebias);
    }
    std::vector<g2o::EdgeNavStatePVRPointXYZ*> vpEdgesMono;
    int maxPointId = maxKFid, e = 0;
    for (int l = 0; l < Np; ++l) {                                  // :5309-5358
        g2o::VertexLMPointXYZ* vPoint = new g2o::VertexLMPointXYZ();
        vPoint->setEstimate(Vector3d(pts[3 * l], pts[3 * l + 1], pts[3 * l + 2]));
        const int id = l + maxKFid + 1;
        vPoint->setId(id); vPoint->setFixed(false); vPoint->setMarginalized(true);
        optimizer.addVertex(vPoint);
        for (; e < Ep && po_pt[e] == l; ++e) {
            g2o::EdgeNavStatePVRPointXYZ* ed = new g2o::EdgeNavStatePVRPointXYZ();
            ed->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id)));
            ed->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[po_kf[e]])));
            ed->setMeasurement(Vector2d(po_uv[2 * e], po_uv[2 * e + 1]));
            const float invSigma2 = 1.0 / po_sig[e];
            ed->setInformation(Eigen::Matrix2d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[0]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed); vpEdgesMono.push_back(ed);
        }
        maxPointId = id + 1;
    }
    std::vector<g2o::EdgeNavStateLine*> vlEdgesMono;
    e = 0;
    for (int l = 0; l < Nl; ++l) {                                  // :5366-5412
        g2o::VertexLine* vLine = new g2o::VertexLine();
        Vector6d l6; for (int c = 0; c < 6; ++c) l6(c) = lns[6 * l + c];
        vLine->setEstimate(l6);
        const int id = l + maxPointId + 1;
        vLine->setId(id); vLine->setMarginalized(true);
        optimizer.addVertex(vLine);
        for (; e < El && lo_ln[e] == l; ++e) {
            g2o::EdgeNavStateLine* ed = new g2o::EdgeNavStateLine();
            ed->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id)));
            ed->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(2 * kf_idx[lo_kf[e]])));
            ed->setMeasurement(Vector3d(lo_l[3 * e], lo_l[3 * e + 1], lo_l[3 * e + 2]));
            const float invSigma2 = 1.0 / lo_sig[e];
            ed->setInformation(Eigen::Matrix3d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[1]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed); vlEdgesMono.push_back(ed);
        }
    }
    if (mbaAbort) if (*mbaAbort) return 1;                          // :5487-5489
    optimizer.initializeOptimization();
    optimizer.optimize(5);
    bool bDoMore = true;
    if (mbaAbort) if (*mbaAbort) bDoMore = false;
    int gated_pt = 0, gated_ln = 0;
    if (bDoMore) {
        for (size_t i = 0, iend = vpEdgesMono.size(); i < iend; i++) {
            g2o::EdgeNavStatePVRPointXYZ* ed = vpEdgesMono[i];
            if (ed->chi2() > 5.991 || !ed->isDepthPositive()) { ed->setLevel(1); ++gated_pt; }
            ed->setRobustKernel(0);
        }
        for (size_t i = 0; i < vlEdgesMono.size(); i++) {
            g2o::EdgeNavStateLine* ed = vlEdgesMono[i];
            if (ed->chi2() > 5.991 || !ed->isDepthPositive()) { ed->setLevel(1); ++gated_ln; }
            ed->setRobustKernel(0);
        }
        optimizer.initializeOptimization(0);
        optimizer.optimize(10);
    }
    const double chi2_final = optimizer.lastStats().chi2_final;
    // culling decision (:5541-5556 points, :5611-5620 lines); erasing the observation from the map is map surgery (out of scope)
    std::vector<uint8_t> bad_pt(vpEdgesMono.size(), 0), bad_ln(vlEdgesMono.size(), 0);
    for (int i = (int)vpEdgesMono.size() - 1; i >= 0; i--) {
        g2o::EdgeNavStatePVRPointXYZ* ed = vpEdgesMono[i];
        if (ed->level() == 1) ed->computeError();
        if (ed->chi2() > 5.991 || !ed->isDepthPositive()) bad_pt[i] = 1;
    }
    for (int i = (int)vlEdgesMono.size() - 1; i >= 0; i--) {
        g2o::EdgeNavStateLine* ed = vlEdgesMono[i];
        if (ed->level() == 1) ed->computeError();
        if (ed->chi2() > 5.991 || !ed->isDepthPositive()) bad_ln[i] = 1;
    }
    std::vector<double> oP(3 * K), oV(3 * K), oq(4 * K), odbg(3 * K, 0.0), odba(3 * K, 0.0), opts(3 * (size_t)Np), olns(6 * (size_t)Nl);
    for (int k = 0; k < K; ++k) {
        g2o::VertexNavStatePVR* vNSPVR = static_cast<g2o::VertexNavStatePVR*>(optimizer.vertex(2 * kf_idx[k]));
        const NavState& a = vNSPVR->estimate();
        Vector3d p = a.Get_P(), v = a.Get_V();
        Quaterniond qq = a.Get_R().unit_quaternion();
        for (int i = 0; i < 3; ++i) { oP[3 * k + i] = p(i); oV[3 * k + i] = v(i); }
        oq[4 * k] = qq.x(); oq[4 * k + 1] = qq.y(); oq[4 * k + 2] = qq.z(); oq[4 * k + 3] = qq.w();
        if (role[k] != 1) {
            g2o::VertexNavStateBias* vNSBias = static_cast<g2o::VertexNavStateBias*>(optimizer.vertex(2 * kf_idx[k] + 1));
            Vector3d g = vNSBias->estimate().Get_dBias_Gyr(), c = vNSBias->estimate().Get_dBias_Acc();
            for (int i = 0; i < 3; ++i) { odbg[3 * k + i] = g(i); odba[3 * k + i] = c(i); }
        }
    }
    for (int l = 0; l < Np; ++l) { const Vector3d& p = static_cast<g2o::VertexLMPointXYZ*>(optimizer.vertex(l + maxKFid + 1))->estimate(); for (int i = 0; i < 3; ++i) opts[3 * l + i] = p(i); }
    for (int l = 0; l < Nl; ++l) { const Vector6d& p = static_cast<g2o::VertexLine*>(optimizer.vertex(l + maxPointId + 1))->estimate(); for (int i = 0; i < 6; ++i) olns[6 * l + i] = p(i); }
    FILE* o = fopen(out, "wb");
    if (!o) { perror("result"); return 2; }
    std::vector<int32_t> oh{gated_pt, gated_ln, 0, 0, 0};
    wr(o, oh); wr(o, std::vector<double>{chi2_final});
    wr(o, oP); wr(o, oV); wr(o, oq); wr(o, odbg); wr(o, odba); wr(o, opts); wr(o, olns);
    wr(o, bad_pt); wr(o, bad_ln);
    fclose(o);
    printf("local_ba_with_imu: gated %d+%d, chi2 %.6f\n", gated_pt, gated_ln, chi2_final);
    return 0;
}

// g2o::StructureOnlySolver (include/g2o/solvers/structure_only/structure_only_solver.h, pulled in by include/mapHandler.h:43) on a small
// graph: the window's keyframes as VertexNavStatePVR (held), its points and lines with their observation edges; calc() on every second
// point (PointDoF 3) and every second line (6).  Input: the window file of tools/harness_io.py (its IMU part is not used).  Output:
// [P 3K | q 4K as the vertices hold them | points 3Np | lines 6Nl] after calc.  bad_vertex: calc on a keyframe vertex instead — the
// facade must throw (exit code 3); 0 would mean it ignored the vertex.
static int structure_only(const char* in, const char* out, bool bad_vertex) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("window"); return 2; }
    auto hdr = rd<int32_t>(f, 8);
    const int K = hdr[0], Np = hdr[1], Nl = hdr[2], Ep = hdr[3], El = hdr[4];
    auto cam = rd<double>(f, 4); auto Rbcv = rd<double>(f, 9); auto Pbcv = rd<double>(f, 3); auto gwv = rd<double>(f, 3); auto hub = rd<double>(f, 4);
    auto kf_idx = rd<int32_t>(f, K);
    auto P = rd<double>(f, 3 * K), V = rd<double>(f, 3 * K), q = rd<double>(f, 4 * K), bg = rd<double>(f, 3 * K), ba = rd<double>(f, 3 * K);
    auto pts = rd<double>(f, 3 * (size_t)Np), lns = rd<double>(f, 6 * (size_t)Nl);
    auto po_pt = rd<int32_t>(f, Ep), po_kf = rd<int32_t>(f, Ep); auto po_uv = rd<double>(f, 2 * (size_t)Ep), po_sig = rd<double>(f, Ep);
    auto lo_ln = rd<int32_t>(f, El), lo_kf = rd<int32_t>(f, El); auto lo_l = rd<double>(f, 3 * (size_t)El), lo_sig = rd<double>(f, El);
    fclose(f);
    (void)gwv; (void)bg; (void)ba;
    Matrix3d Rbc; Vector3d tbc;
    for (int i = 0; i < 3; ++i) { tbc(i) = Pbcv[i]; for (int j = 0; j < 3; ++j) Rbc(i, j) = Rbcv[i * 3 + j]; }
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    g2o::SparseOptimizer optimizer;
    auto linearSolver = g2o::make_unique<SlamLinearSolver>();
    auto blockSolver = g2o::make_unique<g2o::BlockSolverX>(std::move(linearSolver));
    optimizer.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(std::move(blockSolver)));
    int maxKFid = 0;
    for (int k = 0; k < K; ++k) {
        NavState ns;
        ns.Set_Pos(Vector3d(P[3 * k], P[3 * k + 1], P[3 * k + 2])); ns.Set_Vel(Vector3d(V[3 * k], V[3 * k + 1], V[3 * k + 2]));
        ns.Set_Rot(Sophus::SO3(Quaterniond(q[4 * k + 3], q[4 * k], q[4 * k + 1], q[4 * k + 2])));
        g2o::VertexNavStatePVR* v = new g2o::VertexNavStatePVR();
        v->setEstimate(ns); v->setId(kf_idx[k] * 2); v->setFixed(k == 0);
        optimizer.addVertex(v);
        maxKFid = std::max(maxKFid, kf_idx[k] * 2 + 1);
    }
    std::vector<g2o::OptimizableGraph::Vertex*> sel_pt, sel_ln, sel_bad;
    int e = 0;
    for (int l = 0; l < Np; ++l) {
        g2o::VertexLMPointXYZ* vPoint = new g2o::VertexLMPointXYZ();
        vPoint->setEstimate(Vector3d(pts[3 * l], pts[3 * l + 1], pts[3 * l + 2]));
        const int id = l + maxKFid + 1;
        vPoint->setId(id); vPoint->setMarginalized(true);
        optimizer.addVertex(vPoint);
        if (l % 2 == 0) sel_pt.push_back(vPoint);
        for (; e < Ep && po_pt[e] == l; ++e) {
            g2o::EdgeNavStatePVRPointXYZ* ed = new g2o::EdgeNavStatePVRPointXYZ();
            ed->setVertex(0, optimizer.vertex(id)); ed->setVertex(1, optimizer.vertex(2 * kf_idx[po_kf[e]]));
            ed->setMeasurement(Vector2d(po_uv[2 * e], po_uv[2 * e + 1]));
            const float invSigma2 = 1.0 / po_sig[e];
            ed->setInformation(Eigen::Matrix2d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[0]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed);
        }
    }
    const int maxPointId = Np + maxKFid + 1;
    e = 0;
    for (int l = 0; l < Nl; ++l) {
        g2o::VertexLine* vLine = new g2o::VertexLine();
        Vector6d l6; for (int c = 0; c < 6; ++c) l6(c) = lns[6 * l + c];
        vLine->setEstimate(l6);
        const int id = l + maxPointId + 1;
        vLine->setId(id); vLine->setMarginalized(true);
        optimizer.addVertex(vLine);
        if (l % 2 == 0) sel_ln.push_back(vLine);
        for (; e < El && lo_ln[e] == l; ++e) {
            g2o::EdgeNavStateLine* ed = new g2o::EdgeNavStateLine();
            ed->setVertex(0, optimizer.vertex(id)); ed->setVertex(1, optimizer.vertex(2 * kf_idx[lo_kf[e]]));
            ed->setMeasurement(Vector3d(lo_l[3 * e], lo_l[3 * e + 1], lo_l[3 * e + 2]));
            const float invSigma2 = 1.0 / lo_sig[e];
            ed->setInformation(Eigen::Matrix3d::Identity() * invSigma2);
            g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber; ed->setRobustKernel(rk); rk->setDelta(hub[1]);
            ed->SetParams(fx, fy, cx, cy, Rbc, tbc);
            optimizer.addEdge(ed);
        }
    }
    optimizer.initializeOptimization();
    g2o::StructureOnlySolver<3> structure_only_ba;
    g2o::StructureOnlySolver<6> structure_only_lines;
    if (bad_vertex) {
        sel_bad.push_back(optimizer.vertex(2 * kf_idx[K - 1]));
        try { structure_only_ba.calc(sel_bad, 3); } catch (const std::exception& ex) { fprintf(stderr, "structonly_bad: refused: %s\n", ex.what()); return 3; }
        return 0;
    }
    structure_only_ba.calc(sel_pt, 3);
    structure_only_lines.calc(sel_ln, 3, 10);
    std::vector<double> oP(3 * K), oq(4 * K), opts(3 * (size_t)Np), olns(6 * (size_t)Nl);
    for (int k = 0; k < K; ++k) {
        const NavState& a = static_cast<g2o::VertexNavStatePVR*>(optimizer.vertex(2 * kf_idx[k]))->estimate();
        std::memcpy(&oP[3 * k], a.raw(), 24); std::memcpy(&oq[4 * k], a.raw() + 6, 32);
    }
    for (int l = 0; l < Np; ++l) { const Vector3d& p = static_cast<g2o::VertexLMPointXYZ*>(optimizer.vertex(l + maxKFid + 1))->estimate(); for (int i = 0; i < 3; ++i) opts[3 * l + i] = p(i); }
    for (int l = 0; l < Nl; ++l) { const Vector6d& p = static_cast<g2o::VertexLine*>(optimizer.vertex(l + maxPointId + 1))->estimate(); for (int i = 0; i < 6; ++i) olns[6 * l + i] = p(i); }
    FILE* o = fopen(out, "wb");
    if (!o) { perror("result"); return 2; }
    wr(o, oP); wr(o, oq); wr(o, opts); wr(o, olns);
    fclose(o);
    const plba_refine_stats& st = optimizer.lastRefineStats();
    printf("structure_only: %zu points + %zu lines refined, last call chi2 %.6f -> %.6f\n", sel_pt.size(), sel_ln.size(), st.chi2_before, st.chi2_after);
    return 0;
}

// MapHandler::isLoopClosure's call site (src/mapHandler.cpp:3301-3409) for B candidates at once: from the matched lists (lc_points, lc_lines
// with lc_pt_idx, lc_ls_idx, as the two matching loops fill them) to the arrays of plba_relative_pose, through the call, to the decision, the
// compaction of lc_pt_idx / lc_ls_idx by the masks and pose_inc.  (The reference compacts lc_points twice and lc_lines never, :3662-3665 and
// :4055-4058; here every list keeps its inliers.)  Input and output: the files of csrc/plba_relpose_hostcheck.cpp, so that the two can be
// compared; `returned` is isLoopClosure's return value and the masks say which entries of the index lists stayed.
#include "plba_g2o/relative_pose.h"
static int relpose(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) { perror("batch"); return 2; }
    auto hd = rd<int32_t>(f, 6); auto par = rd<double>(f, 11);
    const int B = hd[0];
    auto ps = rd<int32_t>(f, (size_t)B + 1), ls = rd<int32_t>(f, (size_t)B + 1);
    const size_t Np = (size_t)ps[B], Nl = (size_t)ls[B];
    auto P = rd<double>(f, 3 * Np), uv = rd<double>(f, 2 * Np), pq = rd<double>(f, 6 * Nl), l3 = rd<double>(f, 3 * Nl);
    std::vector<double> T0; if (hd[4]) T0 = rd<double>(f, 16 * (size_t)B);
    std::vector<uint8_t> pm(Np, 1), lm(Nl, 1);
    if (hd[5]) { pm = rd<uint8_t>(f, Np); lm = rd<uint8_t>(f, Nl); }
    fclose(f);
    // the matched lists of every candidate, as isLoopClosure builds them
    std::vector<std::vector<plba_g2o::PointFeature>> lc_points(B);
    std::vector<std::vector<plba_g2o::LineFeature>> lc_lines(B);
    std::vector<std::vector<plba_g2o::Vector4i>> lc_pt_idx(B), lc_ls_idx(B);
    for (int b = 0; b < B; ++b) {
        for (int k = ps[b]; k < ps[b + 1]; ++k) {
            plba_g2o::PointFeature pt; std::memcpy(pt.P, &P[3 * (size_t)k], 24); std::memcpy(pt.pl_obs, &uv[2 * (size_t)k], 16); pt.inlier = pm[k] != 0;
            lc_points[b].push_back(pt); lc_pt_idx[b].push_back({k - ps[b], k - ps[b], k - ps[b], k - ps[b]});
        }
        for (int k = ls[b]; k < ls[b + 1]; ++k) {
            plba_g2o::LineFeature ln; std::memcpy(ln.sP, &pq[6 * (size_t)k], 24); std::memcpy(ln.eP, &pq[6 * (size_t)k + 3], 24); std::memcpy(ln.le_obs, &l3[3 * (size_t)k], 24); ln.inlier = lm[k] != 0;
            lc_lines[b].push_back(ln); lc_ls_idx[b].push_back({k - ls[b], k - ls[b], k - ls[b], k - ls[b]});
        }
    }
    // lists -> arrays
    std::vector<int32_t> pt_start(B + 1, 0), ln_start(B + 1, 0);
    std::vector<double> aP, auv, apq, al3;
    std::vector<uint8_t> apm, alm;
    for (int b = 0; b < B; ++b) {
        for (const auto& pt : lc_points[b]) { aP.insert(aP.end(), pt.P, pt.P + 3); auv.insert(auv.end(), pt.pl_obs, pt.pl_obs + 2); apm.push_back(pt.inlier ? 1 : 0); }
        for (const auto& ln : lc_lines[b]) { apq.insert(apq.end(), ln.sP, ln.sP + 3); apq.insert(apq.end(), ln.eP, ln.eP + 3); al3.insert(al3.end(), ln.le_obs, ln.le_obs + 3); alm.push_back(ln.inlier ? 1 : 0); }
        pt_start[b + 1] = (int32_t)apm.size(); ln_start[b + 1] = (int32_t)alm.size();
    }
    apm.push_back(0); alm.push_back(0);
    plba_problem* p = nullptr;
    if (plba_create(nullptr, &p) != PLBA_OK) { fprintf(stderr, "relpose: %s\n", plba_last_error(nullptr)); return 2; }
    plba_relpose_options ro; plba_relpose_default_options(&ro);
    ro.protocol = hd[1]; ro.max_iters = hd[2]; ro.max_iters_ref = hd[3]; ro.homog_th = par[0]; ro.chi2_th = par[1];
    ro.lc_res = par[2]; ro.lc_unc = par[3]; ro.lc_inl = par[4]; ro.lc_trs = par[5]; ro.lc_rot = par[6];
    std::vector<plba_relpose_result> res(B);
    const int rc = plba_relative_pose(p, &ro, B, pt_start.data(), aP.empty() ? nullptr : aP.data(), auv.empty() ? nullptr : auv.data(), ln_start.data(),
                                      apq.empty() ? nullptr : apq.data(), al3.empty() ? nullptr : al3.data(), par[7], par[8], par[9], par[10],
                                      hd[4] ? T0.data() : nullptr, apm.data(), alm.data(), res.data());
    if (rc != PLBA_OK) { fprintf(stderr, "relpose: %s\n", plba_last_error(p)); plba_destroy(p); return 2; }
    plba_destroy(p);
    // the decision, the compaction and pose_inc, per candidate
    std::vector<double> od((size_t)B * 73, 0.0);
    std::vector<int32_t> oi((size_t)B * 11, 0);
    std::vector<uint8_t> pmo(Np, 0), lmo(Nl, 0);
    int n_loops = 0;
    for (int b = 0; b < B; ++b) {
        const plba_relpose_result& r = res[b];
        double pose_inc[6] = {0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < lc_points[b].size(); ++i) lc_points[b][i].inlier = apm[(size_t)pt_start[b] + i] != 0;
        for (size_t i = 0; i < lc_lines[b].size(); ++i) lc_lines[b][i].inlier = alm[(size_t)ln_start[b] + i] != 0;
        const bool is_loop = r.accepted != 0;
        if (is_loop) {
            std::vector<plba_g2o::Vector4i> pi, li;
            std::vector<plba_g2o::PointFeature> pts; std::vector<plba_g2o::LineFeature> lns;
            for (size_t i = 0; i < lc_points[b].size(); ++i) if (lc_points[b][i].inlier) { pts.push_back(lc_points[b][i]); pi.push_back(lc_pt_idx[b][i]); }
            for (size_t i = 0; i < lc_lines[b].size(); ++i) if (lc_lines[b][i].inlier) { lns.push_back(lc_lines[b][i]); li.push_back(lc_ls_idx[b][i]); }
            lc_points[b].swap(pts); lc_lines[b].swap(lns); lc_pt_idx[b].swap(pi); lc_ls_idx[b].swap(li);
            std::memcpy(pose_inc, r.pose_inc6, 48);
            for (const auto& v : lc_pt_idx[b]) pmo[(size_t)ps[b] + (size_t)v[0]] = 1;
            for (const auto& v : lc_ls_idx[b]) lmo[(size_t)ls[b] + (size_t)v[0]] = 1;
            ++n_loops;
        } else {
            for (size_t i = 0; i < lc_points[b].size(); ++i) pmo[(size_t)ps[b] + i] = lc_points[b][i].inlier ? 1 : 0;
            for (size_t i = 0; i < lc_lines[b].size(); ++i) lmo[(size_t)ls[b] + i] = lc_lines[b][i].inlier ? 1 : 0;
        }
        double* o = &od[(size_t)b * 73];
        std::memcpy(o, r.T_inc16, 128); std::memcpy(o + 16, r.pose_inc6, 48); std::memcpy(o + 22, r.H36, 288); o[58] = r.e; std::memcpy(o + 59, r.cov_eig6, 48);
        o[65] = r.t; o[66] = r.r; std::memcpy(o + 67, pose_inc, 48);
        int32_t* q = &oi[(size_t)b * 11];
        q[0] = r.n_inliers; q[1] = r.iters[0]; q[2] = r.iters[1]; q[3] = r.status; q[4] = r.accepted; q[5] = r.lc_res; q[6] = r.lc_unc; q[7] = r.lc_inl; q[8] = r.lc_trs;
        q[9] = r.lc_rot; q[10] = is_loop ? 1 : 0;
    }
    FILE* o = fopen(out, "wb");
    if (!o) { perror("result"); return 2; }
    wr(o, od); wr(o, oi); wr(o, pmo); wr(o, lmo);
    fclose(o);
    printf("relpose: %d of %d candidates are loop closures\n", n_loops, B);
    return 0;
}

// MapHandler::lookForCommonMatches' pose refinement between two keyframes (src/mapHandler.cpp:819-859) for B keyframe pairs at once: from
// the matched lists (stf->matched_pt, stf->matched_ls with every feature an inlier unless the file says otherwise, :821-829) to the arrays
// of plba_track_pose, through the call (stf->optimizePose(), :831), to the inlier ratios against SlamConfig::kfInlierRatio() (30, :833-846)
// and kf1->T_kf_w (:848-852).  kf0->T_kf_w is the identity here and the tracker's DT of :852 is the start pose of the file.  A kind
// without a match counts as absent (SlamConfig::hasPoints() / hasLines()): the reference would divide by its zero count.  Input: the file
// of csrc/plba_track_hostcheck.cpp.  Output: that program's, then per pair double T_kf_w[16] and int32 [used the refined DT].
#include "plba_g2o/track_pose.h"
static int track(const char* in, const char* out) {
    namespace rp = plba::relpose;
    FILE* f = fopen(in, "rb");
    if (!f) { perror("batch"); return 2; }
    auto hd = rd<int32_t>(f, 6); auto par = rd<double>(f, 8);
    const int B = hd[0];
    auto ps = rd<int32_t>(f, (size_t)B + 1), ls = rd<int32_t>(f, (size_t)B + 1);
    const size_t Np = (size_t)ps[B], Nl = (size_t)ls[B];
    auto P = rd<double>(f, 3 * Np), uv = rd<double>(f, 2 * Np), s2p = rd<double>(f, Np), pq = rd<double>(f, 6 * Nl), l3 = rd<double>(f, 3 * Nl), se = rd<double>(f, 4 * Nl),
         s2l = rd<double>(f, Nl);
    std::vector<double> T0; if (hd[4]) T0 = rd<double>(f, 16 * (size_t)B);
    std::vector<uint8_t> pm(Np, 1), lm(Nl, 1);
    if (hd[5]) { pm = rd<uint8_t>(f, Np); lm = rd<uint8_t>(f, Nl); }
    fclose(f);
    // the matched lists of every pair
    std::vector<std::vector<plba_g2o::TrackPoint>> matched_pt(B);
    std::vector<std::vector<plba_g2o::TrackLine>> matched_ls(B);
    for (int b = 0; b < B; ++b) {
        for (int k = ps[b]; k < ps[b + 1]; ++k) {
            plba_g2o::TrackPoint pt; std::memcpy(pt.P, &P[3 * (size_t)k], 24); std::memcpy(pt.pl_obs, &uv[2 * (size_t)k], 16); pt.sigma2 = s2p[k]; pt.inlier = pm[k] != 0;
            matched_pt[b].push_back(pt);
        }
        for (int k = ls[b]; k < ls[b + 1]; ++k) {
            plba_g2o::TrackLine ln; std::memcpy(ln.sP, &pq[6 * (size_t)k], 24); std::memcpy(ln.eP, &pq[6 * (size_t)k + 3], 24); std::memcpy(ln.le_obs, &l3[3 * (size_t)k], 24);
            std::memcpy(ln.spl, &se[4 * (size_t)k], 16); std::memcpy(ln.epl, &se[4 * (size_t)k + 2], 16); ln.sigma2 = s2l[k]; ln.inlier = lm[k] != 0;
            matched_ls[b].push_back(ln);
        }
    }
    // lists -> arrays
    std::vector<int32_t> pt_start(B + 1, 0), ln_start(B + 1, 0);
    std::vector<double> aP, auv, as2p, apq, al3, ase, as2l;
    std::vector<uint8_t> apm, alm;
    for (int b = 0; b < B; ++b) {
        for (const auto& pt : matched_pt[b]) { aP.insert(aP.end(), pt.P, pt.P + 3); auv.insert(auv.end(), pt.pl_obs, pt.pl_obs + 2); as2p.push_back(pt.sigma2); apm.push_back(pt.inlier ? 1 : 0); }
        for (const auto& ln : matched_ls[b]) {
            apq.insert(apq.end(), ln.sP, ln.sP + 3); apq.insert(apq.end(), ln.eP, ln.eP + 3); al3.insert(al3.end(), ln.le_obs, ln.le_obs + 3);
            ase.insert(ase.end(), ln.spl, ln.spl + 2); ase.insert(ase.end(), ln.epl, ln.epl + 2); as2l.push_back(ln.sigma2); alm.push_back(ln.inlier ? 1 : 0);
        }
        pt_start[b + 1] = (int32_t)apm.size(); ln_start[b + 1] = (int32_t)alm.size();
    }
    apm.push_back(0); alm.push_back(0);
    plba_problem* p = nullptr;
    if (plba_create(nullptr, &p) != PLBA_OK) { fprintf(stderr, "track: %s\n", plba_last_error(nullptr)); return 2; }
    plba_track_options to; plba_track_default_options(&to);
    to.max_iters = hd[1]; to.max_iters_ref = hd[2]; to.min_features = hd[3]; to.homog_th = par[0]; to.min_error = par[1]; to.min_error_change = par[2]; to.inlier_k = par[3];
    std::vector<plba_track_result> res(B);
    auto ptr = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
    const int rc = plba_track_pose(p, &to, B, pt_start.data(), ptr(aP), ptr(auv), ptr(as2p), ln_start.data(), ptr(apq), ptr(al3), ptr(ase), ptr(as2l),
                                   par[4], par[5], par[6], par[7], hd[4] ? T0.data() : nullptr, apm.data(), alm.data(), res.data());
    if (rc != PLBA_OK) { fprintf(stderr, "track: %s\n", plba_last_error(p)); plba_destroy(p); return 2; }
    plba_destroy(p);
    std::vector<double> od((size_t)B * 115, 0.0), Tkf((size_t)B * 16, 0.0);
    std::vector<int32_t> oi((size_t)B * 8, 0), used(B, 0);
    std::vector<uint8_t> pmo(Np, 0), lmo(Nl, 0);
    const double kf_inlier_ratio = 30.0;      // SlamConfig::kfInlierRatio(), src/slamConfig.cpp:57
    int n_used = 0;
    for (int b = 0; b < B; ++b) {
        const plba_track_result& r = res[b];
        for (size_t i = 0; i < matched_pt[b].size(); ++i) { matched_pt[b][i].inlier = apm[(size_t)pt_start[b] + i] != 0; pmo[(size_t)ps[b] + i] = apm[(size_t)pt_start[b] + i]; }
        for (size_t i = 0; i < matched_ls[b].size(); ++i) { matched_ls[b][i].inlier = alm[(size_t)ln_start[b] + i] != 0; lmo[(size_t)ls[b] + i] = alm[(size_t)ln_start[b] + i]; }
        const bool has_pt = !matched_pt[b].empty(), has_ls = !matched_ls[b].empty();
        bool condition_pt = true, condition_ls = true;
        if (has_pt) condition_pt = 100.0 * r.n_inliers_pt / (double)matched_pt[b].size() >= kf_inlier_ratio;
        if (has_ls) condition_ls = 100.0 * r.n_inliers_ln / (double)matched_ls[b].size() >= kf_inlier_ratio;
        if (!has_pt && !has_ls) condition_pt = condition_ls = false;
        const bool use = r.n_inliers_pt + r.n_inliers_ln > to.min_features && condition_pt && condition_ls;      // :848
        rp::Pose D, A, E;
        double x[6];
        const double* m = use ? r.DT16 : (hd[4] ? &T0[16 * (size_t)b] : nullptr);
        if (m) { for (int i = 0; i < 3; ++i) { D.R[i * 3] = m[i * 4]; D.R[i * 3 + 1] = m[i * 4 + 1]; D.R[i * 3 + 2] = m[i * 4 + 2]; D.t[i] = m[i * 4 + 3]; } }
        else rp::se3_identity(D);
        if (use) A = D; else rp::se3_inv(D, A);      // :850 / :852 with kf0->T_kf_w = I
        rp::se3_log(A, x); rp::se3_exp(x, E);
        double* t = &Tkf[(size_t)b * 16];
        for (int i = 0; i < 3; ++i) { t[i * 4] = E.R[i * 3]; t[i * 4 + 1] = E.R[i * 3 + 1]; t[i * 4 + 2] = E.R[i * 3 + 2]; t[i * 4 + 3] = E.t[i]; }
        t[15] = 1.0;
        used[b] = use ? 1 : 0; n_used += used[b];
        double* o = &od[(size_t)b * 115];
        std::memcpy(o, r.DT16, 128); std::memcpy(o + 16, r.T_opt16, 128); std::memcpy(o + 32, r.H36, 288); std::memcpy(o + 68, r.cov36, 288); std::memcpy(o + 104, r.cov_eig6, 48);
        o[110] = r.err; o[111] = r.pt_mean; o[112] = r.pt_stdv; o[113] = r.ln_mean; o[114] = r.ln_stdv;
        int32_t* q = &oi[(size_t)b * 8];
        q[0] = r.n_inliers_pt; q[1] = r.n_inliers_ln; q[2] = r.iters[0]; q[3] = r.iters[1]; q[4] = r.iters[2]; q[5] = r.path; q[6] = r.status; q[7] = r.good;
    }
    FILE* o = fopen(out, "wb");
    if (!o) { perror("result"); return 2; }
    wr(o, od); wr(o, oi); wr(o, pmo); wr(o, lmo); wr(o, Tkf); wr(o, used);
    fclose(o);
    printf("track: %d of %d keyframe pairs take the refined pose\n", n_used, B);
    return 0;
}
