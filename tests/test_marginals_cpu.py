"""plba_compute_marginals without a GPU: the C ABI surface, and the numpy reference of tests/marginals_ref.py checked against
itself (Schur formula vs. the dense inverse of the full undamped Hessian) and against the oracle's own landmark blocks."""
import ctypes
import os

import numpy as np

from tests import marginals_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_compute_marginals(pkg, hip_lib_path):
    hdr = open(os.path.join(ROOT, "include", "plba.h")).read()
    assert "typedef struct plba_marginals" in hdr
    assert "int plba_compute_marginals(plba_problem* p, plba_marginals* m);" in hdr
    assert hasattr(ctypes.CDLL(hip_lib_path), "plba_compute_marginals")
    assert "compute_marginals" in pkg.abi.SIGNATURES and "compute_marginals" in pkg.abi.PRODUCT_ONLY
    assert [f[0] for f in pkg.abi.Marginals._fields_] == ["want", "n_pairs", "pairs", "kf_cov", "pair_cov", "pt_cov", "pt_status",
                                                          "ln_cov", "ln_status", "n_excluded"]


def small_window(pkg):
    """4 keyframes, ~40 points, 10 lines, IMU, keyframe 0 fixed, a prior on keyframes 1-2."""
    w = pkg.window.make_window(4, 40, 10, imu=True, seed=0x3A11C0, track=(2, 4))
    k = w["kf"]
    k["fixed_pvr"][:] = 0; k["fixed_bias"][:] = 0
    k["fixed_pvr"][0] = 1; k["fixed_bias"][0] = 1
    n = 15
    rng = np.random.default_rng(7)
    J0 = np.eye(n) * 30.0 + rng.normal(size=(n, n)) * 0.5
    x0 = np.concatenate([k["P"][1], k["V"][1], k["q"][1], k["bg"][1] + k["dbg"][1], k["ba"][1] + k["dba"][1]])
    w["prior"] = dict(n=n, vid=np.array([k["vid_pvr"][1], k["vid_bias"][1]], np.int32), size=np.array([9, 6], np.int32),
                      idx=np.array([0, 9], np.int32), x0=x0, J0=J0, r0=np.zeros(n))
    return w


def test_reference_self_consistent(pkg, orc):
    w = small_window(pkg)
    op = orc.new_problem()
    op.upload_window(w)
    robust = {0: w["huber"].get(0), 1: w["huber"].get(1)}
    out, ref, res, Hs = mr.reference(op, w, robust, lams=(1e-3, 10.0), dense_check=True)
    # the pose side does not depend on the damping it was recovered through
    assert np.abs(Hs[0] - Hs[1]).max() <= 1e-10 * np.abs(Hs[0]).max()
    # the Hll the reference builds from the per-edge evaluators is the oracle's (weighting, levels, Huber)
    op.debug_build(1e-3)
    hpt = op.debug_get("hll_pt").reshape(-1, 3, 3)
    hln = op.debug_get("hll_ln").reshape(-1, 6, 6)
    for lm in ref.lm:
        if lm["fixed"] or not lm["edges"]:
            continue
        Hll = ref.landmark_blocks(lm)[0]
        o = hpt[lm["idx"]] if lm["kind"] == 0 else hln[lm["idx"]]
        assert np.abs(Hll - o).max() <= 1e-12 * max(np.abs(o).max(), 1.0)
    # Schur formula == dense inverse of the full undamped Hessian in the reduced landmark coordinates
    d = res["dense"]
    assert np.abs(res["Spp"] - d["Spp"]).max() <= 1e-10 * np.abs(d["Spp"]).max()
    for i, c in d["cov"].items():
        assert np.abs(res["cov"][i] - c).max() <= 1e-10 * np.abs(c).max()
    assert (out["pt_status"] == 0).sum() > 10 and (out["ln_status"] == 0).sum() > 2
    # lines: rank 4, both line directions in the null space
    for lm, c, s in zip(ref.lm[ref.Np:], out["ln"], out["ln_status"]):
        if s:
            continue
        dv = lm["x"][3:] - lm["x"][:3]
        assert np.abs(c[:3, :3] @ dv).max() <= 1e-9 * np.abs(c).max() and np.abs(c[3:, 3:] @ dv).max() <= 1e-9 * np.abs(c).max()
        assert np.linalg.matrix_rank(c, tol=1e-9 * np.abs(c).max()) == 4
    op.close()


def test_recovered_hpp_equals_direct(pkg, orc):
    """the Hpp the reference recovers through the damped Schur complement against the one tests/marginals_exact.py builds directly in
    extended precision from the IMU, bias, prior and observation edges: the recovery's subtraction cancels, the direct sum does not"""
    from tests import marginals_exact as mx
    w = small_window(pkg)
    op = orc.new_problem()
    op.upload_window(w)
    ex = mx.Exact(op, w, {k: w["huber"].get(k) for k in range(4)})
    Hs = [ex.ref.hpp(op, lam) for lam in (1e-3, 10.0)]
    op.close()
    H = mx.narrow(ex.Hpp)
    assert ex.P == 45 and np.abs(H).max() > 0
    for Hr in Hs:
        assert np.abs(Hr - H).max() <= 1e-10 * np.abs(H).max()
    assert np.array_equal(ex.status, ex.ref.solve(Hs[0])["status"])
