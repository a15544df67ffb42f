"""plba_relative_pose on the device against the wide run of tests/relpose_ref.py, under lba_ref.hold's rule: T_inc, pose_inc, H, e and
cov_eig within 8 x the float64 reference's own rounding noise (floor m u |value|, m the inlier features), masks, pass counts, statuses and
decision bits exactly.  tests/test_relpose_cpu.py asserts that every case has the margin an exact comparison needs.  It also asserts that every case's noise sample is
representative (the float64 reference reordered stays within half the tolerance): how the seeds of tests/relpose_cases.py were chosen."""
import ctypes as C

import numpy as np
import pytest

from . import lba_ref as LR
from . import relpose_cases as RC
from . import relpose_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _call(prob, cases, opts, masks=None, T0=None):
    has_T0 = T0 is not None or any(c.get("T0") is not None for c in cases)
    if T0 is None and has_T0:
        T0 = np.stack([np.eye(4) if c.get("T0") is None else c["T0"] for c in cases])
    pm, lm = (None, None) if masks is None else masks
    return prob.relative_pose([c["P3"] for c in cases], [c["uv"] for c in cases], [c["pq"] for c in cases], [c["l3"] for c in cases], RC.CAM,
                              T0=T0, pt_inlier=pm, ln_inlier=lm, **opts)


def _hold(prob, name):
    case, r64, rw = RC.runs(name)
    out = _call(prob, [case], case["opts"])
    RR.hold(RC.as_result(out, 0), r64, rw, "hip", name)
    return case, out, rw


@pytest.mark.parametrize("name", [n for n in sorted(RC.CASES) if n.startswith("size_")])
def test_feature_counts_around_the_wave(prob, name):
    _hold(prob, name)


@pytest.mark.parametrize("protocol", [0, 1])
def test_outliers_cut_and_refinement(prob, protocol):
    case, out, rw = _hold(prob, "outliers_p%d" % protocol)
    assert 0 < rw["n_inliers"] < len(case["P3"]) + len(case["pq"])
    if protocol == 0:
        # the first stage alone, then its pose and its mask fed back with no first stage: the cut finds nothing more to remove and the
        # refinement runs over the same lanes from the same pose, so every number of the full run comes back bit for bit
        a = _call(prob, [case], dict(max_iters_ref=0))
        b = _call(prob, [case], dict(max_iters=0), masks=(a["pt_inlier"], a["ln_inlier"]), T0=a["T_inc"])
        assert np.array_equal(a["pt_inlier"][0], out["pt_inlier"][0]) and np.array_equal(a["ln_inlier"][0], out["ln_inlier"][0])
        assert np.array_equal(b["pt_inlier"][0], out["pt_inlier"][0]) and np.array_equal(b["ln_inlier"][0], out["ln_inlier"][0])
        for k in ("T_inc", "pose_inc", "H", "e", "cov_eig", "n_inliers", "status", "accepted"):
            assert np.array_equal(b[k], out[k]), k
        assert int(b["iters"][0, 0]) == 0 and int(b["iters"][0, 1]) == int(out["iters"][0, 1])


@pytest.fixture(scope="module")
def alone(prob):
    """each default-option case called alone, once"""
    return {n: _call(prob, [RC.runs(n)[0]], {}) for n in RC.DEFAULT_OPTS}


KEYS = ("T_inc", "pose_inc", "H", "e", "cov_eig", "t", "r", "n_inliers", "iters", "status", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot")


@pytest.mark.parametrize("B", [1, 2, 65, 257])
def test_batch_is_the_candidates_alone(prob, alone, B):
    """mixed sizes in one call, an empty and a rank-deficient candidate among them: every candidate bit-identical to itself called alone"""
    names = [RC.DEFAULT_OPTS[(3 * b + b // 12) % len(RC.DEFAULT_OPTS)] for b in range(B)]
    if B >= 2:
        names[0], names[1] = "empty", "collinear3"
    out = _call(prob, [RC.runs(n)[0] for n in names], {})
    assert out["status"][0] == (RR.EMPTY if B >= 2 else out["status"][0])
    if B >= 2:
        assert out["status"][1] == RR.RANK and not out["accepted"][:2].any() and np.isinf(out["cov_eig"][1]).all()
    for b, n in enumerate(names):
        for k in KEYS:
            assert np.array_equal(out[k][b], alone[n][k][0]), (b, n, k)
        assert np.array_equal(out["pt_inlier"][b], alone[n]["pt_inlier"][0]) and np.array_equal(out["ln_inlier"][b], alone[n]["ln_inlier"][0]), (b, n)


@pytest.mark.parametrize("name", ["t0_general", "t0_identity_rotation", "t0_tiny_rotation", "t0_tiny_rotation_eval"])
def test_start_increment(prob, name):
    case, out, rw = _hold(prob, name)
    if name == "t0_tiny_rotation_eval":      # nothing ran: T_inc is T0, and logmap took its small-angle branch
        assert np.array_equal(out["T_inc"][0], case["T0"]) and out["r"][0] == 0.0 and list(out["iters"][0]) == [0, 0]


@pytest.mark.parametrize("name", ["iters_0_first", "iters_0_ref", "iters_0_both", "iters_1_only", "iters_0_p1", "stall"])
def test_iteration_limits_and_exits(prob, name):
    case, out, rw = _hold(prob, name)
    o = dict(RR.DEFAULTS, **case["opts"])
    assert out["iters"][0, 0] <= o["max_iters"] and out["iters"][0, 1] <= o["max_iters_ref"]
    if name in ("iters_0_both", "iters_0_p1"):      # no pass evaluated: H and e are zeros, the cut still ran at T0
        assert not out["H"][0].any() and out["e"][0] == 0.0 and out["status"][0] == RR.RANK and np.array_equal(out["T_inc"][0], case["T0"])


@pytest.mark.parametrize("name,bit", [("fail_res", "lc_res"), ("fail_unc", "lc_unc"), ("fail_trs", "lc_trs"), ("fail_rot", "lc_rot"), ("fail_inl_p1", "lc_inl"),
                                      ("pass_all_p1", None), ("size_40_24_p0", None)])
def test_decisions(prob, name, bit):
    case, out, rw = _hold(prob, name)
    bits = {k: int(out[k][0]) for k in ("lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot")}
    assert bits == {k: int(k != bit) for k in bits}, bits
    assert int(out["accepted"][0]) == int(bit is None)


def test_two_calls_give_the_same_bits(prob):
    cases = [RC.runs(n)[0] for n in ("size_300_100_p0", "outliers_p0", "size_65_0_p0")]
    a, b = _call(prob, cases, {}), _call(prob, cases, {})
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(a["pt_inlier"] + a["ln_inlier"], b["pt_inlier"] + b["ln_inlier"]):
        assert np.array_equal(x, y)


def test_window_state_untouched_and_one_wait(pkg, hip):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    res = []
    for with_call in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_call:
            before = p.debug_get("host_waits")[0]
            out = _call(p, [RC.runs("size_40_24_p0")[0]], {})
            assert p.debug_get("host_waits")[0] == before + 1
            assert out["accepted"][0] == 1
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_refusals_leave_the_outputs_untouched(pkg, prob):
    abi = pkg.abi
    case = RC.runs("size_40_24_p0")[0]
    P, uv, pq, l3 = (np.ascontiguousarray(case[k], np.float64) for k in ("P3", "uv", "pq", "l3"))
    ps, ls = np.array([0, len(P)], np.int32), np.array([0, len(pq)], np.int32)
    dp, ip, up = abi._dp, abi._ip, abi._up

    def attempt(B=1, ps=ps, ls=ls, P=P, uv=uv, pq=pq, l3=l3, T0=None, opt=True, out=True, **o):
        op = abi.RelposeOptions()
        prob.lib.fn["relpose_default_options"](C.byref(op))
        for k, v in o.items():
            setattr(op, k, v)
        res = (abi.RelposeResult * 2)()
        C.memset(res, 0x5A, C.sizeof(res))
        pm, lm = np.full(len(case["P3"]), 7, np.uint8), np.full(len(case["pq"]), 7, np.uint8)
        rc = prob.lib.fn["relative_pose"](prob._h, C.byref(op) if opt else None, B, ip(ps), dp(P), dp(uv), ip(ls), dp(pq), dp(l3), *[float(v) for v in RC.CAM],
                                          dp(T0), up(pm), up(lm), res if out else None)
        assert rc == -1, rc      # PLBA_ERR_INVALID
        assert bytes(res) == b"\x5a" * C.sizeof(res) and (pm == 7).all() and (lm == 7).all()
    bad = P.copy(); bad[3, 1] = np.nan
    badT = np.eye(4).reshape(1, 16).copy(); badT[0, 3] = np.inf
    attempt(B=0)
    attempt(ps=np.array([0, -1], np.int32))
    attempt(ps=np.array([1, len(P)], np.int32))
    attempt(B=2, ps=np.array([0, len(P), len(P) - 1], np.int32), ls=np.array([0, len(pq), len(pq)], np.int32))
    attempt(P=None)
    attempt(l3=None)
    attempt(out=False)
    attempt(opt=False)
    attempt(P=bad)
    attempt(T0=badT)
    attempt(protocol=2)
    attempt(max_iters=-1)
    attempt(max_iters_ref=-1)
    assert _call(prob, [case], {})["accepted"][0] == 1      # the handle still works


def test_loop_closure_end_to_end(prob):
    """pose_inc of an accepted candidate as the loop edge of a 20-vertex pose graph: kf0 is vertex 0, kf1 vertex 19, and
    expmap(pose_inc) = T_inc^-1 = X_0^-1 X_19 is the measurement of the edge (0, 19).  A sanity check: the closed vertex moves towards its
    true pose."""
    case = RC.runs("size_129_70_p0")[0]
    out = _call(prob, [case], {})
    assert out["accepted"][0] == 1
    rng = np.random.default_rng(5)
    X = [np.eye(4)]
    for k in range(1, 19):
        D = RC._offset(np.eye(4), [0.5, 0.02 * rng.normal(), 0.02 * rng.normal()], np.array([0.0, 0.33, 0.0]) + 0.01 * rng.normal(size=3))
        X.append(X[-1] @ D)
    X.append(np.linalg.inv(case["T_true"]))      # kf1 sees kf0's points through T_true = X_19^-1 X_0
    est, ei, ej, Z = [np.eye(4)], [], [], []
    for k in range(19):
        drift = RC._offset(np.eye(4), 0.01 * rng.normal(size=3), np.deg2rad(0.3) * rng.normal(size=3))
        Zk = np.linalg.inv(X[k]) @ X[k + 1] @ drift
        ei.append(k); ej.append(k + 1); Z.append(Zk)
        est.append(est[-1] @ Zk)
    R, t = LR.se3_exp(out["pose_inc"][0], np.float64)
    Zl = np.eye(4); Zl[:3, :3] = R; Zl[:3, 3] = t
    ei.append(0); ej.append(19); Z.append(Zl)
    p12 = lambda T: np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]])
    fixed = np.zeros(20, np.uint8); fixed[0] = 1
    Xo, stats, _ = prob.pgo(np.stack([p12(T) for T in est]), ei, ej, np.stack([p12(T) for T in Z]), fixed=fixed, iters=20)
    before = np.linalg.norm(est[19][:3, 3] - X[19][:3, 3])
    after = np.linalg.norm(Xo[19, 9:] - X[19][:3, 3])
    print("loop closure: vertex 19 position error %.4f -> %.4f, chi2 %.3e -> %.3e" % (before, after, stats["chi2_initial"], stats["chi2_final"]))
    assert stats["chi2_final"] < stats["chi2_initial"] and after < before


def test_harness_relpose_mode_is_the_c_abi(prob, tmp_path):
    """tools/localba_harness.cpp `relpose`: isLoopClosure's call site from the matched lists to pose_inc, against the direct call bit for
    bit; an accepted candidate's index lists keep exactly the inliers and it alone assigns pose_inc"""
    import sys
    sys.path.insert(0, RC.ROOT + "/tools")
    import harness_io
    exe = harness_io.build_harness()
    cases = [RC.runs(n)[0] for n in RC.DEFAULT_OPTS]
    got = RC.host_run(exe, str(tmp_path), cases, {})
    out = _call(prob, cases, {})
    assert out["accepted"].sum() >= 5 and (out["accepted"] == 0).sum() >= 3
    for b, g in enumerate(got):
        r = RC.as_result(out, b)
        for k in ("T", "pose_inc", "H", "e", "cov_eig", "iters", "status", "n_inliers", "accepted", "pt_in", "ln_in"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(r[k])), (b, k)
        assert g["returned"] == r["accepted"]
        assert np.array_equal(g["pose_out"], r["pose_inc"] if r["accepted"] else np.zeros(6))
