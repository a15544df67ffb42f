"""plba_optimize_pose_graph's sparse multifrontal solver (options.pgo_solver = 1) on the device: against the numpy references
(tests/pgo_ref.py, and tests/pgo_sparse_ref.py where the dense one cannot run), against the dense device path, on graphs whose dense
system would not fit a device (20 000 keyframes), on the structures that stress the elimination tree, and on a failing factorisation.
Every sparse call goes through _sparse(), which first checks that the option exists (ctypes would otherwise take an unknown attribute
and run the dense path) and afterwards that the sparse path ran."""
import ctypes as C

import numpy as np
import pytest

from . import pgo_ref, pgo_sparse_ref
from .test_pgo import LAM, SHAPES, _dev, _ref, _shape

pytestmark = pytest.mark.gpu


def _sparse(pkg, g, want_info=False, **kw):
    assert "pgo_solver" in [f[0] for f in pkg.abi.Options._fields_], "options.pgo_solver is missing"
    p = pkg.new_problem(pgo_solver=1)
    try:
        X, st, tr = p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], user_lambda=kw.pop("user_lambda", LAM), **kw)
        info = p.debug_get("pgo_sparse")
    finally:
        p.close()
    assert len(info) == 8 and info[0] == 1, "the sparse path did not run"
    return (X, st, tr, info) if want_info else (X, st, tr)


def _three(X3, st3, r3):
    assert st3["chi2_initial"] == pytest.approx(r3["chi2_initial"], rel=1e-12)
    assert st3["iterations"] == r3["iterations"] and st3["trials"] == r3["trials"]
    assert np.abs(X3 - r3["poses"]).max() <= 1e-8


def _whole(X, st, tr, r, g):
    """test_pose_graph_against_the_reference's bars over a whole run; r: dict with poses, chi2_initial, chi2_final, trace"""
    assert st["chi2_initial"] == pytest.approx(r["chi2_initial"], rel=1e-12)
    assert st["n_trace"] == st["trials"] == len(tr)
    for a, b in zip(tr, r["trace"]):
        if abs(b["chi2_current"] - b["chi2_trial"]) < 1e-10 * b["chi2_current"]:
            break
        assert (a["iteration"], a["trial"], a["accepted"], a["solver_ok"]) == (b["iteration"], b["trial"], b["accepted"], b["solver_ok"])
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
        assert a["chi2_current"] == pytest.approx(b["chi2_current"], rel=1e-9)
    else:
        pytest.fail("the reference never reached its rounding-level end game")
    assert st["chi2_final"] <= r["chi2_final"] * (1 + 1e-6)
    assert np.abs(X - r["poses"]).max() <= 1e-5
    fx = g["fixed"].astype(bool)
    assert np.array_equal(X[fx], g["pose"][fx])


def test_guard_the_option_exists_and_the_sparse_path_runs(pkg, orc, hip):
    _sparse(pkg, pgo_ref.cov_graph(20, seed=3), iters=2)


@pytest.mark.parametrize("name", SHAPES)
def test_sparse_against_the_reference(pkg, orc, hip, name):
    g = _shape(pkg, orc, name)
    X3, st3, _ = _sparse(pkg, g, iters=3)
    _three(X3, st3, _ref(g, iters=3))
    X, st, tr = _sparse(pkg, g, iters=100)
    _whole(X, st, tr, _ref(g, iters=100), g)
    assert st["stop_reason"] == 1 and st["solver_failures"] == 0


@pytest.mark.parametrize("name", SHAPES)
def test_sparse_against_the_dense_device_path(pkg, orc, hip, name):
    g = _shape(pkg, orc, name)
    X3, st3, _ = _sparse(pkg, g, iters=3)
    D3, sd3, _ = _dev(pkg, g, iters=3)
    _three(X3, st3, dict(sd3, poses=D3))
    X, st, tr = _sparse(pkg, g, iters=100)
    D, sd, td = _dev(pkg, g, iters=100)
    _whole(X, st, tr, dict(sd, poses=D, trace=td), g)


@pytest.mark.parametrize("nv,loops", [(20000, 3), (2000, 200)])
def test_large_graphs_against_the_sparse_reference(pkg, orc, hip, nv, loops):
    g = pgo_ref.cov_graph(nv, seed=7, n_loops=loops)
    X, st, tr, info = _sparse(pkg, g, want_info=True, iters=3)
    r = pgo_sparse_ref.optimize(g["pose"], g["ei"], g["ej"], g["meas"], g["info"], g["fixed"], iters=3, user_lambda=LAM)
    # 20 000 keyframes of the looping trajectory reach translations of ~200 m, and the chain's condition number turns rounding into a
    # few 1e-8 m between two correct orderings (the reference's LU and the device's tree): a fixed bar a few times that gap
    assert st["chi2_initial"] == pytest.approx(r["chi2_initial"], rel=1e-12)
    assert st["iterations"] == r["iterations"] and st["trials"] == r["trials"]
    assert np.abs(X - r["poses"]).max() <= 2e-7
    assert st["chi2_final"] == pytest.approx(r["chi2_final"], rel=1e-9)
    for a, b in zip(tr, r["trace"]):
        assert (a["iteration"], a["trial"], a["accepted"], a["solver_ok"]) == (b["iteration"], b["trial"], b["accepted"], b["solver_ok"])
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
    P = 6 * (nv - 2)
    assert info[1] == nv - 2 and info[2] > 1 and info[3] > 1 and info[4] >= nv - 2 and info[5] > 0
    if nv >= 20000:
        assert info[6] < 0.02 * 8.0 * P * P


def _poses_meas(pose, edges, seed, noise=1e-3):
    rng = np.random.default_rng(seed)
    meas = np.array([pgo_ref.iso_mul(pgo_ref.iso_inv(pose[i]), pose[j]) for i, j in edges])
    meas[:, 9:] += rng.normal(size=(len(edges), 3)) * noise
    return meas


def _make(pose, edges, fixed, seed=1, info=None):
    e = np.array(edges, np.int32).reshape(-1, 2)
    drift = pose.copy()
    rng = np.random.default_rng(seed + 100)
    drift[:, 9:] += rng.normal(size=(len(pose), 3)) * 1e-2
    fx = np.zeros(len(pose), np.uint8); fx[list(fixed)] = 1
    drift[fx.astype(bool)] = pose[fx.astype(bool)]
    om = np.tile(np.diag([50.0, 50.0, 50.0, 200.0, 200.0, 200.0]), (len(e), 1, 1)) if info is None else info
    return dict(nv=len(pose), pose=drift, ei=e[:, 0].copy(), ej=e[:, 1].copy(), meas=_poses_meas(pose, edges, seed), info=om, fixed=fx)


def _base_poses(nv, seed=11):
    return pgo_ref.cov_graph(max(nv, 8), seed=seed)["pose"][:nv]


def _structures():
    out = {}
    P80 = _base_poses(80)
    out["complete80"] = _make(P80, [(i, j) for i in range(80) for j in range(i + 1, 80)], fixed=[0])
    P41 = _base_poses(41)
    out["star"] = _make(P41, [(0, i) for i in range(1, 41)], fixed=[5])
    out["fixed_hub"] = _make(P41, [(0, i) for i in range(1, 41)] + [(3, 4)], fixed=[0])
    P60 = _base_poses(60)
    chain_a = [(i, i + 1) for i in range(0, 24)] + [(i, i + 2) for i in range(0, 23, 3)]
    chain_b = [(i, i + 1) for i in range(30, 55)] + [(i, i + 3) for i in range(30, 52, 4)]
    out["two_components"] = _make(P60, chain_a + chain_b, fixed=[0, 30])      # 25 .. 29 and 56 .. 59 untouched
    out["one_free"] = _make(_base_poses(2), [(0, 1)], fixed=[0])
    return out


STRUCT = ["complete80", "star", "fixed_hub", "two_components", "one_free"]


@pytest.mark.parametrize("name", STRUCT)
def test_structures_sparse_against_dense(pkg, orc, hip, name):
    g = _structures()[name]
    X3, st3, _, info = _sparse(pkg, g, want_info=True, iters=3)
    D3, sd3, _ = _dev(pkg, g, iters=3)
    _three(X3, st3, dict(sd3, poses=D3))
    X, st, tr = _sparse(pkg, g, iters=30)
    D, sd, td = _dev(pkg, g, iters=30)
    assert st["chi2_initial"] == pytest.approx(sd["chi2_initial"], rel=1e-12)
    assert np.abs(X - D).max() <= 1e-5
    touched = np.zeros(g["nv"], bool); touched[g["ei"]] = True; touched[g["ej"]] = True
    keep = ~touched | g["fixed"].astype(bool)
    assert np.array_equal(X[keep], g["pose"][keep]) and np.array_equal(X3[keep], g["pose"][keep])
    if name == "complete80":
        assert info[2] == 1 and info[5] == 6 * 79                               # one front, wider than LDS holds
    if name == "one_free":
        assert info[2] == 1 and info[5] == 6                                    # one front without children: the plan's child list is empty
    assert info[1] == (touched & ~g["fixed"].astype(bool)).sum()


def test_no_iterations_and_initial_guess_with_an_unreached_component(pkg, orc, hip):
    g = dict(pgo_ref.cov_graph(40, seed=3))
    X0, s0, t0, info = _sparse(pkg, g, want_info=True, iters=0)
    D0, d0, _ = _dev(pkg, g, iters=0)
    assert np.array_equal(X0, D0) and s0["chi2_initial"] == d0["chi2_initial"] and s0["iterations"] == 0 and not t0
    assert np.all(info[1:] == 0)
    rng = np.random.default_rng(5)
    extra = np.array([pgo_ref.join(pgo_ref._rot(rng.normal(size=3))[None], rng.normal(size=(1, 3)))[0] for _ in range(5)])
    g["pose"] = np.concatenate([g["pose"], extra]); g["fixed"] = np.concatenate([g["fixed"], np.zeros(5, np.uint8)])
    add = [(40, 41), (41, 42), (42, 43), (43, 44), (40, 42)]
    g["ei"] = np.concatenate([g["ei"], [a for a, _ in add]]).astype(np.int32); g["ej"] = np.concatenate([g["ej"], [b for _, b in add]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], [pgo_ref.iso_mul(pgo_ref.iso_inv(extra[a - 40]), extra[b - 40]) for a, b in add]])
    g["info"] = np.concatenate([g["info"], np.tile(np.eye(6), (5, 1, 1))])
    X, st, _ = _sparse(pkg, g, iters=3, initial_guess=True)
    D, sd, _ = _dev(pkg, g, iters=3, initial_guess=True)
    _three(X, st, dict(sd, poses=D))
    _three(X, st, _ref(g, iters=3, initial=True))


def test_a_failing_factorisation_matches_the_dense_path(pkg, orc, hip):
    g = dict(pgo_ref.cov_graph(60, seed=8))
    g["info"] = g["info"].copy()
    g["info"][20] = -1e7 * np.eye(6)
    X, st, tr = _sparse(pkg, g, iters=4)
    D, sd, td = _dev(pkg, g, iters=4)
    assert sd["solver_failures"] > 0 and st["solver_failures"] == sd["solver_failures"]
    assert (st["iterations"], st["trials"], st["stop_reason"]) == (sd["iterations"], sd["trials"], sd["stop_reason"])
    assert len(tr) == len(td)
    for a, b in zip(tr, td):
        assert (a["iteration"], a["trial"], a["accepted"], a["solver_ok"]) == (b["iteration"], b["trial"], b["accepted"], b["solver_ok"])
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
    assert np.abs(X - D).max() <= 1e-8


def test_determinism_isolation_and_refusal(pkg, orc, hip):
    g = pgo_ref.cov_graph(300, seed=7)
    X1, s1, t1 = _sparse(pkg, g, iters=100)
    X2, s2, t2 = _sparse(pkg, g, iters=100)
    assert np.array_equal(X1.view(np.uint64), X2.view(np.uint64)) and s1["chi2_final"] == s2["chi2_final"] and t1 == t2
    # the problem's window: a following optimize is bit-identical (test_pgo.test_the_problem_window_is_left_alone, sparse)
    w = pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AA)
    gs = pgo_ref.cov_graph(60, seed=9)
    out = []
    for with_pgo in (False, True):
        p = pkg.new_problem(pgo_solver=1)
        p.upload_window(w)
        p.optimize(3)
        if with_pgo:
            p.pgo(gs["pose"], gs["ei"], gs["ej"], gs["meas"], info=gs["info"], fixed=gs["fixed"], iters=20, user_lambda=LAM)
            assert p.debug_get("pgo_sparse")[0] == 1
        st = p.optimize(5)
        out.append((pkg.protocol.results(p), st))
        p.close()
    (a, _), (b, _) = out
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # an invalid pgo_solver is refused and leaves the poses untouched
    abi = pkg.abi
    for bad in (2, -1):
        p = pkg.new_problem(pgo_solver=bad)
        X = np.ascontiguousarray(gs["pose"], np.float64).copy()
        X0 = X.copy()
        gr = abi.PoseGraph(len(X), abi._dp(X), abi._up(np.ascontiguousarray(gs["fixed"], np.uint8)), len(gs["ei"]), abi._ip(np.ascontiguousarray(gs["ei"], np.int32)),
                           abi._ip(np.ascontiguousarray(gs["ej"], np.int32)), abi._dp(np.ascontiguousarray(gs["meas"], np.float64)),
                           abi._dp(np.ascontiguousarray(gs["info"], np.float64)))
        st = abi.Stats()
        rc = p.lib.fn["optimize_pose_graph"](p._h, C.byref(gr), 5, LAM, 0, C.byref(st), None, 0, None)
        assert rc == -1 and np.array_equal(X.view(np.uint64), X0.view(np.uint64))
        p.close()
