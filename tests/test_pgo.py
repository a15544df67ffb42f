"""plba_optimize_pose_graph on the device against the numpy restatement (tests/pgo_ref.py) and the oracle (orc_pgo).

Graph shapes: `pgo24` = test_host_graphs._pgo_problem (138 dims), `ess80` = its essential-graph shape with both loop ends fixed
(468 dims), `cov300` / `cov1000` = loopClosureOptimizationCovGraphG2O's shape (pgo_ref.cov_graph: odometry and covisibility
edges within +-8 keyframes, three loop closures, non-identity information, two fixed vertices; 1788 and 5988 dims, the second
past the explicit-inverse limit of the dense solve).  lambda = 1e-10 as the reference sets it: once the relative chi2 change is
at rounding level the accept / reject decisions are too (test_host_graphs.py), so traces are compared up to there."""
import ctypes as C

import numpy as np
import pytest

from . import pgo_ref
from .test_host_graphs import _ess_graph_problem, _pgo_problem, _pose12, _se3_exp

pytestmark = pytest.mark.gpu
LAM = 1e-10


def _from_log6(orc, g):
    ne = len(g["edges"])
    return dict(nv=g["nv"], pose=np.array([_pose12(*_se3_exp(orc, x)) for x in g["est"]]),
                meas=np.array([_pose12(*_se3_exp(orc, x)) for x in g["meas"]]), ei=np.ascontiguousarray(g["edges"][:, 0], np.int32),
                ej=np.ascontiguousarray(g["edges"][:, 1], np.int32), info=None, fixed=np.asarray(g["fixed"], np.uint8), ne=ne)


_CACHE = {}


def _shape(pkg, orc, name):
    if name not in _CACHE:
        if name == "pgo24":
            g = _from_log6(orc, _pgo_problem(pkg, orc))
        elif name == "ess80":
            g = _from_log6(orc, _ess_graph_problem(pkg, orc))
        else:
            g = pgo_ref.cov_graph(int(name[3:]), seed=7)
        _CACHE[name] = g
    return _CACHE[name]


def _dev(pkg, g, **kw):
    p = pkg.new_problem()
    try:
        return p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], user_lambda=kw.pop("user_lambda", LAM), **kw)
    finally:
        p.close()


def _ref(g, iters=100, initial=False, user_lambda=LAM):
    return pgo_ref.optimize(g["pose"], g["ei"], g["ej"], g["meas"], g["info"], g["fixed"], iters=iters, user_lambda=user_lambda, initial=initial)


SHAPES = ["pgo24", "ess80", "cov300", "cov1000"]


@pytest.mark.parametrize("name", SHAPES)
def test_pose_graph_against_the_reference(pkg, orc, hip, name):
    g = _shape(pkg, orc, name)
    # first three iterations: the same steps
    X3, st3, tr3 = _dev(pkg, g, iters=3)
    r3 = _ref(g, iters=3)
    assert st3["chi2_initial"] == pytest.approx(r3["chi2_initial"], rel=1e-12)
    assert st3["iterations"] == r3["iterations"] == 3 and st3["trials"] == r3["trials"]
    assert np.abs(X3 - r3["poses"]).max() <= 1e-8
    # the whole run
    X, st, tr = _dev(pkg, g, iters=100)
    r = _ref(g, iters=100)
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
    assert st["chi2_final"] < 0.5 * st["chi2_initial"] and st["stop_reason"] == 1 and st["solver_failures"] == 0
    fx = g["fixed"].astype(bool)
    assert np.array_equal(X[fx], g["pose"][fx])


@pytest.mark.parametrize("name", ["pgo24", "ess80"])
def test_small_shapes_against_the_oracle(pkg, orc, hip, name):
    """test_host_graphs' bars between numeric (oracle) and analytic Jacobians, before the end game"""
    from .test_pgo_cpu import _orc_pgo
    g = _shape(pkg, orc, name)
    pose, st4 = _orc_pgo(orc, g, 4, 0)
    X, st, _ = _dev(pkg, g, iters=4)
    assert st["chi2_initial"] == pytest.approx(st4[0], rel=1e-9)
    assert st["iterations"] == int(st4[2]) and st["trials"] == int(st4[3])
    assert st["chi2_final"] == pytest.approx(st4[1], rel=1e-5)
    assert np.abs(X - pose).max() < 1e-6


def test_initial_guess_and_an_unreached_component(pkg, orc, hip):
    g = dict(pgo_ref.cov_graph(40, seed=3))
    rng = np.random.default_rng(5)
    extra = np.array([pgo_ref.join(pgo_ref._rot(rng.normal(size=3))[None], rng.normal(size=(1, 3)))[0] for _ in range(5)])
    g["pose"] = np.concatenate([g["pose"], extra]); g["fixed"] = np.concatenate([g["fixed"], np.zeros(5, np.uint8)])
    add = [(40, 41), (41, 42), (42, 43), (43, 44), (40, 42)]
    g["ei"] = np.concatenate([g["ei"], [a for a, _ in add]]).astype(np.int32); g["ej"] = np.concatenate([g["ej"], [b for _, b in add]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], [pgo_ref.iso_mul(pgo_ref.iso_inv(extra[a - 40]), extra[b - 40]) for a, b in add]])
    g["info"] = np.concatenate([g["info"], np.tile(np.eye(6), (5, 1, 1))])
    X0, st0, _ = _dev(pkg, g, iters=0, initial_guess=True)
    r0 = _ref(g, iters=0, initial=True)
    assert np.array_equal(X0, r0["poses"])                           # the same products in the same order
    assert np.array_equal(X0[40:], extra)                            # no fixed vertex reaches them
    assert st0["chi2_initial"] == pytest.approx(r0["chi2_initial"], rel=1e-12) and st0["iterations"] == 0
    X, st, _ = _dev(pkg, g, iters=3, initial_guess=True)
    r = _ref(g, iters=3, initial=True)
    assert st["chi2_initial"] == pytest.approx(r["chi2_initial"], rel=1e-12)
    assert np.abs(X - r["poses"]).max() <= 1e-8


def test_exact_properties(pkg, orc, hip):
    base = pgo_ref.cov_graph(30, seed=4)
    # edge-less vertices (before, between and after the graph's) and fixed ones come back bit for bit
    g = dict(base)
    nv = base["nv"]
    lone = np.array([pgo_ref.join(pgo_ref._rot(np.array([0.1, 0.2, 0.3 + k]))[None], np.array([[k, 2.0, 3.0]]))[0] for k in range(3)])
    g["pose"] = np.concatenate([lone[:1], base["pose"], lone[1:]]); g["fixed"] = np.concatenate([[0], base["fixed"], [0, 0]]).astype(np.uint8)
    g["ei"] = (base["ei"] + 1).astype(np.int32); g["ej"] = (base["ej"] + 1).astype(np.int32)
    X, st, _ = _dev(pkg, g, iters=100)
    keep = np.zeros(nv + 3, bool); keep[[0, nv + 1, nv + 2]] = True; keep |= g["fixed"].astype(bool)
    assert np.array_equal(X[keep], g["pose"][keep]) and not np.array_equal(X[~keep], g["pose"][~keep])
    # two calls: identical bits
    X2, st2, tr2 = _dev(pkg, g, iters=100)
    assert np.array_equal(X, X2) and st2["chi2_final"] == st["chi2_final"] and st2["trials"] == st["trials"]
    # an edge between the two fixed vertices changes chi2 only
    r = _ref(base, iters=0)
    g2 = dict(base); g2["ei"] = np.append(base["ei"], 0).astype(np.int32); g2["ej"] = np.append(base["ej"], 1).astype(np.int32)
    g2["meas"] = np.concatenate([base["meas"], [pgo_ref.iso_mul(pgo_ref.iso_inv(base["pose"][0]), base["pose"][1])]])
    g2["meas"][-1, 9:] += 0.1
    g2["info"] = np.concatenate([base["info"], np.eye(6)[None]])
    Xa, sa, _ = _dev(pkg, base, iters=3)
    Xb, sb, _ = _dev(pkg, g2, iters=3)
    e = pgo_ref.edge_error(base["pose"][0][None], base["pose"][1][None], pgo_ref.iso_inv(g2["meas"][-1])[None])
    assert sb["chi2_initial"] - sa["chi2_initial"] == pytest.approx(float(e[0] @ e[0]), rel=1e-9) and float(e[0] @ e[0]) > 1e-3
    assert sa["trials"] == sb["trials"] and np.abs(Xa - Xb).max() < 1e-12
    assert r["chi2_initial"] == pytest.approx(sa["chi2_initial"], rel=1e-12)
    # every vertex fixed: nothing to optimise, chi2 reported
    g3 = dict(base); g3["fixed"] = np.ones(nv, np.uint8)
    X3, s3, t3 = _dev(pkg, g3, iters=100)
    assert s3["iterations"] == 0 and s3["trials"] == 0 and not t3 and np.array_equal(X3, base["pose"])
    assert s3["chi2_initial"] == s3["chi2_final"] == pytest.approx(r["chi2_initial"], rel=1e-12)
    # max_iters = 0: chi2 only
    X4, s4, _ = _dev(pkg, base, iters=0)
    assert s4["iterations"] == 0 and np.array_equal(X4, base["pose"]) and s4["chi2_final"] == s4["chi2_initial"] == pytest.approx(r["chi2_initial"], rel=1e-12)
    # duplicate edges are two edges
    g5 = dict(base)
    dup = [3, 10, 10]
    g5["ei"] = np.append(base["ei"], base["ei"][dup]).astype(np.int32); g5["ej"] = np.append(base["ej"], base["ej"][dup]).astype(np.int32)
    g5["meas"] = np.concatenate([base["meas"], base["meas"][dup]]); g5["info"] = np.concatenate([base["info"], base["info"][dup]])
    X5, s5, _ = _dev(pkg, g5, iters=3)
    r5 = _ref(g5, iters=3)
    assert s5["chi2_initial"] == pytest.approx(r5["chi2_initial"], rel=1e-12) and np.abs(X5 - r5["poses"]).max() <= 1e-8


def test_the_problem_window_is_left_alone(pkg, orc, hip):
    w = pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AA)
    g = pgo_ref.cov_graph(60, seed=9)
    out = []
    for with_pgo in (False, True):
        p = pkg.new_problem()
        p.upload_window(w)
        p.optimize(3)
        if with_pgo:
            p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], iters=20, user_lambda=LAM)
        st = p.optimize(5)
        out.append((pkg.protocol.results(p), st))
        p.close()
    (a, sa), (b, sb) = out
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_refusals_leave_the_poses_untouched(pkg, orc, hip):
    g = pgo_ref.cov_graph(10, seed=2)
    abi = pkg.abi
    p = pkg.new_problem()
    fn = p.lib.fn["optimize_pose_graph"]

    def call(nv=None, pose=None, ei=None, ej=None, meas=None, info="g", fixed=None, iters=5, lam=LAM, stats=True, ne=None):
        X = np.ascontiguousarray(g["pose"] if pose is None else pose, np.float64).copy()
        X0 = X.copy()
        a = np.ascontiguousarray(g["ei"] if ei is None else ei, np.int32); b = np.ascontiguousarray(g["ej"] if ej is None else ej, np.int32)
        Z = np.ascontiguousarray(g["meas"] if meas is None else meas, np.float64)
        om = np.ascontiguousarray(g["info"] if isinstance(info, str) else info, np.float64) if info is not None else None
        gr = abi.PoseGraph(len(X) if nv is None else nv, abi._dp(X), abi._up(None if fixed is None else np.ascontiguousarray(fixed, np.uint8)),
                           len(a) if ne is None else ne, abi._ip(a), abi._ip(b), abi._dp(Z), abi._dp(om))
        st = abi.Stats()
        rc = fn(p._h, C.byref(gr), iters, lam, 0, C.byref(st) if stats else None, None, 0, None)
        return rc, np.array_equal(X.view(np.uint64), X0.view(np.uint64))

    rc, same = call()
    assert rc == 0 and not same                                   # the control: a valid call moves the poses
    bad = dict(nv0=dict(nv=0), nvneg=dict(nv=-1), ei_range=dict(ei=np.where(np.arange(len(g["ei"])) == 4, 10, g["ei"])),
               ej_neg=dict(ej=np.where(np.arange(len(g["ej"])) == 2, -1, g["ej"])), self_edge=dict(ej=np.where(np.arange(len(g["ej"])) == 3, g["ei"], g["ej"])),
               nan_pose=dict(pose=np.where(np.arange(12)[None] == 10, np.nan, g["pose"])), inf_meas=dict(meas=np.where(np.arange(12)[None] == 1, np.inf, g["meas"])),
               nan_info=dict(info=np.where(np.arange(36).reshape(6, 6)[None] == 7, np.nan, g["info"])), nan_lambda=dict(lam=float("nan")),
               no_stats=dict(stats=False), neg_iters=dict(iters=-1))
    for k, kw in bad.items():
        rc, same = call(**kw)
        assert rc == -1 and same, k
    p.close()
