"""tests/refine_ref.py — the reference of plba_refine_landmarks — held to the oracle's edges, the 40-digit vectors, numeric derivatives
and its own invariants; the conditions under which tests/test_refine.py may use it (left-out share, noise caps); the library's exports."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import refine_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = RR.wide()

# The windows of tests/test_refine.py (shared: the GPU tests import these builders and the cached reference runs).
# Parity windows run THREE iterations: from the generators' 5 cm starts the LM is at rounding level after four, and the gain ratio of a
# fifth is 0 / 0 in any precision (measured on the generated window: 29 of 600 landmarks decide differently in float64 and long double
# at five iterations, 2 at four, none at three).  The far-start window keeps its decisions apart from noise for the same reason.
TRACKS = [1, 2, 7, 8, 9, 15, 16, 17, 40]      # the 8-lane sub-group and its loop: at / below / above 8 and 16, and a long track
PARITY = dict(max_iters=3, max_trials=10, lambda_init=1e-2)


def window(name):
    import __graft_entry__ as g
    W = g.load_package().window
    if name == "tracks":
        return RR.hand_window(48, TRACKS, TRACKS, seed=3)
    if name == "generated":
        return W.make_window(12, 500, 100, imu=True, seed=0x5EED0A01)
    if name == "far":      # depth off by half, seen from the middle of the window
        w = W.make_window(12, 60, 20, imu=True, seed=0x5EED0B02)
        c0 = w["kf"]["P"].mean(0)
        w["points"] = c0 + (w["truth"]["points"] - c0) * 1.5
        w["lines"] = np.concatenate([c0 + (w["truth"]["lines"][:, :3] - c0) * 1.5, c0 + (w["truth"]["lines"][:, 3:] - c0) * 1.5], 1)
        return w
    raise KeyError(name)


_cache = {}


def reference(name, **kw):
    """(window, float64 run, wide run, compare()) of a named window, computed once per process"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        w = window(name)
        opts = dict(PARITY); opts.update(kw)
        r64, rw = RR.refine(w, np.float64, **opts), RR.refine(w, WIDE, **opts)
        _cache[key] = (w, r64, rw, RR.compare(r64, rw, len(w["points"])))
    return _cache[key]


def _camv(c):
    return np.array([c["fx"], c["fy"], c["cx"], c["cy"]] + list(np.ravel(c["Rbc"])) + list(c["Pbc"]), float)


def _nav(P, q):
    return np.concatenate([P, np.zeros(3), q, np.zeros(12)])


def test_edges_match_the_oracle(orc):
    w = window("tracks")
    rig = RR.Rig(w, np.float64)
    cam = _camv(w["cam"])
    for e in range(0, len(w["po_pt"]), 7):
        k, i = int(w["po_kf"][e]), int(w["po_pt"][e])
        er, Jr = rig.point_edge(k, w["points"][i], w["po_uv"][e])
        eo, Ji, _, _ = orc.eval_point_edge(cam, _nav(w["kf"]["P"][k], w["kf"]["q"][k]), w["points"][i], w["po_uv"][e])
        assert np.abs(er - eo).max() <= 1e-12 * max(1.0, np.abs(eo).max()) and np.abs(Jr - np.asarray(Ji).reshape(2, 3)).max() <= 1e-12 * np.abs(Ji).max()
    for e in range(0, len(w["lo_ln"]), 7):
        k, i = int(w["lo_kf"][e]), int(w["lo_ln"][e])
        er, Js, Je = rig.line_edge(k, w["lines"][i], w["lo_l"][e])
        eo, Ji, _, _ = orc.eval_line_edge(cam, _nav(w["kf"]["P"][k], w["kf"]["q"][k]), w["lines"][i], w["lo_l"][e])
        Ji = np.asarray(Ji).reshape(3, 6)
        sc = np.abs(Ji).max()
        assert np.abs(er - eo[:2]).max() <= 1e-12 * max(1.0, np.abs(eo).max())
        assert np.abs(Js - Ji[0, 0:3]).max() <= 1e-12 * sc and np.abs(Je - Ji[1, 3:6]).max() <= 1e-12 * sc


def test_edges_match_the_40_digit_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "mp_vectors.json")) as f:
        vec = json.load(f)
    c = vec["cam"]
    for dt, tol in ((np.float64, 1e-12), (WIDE, 1e-15)):
        with RR._prec(dt):
            for v in vec["point"]:
                w = dict(cam=dict(c, Rbc=np.array(c["Rbc"], float), Pbc=np.array(c["Pbc"], float)), kf=dict(P=np.array([v["nav"]["P"]]), q=np.array([v["nav"]["q"]])))
                rig = RR.Rig(w, dt)
                e, J = rig.point_edge(0, RR.cast(np.array(v["Pw"]), dt), RR.cast(np.array(v["obs"]), dt))
                sc = np.abs(v["Jl"]).max()
                assert np.abs(RR.f64(e) - np.array(v["e"])).max() <= tol * 1e3 * max(1.0, np.abs(v["e"]).max()), (dt, v["e"])
                assert np.abs(RR.f64(J) - np.array(v["Jl"])).max() <= max(tol, 4e-16) * 1e3 * sc
            for v in vec["line"]:
                w = dict(cam=dict(c, Rbc=np.array(c["Rbc"], float), Pbc=np.array(c["Pbc"], float)), kf=dict(P=np.array([v["nav"]["P"]]), q=np.array([v["nav"]["q"]])))
                rig = RR.Rig(w, dt)
                e, Js, Je = rig.line_edge(0, RR.cast(np.array(v["L"]), dt), RR.cast(np.array(v["obs"]), dt))
                sc = max(np.abs(v["Jl_s"]).max(), np.abs(v["Jl_e"]).max())
                assert np.abs(RR.f64(e) - np.array(v["e"])).max() <= tol * 1e3 * max(1.0, np.abs(v["e"]).max())
                assert np.abs(RR.f64(Js) - np.array(v["Jl_s"])[0]).max() <= max(tol, 4e-16) * 1e3 * sc and np.abs(RR.f64(Je) - np.array(v["Jl_e"])[0]).max() <= max(tol, 4e-16) * 1e3 * sc


def test_point_rows_match_numeric_derivatives():
    w = window("tracks")
    with RR._prec(WIDE):
        rig = RR.Rig(w, WIDE)
        h = RR.cast(np.array([1e-7]), WIDE)[0]
        for e in range(0, len(w["po_pt"]), 11):
            k, i = int(w["po_kf"][e]), int(w["po_pt"][e])
            x, m = RR.cast(w["points"][i], WIDE), RR.cast(w["po_uv"][e], WIDE)
            _, J = rig.point_edge(k, x, m)
            for c in range(3):
                xp, xm = x.copy(), x.copy()
                xp[c] = xp[c] + h; xm[c] = xm[c] - h
                num = (rig.point_edge(k, xp, m)[0] - rig.point_edge(k, xm, m)[0]) / (2 * h)
                assert np.abs(RR.f64(num) - RR.f64(J[:, c])).max() <= 1e-9 * max(1.0, np.abs(RR.f64(J)).max())


def test_invariants():
    w, r64, rw, _ = reference("generated")
    for r in rw:
        ch = [float(v) for v in r["chis"]]
        assert all(b <= a for a, b in zip(ch, ch[1:])), "chi2 grew over an accepted step"
        assert r["iters"] == r["path"].count("a") and r["trials"] == len(r["path"])
    # a rejected trial leaves x unchanged: a run whose every trial is rejected (a damping no step survives is not available, so the
    # far window's exhausted landmarks serve) returns its input bits
    wf, f64, fw, _ = reference("far", max_trials=2)
    ex = [i for i, r in enumerate(fw) if r["status"] == RR.EXHAUSTED and r["iters"] == 0]
    assert ex
    Np = len(wf["points"])
    for i in ex:
        x0 = wf["points"][i] if i < Np else wf["lines"][i - Np]
        assert np.array_equal(RR.f64(f64[i]["x"]), x0)
    # a noise-free landmark ends at the truth
    wn = RR.hand_window(24, [2, 5, 9], [2, 5, 9], seed=9, noise_px=0.0, lm_noise=0.02)
    rn = RR.refine(wn, WIDE, max_iters=8, huber_on=False)
    a = RR.arrays(rn, 3)
    assert np.abs(a["points"] - wn["truth"]["points"]).max() < 1e-9 and a["chi2_after"].max() < 1e-12
    # (a line is free along its own direction: across it the end points are on the truth — their residuals vanish)
    assert a["chi2_after"][3:].max() < 1e-12


@pytest.mark.parametrize("name,kw,cap", [("tracks", {}, 0.0), ("tracks", {"huber_on": False}, 0.0), ("generated", {}, 0.02), ("far", {"max_trials": 2}, 0.0)])
def test_reference_conditions(name, kw, cap):
    """What tests/test_refine.py relies on, asserted on the reference alone: the share of landmarks whose float64 and wide runs decide
    differently, and the noise caps (8 x noise <= 1e-8 m on points; on line end points, unobservable along the line — noise = rounding /
    mu —, the measured worst case of these windows is 2.1e-10 m: the same cap holds with the same factor)."""
    w, r64, rw, c = reference(name, **kw)
    ref = np.array([r["status"] in (RR.DONE, RR.EXHAUSTED) for r in rw])
    left = int((~c["same"] & ref).sum())
    print(name, kw, "left out", left, "of", int(ref.sum()), "exact", int(c["exact"].sum()), "noise", c["noise_pt"], c["noise_ln"])
    assert left <= cap * ref.sum()
    assert 8 * c["noise_pt"] <= 1e-8 and 8 * c["noise_ln"] <= 1e-8
    if name == "far":
        paths = [r["path"] for r in rw]
        assert any("ra" in p for p in paths), "no rejected-then-accepted iteration in the far window"
        assert any(r["status"] == RR.EXHAUSTED for r in rw), "no exhausted landmark in the far window"


def test_library_exports_and_refuses_without_a_device(hip_lib_path):
    import __graft_entry__ as g
    abi = g.load_package().abi
    assert {"refine_default_options", "refine_landmarks"} <= set(abi.SIGNATURES) and {"refine_default_options", "refine_landmarks"} <= abi.PRODUCT_ONLY
    lib = C.CDLL(hip_lib_path)
    o = abi.RefineOptions()
    lib.plba_refine_default_options(C.byref(o))
    assert (o.max_iters, o.max_trials, o.lambda_init) == (5, 10, 1e-2) and not o.select_point and not o.status
    lib.plba_refine_landmarks.restype = C.c_int
    assert lib.plba_refine_landmarks(None, C.byref(o), None) < 0
    import torch
    if not torch.cuda.is_available():      # no device: a handle cannot be made, so nothing can be computed
        h = C.c_void_p()
        opt = abi.Options()
        lib.plba_default_options(C.byref(opt))
        lib.plba_create.restype = C.c_int
        assert lib.plba_create(C.byref(opt), C.byref(h)) < 0 and not h.value
