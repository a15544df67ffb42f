"""CPU-side checks of the device pose graph (plba_optimize_pose_graph): the entry point exists on the C boundary, and the numpy
restatement the GPU tests compare with (tests/pgo_ref.py) agrees with the oracle's independent one (orc_pgo: numeric Jacobians,
oracle/plba_oracle.c) and with central differences of the oracle's edge error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import pgo_ref
from .test_host_graphs import _dp, _ip, _pgo_problem, _pose12, _se3_exp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_table_hold_the_entry(pkg):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plba.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+plba_optimize_pose_graph\s*\(", txt) and "plba_pose_graph" in txt
    import __graft_entry__ as g
    g.build_hip()
    assert hasattr(C.CDLL(g.HIP_LIB), "plba_optimize_pose_graph")
    assert "optimize_pose_graph" in pkg.abi.SIGNATURES and "optimize_pose_graph" in pkg.abi.PRODUCT_ONLY
    assert [f[0] for f in pkg.abi.PoseGraph._fields_] == ["nv", "pose12", "fixed", "ne", "ei", "ej", "meas12", "info36"]


def _graph(pkg, orc, **kw):
    g = _pgo_problem(pkg, orc, **kw)
    pose = np.array([_pose12(*_se3_exp(orc, x)) for x in g["est"]])
    meas = np.array([_pose12(*_se3_exp(orc, x)) for x in g["meas"]])
    return dict(nv=g["nv"], pose=pose, meas=meas, ei=np.ascontiguousarray(g["edges"][:, 0], np.int32),
                ej=np.ascontiguousarray(g["edges"][:, 1], np.int32), fixed=g["fixed"])


def _orc_pgo(orc, g, iters, init, info=None):
    ne = len(g["ei"])
    pose = np.ascontiguousarray(g["pose"].copy())
    info = np.ascontiguousarray(np.tile(np.eye(6).ravel(), (ne, 1)) if info is None else info.reshape(ne, 36))
    st = np.zeros(4)
    orc.lib().cdll.orc_pgo(g["nv"], _ip(np.ascontiguousarray(g["fixed"], np.int32)), _dp(pose), ne, _ip(g["ei"]), _ip(g["ej"]),
                           _dp(np.ascontiguousarray(g["meas"])), _dp(info), iters, C.c_double(1e-10), 0, init, _dp(st))
    return pose, st


def test_ref_jacobians_against_central_differences_of_the_oracle(orc):
    lib = orc.lib().cdll
    rng = np.random.default_rng(3)
    for _ in range(5):
        Xi, Xj, Z = (pgo_ref.join(pgo_ref._rot(rng.normal(size=3) * 0.8)[None], rng.normal(size=(1, 3)))[0] for _ in range(3))
        Zi = pgo_ref.iso_inv(Z)
        J0, J1 = pgo_ref.edge_jacobians(Xi[None], Xj[None], Zi[None])
        h = 1e-6
        for which, J in ((0, J0[0]), (1, J1[0])):
            N = np.zeros((6, 6))
            for c in range(6):
                ev = []
                for sgn in (1, -1):
                    u = np.zeros(6); u[c] = sgn * h
                    Xp = np.zeros(12)
                    lib.orc_se3_vertex_oplus(_dp(np.ascontiguousarray(Xj if which else Xi)), _dp(u), _dp(Xp))
                    e = np.zeros(6)
                    a, b = (Xi, Xp) if which else (Xp, Xj)
                    lib.orc_se3_edge_error(_dp(np.ascontiguousarray(a)), _dp(np.ascontiguousarray(b)), _dp(np.ascontiguousarray(Z)), _dp(e))
                    ev.append(e)
                N[:, c] = (ev[0] - ev[1]) / (2 * h)
            assert np.abs(J - N).max() <= 1e-6 * np.abs(N).max()
        e_ref = pgo_ref.edge_error(Xi[None], Xj[None], Zi[None])[0]
        e_orc = np.zeros(6)
        lib.orc_se3_edge_error(_dp(np.ascontiguousarray(Xi)), _dp(np.ascontiguousarray(Xj)), _dp(np.ascontiguousarray(Z)), _dp(e_orc))
        assert np.abs(e_ref - e_orc).max() < 1e-14


def test_ref_matches_the_oracle_pose_graph(pkg, orc):
    """the bars test_host_graphs uses between numeric (oracle) and analytic (facade) Jacobians, over the iterations before the
    rounding-level end game (this graph's sixth iteration accepts or rejects on the last bits of chi2)"""
    g = _graph(pkg, orc)
    pose, st = _orc_pgo(orc, g, 4, 0)
    r = pgo_ref.optimize(g["pose"], g["ei"], g["ej"], g["meas"], fixed=g["fixed"], iters=4, user_lambda=1e-10)
    assert r["chi2_initial"] == pytest.approx(st[0], rel=1e-12)
    assert r["iterations"] == int(st[2]) and r["trials"] == int(st[3])
    assert r["chi2_final"] == pytest.approx(st[1], rel=1e-5)
    assert np.abs(r["poses"] - pose).max() < 1e-6
    assert r["chi2_final"] < 0.2 * r["chi2_initial"]


def test_ref_initial_guess_equals_the_oracle(pkg, orc):
    g = _graph(pkg, orc)
    g["fixed"] = np.zeros(g["nv"], np.int32); g["fixed"][[0, 11]] = 1      # two sources: frontier order matters
    pose, st = _orc_pgo(orc, g, 0, 1)
    X = pgo_ref.initial_guess(g["pose"], g["fixed"].astype(bool), g["ei"], g["ej"], g["meas"])
    assert np.array_equal(X, pose)
    r = pgo_ref.optimize(g["pose"], g["ei"], g["ej"], g["meas"], fixed=g["fixed"], iters=0, initial=True)
    assert np.array_equal(r["poses"], pose) and r["chi2_initial"] == pytest.approx(st[0], rel=1e-12)
