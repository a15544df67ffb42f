"""CPU-side checks of the sparse pose-graph solver (options.pgo_solver = 1): the default keeps the dense path, and the sparse numpy
reference the GPU tests compare the large graphs with (tests/pgo_sparse_ref.py) agrees with pgo_ref.optimize where both run."""
import ctypes as C

import numpy as np
import pytest

from . import pgo_ref, pgo_sparse_ref

LAM = 1e-10


def test_default_options_keep_the_dense_solver(pkg, hip_lib_path):
    assert "pgo_solver" in [f[0] for f in pkg.abi.Options._fields_]
    assert pkg.abi.Options._fields_[-1][0] == "pgo_solver"                # appended after diag: the older fields keep their offsets
    lib = C.CDLL(hip_lib_path)
    o = pkg.abi.Options()
    o.pgo_solver = 7
    lib.plba_default_options(C.byref(o))
    assert o.pgo_solver == 0


@pytest.mark.parametrize("nv", [300, 1000])
def test_sparse_reference_agrees_with_the_dense_one(nv):
    g = pgo_ref.cov_graph(nv, seed=7)
    args = (g["pose"], g["ei"], g["ej"], g["meas"], g["info"], g["fixed"])
    r = pgo_ref.optimize(*args, iters=3, user_lambda=LAM)
    s = pgo_sparse_ref.optimize(*args, iters=3, user_lambda=LAM)
    assert s["chi2_initial"] == r["chi2_initial"]
    assert (s["iterations"], s["trials"], s["solver_failures"]) == (r["iterations"], r["trials"], r["solver_failures"])
    for a, b in zip(s["trace"], r["trace"]):
        assert (a["iteration"], a["trial"], a["accepted"], a["solver_ok"]) == (b["iteration"], b["trial"], b["accepted"], b["solver_ok"])
        assert a["lam"] == pytest.approx(b["lam"], rel=1e-9)
    assert np.abs(s["poses"] - r["poses"]).max() <= 1e-8


def test_sparse_reference_reports_an_indefinite_system_as_the_dense_one():
    g = pgo_ref.cov_graph(60, seed=8)
    info = g["info"].copy()
    info[20] = -1e3 * np.eye(6)
    args = (g["pose"], g["ei"], g["ej"], g["meas"], info, g["fixed"])
    with np.errstate(over="ignore"):
        r = pgo_ref.optimize(*args, iters=3, user_lambda=LAM)
        s = pgo_sparse_ref.optimize(*args, iters=3, user_lambda=LAM)
    assert r["solver_failures"] > 0 and s["solver_failures"] == r["solver_failures"]
    assert [t["solver_ok"] for t in s["trace"]] == [t["solver_ok"] for t in r["trace"]]
    assert np.abs(s["poses"] - r["poses"]).max() <= 1e-8
