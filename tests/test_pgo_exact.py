"""plba_optimize_pose_graph (dense and sparse solver) and the H of plba_pose_graph_marginals on the device, held to the extended-precision
reference (tests/pgo_exact.py) over the cases of tests/pgo_exact_cases.py under the rule stated there: a quantity within
max(8 x noise, m u |value|) of the wide run, noise = |fp64 reference - wide reference|, discrete outputs exactly, each case over the
trials whose decisions have 1000 x their noise in the reference (pgo_exact_cases.TRIALS).  The device is read through what the ABI offers:
chi2_initial of a max_iters = 0 call, the summed H blocks of the marginals' diagnostic dump, poses and trace rows after 1, 2 and 3 iterations.
Every test prints error, noise, tolerance and error / noise before it asserts."""
import numpy as np
import pytest

from . import pgo_exact as PX
from . import pgo_exact_cases as C

pytestmark = pytest.mark.gpu
DUMP = 32      # PLBA_DIAG_PGO_COV_DUMP
COMPARED = [n for n in C.NAMES if n not in C.NOT_COMPARED]
SOLVERS = [0, 1]


def _dev(pkg, case, solver, iters, extra_vertex=False):
    pose, fixed = case["pose"], case["fixed"]
    if extra_vertex:      # a vertex no edge touches, behind the graph's
        pose = np.concatenate([pose, [np.concatenate([np.eye(3).ravel(), [7.0, 8.0, 9.0]])]]); fixed = np.concatenate([fixed, [0]]).astype(np.uint8)
    p = pkg.new_problem(pgo_solver=solver)
    try:
        return p.pgo(pose, case["ei"], case["ej"], case["meas"], info=case["info"], fixed=fixed, iters=iters, user_lambda=case["opts"]["user_lambda"],
                     initial_guess=case["opts"]["initial"])
    finally:
        p.close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", COMPARED)
def test_chi2_of_the_start(pkg, hip, name, solver):
    case, r64, rw, T = C.runs(name)
    X, st, tr = _dev(pkg, case, solver, 0)
    tol, noise, _ = PX.tolerances(case, r64, rw, T)
    bad = []
    PX.hold("device %s solver %d" % (name, solver), "chi2_initial", st["chi2_initial"], rw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    nz, t = PX._noise_tol(r64["X_start"], rw["X_start"], 64)
    PX.hold("device %s solver %d" % (name, solver), "start (initial guess)", X, rw["X_start"], t, nz, bad)
    assert st["iterations"] == 0 and st["trials"] == 0 and not tr and st["chi2_final"] == st["chi2_initial"]
    assert not bad, bad


@pytest.mark.parametrize("name", C.H_READABLE)
def test_h_blocks_of_the_marginals(pkg, hip, name):
    """the blocks k_pgo_sum leaves (one summation for both solvers and the marginals), per block against the wide J^T O J"""
    case, r64, rw, T = C.runs(name)
    p = pkg.new_problem(diag=DUMP)
    try:
        p.pgo_marginals(PX.f64(r64["X_start"]), case["ei"], case["ej"], case["meas"], info=case["info"], fixed=case["fixed"])
        Hb = p.debug_get("pgo_cov_H").copy()
    finally:
        p.close()
    rows, cols, cnt = PX.block_sources(case)
    assert Hb.size == 36 * len(rows) == 36 * len(C.host_blocks(case)[3])
    Hb = Hb.reshape(-1, 6, 6)
    tol, noise, _ = PX.tolerances(case, r64, rw, T)
    Bw = PX.h_blocks(case, rw)
    e = np.abs(Hb - Bw).reshape(len(Bw), -1).max(-1)
    q = int(np.argmax(e / tol["H"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        en = np.where(noise["H"] > 0, e / noise["H"], np.where(e > 0, np.inf, 0.0))
    print("device %s H: %d blocks, worst error / tolerance %.3f (block %d,%d: error %.3e noise %.3e tolerance %.3e, %d sources), worst error / noise %.2f" % (
        name, len(Bw), float(e[q] / tol["H"][q]), rows[q], cols[q], e[q], noise["H"][q], tol["H"][q], cnt[q], float(en.max())))
    assert np.all(e <= tol["H"]), [(int(k), float(e[k]), float(tol["H"][k])) for k in np.flatnonzero(~(e <= tol["H"]))]


def test_h_blocks_of_the_relabelled_graph_equal_the_unrelabelled_ones(pkg, hip):
    """`relabelled` (every edge with the lower free rank at its vertex 1, measurements untouched: every off-diagonal source goes through slot
    3) gives the blocks of the unrelabelled graph, renumbered and transposed, under the rule.  (An edge reversed with its measurement inverted
    has another error, E' = Z E^-1 Z^-1, and no such equality: pgo_exact_cases.py; those graphs are held to their own wide reference above.)"""
    gb, b64, bw, _ = C.runs("base12")
    gr, _, _, _ = C.runs("relabelled")
    p = pkg.new_problem(diag=DUMP)
    try:
        p.pgo_marginals(gr["pose"], gr["ei"], gr["ej"], gr["meas"], info=gr["info"], fixed=gr["fixed"])
        Hr = p.debug_get("pgo_cov_H").copy().reshape(-1, 6, 6)
    finally:
        p.close()
    rows_r, cols_r, _ = PX.block_sources(gr)
    idx = {(int(a), int(c)): k for k, (a, c) in enumerate(zip(rows_r, cols_r))}
    rows, cols, _ = PX.block_sources(gb)
    tol, noise, _ = PX.tolerances(gb, b64, bw, 0)
    Bw = PX.h_blocks(gb, bw)
    n = bw["n"]
    bad = []
    for k, (a, c) in enumerate(zip(rows, cols)):      # block (a, c), a >= c, is block (n - 1 - c, n - 1 - a) of the relabelled graph, transposed
        got = Hr[idx[(n - 1 - c, n - 1 - a)]].T
        PX.hold("device relabelled", "H[%d,%d]" % (a, c), got, Bw[k], tol["H"][k], noise["H"][k], bad)
    assert not bad, bad


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", COMPARED)
def test_steps_and_trace_rows(pkg, hip, name, solver):
    """poses and every field of every trace row after max_iters = 1, 2 and 3, up to the trial the case is compared to; b and the solve are
    held through the first trial's scale, chi2_trial and poses"""
    case, r64, rw, T = C.runs(name)
    bad = []
    for k in (1, 2, 3):
        X, st, tr = _dev(pkg, case, solver, k)
        res = dict(poses=X, chi2_initial=st["chi2_initial"], trace=tr, iterations=st["iterations"], trials=st["trials"])
        bad += PX.hold_run("device %s solver %d iters %d" % (name, solver, k), case, res, r64, rw, T, k)
        assert st["n_trace"] == st["trials"] == len(tr)
        fx = case["fixed"].astype(bool)
        assert np.array_equal(X[fx].view(np.uint64), PX.f64(r64["X_start"])[fx].view(np.uint64))      # fixed vertices: bit for bit
    assert not bad, bad


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", COMPARED)
def test_exact_properties(pkg, hip, name, solver):
    case, _, _, _ = C.runs(name)
    Xa, sa, ta = _dev(pkg, case, solver, 3, extra_vertex=True)
    Xb, sb, tb = _dev(pkg, case, solver, 3, extra_vertex=True)
    assert np.array_equal(Xa.view(np.uint64), Xb.view(np.uint64)) and ta == tb and sa["chi2_final"] == sb["chi2_final"]      # two calls: the same bits
    keep = np.concatenate([case["fixed"].astype(bool), [True]])      # fixed vertices (the initial guess leaves them too) and the untouched one: bit for bit
    assert np.array_equal(Xa[keep][:-1].view(np.uint64), case["pose"][keep[:-1]].view(np.uint64))
    assert np.array_equal(Xa[-1], np.concatenate([np.eye(3).ravel(), [7.0, 8.0, 9.0]]))
    assert not np.array_equal(Xa[~keep], case["pose"][~keep[:-1]])
