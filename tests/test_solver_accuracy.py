"""Every form of the reduced-camera solve against an extended-precision solution of the system the device itself built, in the
diagonal-scaled norm E_D of tests/solver_ref.py.

(a) windows (tests/solver_cases.py): the chain elimination in front of the plain dense factorisation with and without the explicit L^-T,
    the multi-chain factorisation with two / four / nested chains, the two-ended in-LDS band solver, and the pose system factored as it is.
    Two assertions per case:
      1. E_D(device) <= n u kappa_s(H)                            — the a-priori forward bound of an fp64 Cholesky, fixed;
      2. E_D(device) <= 32 x max(E_D(oracle), CPU solvers)        — 32: the largest ratio seen between two CORRECT fp64 solvers on such
         systems was 22; a margin over the reference, not over the device.
    Each case also asserts that the plan it was chosen for is the one that ran (debug_get "solver_plan"), and the last test that the sweep
    reached every plan kind.
(b) plba_dense_solve on graded and block-tridiagonal matrices at sizes around the tile and path boundaries, with the same two assertions
    (the CPU solvers alone are the reference), and the non-positive pivot at five positions.
The tile factorisation on its own is tests/test_factor32_tile.py."""
import numpy as np
import pytest

from tests import solver_cases as C
from tests import solver_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 32.0
_SEEN = {}


def _system(g, P):
    return g.debug_get("Hschur").reshape(P, P).copy(), g.debug_get("bschur").copy()


@pytest.mark.parametrize("name,sh,opts,expected", C.CASES, ids=[c[0] for c in C.CASES])
def test_window_solve(pkg, orc, hip, name, sh, opts, expected):
    ref = C.oracle_reference(pkg, orc, sh)
    assert ref["omega"] <= R.RESIDUAL_MAX
    lam, P = sh[2], ref["P"]
    g = pkg.new_problem(**opts); g.upload_window(ref["w"])
    g.debug_build(lam, False)
    assert int(g.debug_get("pose_dim")[0]) == P
    H0, b0 = _system(g, P)
    g.debug_build(lam, True)
    plan = g.debug_get("solver_plan").copy()
    assert g.debug_get("solver_ok")[0] == 1
    x = g.debug_get("x")[:P].copy()
    if plan[0] == 0:
        # the pose system is factored where it stands (the trailing updates go back into it): the system is the one read before the solve
        H, b = H0, b0
    else:
        # the chain elimination writes a compact system of its own: the pose system is intact after the solve, and it is the one solved
        H, b = _system(g, P)
        d = np.sqrt(np.diag(H))
        drift = np.abs(H - H0).max() if np.array_equal(H, H0) else (np.abs(H - H0) / np.outer(d, d)).max()
        assert drift <= 64 * R.U, "the pose system read after the solve is not the one built: %.2e" % drift      # (atomic sums may reorder)
    g.close()
    xref, om = R.refine(H, b)
    assert om <= R.RESIDUAL_MAX, om
    E, ks = R.scaled_error(x, xref, H), R.kappa_s(H)
    bnd, refE = P * R.U * ks, max(ref["E"], ref["cpu"])
    _SEEN[name] = plan
    print("%s: plan %s | E_D %.2e, n u kappa_s %.2e, oracle %.2e, cpu solvers %.2e, ratio to reference %.1f" % (
        name, [int(v) for v in plan], E, bnd, ref["E"], ref["cpu"], E / refE))
    # the plan the case is there for
    assert int(plan[0]) == expected["form"], (name, plan)
    for key, idx in (("ninv", 2), ("hbt", 3)):
        if key in expected:
            assert int(plan[idx]) == expected[key], (name, key, plan)
    assert plan[3] >= expected.get("hbt_min", -1), (name, plan)
    assert E <= bnd, "assertion 1: E_D %.3e > n u kappa_s %.3e" % (E, bnd)
    assert E <= MARGIN * refE, "assertion 2: E_D %.3e > %g x %.3e" % (E, MARGIN, refE)


def test_every_plan_kind_was_reached():
    """runs after the sweep (same module, file order): every case ran, and together they reached every plan kind"""
    assert set(_SEEN) == {c[0] for c in C.CASES}, sorted({c[0] for c in C.CASES} - set(_SEEN))
    reached = {}
    for name, plan in _SEEN.items():
        for k in C.plan_kinds(plan):
            reached.setdefault(k, []).append(name)
    for k in sorted(reached):
        print("%-45s %s" % (k, " ".join(reached[k])))
    assert C.REQUIRED_KINDS <= set(reached), sorted(C.REQUIRED_KINDS - set(reached))
    assert "band, T odd" not in reached and all(int(plan[1]) % 2 == 0 for plan in _SEEN.values() if plan[0] >= 2)      # see solver_cases.REQUIRED_KINDS
    T = {name: int(plan[1]) for name, plan in _SEEN.items()}
    dflt = [T["K%d" % K] for K in C.SIZES]
    # the thresholds are straddled by default-option cases: under 8 tiles, NINV_MAX_T = 32, TWIN_MAX_TILES = 64
    assert min(dflt) < 8 and any(t <= 32 for t in dflt) and any(32 < t <= 64 for t in dflt) and max(dflt) > 64, dflt


# ---- (b) the direct entry -------------------------------------------------------------------------------------------------------------------
SIZES = [31, 32, 33, 95, 96, 97, 383, 384, 385, 1023, 1024, 1025, 1056, 1500]
OPTS = [(1, 32, 0, 1), (1, 32, 0, 0), (1, 32, 1, 0), (0, 32, 0, 0), (1, 64, 0, 0), (0, 64, 0, 0)]      # test_dense_solver_vs_numpy's
KINDS = ["graded0", "graded3", "graded6", "blocktri"]
_MAT = {}


def _matrix(n, kind):
    if (n, kind) not in _MAT:
        A, b = R.block_tridiagonal_spd(n, 7 * n) if kind == "blocktri" else R.graded_spd(n, int(kind[6:]), 7 * n)
        xref, om = R.refine(A, b)
        _MAT[(n, kind)] = (A, b, xref, om, n * R.U * R.kappa_s(A), R.cpu_solvers(A, b, xref))
    return _MAT[(n, kind)]


@pytest.mark.parametrize("mfma,fb,flow,wide", OPTS)
@pytest.mark.parametrize("n", SIZES)
def test_dense_entry_accuracy(pkg, hip, n, mfma, fb, flow, wide):
    p = pkg.new_problem(use_mfma=mfma, factor_block=fb, factor_flow=flow, wide_steps=wide)
    bad = []
    for kind in KINDS:
        A, b, xref, om, bnd, cpu = _matrix(n, kind)
        assert om <= R.RESIDUAL_MAX, om
        x, ok = p.debug_dense_solve(A, b)
        assert ok, kind
        E = R.scaled_error(x, xref, A)
        print("n %d %s (%d %d %d %d): E_D %.2e, n u kappa_s %.2e, cpu solvers %.2e, ratio %.1f" % (n, kind, mfma, fb, flow, wide, E, bnd, cpu, E / cpu))
        if not E <= bnd:
            bad.append("assertion 1, %s: E_D %.3e > n u kappa_s %.3e" % (kind, E, bnd))
        if not E <= MARGIN * cpu:
            bad.append("assertion 2, %s: E_D %.3e > %g x %.3e" % (kind, E, MARGIN, cpu))
    p.close()
    assert not bad, bad


@pytest.mark.parametrize("mfma,fb,flow,wide", OPTS)
@pytest.mark.parametrize("n", SIZES)
def test_dense_entry_reports_a_non_positive_pivot(pkg, hip, n, mfma, fb, flow, wide):
    """one diagonal entry made negative at row 0, 31, 32, n / 2 and the last row: the factorisation reports it through the control block"""
    A0, b = _matrix(n, "graded0")[:2]
    p = pkg.new_problem(use_mfma=mfma, factor_block=fb, factor_flow=flow, wide_steps=wide)
    for row in sorted({0, min(31, n - 1), min(32, n - 1), n // 2, n - 1}):
        A = A0.copy(); A[row, row] = -1.0
        _, ok = p.debug_dense_solve(A, b)
        assert not ok, (n, row)
    _, ok = p.debug_dense_solve(A0, b)      # ... and the handle is good for a sound system afterwards
    assert ok
    p.close()
