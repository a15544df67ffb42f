"""The reference and the inputs of tests/test_solver_accuracy.py, pinned without a GPU: refine() on systems with known solutions, and the
oracle's own solve of every window shape of the sweep inside the a-priori bound n u kappa_s in the diagonal-scaled norm (tests/solver_ref.py).
A device failure on the sweep can then not be blamed on the helper or on inputs for which no fp64 Cholesky would meet the bound."""
from fractions import Fraction

import numpy as np
import pytest

from tests import solver_cases as C
from tests import solver_ref as R

LD = np.longdouble


def _rhs_extended(H, x0):
    """b = H x0 for integer-valued H and x0 given as fractions p / q with a common denominator q: exact integers, then one division"""
    q = x0[0].denominator
    assert all(v.denominator in (1, q) or q % v.denominator == 0 for v in x0)
    num = [int(v * q) for v in x0]
    return [sum(int(h) * p for h, p in zip(row, num)) for row in H], q


@pytest.mark.parametrize("kind", ["hilbert", "graded"])
def test_refine_known_rational_solution(kind):
    """H with integer entries, x0 rational: b = H x0 computed exactly and rounded ONCE to fp64 would already differ from H x0 by more than
    the refinement resolves, so b is chosen representable: x0 = p / 2^k with small p makes H x0 exact in fp64."""
    n = 7
    if kind == "hilbert":      # the Hilbert matrix times lcm(1 .. 2n - 1): integer entries, condition number 5e8
        lcm = int(np.lcm.reduce(np.arange(1, 2 * n)))
        H = np.array([[lcm // (i + j + 1) for j in range(n)] for i in range(n)], dtype=object)
    else:                      # D (B B^T + I) D with integer B and D = diag(1, 10, .., 10^8): condition number beyond 1e16, kappa_s small
        rng = np.random.default_rng(5)
        B = rng.integers(-3, 4, size=(n, n))
        G = B @ B.T + np.eye(n, dtype=np.int64)
        H = np.array([[int(G[i, j]) * 10 ** (i + j) for j in range(n)] for i in range(n)], dtype=object)
    x0 = [Fraction((-1) ** i * (3 * i + 1), 64) for i in range(n)]
    b_int, q = _rhs_extended(H, x0)
    Hf = np.array(H, dtype=np.float64)
    assert all(int(Hf[i, j]) == H[i, j] for i in range(n) for j in range(n))      # H is exact in fp64
    b = np.array([Fraction(v, q) for v in b_int], dtype=np.float64)
    assert all(Fraction(float(b[i])) == Fraction(b_int[i], q) for i in range(n))  # ... and so is b
    x, om = R.refine(Hf, b)
    assert om <= R.RESIDUAL_MAX, om
    xe = np.array([LD(v.numerator) / LD(v.denominator) for v in x0])
    err = R.scaled_error(x, xe, Hf)
    # refinement with residuals in precision eps_r leaves a forward error of (condition) x eps_r: with long double, 2^-64, that is 2^-11 of
    # what the tests allow an fp64 solver (n u kappa_s); the constant 8 is the margin the bound's "modest constant" gets here
    plain = float(np.max(np.abs(np.linalg.solve(Hf, b) - xe.astype(np.float64)) / np.abs(xe.astype(np.float64))))
    print("%s: refined %.2e, numpy.linalg.solve %.2e, omega %.1e, kappa_s %.2e" % (kind, err, plain, om, R.kappa_s(Hf)))
    assert err <= 8 * n * 2.0 ** -64 * R.kappa_s(Hf), (err, R.kappa_s(Hf))


def test_scaled_error_weighs_small_variables():
    H = np.diag([1e10, 1e2]); xref = np.array([1e-7, 0.1])
    assert R.scaled_error(xref * [1.01, 1.0], xref, H) == pytest.approx(0.01 * 1e-2 / 1.0, rel=1e-6)      # 1 % of the bias entry: seen
    assert np.abs(xref * [1.01, 1.0] - xref).max() / np.abs(xref).max() < 1e-7                           # ... and invisible in the max-norm
    assert R.kappa_s(np.diag([1e10, 1e2])) == pytest.approx(1.0)


def test_synthetic_matrices_are_what_they_claim():
    for g in (0, 3, 6):
        A, b = R.graded_spd(97, g, 1)
        assert R.kappa_s(A) < 10 and np.linalg.cond(A) > 10.0 ** (2 * g) / 10
    A, b = R.block_tridiagonal_spd(1500, 1)
    assert 1e3 < R.kappa_s(A) < 3e4
    assert np.count_nonzero(A[0:15, 30:]) == 0 and np.count_nonzero(A[15:30, 0:15]) > 0


@pytest.mark.parametrize("sh", C.SHAPES, ids=C.shape_id)
def test_oracle_inside_the_bound(pkg, orc, sh):
    r = C.oracle_reference(pkg, orc, sh)
    bnd = r["P"] * R.U * r["kappa_s"]
    print("%s: P %d, omega %.1e, E_D(oracle) %.2e, cpu solvers %.2e, n u kappa_s %.2e (kappa_s %.2e)" % (C.shape_id(sh), r["P"], r["omega"], r["E"], r["cpu"], bnd, r["kappa_s"]))
    assert r["omega"] <= R.RESIDUAL_MAX
    assert r["E"] <= bnd and r["cpu"] <= bnd


def test_sweep_has_the_cases_the_issue_lists():
    names = [c[0] for c in C.CASES]
    assert len(names) == len(set(names)) and len(names) >= 40
    assert {c[1][0] for c in C.CASES} >= set(C.SIZES)
    assert {c[1][1] for c in C.CASES} >= {(2, 4), (2, 8), (6, 12)} and {c[1][2] for c in C.CASES} == {1e-4, 3.0, 1e3}
