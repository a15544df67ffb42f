"""The exact marginal-covariance rules without a GPU: the fp64 reference of tests/marginals_ref.py held to the three rules of
tests/marginals_exact.py on every case of tests/marginals_cases.py, and mutations of its output that every rule must catch.

What this shows: the reference alone stays inside each tolerance (so a device failure is the device's), every residual precondition
holds on these inputs, the constant C_INV of assertion (b)1 has the derivation its docstring gives, and the direct Hpp pins the one
marginals_ref recovers through the damped Schur complement.  Run with -s for the figures."""
import numpy as np
import pytest

from tests import marginals_cases as C
from tests import marginals_exact as X
from tests import solver_ref as R
from tests.test_marginals import _close, _kf_blockwise

# Assertion (b)1, E <= C_INV n u kappa_s(S).  For a solve the solver tests use 1.  An inverse is held to the smallest power of two under which
# the three correct fp64 inverses of assertion (b)2 stay within a factor 4 on every case (test_reference_within_rules asserts it): their
# largest E / (n u kappa_s) over the cases is 7.7 (np.linalg.inv at P66, whose row pivoting is not invariant under the diagonal scaling;
# the two Cholesky inverses stay under 0.4), and 4 x 7.7 = 31 -> 32.  Decided on the CPU reference, before any device run.
C_INV = 32.0


def symmetric(S):
    """the lower triangle in both, as k_cov_init / k_cov_pairs leave the device's S"""
    return np.tril(S) + np.tril(S, -1).T


def old_tolerance(S):
    """tests/test_marginals.py's: max(1e-9, kappa(S) 1e-14)"""
    return max(1e-9, np.linalg.cond(S) * 1e-14)


@pytest.mark.parametrize("name", C.NAMES)
def test_reference_within_rules(pkg, orc, name):
    c = C.prepare(pkg, orc, name)
    ex, res = c["ex"], c["res64"]
    assert c["omega"] <= R.RESIDUAL_MAX
    # the recovered Hpp against the direct one (both lambdas), as test_marginals_cpu holds the two lambdas against each other
    hmax = float(np.abs(X.narrow(ex.Hpp)).max())
    rec = max(float(np.abs(X.narrow(X.wide(H) - ex.Hpp)).max()) for H in c["Hs"]) / hmax
    assert rec <= 1e-10, rec
    # (a) the fp64 S: its noise is the rule's own yardstick, so its ratio is 1 / FACTOR wherever the m u floor does not lead
    ra, noise_a, _ = X.rule_S(res["S"], res["S"], ex)
    assert ra <= 1.0 and noise_a < 1e-11      # (8 x the noise stays under the 1e-10 d_i d_j of the mutation below on every case)
    # (b) the three fp64 inverses of the (symmetric) fp64 S against its extended inverse
    S = symmetric(res["S"])
    ext, om = X.inverse_ext(S, c["cols"])
    assert om <= R.RESIDUAL_MAX
    rb = X.rule_inverse(np.linalg.inv(S), S, ext, C_INV)
    assert rb["E"] <= rb["bound"] and rb["E"] <= X.MARGIN * rb["cpu"]
    assert max(rb["each"]) <= rb["bound"] / 4, (rb["each"], rb["bound"])      # C_INV's derivation
    # (c) the fp64 landmark covariances
    rc, noise_c, _ = X.rule_landmarks(res["cov"], c["cov_ref"], c["formulas"], X.landmark_terms(ex))
    assert rc <= 1.0
    st = np.bincount(ex.status, minlength=4)
    print("%-10s P %4d kappa_s %.2e | Hpp recovered - direct %.1e | (a) fp64 noise %.2e ratio %.2f | (b) E / (n u kappa_s): inv %.3f chol %.3f "
          "reversed %.3f, omega %.1e | (c) fp64 noise %.2e ratio %.2f over %d landmarks | statuses %s, pivot margin %.1e" % (
              name, ex.P, rb["kappa_s"], rec, noise_a, ra, *(e * C_INV / rb["bound"] for e in rb["each"]), max(om, c["omega"]), noise_c, rc,
              len(c["cov_ref"]), [int(v) for v in st], ex.pivot_margin()))


def test_direct_hpp_pins_the_recovered_one(pkg, orc):
    """a wrong entry of either shows: the recovered Hpp carries its cancellation (1e-12 at the all-bias-fixed window), the direct one none"""
    c = C.prepare(pkg, orc, "mixed")
    H = X.narrow(c["ex"].Hpp)
    assert np.abs(c["Hs"][0] - H).max() <= 1e-10 * np.abs(H).max()
    bad = c["Hs"][0].copy()
    bad[np.unravel_index(np.abs(H).argmax(), H.shape)] *= 1 + 1e-8
    assert np.abs(bad - H).max() > 1e-10 * np.abs(H).max()


# ---- mutations -------------------------------------------------------------------------------------------------------------------------------------
def _mutation_setup(pkg, orc):
    """P195, thirteen free keyframes: kappa(S) = 5e8, so the old tolerance is 5e-6 there (and 3e-4 at 150 keyframes)"""
    c = C.prepare(pkg, orc, "P195")
    ex, res = c["ex"], c["res64"]
    S = symmetric(res["S"])
    ext, _ = X.inverse_ext(S, c["cols"])
    return c, ex, res, S, ext, np.linalg.inv(S), old_tolerance(S)


def _passes(fn, *a):
    try:
        fn(*a)
        return True
    except AssertionError:
        return False


def test_mutation_bias_block_scaled(pkg, orc):
    """one bias-bias sub-block of Sigma_pp times 1 + 1e-6.  NEW: fails (b).  OLD: passed — _kf_blockwise floors the sub-block's scale at
    1e-3 of the 15 x 15 block's largest entry, a position variance orders above the bias variances."""
    c, ex, res, S, ext, Sig, tol = _mutation_setup(pkg, orc)
    ref = ex.ref
    o = ref.ob_off[1]
    bad = Sig.copy()
    bad[o:o + 6, o:o + 6] *= 1 + 1e-6
    good, r = X.rule_inverse(Sig, S, ext, C_INV), X.rule_inverse(bad, S, ext, C_INV)
    assert good["E"] <= good["bound"] and good["E"] <= X.MARGIN * good["cpu"]
    assert r["E"] > r["bound"] and r["E"] > X.MARGIN * r["cpu"]
    gmax = np.abs(c["out64"]["kf"]).max()
    assert _passes(_kf_blockwise, [ref.block(bad, 1, 1)], [ref.block(Sig, 1, 1)], tol, gmax)


def test_mutation_coupling_term_dropped(pkg, orc):
    """one landmark's covariance without its coupling term, B Hr^-1 B^T alone.  NEW: fails (c).  OLD: caught as well (the term is a large part
    of the covariance) — asserted here so that the statement is checked, not remembered."""
    c, ex, res, S, ext, Sig, tol = _mutation_setup(pkg, orc)
    i = next(i for i, red in enumerate(ex.red) if red is not None and len(red[2]) >= 2)
    B, Hi, _ = ex.red[i]
    cov = list(res["cov"])
    cov[i] = X.narrow(B @ Hi @ B.T)
    assert X.rule_landmarks(res["cov"], c["cov_ref"], c["formulas"], X.landmark_terms(ex))[0] <= 1.0
    assert X.rule_landmarks(cov, c["cov_ref"], c["formulas"], X.landmark_terms(ex))[0] > 1.0
    assert not _passes(_close, cov[i], res["cov"][i], tol)


def test_mutation_pair_rows_swapped(pkg, orc):
    """dv and dphi rows of one pair block exchanged (a wrong pmap / kf_dim).  NEW: fails the bit-for-bit comparison of the returned blocks
    with the entries of Sigma_pp.  OLD: caught as well, the rows differ by far more than the tolerance."""
    c, ex, res, S, ext, Sig, tol = _mutation_setup(pkg, orc)
    ref = ex.ref
    blocks = [ref.block(Sig, i, j) for i, j in c["pairs"]]
    assert X.gather_mismatches(blocks, Sig, ref, c["pairs"]) == []
    bad = [b.copy() for b in blocks]
    bad[0][[3, 4, 5, 6, 7, 8]] = bad[0][[6, 7, 8, 3, 4, 5]]
    assert X.gather_mismatches(bad, Sig, ref, c["pairs"]) == [0]
    assert not _passes(_kf_blockwise, [bad[0]], [blocks[0]], tol, np.abs(c["out64"]["kf"]).max())


def test_mutation_entry_of_S(pkg, orc):
    """one entry of S (and its mirror) off by 1e-10 d_i d_j: a wrong Schur term of k_cov_pairs.  NEW: fails (a).  OLD: passed — the covariances
    it leads to stay within kappa 1e-14 of the reference's, the inverse being compared, not what was inverted."""
    c, ex, res, S, ext, Sig, tol = _mutation_setup(pkg, orc)
    ref = ex.ref
    i, j = ref.op_off[1] + 7, ref.op_off[1] + 1
    bad = res["S"].copy()
    bad[i, j] += 1e-10 * float(ex.d[i] * ex.d[j]); bad[j, i] = bad[i, j]
    assert X.rule_S(res["S"], res["S"], ex)[0] <= 1.0
    assert X.rule_S(bad, res["S"], ex)[0] > 1.0
    badSig = np.linalg.inv(symmetric(bad))
    gmax = np.abs(c["out64"]["kf"]).max()
    K = ref.K
    assert _passes(_kf_blockwise, [ref.block(badSig, k, k) for k in range(K)], [ref.block(Sig, k, k) for k in range(K)], tol, gmax)


def test_wide_switch_mpmath(pkg, orc, monkeypatch):
    """the mpmath side of the switch (taken where long double is no wider than a double) builds the same S on the smallest case"""
    if not R.LD_IS_EXTENDED:
        return      # it is the side every other test here has taken
    c = C.prepare(pkg, orc, "P9")
    op = C.oracle_problem(orc, c)
    monkeypatch.setattr(R, "LD_IS_EXTENDED", False)
    ex = X.Exact(op, c["w"], C.robust_of(c["w"]))
    monkeypatch.undo()
    op.close()
    assert np.array_equal(ex.status, c["ex"].status)
    d = X.narrow(np.outer(c["ex"].d, c["ex"].d))
    assert (np.abs(np.array(ex.S, dtype=np.float64) - X.narrow(c["ex"].S)) / d).max() <= 4 * R.U
