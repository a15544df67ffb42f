"""plba_compute_marginals against the extended-precision reference of tests/marginals_exact.py, stage by stage, on the cases of
tests/marginals_cases.py and on both landmark storages.  The device's own intermediate results come through options.diag bit
PLBA_DIAG_COV_DUMP (plba_debug_get "cov_S", "cov_Sigma").

(a) the device's S against S_ref, entrywise relative to d_i d_j (d^2 the diagonal of the absolutely accumulated S): tolerance
    max(8 x the fp64 reference's own noise in that measure, m u) for an entry of m products — the rule of the pre-init visual BA tests.
(b) the device's Sigma_pp against the extended inverse of the device's OWN S (the factorisation, k_cov_nlast, k_cov_syrk alone), in
        E = max_ij d_i d_j |Sig_ij - Sigma_ij| / max_ij d_i d_j |Sigma_ij|,   d = sqrt(diag S):
      1. E <= C_INV n u kappa_s(S), C_INV = 32 (tests/test_marginals_exact_cpu.py: derived and asserted there on the CPU inverses);
      2. E <= 32 x the largest E of three correct fp64 inverses of the same S (MARGIN of the solver tests);
    every column up to P = 256, beyond it the first and last tile and two columns either side of each tile boundary.  Sigma_pp is exactly
    symmetric, and the keyframe / pair blocks the call returns are bit for bit its entries (k_cov_gather, kf_dim), zeros at fixed vertices.
(c) Sigma_ll against Sigma_ll_ref per landmark, relative to its own largest entry: tolerance max(8 x noise, m u), the noise the larger of
    the reference's two fp64 formulas (Schur form, dense inverse) against the extended one.  Statuses equal; NaN exactly at status 2 / 3,
    zero at 1.
With the dump bit the reported covariances keep their bits, and without it the call blocks once, as before.  Run with -s for the figures."""
import numpy as np
import pytest

from tests import marginals_cases as C
from tests import marginals_exact as X
from tests import solver_ref as R
from tests.test_marginals_exact_cpu import C_INV

pytestmark = pytest.mark.gpu

DUMP = 16      # PLBA_DIAG_COV_DUMP
_EXT = {}      # the extended inverse of a device S, shared between the storages where they build the same bits
_DEVICE_ERROR = []      # a library error in one case: the cases after it do not touch the device again


def _guarded(pkg, fn, *a, **k):
    if _DEVICE_ERROR:
        pytest.fail("not run: an earlier case ended in a library error (%s)" % _DEVICE_ERROR[0])
    try:
        return fn(*a, **k)
    except pkg.abi.PlbaError as e:
        _DEVICE_ERROR.append(str(e))
        raise


def _problem(pkg, c, fused, diag):
    hp = pkg.new_problem(lm_fused_min_obs=1, diag=diag) if fused else pkg.new_problem(lm_fused=0, diag=diag)
    hp.upload_window(c["w"])
    for kind, lev in c.get("levels", {}).items():
        hp.set_levels(kind, lev)
    hp.debug_build(1.0)
    assert int(hp.debug_get("lm_fused")[0]) == (1 if fused else 0)
    return hp


def _waits(hp, pairs):
    """the result of a second call and the blocking waits it took (the first call also prepares the problem)"""
    hp.marginals(pairs=pairs)
    h0 = hp.debug_get("host_waits")[0]
    out = hp.marginals(pairs=pairs)
    return out, int(hp.debug_get("host_waits")[0] - h0)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", C.NAMES)
def test_stages(pkg, orc, hip, name, fused):
    c = C.prepare(pkg, orc, name)
    ex, ref, P = c["ex"], c["ex"].ref, c["ex"].P
    assert c["omega"] <= R.RESIDUAL_MAX
    plain = _guarded(pkg, _problem, pkg, c, fused, 0)
    want, waits_plain = _guarded(pkg, _waits, plain, c["pairs"])
    assert plain.debug_get("cov_S").size == 0 and plain.debug_get("cov_Sigma").size == 0
    plain.close()
    hp = _guarded(pkg, _problem, pkg, c, fused, DUMP)
    for kind in (0, 1):
        if len(c["w"]["po_pt"] if kind == 0 else c["w"]["lo_ln"]):
            assert np.array_equal(hp.get_levels(kind), c.get("levels", {}).get(kind, np.zeros(len(hp.get_levels(kind)), np.uint8)))
    got, waits_dump = _guarded(pkg, _waits, hp, c["pairs"])
    S = hp.debug_get("cov_S").reshape(P, P).copy()
    Sig = hp.debug_get("cov_Sigma").reshape(P, P).copy()
    hp.close()
    # the dump changes nothing that is reported, and costs its two copies only where it is asked for
    for key in ("kf", "pairs", "pt", "ln", "pt_status", "ln_status"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert got["n_excluded"] == want["n_excluded"]
    # (a)
    assert np.array_equal(S, S.T)
    ra, noise_a, err_a = X.rule_S(S, c["res64"]["S"], ex)
    # (b)
    assert np.array_equal(Sig, Sig.T)
    key = (name, S.tobytes())
    if key not in _EXT:
        _EXT.clear()
        _EXT[key] = X.inverse_ext(S, c["cols"])
    ext, om = _EXT[key]
    assert om <= R.RESIDUAL_MAX
    rb = X.rule_inverse(Sig, S, ext, C_INV)
    K = ref.K
    assert X.gather_mismatches(got["kf"], Sig, ref, [(k, k) for k in range(K)]) == []
    assert X.gather_mismatches(got["pairs"], Sig, ref, c["pairs"]) == []
    # (c)
    status = np.concatenate([got["pt_status"], got["ln_status"]])
    cov = list(got["pt"]) + list(got["ln"])
    rc, noise_c, err_c = X.rule_landmarks(cov, c["cov_ref"], c["formulas"], X.landmark_terms(ex))
    print("%-10s %s P %4d kappa_s %.2e | (a) fp64 noise %.2e device %.2e ratio %.3f | (b) E %.2e: / (C n u kappa_s) %.3f, / cpu inverses %.2f "
          "(cpu %.2e) | (c) fp64 noise %.2e device %.2e ratio %.3f over %d landmarks | statuses %s | waits %d / %d" % (
              name, "fused  " if fused else "records", P, rb["kappa_s"], noise_a, err_a, ra, rb["E"], rb["E"] / rb["bound"], rb["E"] / rb["cpu"], rb["cpu"],
              noise_c, err_c, rc, len(c["cov_ref"]), [int(v) for v in np.bincount(status, minlength=4)], waits_plain, waits_dump))
    assert np.array_equal(status, ex.status)
    for s, cv in zip(status, cov):
        assert np.isnan(cv).all() if s >= 2 else (not np.isnan(cv).any() and (s == 0 or not cv.any()))
    assert got["n_excluded"] == (int((got["pt_status"] >= 2).sum()), int((got["ln_status"] >= 2).sum()))
    assert waits_plain == 1 and waits_dump == 3, (waits_plain, waits_dump)
    assert ra <= 1.0, "(a): S off by %.3e d_i d_j, %.2f x the tolerance (fp64 noise %.3e)" % (err_a, ra, noise_a)
    assert rb["E"] <= rb["bound"], "(b)1: E %.3e > %g n u kappa_s = %.3e" % (rb["E"], C_INV, rb["bound"])
    assert rb["E"] <= X.MARGIN * rb["cpu"], "(b)2: E %.3e > %g x %.3e" % (rb["E"], X.MARGIN, rb["cpu"])
    assert rc <= 1.0, "(c): Sigma_ll off by %.3e, %.2f x the tolerance (fp64 noise %.3e)" % (err_c, rc, noise_c)
    if name == "landmarks":      # a landmark seen from fixed keyframes only: no coupling term, whatever Sigma_pp holds
        for kind in (0, 1):
            i = c["tag"]["fixed_kf_only_%d" % kind] + kind * ref.Np
            B, Hi, W = ex.red[i]
            assert W == [] and status[i] == 0
