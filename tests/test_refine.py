"""plba_refine_landmarks on the GPU: parity with tests/refine_ref.py under the tolerance rule of DESIGN.md 9 (noise = |reference in
float64 - reference in long double|; a device value passes within max(8 noise, m u |value|), m = terms of the landmark's sums; counts
exactly where every decision of the wide run is 1000 x its noise from the threshold; landmarks the two reference runs decide differently
are left out), on the smallest windows at which the kernel can go wrong; then the exact properties: the next plba_optimize sees the
refined landmarks bit for bit as a fresh upload of them would, everything else is untouched, two calls give the same bits, the closing
evaluation pass, the refusals."""
import numpy as np
import pytest

from tests import refine_ref as RR
from tests.test_refine_cpu import PARITY, WIDE, reference, window

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _problem(pkg, w, fused=False, huber=True, levels=None):
    hp = pkg.new_problem(lm_fused=2) if fused else pkg.new_problem(lm_fused=0)
    hp.upload_window(w)
    if not huber:
        hp.set_robust(0, False, 0.0); hp.set_robust(1, False, 0.0)
    if levels is not None:
        if len(levels[0]):
            hp.set_levels(0, levels[0])
        if len(levels[1]):
            hp.set_levels(1, levels[1])
    return hp


def _check(w, got, pts, lns, r64, rw, cmp, what=""):
    """the tolerance rule; returns the number of landmarks compared"""
    Np = len(w["points"])
    ref = RR.arrays(rw, Np)
    nterms = np.concatenate([np.bincount(w["po_pt"], minlength=Np) * 2, np.bincount(w["lo_ln"], minlength=len(w["lines"]))]) if Np + len(w["lines"]) else np.zeros(0)
    assert np.array_equal(got["status"] >= RR.FIXED, ref["status"] >= RR.FIXED), what      # (which landmarks are skipped is no matter of rounding)
    assert np.array_equal(got["status"][ref["status"] >= RR.FIXED], ref["status"][ref["status"] >= RR.FIXED]), what
    n = 0
    worst = 0.0
    for i in range(len(rw)):
        x = pts[i] if i < Np else lns[i - Np]
        xr = ref["points"][i] if i < Np else ref["lines"][i - Np]
        if ref["status"][i] >= RR.FIXED:
            x0 = w["points"][i] if i < Np else w["lines"][i - Np]
            assert np.array_equal(x, x0), (what, i, "a skipped landmark moved")
            continue
        if not cmp["same"][i]:
            continue
        n += 1
        noise = cmp["noise_pt"] if i < Np else cmp["noise_ln"]
        tol = max(8 * noise, nterms[i] * U * np.abs(xr).max())
        err = np.abs(x - xr).max()
        worst = max(worst, err / tol)
        assert err <= tol, (what, i, err, tol, got["status"][i], ref["status"][i])
        if cmp["exact"][i]:
            assert (got["status"][i], got["iters"][i], got["trials_per_landmark"][i]) == (ref["status"][i], ref["iters"][i], ref["trials"][i]), (what, i)
    print(what, "compared", n, "of", len(rw), "worst error / tolerance %.3f" % worst, "noise", cmp["noise_pt"], cmp["noise_ln"])
    return n


def _parity(pkg, w, r64, rw, cmp, what, fused=False, huber=True, levels=None, **kw):
    hp = _problem(pkg, w, fused, huber, levels)
    opts = dict(PARITY); opts.update(kw)
    got = hp.refine_landmarks(**opts)
    n = _check(w, got, hp.get_points(), hp.get_lines(), r64, rw, cmp, what)
    hp.close()
    return got, n


@pytest.mark.parametrize("huber", [True, False])
def test_track_lengths(pkg, hip, huber):
    """one point and one line of every track length 1 (rank-deficient: held by the damping), 2, 7, 8, 9, 15, 16, 17 and 40: at, below and
    above the 8-lane sub-group and each round of its loop"""
    kw = {} if huber else {"huber_on": False}
    w, r64, rw, cmp = reference("tracks", **kw)
    _, n = _parity(pkg, w, r64, rw, cmp, "tracks huber=%s" % huber, huber=huber)
    assert n == len(rw)


@pytest.mark.parametrize("Np,Nl", [(1, 0), (0, 1), (63, 0), (64, 0), (0, 65), (20, 17), (70, 30)])
def test_landmark_counts(pkg, hip, Np, Nl):
    """1, 63, 64, 65 landmarks and 100 (32 per workgroup: the last one partly filled); points only, lines only, and mixed with a
    workgroup that holds both kinds"""
    lens = [2 + (3 * i) % 7 for i in range(Np + Nl)]
    w = RR.hand_window(12, lens[:Np], lens[Np:], seed=100 + Np + Nl)
    r64, rw = RR.refine(w, np.float64, **PARITY), RR.refine(w, WIDE, **PARITY)
    cmp = RR.compare(r64, rw, Np)
    got, n = _parity(pkg, w, r64, rw, cmp, "counts %d + %d" % (Np, Nl))
    assert n == Np + Nl and got["n_refined"] == Np + Nl and got["n_skipped"] == 0


@pytest.mark.parametrize("K", [256, 257])
def test_camera_blocks_in_lds_and_through_l2(pkg, hip, K):
    """K at the largest count whose camera blocks are staged in LDS (REFINE_KC_LDS_MAX = 256) and one above it, a dozen landmarks"""
    w = RR.hand_window(K, [2, 3, 5, 8, 9, 12], [2, 3, 5, 8, 9, 12], seed=K)
    r64, rw = RR.refine(w, np.float64, **PARITY), RR.refine(w, WIDE, **PARITY)
    cmp = RR.compare(r64, rw, 6)
    _, n = _parity(pkg, w, r64, rw, cmp, "K = %d" % K)
    assert n == 12


@pytest.mark.parametrize("fused", [False, True])
def test_generated_window(pkg, hip, fused):
    """500 points + 100 lines over 12 keyframes, 5 % outliers far beyond the Huber delta; on both landmark storage orders"""
    w, r64, rw, cmp = reference("generated")
    got, n = _parity(pkg, w, r64, rw, cmp, "generated fused=%s" % fused, fused=fused)
    assert n >= 0.98 * len(rw)
    a = RR.arrays(rw, len(w["points"]))
    assert abs(got["chi2_before"] - a["chi2_before"].sum()) <= 1e-9 * a["chi2_before"].sum() and abs(got["chi2_after"] - a["chi2_after"].sum()) <= 1e-6 * a["chi2_after"].sum()


def test_mixed_levels(pkg, hip):
    """some observations at level 1; point 3 and line 2 with ALL of theirs at level 1: NO_OBS and untouched bits"""
    w = window("tracks")
    lp, ll = np.zeros(len(w["po_pt"]), np.uint8), np.zeros(len(w["lo_ln"]), np.uint8)
    lp[::5] = 1; ll[::4] = 1
    lp[w["po_pt"] == 3] = 1; ll[w["lo_ln"] == 2] = 1
    kw = dict(PARITY, levels_pt=lp, levels_ln=ll)
    r64, rw = RR.refine(w, np.float64, **kw), RR.refine(w, WIDE, **kw)
    cmp = RR.compare(r64, rw, len(w["points"]))
    got, _ = _parity(pkg, w, r64, rw, cmp, "levels", levels=(lp, ll))
    assert got["status"][3] == RR.NO_OBS and got["status"][len(w["points"]) + 2] == RR.NO_OBS
    assert got["n_skipped"] == int((got["status"] >= RR.FIXED).sum()) >= 2


def test_fixed_landmarks_and_select_mask(pkg, hip):
    w = dict(window("tracks"))
    Np, Nl = len(w["points"]), len(w["lines"])
    w["point_fixed"] = np.zeros(Np, np.uint8); w["point_fixed"][[1, 4]] = 1
    w["line_fixed"] = np.zeros(Nl, np.uint8); w["line_fixed"][[0]] = 1
    sp, sl = np.ones(Np, bool), np.ones(Nl, bool)
    sp[[2, 4]] = False; sl[[5]] = False
    kw = dict(PARITY, select_point=sp, select_line=sl)
    r64, rw = RR.refine(w, np.float64, **kw), RR.refine(w, WIDE, **kw)
    cmp = RR.compare(r64, rw, Np)
    hp = _problem(pkg, w)
    got = hp.refine_landmarks(select_point=sp, select_line=sl, **PARITY)
    _check(w, got, hp.get_points(), hp.get_lines(), r64, rw, cmp, "fixed / select")
    assert list(got["status"][[1, 2, 4, Np, Np + 5]]) == [RR.FIXED, RR.UNSELECTED, RR.FIXED, RR.FIXED, RR.UNSELECTED]
    hp.close()


def test_far_starts_with_two_trials(pkg, hip):
    """depth off by half, max_trials = 2: rejected-then-accepted iterations and exhausted landmarks (asserted on the reference in
    tests/test_refine_cpu.py::test_reference_conditions)"""
    w, r64, rw, cmp = reference("far", max_trials=2)
    got, n = _parity(pkg, w, r64, rw, cmp, "far", max_trials=2)
    assert n == len(rw) and got["n_exhausted"] == sum(r["status"] == RR.EXHAUSTED for r in rw) > 0


def _state(hp):
    k = hp.get_keyframes()
    return dict(k, points=hp.get_points(), lines=hp.get_lines())


def _same_state(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key, np.abs(a[key] - b[key]).max())


def _with_state(w, st):
    w = dict(w)
    w["kf"] = dict(w["kf"]); w["kf"].update({k: st[k] for k in ("P", "V", "q", "dbg", "dba")})
    w["points"], w["lines"] = st["points"], st["lines"]
    return w


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("slid", [False, True])
def test_next_optimize_sees_the_refined_landmarks(pkg, hip, fused, slid):
    """After a refine: plba_optimize(5) on the handle == a fresh handle given the same window with the refined landmarks through
    plba_set_*, then plba_optimize(5) — poses, landmarks and trace bit for bit (a stale landmark copy would show here).  On a freshly
    uploaded window and on a slid one (refining the added landmarks only), record-based and with the fused passes' grouped storage."""
    W = pkg.window
    K = 12
    seq = W.make_sequence(K, 2, 400, 80, seed=0x5EED0C00 + fused, kf_dt=0.1)
    w0 = W.window_at(seq, 0, K)
    a = pkg.new_problem(lm_fused=fused)
    a.upload_window(w0)
    w, sel = w0, {}
    if slid:
        a.optimize(5)
        w = W.window_at(seq, 1, K, prev=w0)
        pm, lm = a.slide_window(W.slide_delta(w0, w))
        for kind, d in w["huber"].items():
            a.set_robust(kind, True, d)
        nstay_p, nstay_l = int((pm >= 0).sum()), int((lm >= 0).sum())
        sel = dict(select_point=np.arange(len(w["points"])) >= nstay_p, select_line=np.arange(len(w["lines"])) >= nstay_l)
        assert sel["select_point"].any() and sel["select_line"].any()
    before = _state(a)
    got = a.refine_landmarks(**sel)
    assert int(a.debug_get("lm_fused")[0]) == (1 if fused else 0)
    mid = _state(a)
    moved_p, moved_l = np.any(mid["points"] != before["points"], 1), np.any(mid["lines"] != before["lines"], 1)
    assert moved_p.any() and moved_l.any()
    if slid:
        assert not moved_p[~sel["select_point"]].any() and not moved_l[~sel["select_line"]].any()
    for key in ("P", "V", "q", "dbg", "dba"):
        assert np.array_equal(mid[key], before[key])
    b = pkg.new_problem(lm_fused=fused)
    b.upload_window(_with_state(w, mid))
    sa, sb = a.optimize(5), b.optimize(5)
    assert (sa.iterations, sa.trials, sa.chi2_initial, sa.chi2_final) == (sb.iterations, sb.trials, sb.chi2_initial, sb.chi2_final)
    _same_state(_state(a), _state(b), "after optimize")
    assert a.trace() == b.trace() and len(a.trace()) > 0
    assert got["n_refined"] > 0
    a.close(); b.close()


def test_everything_else_is_untouched_and_two_calls_agree(pkg, hip):
    w = window("generated")
    W = pkg.window
    res = []
    for rep in range(2):
        hp = pkg.new_problem()
        hp.upload_window(w)
        hp.optimize(3)
        prior = hp.marginalize_to_prior(0, pkg.protocol.MARG_NUM)
        assert prior["n"] > 0
        hp.gate_outliers(W.CHI2_GATE)
        hp.save_state()
        kf0, lv0, pr0 = hp.get_keyframes(), (hp.get_levels(0), hp.get_levels(1)), hp.get_prior()
        saved = _state(hp)
        got = hp.refine_landmarks()
        res.append((got, hp.get_points(), hp.get_lines()))
        kf1, lv1, pr1 = hp.get_keyframes(), (hp.get_levels(0), hp.get_levels(1)), hp.get_prior()
        for k in kf0:
            assert np.array_equal(kf0[k], kf1[k]), k
        assert np.array_equal(lv0[0], lv1[0]) and np.array_equal(lv0[1], lv1[1])
        for k in ("vid", "size", "idx", "x0", "J0", "r0", "Ar", "br"):
            assert np.array_equal(pr0[k], pr1[k]), k
        # the closing pass: the cached per-edge chi2 is that of the state the call left
        c_pt, c_ln = hp.edge_chi2(0)[0], hp.edge_chi2(1)[0]
        hp.recompute_errors()
        assert np.array_equal(c_pt, hp.edge_chi2(0)[0]) and np.array_equal(c_ln, hp.edge_chi2(1)[0])
        assert not np.array_equal(hp.get_points(), saved["points"])
        hp.restore_state()
        _same_state(_state(hp), saved, "restore_state")
        # the arrays and the totals of one call agree with each other
        st, it, tr = got["status"], got["iters"], got["trials_per_landmark"]
        refined = st <= RR.NONFINITE
        assert got["n_refined"] == refined.sum() and got["n_skipped"] == (~refined).sum() and got["n_exhausted"] == (st == RR.EXHAUSTED).sum()
        assert got["iterations"] == it[refined].sum() and got["trials"] == tr[refined].sum() and not it[~refined].any() and not tr[~refined].any()
        assert got["chi2_after"] <= got["chi2_before"]
        hp.close()
    (g0, p0, l0), (g1, p1, l1) = res
    assert np.array_equal(p0, p1) and np.array_equal(l0, l1)
    for k in ("status", "iters", "trials_per_landmark"):
        assert np.array_equal(g0[k], g1[k])
    assert (g0["chi2_before"], g0["chi2_after"], g0["iterations"], g0["trials"]) == (g1["chi2_before"], g1["chi2_after"], g1["iterations"], g1["trials"])


def test_refusals_leave_the_window_usable(pkg, hip):
    abi = pkg.abi
    w = window("tracks")
    hp = pkg.new_problem()
    with pytest.raises(abi.PlbaError, match="nothing uploaded"):
        hp.refine_landmarks()
    hp.upload_window(w)
    p0 = hp.get_points()
    for bad in (dict(max_iters=0), dict(max_trials=0), dict(lambda_init=0.0), dict(lambda_init=-1.0), dict(lambda_init=float("nan"))):
        with pytest.raises(abi.PlbaError, match="PLBA_ERR_INVALID"):
            hp.refine_landmarks(**bad)
        assert np.array_equal(hp.get_points(), p0)
    got = hp.refine_landmarks(**PARITY)
    assert got["n_refined"] == len(w["points"]) + len(w["lines"])
    sh = pkg.new_problem()
    sh.upload_window(w)
    sh.set_shard(0, 2, lambda buf, n, op, stream: None)
    with pytest.raises(abi.PlbaError, match="sharded"):
        sh.refine_landmarks()
    sh.set_shard(0, 1, lambda buf, n, op, stream: None)
    assert sh.refine_landmarks(**PARITY)["n_refined"] == got["n_refined"]
    assert np.array_equal(sh.get_points(), hp.get_points())
    hp.close(); sh.close()
