"""plba_track_pose on the device against the wide run of tests/track_ref.py, under lba_ref.hold's rule: DT, T_opt, H, cov, cov_eig, err
and the cut's statistics within 8 x the float64 reference's own rounding noise (floor m u |value|, m the inlier features), masks, counts,
pass counts, path, status and good exactly.  tests/test_track_cpu.py asserts that every case has the margin an exact comparison needs and
that its noise sample is representative: how the seeds of tests/track_cases.py were chosen."""
import ctypes as C

import numpy as np
import pytest

from . import track_cases as TC
from . import track_ref as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _hold(prob, name):
    case, r64, rw = TC.runs(name)
    out = TC.call(prob, [case], case["opts"])
    TR.hold(TC.as_result(out, 0), r64, rw, "hip", name)
    return case, out, rw


@pytest.mark.parametrize("name", [n for n in sorted(TC.CASES) if n.startswith("size_")] + ["duplicates"])
def test_feature_counts_around_the_wave(prob, name):
    """(12, 0), (0, 12), 63 / 64 / 65 points, mixed sizes up to (300, 100), an even and an odd count per kind for the n / 2 index, and
    duplicated residuals around the median; the line cases take every branch and every outcome of lineSegmentOverlap"""
    case, out, rw = _hold(prob, name)
    assert out["path"][0] == TR.REFINED and out["good"][0] == 1


@pytest.mark.parametrize("name", ["outliers", "outliers_t0", "masked", "fed_back"])
def test_cut_and_refinement_from_the_start_pose(prob, name):
    case, out, rw = _hold(prob, name)
    assert out["path"][0] == TR.REFINED
    assert 0 < out["n_inliers_pt"][0] < len(case["P3"]) and 0 < out["n_inliers_ln"][0] < len(case["pq"])
    assert out["n_inliers_pt"][0] == out["pt_inlier"][0].sum() and out["n_inliers_ln"][0] == out["ln_inlier"][0].sum()
    if name in ("masked", "fed_back"):      # an unflagged feature stays unflagged, and the statistics ran over all features: the reference's do
        assert not (out["pt_inlier"][0] & ~case["pt_in"]).any() and not (out["ln_inlier"][0] & ~case["ln_in"]).any()


def test_refinement_starts_from_t0_not_from_the_first_stage(prob):
    """:374 passes DT, not DT_.  With no refinement pass allowed the pose the refinement started from comes back untouched: it is T0 bit
    for bit, and the first stage had moved away from it (the same problem with the refinement on ends elsewhere)"""
    case, out, rw = _hold(prob, "outliers_ref0")
    assert out["path"][0] == TR.REFINED and out["iters"][0, 0] >= 2 and out["iters"][0, 1] == 0 and out["status"][0] == TR.RANK
    assert np.array_equal(out["T_opt"][0], case["T0"])
    full = TC.call(prob, [case], {})
    assert full["good"][0] == 1 and not np.array_equal(full["T_opt"][0], case["T0"])
    assert np.array_equal(full["pt_inlier"][0], out["pt_inlier"][0]) and np.array_equal(full["ln_inlier"][0], out["ln_inlier"][0])
    for k in ("pt_mean", "pt_stdv", "ln_mean", "ln_stdv"):      # the cut ran at the first stage's pose in both
        assert full[k][0] == out[k][0] and out[k][0] > 0


@pytest.mark.parametrize("name", ["poor_start", "iters_0", "negdet", "collinear3", "iters_0_both"])
def test_robust_fallback(prob, name):
    case, out, rw = _hold(prob, name)
    assert out["path"][0] == TR.ROBUST and not out["pt_mean"][0] and not out["ln_stdv"][0]
    if name == "negdet":      # :502-504: the pose restored, err = -1, DT_cov = I
        assert np.array_equal(out["T_opt"][0], case["T0"]) and out["err"][0] == -1.0 and np.array_equal(out["cov"][0], np.eye(6)) and out["good"][0] == 0
        assert np.array_equal(out["DT"][0], np.eye(4)) and not out["cov_eig"][0].any()
    if name in ("collinear3", "iters_0_both"):
        assert out["status"][0] == TR.RANK and out["good"][0] == 0 and not out["cov"][0].any() and out["iters"][0, 2] == 0


@pytest.mark.parametrize("name", ["few_before", "few_after"])
def test_too_few_features(prob, name):
    case, out, rw = _hold(prob, name)
    assert out["path"][0] == (TR.FEW_BEFORE if name == "few_before" else TR.FEW_AFTER)
    assert out["good"][0] == 0 and out["err"][0] == -1.0 and np.array_equal(out["DT"][0], np.eye(4)) and np.array_equal(out["T_opt"][0], np.eye(4))
    assert list(out["iters"][0, 1:]) == [0, 0] and (out["iters"][0, 0] == 0) == (name == "few_before")


def test_err_above_err_prev_breaks_after_the_step(prob):
    case, out, rw = _hold(prob, "gt_break")
    assert (1, "gt") in rw["exits"] and out["iters"][0, 1] < 10


@pytest.mark.parametrize("name", ["t0_general", "t0_identity"])
def test_start_pose(prob, name):
    case, out, rw = _hold(prob, name)
    if name == "t0_identity":      # an identity T0 is the NULL T0
        none = TC.call(prob, [dict(case, T0=None)], case["opts"])
        for k in KEYS:
            assert np.array_equal(none[k], out[k]), k


KEYS = ("DT", "T_opt", "H", "cov", "cov_eig", "err", "pt_mean", "pt_stdv", "ln_mean", "ln_stdv", "n_inliers_pt", "n_inliers_ln", "iters", "path", "status", "good")


@pytest.fixture(scope="module")
def alone(prob):
    """each default-option case called alone, once"""
    return {n: TC.call(prob, [TC.runs(n)[0]], {}) for n in TC.DEFAULT_OPTS}


@pytest.mark.parametrize("B", [1, 2, 65, 257])
def test_batch_is_the_problems_alone(prob, alone, B):
    """mixed sizes and paths in one call: every problem bit-identical to itself called alone"""
    names = [TC.DEFAULT_OPTS[(5 * b + b // 12) % len(TC.DEFAULT_OPTS)] for b in range(B)]
    out = TC.call(prob, [TC.runs(n)[0] for n in names], {})
    if B >= 65:
        assert set(out["path"]) == {TR.REFINED, TR.FEW_BEFORE, TR.FEW_AFTER}
    for b, n in enumerate(names):
        for k in KEYS:
            assert np.array_equal(out[k][b], alone[n][k][0]), (b, n, k)
        assert np.array_equal(out["pt_inlier"][b], alone[n]["pt_inlier"][0]) and np.array_equal(out["ln_inlier"][b], alone[n]["ln_inlier"][0]), (b, n)


def test_two_calls_give_the_same_bits(prob):
    cases = [TC.runs(n)[0] for n in ("size_300_100", "outliers", "size_65_0")]
    a, b = TC.call(prob, cases, {}), TC.call(prob, cases, {})
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(a["pt_inlier"] + a["ln_inlier"], b["pt_inlier"] + b["ln_inlier"]):
        assert np.array_equal(x, y)


def test_window_state_untouched_and_one_wait(pkg, hip):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    res = []
    for with_call in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_call:
            before = p.debug_get("host_waits")[0]
            out = TC.call(p, [TC.runs("size_40_24")[0]], {})
            assert p.debug_get("host_waits")[0] == before + 1
            assert out["good"][0] == 1
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_refusals_leave_the_outputs_untouched(pkg, prob):
    abi = pkg.abi
    case = TC.runs("size_40_24")[0]
    P, uv, s2p, pq, l3, se, s2l = (np.ascontiguousarray(case[k], np.float64) for k, _ in TC._WIDTHS)
    ps, ls = np.array([0, len(P)], np.int32), np.array([0, len(pq)], np.int32)
    dp, ip, up = abi._dp, abi._ip, abi._up

    def attempt(B=1, ps=ps, ls=ls, P=P, uv=uv, s2p=s2p, pq=pq, l3=l3, se=se, s2l=s2l, T0=None, opt=True, out=True, **o):
        op = abi.TrackOptions()
        prob.lib.fn["track_default_options"](C.byref(op))
        for k, v in o.items():
            setattr(op, k, v)
        res = (abi.TrackResult * 2)()
        C.memset(res, 0x5A, C.sizeof(res))
        pm, lm = np.full(len(case["P3"]), 7, np.uint8), np.full(len(case["pq"]), 7, np.uint8)
        rc = prob.lib.fn["track_pose"](prob._h, C.byref(op) if opt else None, B, ip(ps), dp(P), dp(uv), dp(s2p), ip(ls), dp(pq), dp(l3), dp(se), dp(s2l),
                                       *[float(v) for v in TC.CAM], dp(T0), up(pm), up(lm), res if out else None)
        assert rc == -1, rc      # PLBA_ERR_INVALID
        assert bytes(res) == b"\x5a" * C.sizeof(res) and (pm == 7).all() and (lm == 7).all()
    bad = P.copy(); bad[3, 1] = np.nan
    neg = s2l.copy(); neg[2] = -1.0
    badT = np.eye(4).reshape(1, 16).copy(); badT[0, 3] = np.inf
    attempt(B=0)
    attempt(ps=np.array([0, -1], np.int32))
    attempt(ps=np.array([1, len(P)], np.int32))
    attempt(B=2, ps=np.array([0, len(P), len(P) - 1], np.int32), ls=np.array([0, len(pq), len(pq)], np.int32))
    attempt(P=None)
    attempt(s2p=None)
    attempt(se=None)
    attempt(out=False)
    attempt(opt=False)
    attempt(P=bad)
    attempt(s2l=neg)
    attempt(T0=badT)
    attempt(max_iters=-1)
    attempt(max_iters_ref=-1)
    attempt(min_features=-1)
    attempt(inlier_k=float("nan"))
    assert TC.call(prob, [case], {})["good"][0] == 1      # the handle still works


def test_harness_track_mode_is_the_c_abi(prob, tmp_path):
    """tools/localba_harness.cpp `track`: lookForCommonMatches' call site (src/mapHandler.cpp:819-859) from the matched lists to kf1->T_kf_w,
    against the direct call bit for bit; a pair with enough inliers of each kind takes expmap(logmap(DT)), the others the inverse of the
    tracker's DT (here the identity)"""
    import sys
    sys.path.insert(0, TC.ROOT + "/tools")
    import harness_io
    from . import lba_ref as LR
    exe = harness_io.build_harness()
    cases = [TC.runs(n)[0] for n in TC.DEFAULT_OPTS]
    got = TC.host_run(exe, str(tmp_path), cases, {})
    out = TC.call(prob, cases, {})
    assert sum(g["used"] for g in got) >= 5 and sum(1 - g["used"] for g in got) >= 2
    for b, g in enumerate(got):
        r = TC.as_result(out, b)
        for k in TR.QUANT + TR.EXACT + ("pt_in", "ln_in"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(r[k])), (b, k)
        n_pt, n_ln = len(cases[b]["P3"]), len(cases[b]["pq"])
        use = r["n_inliers_pt"] + r["n_inliers_ln"] > 10 and (n_pt == 0 or 100.0 * r["n_inliers_pt"] / n_pt >= 30.0) and (n_ln == 0 or 100.0 * r["n_inliers_ln"] / n_ln >= 30.0)
        assert g["used"] == int(use), b
        R, t = LR.se3_exp(LR.se3_log(r["DT"][:3, :3], r["DT"][:3, 3], np.float64), np.float64) if use else (np.eye(3), np.zeros(3))
        assert np.abs(g["T_kf_w"][:3, :3] - R).max() <= 1e-14 and np.abs(g["T_kf_w"][:3, 3] - t).max() <= 1e-14 and g["T_kf_w"][3, 3] == 1.0, b
