"""The references of the state exactness tests, held to their own conditions without a GPU (tests/step_exact.py states the rule and
conditions (i) - (v); tests/step_exact_cases.py the sequences and what (ii) and (iv) shortened or dropped), and the power of the rule:
four defects of the state that the trial launch leaves, each of which hold() rejects, two of which the comparisons in use —
_pose_delta(...) < 1e-8 on the keyframes, max|a - b| / max|b| < 1e-8 on the landmarks (tests/test_gpu_parity.py) — accept."""
import os

import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC
from . import step_exact as SX
from . import step_exact_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 199235      # tests/test_build_exact_cpu.py: no fixture above the largest file committed before those
_CACHE = {}


def _case(pkg, name):
    """(build_exact fixture, step_exact fixture, size of the latter, window) of a case; loaded once, never written"""
    if name not in _CACHE:
        fx = []
        for kind in ("build_exact", "step_exact"):
            path = os.path.join(GOLDEN, "%s_%s.npz" % (kind, name))
            with np.load(path) as z:
                fx.append({k: z[k] for k in z.files})
        w = BC.CASES[name]["make"](pkg.window, BX.prior_of(fx[0]))
        _CACHE[name] = (fx[0], fx[1], os.path.getsize(path), w)
    return _CACHE[name]


def _ref(fxb, w, name, label):
    i = SC.lambda_index(name, label)
    return BX.load(fxb, w, i)[0], float(fxb["lams"][i])


def test_the_sequence_list():
    """what was shortened, dropped or partly dropped names a planned sequence, nothing is named twice, a fixture exists for every case and
    for nothing else, and condition (v): the lists hide nothing"""
    planned = {(name, k): n for name in BC.CASES for k, _, n, _ in SC.planned(name)}
    assert set(SC.SHORTENED) | SC.DROPPED | set(SC.QUANT_DROPPED) <= set(planned)
    assert not set(SC.SHORTENED) & SC.DROPPED and not SC.DROPPED & set(SC.QUANT_DROPPED) and not set(SC.SHORTENED) & set(SC.QUANT_DROPPED)
    assert all(planned[k] == 3 and n == 2 for k, n in SC.SHORTENED.items())
    assert all(planned[k] == 1 and set(q) <= {"state_pt", "state_ln", "chi2_trial"} for k, q in SC.QUANT_DROPPED.items())      # the keyframes are always compared
    have = {f[len("step_exact_"):-4] for f in os.listdir(GOLDEN) if f.startswith("step_exact_") and f.endswith(".npz")}
    assert have == set(BC.CASES)
    # (v) every case keeps one iteration at lambda = 5 (`behind`, whose build keeps the protocol's first lambda alone, at that one) ...
    for name in BC.CASES:
        keys = [k for k, _, _, _ in SC.sequences(name)]
        assert ("n1-init" if (name, 5.0) in BC.DROPPED else "n1-5") in keys, name
    # ... and at least half of the cases a sequence of two or more iterations
    longer = [name for name in BC.CASES if any(n >= 2 for _, _, n, _ in SC.sequences(name))]
    assert 2 * len(longer) >= len(BC.CASES), longer


def test_the_kept_sequences_reach_what_they_are_for(pkg):
    """(v) among the kept sequences one has IMU edges and lines and one contains a rejected trial; the all-rejected calls are all
    rejected, two of them on IMU windows; the bias-first window has both vertex orders"""
    with_imu_and_lines, with_rejected, all_rejected = [], [], []
    for name in BC.CASES:
        _, fx, _, w = _case(pkg, name)
        assert [str(k) for k in fx["keys"]] == [k for k, _, _, _ in SC.sequences(name)]
        for j, (key, _, n, _) in enumerate(SC.sequences(name)):
            s = SX.load(fx, j)
            acc = s["q"]["trace"][:, 2]
            if w.get("imu") is not None and BX.layout(w)["free_ln"].any() and "state_ln" in s["noise"]:
                with_imu_and_lines.append((name, key))
            if acc.any() and not acc.all():
                with_rejected.append((name, key))
            if key.startswith("rej"):
                assert not acc.any() and len(acc) == 1, (name, key)
                all_rejected.append(name)
            else:
                assert acc.sum() == n == s["n"], (name, key)      # every iteration of the others ends in an accepted trial
    assert with_imu_and_lines and with_rejected
    assert sorted(all_rejected) == sorted(SC.REJECTED) and sum(_case(pkg, n)[3].get("imu") is not None for n in all_rejected) >= 2
    w = _case(pkg, "biasfirst")[3]
    op, ob, _ = SX.offsets(w)
    free = (op >= 0) & (ob >= 0)
    assert (ob[free] < op[free]).sum() >= 4 and (ob[free] > op[free]).sum() >= 4
    assert np.array_equal(w["points"], _case(pkg, "mixed")[3]["points"])


@pytest.mark.parametrize("name", list(BC.CASES))
def test_references(pkg, orc, name):
    fxb, fx, size, w = _case(pkg, name)
    assert size <= LIMIT, (name, size)
    assert BC.window_sha(w) == str(fx["sha"]) == str(fxb["sha"]), "the window generator gives another window than the one the fixture was made from"
    # (i) the fixture is what the quad run (and, for the noise, the fp64 runs) computes now
    now = SX.generate(name, pkg.window, orc, fxb)
    assert sorted(now) == sorted(fx)
    for k in fx:
        assert np.array_equal(now[k], fx[k]), (name, k)
    up = SX.upload(w)
    for j, (key, label, n, opts) in enumerate(SC.sequences(name)):
        s = SX.load(fx, j)
        ref, lam = _ref(fxb, w, name, label)
        assert s["lam"] == lam and s["n"] == n and s["q"]["trace"][0, 4] == lam
        # (iv) decided: the decisions of all four fp64 runs are the quad run's and every rho is clear of 0
        assert s["decided"] and s["margin"] >= SX.MARGIN, (name, key, s["margin"])
        assert np.array_equal(SX.decisions(s["trace_64"]), SX.decisions(s["q"]["trace"]))
        # (ii) 32 x noise within 1e-9, and the state's tolerance within 1e-9 in the units of every kind that is compared
        over, _, ab = SX.misses(s["noise"], s["q"], up, ref, w)
        assert not over, (name, key, over)
        print(name, key, " ".join("%s %.1e" % kv for kv in ab.items()))
        dropped = SC.QUANT_DROPPED.get((name, key), ())
        assert not set(dropped) & set(s["noise"])
        # (iii) the fp64 oracle passes, the exact conditions included
        r64 = SX.run(orc.new_problem, w, lam, n, opts)
        assert np.array_equal(r64["trace"], s["trace_64"])
        SX.hold(r64, s, ref, w, "oracle64", "%s %s" % (name, key), dropped=dropped)


NOT_KEPT = sorted(SC.DROPPED) + sorted(SC.SHORTENED) + sorted(SC.QUANT_DROPPED)


@pytest.mark.parametrize("name,key", NOT_KEPT, ids=["%s-%s" % nk for nk in NOT_KEPT])
def test_what_was_dropped_misses_its_condition(pkg, orc, name, key):
    """conditions (ii) and (iv) the other way round, now: a dropped sequence of three iterations misses at two as well, a dropped
    sequence of one misses on its keyframes (or in more than its landmarks and its trial), a shortened one misses at three, and where
    quantities alone are left out exactly those are over their cap"""
    fxb, _, _, w = _case(pkg, name)
    _, label, n, opts = [p for p in SC.planned(name) if p[0] == key][0]
    ref, lam = _ref(fxb, w, name, label)
    m = 3 if (name, key) in SC.SHORTENED else min(n, 2)
    q, _, noise, decided, margin = SX.references(orc, w, lam, m, opts, ref)
    if not decided:
        print(name, key, "n", m, "undecided, margin %.3g" % margin)
        assert (name, key) not in SC.QUANT_DROPPED
        return
    over, quantities, _ = SX.misses(noise, q, SX.upload(w), ref, w)
    print(name, key, "n", m, "over:", " ".join("%s %.3g" % kv for kv in over.items()))
    if (name, key) in SC.QUANT_DROPPED:
        assert quantities == set(SC.QUANT_DROPPED[(name, key)])
    elif n == 1:
        assert "state_pose" in quantities
    else:
        assert over


# ---- the power of the rule --------------------------------------------------------------------------------------------------------------
def _todays_bars(res, q):
    """(the keyframes pass _pose_delta(...) < 1e-8, the landmarks pass _close(..., 1e-8)) of tests/test_gpu_parity.py, and the figures"""
    dphi = max(float(np.linalg.norm(SX._log(SX._qmul(SX._qinv(b), a)))) for a, b in zip(res["q"], q["q"]))
    kf = (np.abs(res["P"] - q["P"]).max(), np.abs(res["V"] - q["V"]).max(), dphi, max(np.abs(res["dbg"] - q["dbg"]).max(), np.abs(res["dba"] - q["dba"]).max()))
    lm = [float(np.abs(res[k] - q[k]).max() / max(np.abs(q[k]).max(), 1e-300)) for k in ("points", "lines") if q[k].size]
    return max(kf) < 1e-8 and all(v < 1e-8 for v in lm), kf, lm


def _corrupted(pkg, orc, defect):
    name, key = {"gyro_bias_step_scaled_1.01": ("mixed", "n1-5"), "landmark_step_in_fp32": ("mixed", "n1-5"),
                 "bias_not_restored_after_rejection": ("stage2_cross9", "rej-5"), "offsets_of_the_other_vertex_order": ("biasfirst", "n1-5")}[defect]
    fxb, fx, _, w = _case(pkg, name)
    j, (_, label, n, opts) = [(j, s) for j, s in enumerate(SC.sequences(name)) if s[0] == key][0]
    s = SX.load(fx, j)
    ref, lam = _ref(fxb, w, name, label)
    good = SX.run(orc.new_problem, w, lam, n, opts)
    up = SX.upload(w)
    bad = {k: np.array(v, copy=True) for k, v in good.items()}
    op, ob, P = SX.offsets(w)
    if defect == "gyro_bias_step_scaled_1.01":
        k = 3
        assert ob[k] >= 0
        bad["dbg"][k] = up["dbg"][k] + 1.01 * (good["dbg"][k] - up["dbg"][k])
    elif defect == "landmark_step_in_fp32":
        for lm in ("points", "lines"):
            bad[lm] = up[lm] + (good[lm] - up[lm]).astype(np.float32).astype(np.float64)
    else:
        o = orc.new_problem(); o.upload_window(w); BX.apply(o, w); o.debug_build(lam, True)
        x = o.debug_get("x").copy(); o.close()
        if defect == "bias_not_restored_after_rejection":      # the trial's bias half s[16 + i] + x[ob + i] left in place
            k = 4
            assert ob[k] >= 0 and not good["trace"][:, 2].any()
            bad["dbg"][k], bad["dba"][k] = up["dbg"][k] + x[ob[k]:ob[k] + 3], up["dba"][k] + x[ob[k] + 3:ob[k] + 6]
        else:      # keyframe 3, bias first: its state from x as if the PVR block came first
            k = 3
            assert 0 <= ob[k] < op[k] == ob[k] + 6
            nav = orc.nav_vec(up["P"][k], up["V"][k], up["q"][k], w["kf"]["bg"][k], w["kf"]["ba"][k], up["dbg"][k], up["dba"][k])
            out = orc.nav_oplus_bias(orc.nav_oplus_pvr(nav, x[ob[k]:ob[k] + 9]), x[ob[k] + 9:ob[k] + 15])
            bad["P"][k], bad["V"][k], bad["q"][k], bad["dbg"][k], bad["dba"][k] = out[0:3], out[3:6], out[6:10], out[16:19], out[19:22]
    return s, ref, w, good, bad, "%s %s" % (name, key), SC.QUANT_DROPPED.get((name, key), ())


# (defect, the comparisons in use accept it).  The first is 3e-9 on a bar of 1e-8; the second is 6e-8 of a landmark's step on a bar of
# 1e-8 x max|array|.  The last two move a keyframe by far more than 1e-8 and are seen today as well: the rule adds which quantity and
# by how much.
DEFECTS = [("gyro_bias_step_scaled_1.01", True), ("landmark_step_in_fp32", True), ("bias_not_restored_after_rejection", False),
           ("offsets_of_the_other_vertex_order", False)]


@pytest.mark.parametrize("defect,accepted_today", DEFECTS)
def test_the_rule_rejects_a_wrong_state(pkg, orc, defect, accepted_today):
    s, ref, w, good, bad, name, dropped = _corrupted(pkg, orc, defect)
    ok, kf, lm = _todays_bars(bad, s["q"])
    print(defect, "today's bars: keyframes dP %.3e dV %.3e dphi %.3e dbias %.3e (accept below 1e-8), landmarks %s (accept below 1e-8): %s"
          % (kf + (" ".join("%.3e" % v for v in lm), "accepted" if ok else "rejected")))
    assert ok == accepted_today
    assert _todays_bars(good, s["q"])[0]
    SX.hold(good, s, ref, w, "oracle64", name, dropped=dropped)      # (the uncorrupted state passes)
    with pytest.raises(AssertionError, match={"gyro_bias_step_scaled_1.01": "state_pose", "landmark_step_in_fp32": "state_pt",
                                              "bias_not_restored_after_rejection": "not the upload", "offsets_of_the_other_vertex_order": "state_pose"}[defect]):
        SX.hold(bad, s, ref, w, "corrupted", name + " " + defect, dropped=dropped)


def test_at_least_two_of_the_defects_pass_todays_bars():
    assert sum(a for _, a in DEFECTS) >= 2
