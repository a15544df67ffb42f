"""The references of the built-system exactness tests, held to their own conditions without a GPU (tests/build_exact.py states the rule
and conditions (i) - (iv); tests/build_exact_cases.py the windows and what (ii) dropped), and the power of the rule: three defects of
Hschur, each of which hold() rejects, two of which today's criterion — max|a - b| / max|b| < 1e-9 over the whole array — accepts; and,
on the gated system, one gated observation's contribution added back into one block."""
import os

import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 199235      # tests/golden/twin_plan_parent.json, the largest fixture committed before these


def _fixture(name):
    path = os.path.join(GOLDEN, "build_exact_%s.npz" % name)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}, os.path.getsize(path)


def _rel(a, b):      # today's criterion, as tests/test_lm_fused.py has it
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def test_the_case_list():
    """every lambda is one of the three (nothing below 0.05), what was dropped names a case and lambda that exist, and a fixture exists
    for every case and for nothing else"""
    for name, c in BC.CASES.items():
        assert set(c["lambdas"]) <= {"init", 5.0, 0.05} and 5.0 in c["lambdas"], name
    for name, l in BC.DROPPED | BC.TRIAL_DROPPED:
        assert l in BC.CASES[name]["lambdas"], (name, l)
    have = {f[len("build_exact_"):-4] for f in os.listdir(GOLDEN) if f.startswith("build_exact_") and f.endswith(".npz")}
    assert have == set(BC.CASES)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_references(pkg, orc, name):
    fx, size = _fixture(name)
    assert size <= LIMIT, (name, size)
    w = BC.CASES[name]["make"](pkg.window, BX.prior_of(fx))
    assert BC.window_sha(w) == str(fx["sha"]), "the window generator gives another window than the one the fixture was made from"
    # (i) the fixture is what the quad build (and, for the noise, the fp64 build) computes now — the prior of prior13 included
    now = BX.generate(name, pkg.window, orc)
    assert sorted(now) == sorted(fx)
    for k in fx:
        assert np.array_equal(now[k], fx[k]), (name, k)
    lams = BC.lambdas_of(name, float(fx["0/maxdiag"][0]))
    assert [v for _, v in lams] == list(fx["lams"])
    for i, (label, lam) in enumerate(lams):
        ref, tq, t64, noise, decided = BX.load(fx, w, i)
        # (ii) every new bar at least ten times tighter than the one in use
        for q, n in noise.items():
            assert BX.factor(q) * n <= BX.cap(q), (name, label, q, n)
        assert ("chi2_trial" in noise) == ((name, label) not in BC.TRIAL_DROPPED)
        # (iv) a compared decision is the same in both precisions
        assert tq[2] == t64[2] == lam
        if decided:
            assert tq[1] == t64[1]
        # (iii) the fp64 oracle passes
        r64, row = BX.evaluate(orc.new_problem, w, lam)
        assert np.array_equal(row, t64)
        BX.hold(r64, ref, noise, "oracle64", "%s lambda %.4g" % (name, lam), trial=(row, tq, decided))
        # Hschur rebuilt from the stored nonzeros is the matrix the quad run returned
        q = orc.new_quad_problem(); q.upload_window(w); BX.apply(q, w); q.debug_build(lam, True)
        assert np.array_equal(ref.dense().ravel(), q.debug_get("Hschur"))
        q.close()


@pytest.mark.parametrize("name,label", sorted(BC.DROPPED | BC.TRIAL_DROPPED, key=str))
def test_what_was_dropped_is_over_its_cap(pkg, orc, name, label):
    """condition (ii) the other way round: a (case, lambda) left out has a quantity whose FACTOR x noise exceeds its cap, now; where only
    the trial is left out that quantity is chi2_trial and everything else is within"""
    fx, _ = _fixture(name)
    w = BC.CASES[name]["make"](pkg.window, BX.prior_of(fx))
    noise = BX.references(orc, w, float(label))[3]
    over = sorted(q for q, n in noise.items() if BX.factor(q) * n > BX.cap(q))
    print(name, label, "over the cap:", " ".join("%s %.0fu" % (q, noise[q] / BX.U) for q in over))
    if (name, label) in BC.TRIAL_DROPPED:
        assert over == ["chi2_trial"]
    else:
        assert over and over != ["chi2_trial"]


# ---- the power of the rule --------------------------------------------------------------------------------------------------------------
def _pose_blocks(ref):
    """the off-diagonal pose-pose 6 x 6 blocks of an IMU window's Hschur (15 dimensions per free keyframe: P V R bias; the pose is P and R)
    that hold an entry: [(largest |entry|, rows, columns)]"""
    P = ref.P
    assert P % 15 == 0
    H = ref.dense()
    pose = lambda j: 15 * j + np.array([0, 1, 2, 6, 7, 8])
    out = []
    for a in range(P // 15):
        for b in range(a):
            m = np.abs(H[np.ix_(pose(a), pose(b))]).max()
            if m > 0:
                out.append((m, pose(a), pose(b)))
    return sorted(out, key=lambda t: t[0])


@pytest.fixture(scope="module")
def mixed(pkg, orc):
    fx, _ = _fixture("mixed")
    w = BC.CASES["mixed"]["make"](pkg.window, None)
    i = list(fx["lams"]).index(5.0)
    ref, tq, t64, noise, decided = BX.load(fx, w, i)
    r64, _ = BX.evaluate(orc.new_problem, w, 5.0)
    return ref, noise, r64


# (defect, today's criterion accepts it).  The first two are 7.6e-3 and 0.13 absolute on a matrix whose bar is 1e-9 x 2e10 = 20.  The
# third is not accepted today, against what was expected when these tests were planned: the translation-translation part of the smallest
# off-diagonal block of `mixed` (keyframes 8 and 3) has an entry of 838.8 (668.7 for keyframes 8 and 4, if the block is taken as P and V),
# above 20, so the 1e-9 criterion sees it — at 4.2e-8, forty times its bar, where the rule below sees it at 1e10 times its tolerance.  The
# figure is asserted as it is.
DEFECTS = [("block_in_fp32", True), ("block_scaled_1e-6", True), ("smallest_block_without_its_translation_part", False)]


@pytest.mark.parametrize("defect,accepted_today", DEFECTS)
def test_the_rule_rejects_what_the_1e9_criterion_accepts(mixed, defect, accepted_today):
    ref, noise, r64 = mixed
    P = ref.P
    blocks = _pose_blocks(ref)
    H = r64["Hschur"].reshape(P, P).copy()
    if defect == "smallest_block_without_its_translation_part":
        _, ra, cb = blocks[0]
        ra, cb = ra[:3], cb[:3]
        new = np.zeros((3, 3))
    else:
        _, ra, cb = blocks[len(blocks) // 2]      # the median block
        old = H[np.ix_(ra, cb)]
        new = old.astype(np.float32).astype(np.float64) if defect == "block_in_fp32" else old * (1 + 1e-6)
    assert np.abs(H[np.ix_(ra, cb)]).max() > 0
    H[np.ix_(ra, cb)] = new; H[np.ix_(cb, ra)] = new.T
    bad = dict(r64, Hschur=H.ravel())
    old_bar = _rel(bad["Hschur"], ref.dense().ravel())
    print(defect, "today's criterion: %.3e (accepts below 1e-9)" % old_bar)
    assert (old_bar < 1e-9) == accepted_today      # the gap: the comparison in use passes the first two matrices
    assert BX.errors(r64, ref)["Hschur"] <= BX.tolerances(noise, ref.lay)["Hschur"]      # (the uncorrupted matrix passes)
    with pytest.raises(AssertionError, match="Hschur"):
        BX.hold(bad, ref, noise, "corrupted", "mixed " + defect)
    e = BX.errors(bad, ref)
    assert {q for q in e if e[q] > BX.tolerances(noise, ref.lay)[q]} == {"Hschur"}      # and nothing else is what failed


# ---- the gated cases ---------------------------------------------------------------------------------------------------------------------
def _window(pkg, name):
    fx, _ = _fixture(name)
    return fx, BC.CASES[name]["make"](pkg.window, BX.prior_of(fx))


def test_the_gated_cases_reach_their_structures(pkg):
    """what the table of DESIGN.md 9l says each case reaches, on the windows themselves"""
    cnt0 = lambda w, kind: np.bincount((w["lo_ln"] if kind else w["po_pt"])[~BX.levels(w)[kind]], minlength=len(w["lines" if kind else "points"]))
    for name in BC.OLD:      # the twelve windows as uploaded carry no levels and no switches
        if name not in BC.NEEDS_PRIOR:
            w = BC.CASES[name]["make"](pkg.window, None)
            assert "po_level" not in w and "lo_level" not in w and "robust" not in w, name
    for name in ("gated_mixed", "levels_robust_on"):
        _, w = _window(pkg, name)
        lay = BX.layout(w)
        assert (w["po_level"].sum(), w["lo_level"].sum()) >= (9 + 3, 3 + 3)
        for kind, free in ((0, lay["free_pt"]), (1, lay["free_ln"])):
            c = cnt0(w, kind)
            assert (~free).sum() == 1 and (c == 1).sum() >= 1, name      # one landmark without a level-0 observation (x shrinks), one with a single one
        first = np.concatenate([[True], w["po_pt"][1:] != w["po_pt"][:-1]])
        assert (first & w["po_level"].astype(bool) & lay["free_pt"][w["po_pt"]]).sum() >= 4      # a free landmark whose first observation, the bucket's anchor, is gated
        assert ("robust" in w) == (name == "gated_mixed")
    assert np.array_equal(_window(pkg, "gated_mixed")[1]["po_level"], _window(pkg, "levels_robust_on")[1]["po_level"])
    _, w = _window(pkg, "gated_short2")
    assert w["po_level"].sum() == 10 and (cnt0(w, 0) == 1).sum() == 10 and BX.layout(w)["free_pt"].all()
    _, w = _window(pkg, "gated_steps3")
    assert (~BX.layout(w)["free_pt"]).sum() == 32 and w["lo_level"].sum() > 0
    for kind in (0, 1):
        gated = np.zeros(len(w["lines" if kind else "points"]), bool); gated[(w["lo_ln"] if kind else w["po_pt"])[BX.levels(w)[kind]]] = True
        for ch, st in BC._group_steps(w, 3, kind):
            assert not gated[ch[st == 0]].any()      # only the second and third steps hold a gated observation
        assert any(gated[ch[st == 1]].any() for ch, st in BC._group_steps(w, 3, kind)) and any(gated[ch[st == 2]].any() for ch, st in BC._group_steps(w, 3, kind))
    _, w = _window(pkg, "gated_k16")
    allp, alll = np.bincount(w["po_pt"]), np.bincount(w["lo_ln"])
    assert set(w["po_kf"][w["po_level"] == 1]) > {5} and ((cnt0(w, 0) == 1) & (allp > 8)).sum() == 1      # a landmark of a wide group left with one observation
    assert ((allp - cnt0(w, 0) == 1) & (allp > 8)).sum() >= 10 and ((alll - cnt0(w, 1) == 1) & (alll > 8)).sum() > 3      # wide groups with holes in keyframe 5
    _, w = _window(pkg, "lines_all_gated")
    lay = BX.layout(w)
    assert not lay["free_ln"].any() and lay["free_pt"].all() and len(w["lines"]) == 12
    _, w = _window(pkg, "noimu_lostkf")
    pm = BX.pose_map(w)
    assert pm is not None and len(pm) == 54 and (pm < 0).sum() == 9 and list(np.flatnonzero(pm < 0)) == list(range(18, 27))      # keyframe 3 is the third free one
    for name in BC.CASES:
        if name != "noimu_lostkf" and name not in BC.NEEDS_PRIOR:
            assert BX.pose_map(_window(pkg, name)[1]) is None, name
    _, w = _window(pkg, "behind")
    zp = [BC.project(w, w["po_kf"][e], w["points"][w["po_pt"][e]])[2] for e in range(len(w["po_pt"]))]
    zl = [[BC.project(w, w["lo_kf"][e], w["lines"][w["lo_ln"][e], o:o + 3])[2] for o in (0, 3)] for e in range(len(w["lo_ln"]))]
    nb = np.array([int(a < 0) + int(b < 0) for a, b in zl])
    assert (np.array(zp) < 0).sum() >= 3 and (nb == 1).sum() >= 1 and (nb == 2).sum() >= 1      # rows with z < 0 in the build
    assert "po_level" not in w and "robust" not in w
    for name, base in BC.NEEDS_STATE.items():
        fx, w = _window(pkg, name)
        assert w["po_level"].sum() > 0 and w["lo_level"].sum() > 0 and w["robust"][0][0] == 0
        assert not np.array_equal(w["points"], BC.CASES[base]["make"](pkg.window, None)["points"])


@pytest.fixture(scope="module")
def gated_mixed(pkg, orc):
    fx, w = _window(pkg, "gated_mixed")
    i = list(fx["lams"]).index(5.0)
    ref, tq, t64, noise, decided = BX.load(fx, w, i)
    r64, _ = BX.evaluate(orc.new_problem, w, 5.0)
    return ref, noise, r64, w


def test_the_rule_sees_a_gated_observation_added_back(orc, gated_mixed):
    """one gated observation's whole contribution — what the fp64 oracle's Hschur gains when that observation alone is put back to level
    0 — added into the one diagonal block of its keyframe: the defect of a kernel that skips wr = 0 for one slot of one tile"""
    ref, noise, r64, w = gated_mixed
    P = ref.P
    lay = ref.lay
    first = np.concatenate([[True], w["po_pt"][1:] != w["po_pt"][:-1]])
    cand = np.flatnonzero(first & (w["po_level"] == 1) & lay["free_pt"][w["po_pt"]] & ~w["truth"]["point_outlier"] & (w["po_kf"] >= 1))
    e = int(cand[0])
    w2 = dict(w); w2["po_level"] = w["po_level"].copy(); w2["po_level"][e] = 0
    r2, _ = BX.evaluate(orc.new_problem, w2, 5.0)
    k = int(w["po_kf"][e])
    blk = slice(15 * (k - 1), 15 * k)      # keyframe 0 is fixed; 15 dimensions (P V R, bias) per free keyframe
    H = r64["Hschur"].reshape(P, P).copy()
    D = r2["Hschur"].reshape(P, P)[blk, blk] - H[blk, blk]
    assert np.abs(D).max() > 0
    H[blk, blk] += D
    bad = dict(r64, Hschur=H.ravel())
    err, tol = BX.errors(bad, ref)["Hschur"], BX.tolerances(noise, lay)["Hschur"]
    print("observation %d of keyframe %d added back: today's criterion %.3e (accepts below 1e-9); the rule: error %.3e, tolerance %.3e, error / tolerance %.3e"
          % (e, k, _rel(bad["Hschur"], ref.dense().ravel()), err, tol, err / tol))
    assert BX.errors(r64, ref)["Hschur"] <= tol
    with pytest.raises(AssertionError, match="Hschur"):
        BX.hold(bad, ref, noise, "corrupted", "gated_mixed one observation added back")
    assert err > 1e3 * tol
