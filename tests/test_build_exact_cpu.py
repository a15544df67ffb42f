"""The references of the built-system exactness tests, held to their own conditions without a GPU (tests/build_exact.py states the rule
and conditions (i) - (iv); tests/build_exact_cases.py the windows and what (ii) dropped), and the power of the rule: three defects of
Hschur, each of which hold() rejects, two of which today's criterion — max|a - b| / max|b| < 1e-9 over the whole array — accepts."""
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
        q = orc.new_quad_problem(); q.upload_window(w); q.debug_build(lam, True)
        assert np.array_equal(ref.dense().ravel(), q.debug_get("Hschur"))
        q.close()


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
