"""The references of the gate / cull exactness tests, held to their own conditions without a GPU (tests/gate_exact.py states the rule),
and the power of the rule: five defects of the decision, applied to the fp64 oracle's outputs, each of which hold() rejects."""
import os

import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC
from . import gate_exact as GX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 199235
_CACHE = {}


def _case(pkg, orc, name):
    """(fixture, window, window at B, quad run, noise, the fp64 oracle's run now)"""
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, "gate_exact_%s.npz" % name)) as z:
            fx = {k: z[k] for k in z.files}
        carried, ref, noise = GX.load(fx)
        w = GX.window(name, pkg.window, carried); wb = GX.at_b(pkg.window, w)
        _CACHE[name] = (fx, w, wb, ref, noise, GX.run_on(orc.new_problem, w, wb))
    return _CACHE[name]


def test_the_case_list():
    have = {f[len("gate_exact_"):-4] for f in os.listdir(GOLDEN) if f.startswith("gate_exact_") and f.endswith(".npz")}
    assert have == set(GX.CASES)


@pytest.mark.parametrize("name", GX.CASES)
def test_references(pkg, orc, name):
    fx, w, wb, ref, noise, r64 = _case(pkg, orc, name)
    assert os.path.getsize(os.path.join(GOLDEN, "gate_exact_%s.npz" % name)) <= LIMIT
    assert BC.window_sha(w) == str(fx["sha"]) and BC.window_sha(wb) == str(fx["sha_b"]), "the window generator gives another window than the one the fixture was made from"
    # the fixture is what the quad oracle (and, for the noise, the fp64 oracle) computes now, the carried state and planted observations included
    now = GX.generate(name, pkg.window, orc)
    assert sorted(now) == sorted(fx)
    for k in fx:
        assert np.array_equal(now[k], fx[k]), (name, k)
    # the residuals' noise is within the cap of tests/build_exact.py (ii)
    for q, n in noise.items():
        assert BX.FACTOR * n <= BX.CAP, (name, q, n)
    # no edge of any case is excluded
    bnd = GX.bounds(ref, w, noise)
    for k, m in GX.sure(ref, w, wb, bnd).items():
        assert m.all(), (name, k, int((~m).sum()))
    # the fp64 and the quad oracle agree on every flag, and the fp64 oracle passes every bound
    for k in ["dpos%s_%s" % (r, nm) for r in "01ABC" for nm in ("pt", "ln")] + ["lev_pt", "lev_ln", "badA_pt", "badA_ln", "badB_pt", "badB_ln", "badC_pt", "badC_ln", "gate", "gateC",
              "gate_again", "cullA", "cullB", "cullC", "levB_pt", "levB_ln", "levC_pt", "levC_ln", "levC2_pt", "levC2_ln"]:
        assert np.array_equal(np.asarray(r64[k]).astype(np.int64), np.asarray(ref[k]).astype(np.int64)), (name, k)
    GX.hold(r64, ref, w, wb, noise, "oracle64", name)
    # the reference's own sequence: a second gate moves nothing, the setters leave the levels alone, the flags are the decision on what was read
    assert list(ref["gate_again"]) == [0, 0]
    assert np.array_equal(ref["levB_pt"], ref["lev_pt"]) and np.array_equal(ref["levB_ln"], ref["lev_ln"])
    for nm in ("pt", "ln"):      # sequence (c), through the gate's own levels, is sequence (b) in the reference
        for a, b in (("levC_", "lev_"), ("levC2_", "lev_"), ("badC_", "badB_"), ("chiC_", "chiB_"), ("dposC_", "dposB_"), ("dpos1_", "dpos0_"), ("dposA_", "dpos0_")):
            assert np.array_equal(ref[a + nm], ref[b + nm]), (name, a, nm)
    assert np.array_equal(ref["cullC"], ref["cullB"]) and np.array_equal(ref["gateC"], ref["gate"])
    gp, gl = BX.levels(w)
    for nm, g0 in (("pt", gp), ("ln", gl)):
        assert np.array_equal(ref["chi1_" + nm], ref["chi0_" + nm])
        assert np.array_equal(ref["lev_" + nm].astype(bool), g0 | GX.decide(ref["chi0_" + nm], ref["dpos0_" + nm]))
        assert np.array_equal(ref["badA_" + nm], GX.decide(ref["chiA_" + nm], ref["dpos0_" + nm]))
        lv = ref["lev_" + nm].astype(bool)
        assert np.array_equal(ref["chiA_" + nm][~lv], ref["chi0_" + nm][~lv])      # a level-0 edge keeps the evaluation pass's value through the cull
        assert np.array_equal(ref["chiB_" + nm][~lv], ref["chi0_" + nm][~lv])      # ... also in sequence (b): the cached error, at state A
        if lv.any() and name != "behind":
            assert not np.array_equal(ref["chiB_" + nm][lv], ref["chiA_" + nm][lv])      # a level-1 edge is evaluated at B


def test_behind_is_bad_by_depth_alone(pkg, orc):
    fx, w, wb, ref, noise, r64 = _case(pkg, orc, "behind")
    low = ref["chi0_pt"] < GX.THRESH / 2
    assert (low & (ref["dpos0_pt"] == 0) & (ref["lev_pt"] == 1) & ref["badA_pt"]).sum() >= 3
    _, rl = GX.depth_ratio(w)
    nb = (rl < 0).sum(axis=1)
    lowl = (ref["chi0_ln"] < GX.THRESH / 2) & (ref["dpos0_ln"] == 0) & (ref["lev_ln"] == 1) & ref["badA_ln"]
    assert (lowl & (nb == 1)).sum() >= 2 and (lowl & (nb == 2)).sum() >= 1
    assert (lowl & (nb == 1) & (rl[:, 0] < 0)).sum() >= 1 and (lowl & (nb == 1) & (rl[:, 1] < 0)).sum() >= 1      # the first end alone, and the second end alone
    print("behind: %d point edges, %d line edges with one end and %d with both ends behind are bad with chi2 < %.4g" % ((low & (ref["dpos0_pt"] == 0)).sum(), (lowl & (nb == 1)).sum(), (lowl & (nb == 2)).sum(), GX.THRESH / 2))


def test_threshold_edges_fall_on_their_sides(pkg, orc):
    fx, w, wb, ref, noise, r64 = _case(pkg, orc, "threshold")
    bnd = GX.bounds(ref, w, noise)
    ok = GX.sure(ref, w, wb, bnd)
    for nm, n in zip(("pt", "ln"), GX.N_PLANT):
        idx, side = fx["plant/%s_idx" % nm], fx["plant/%s_side" % nm]
        assert len(idx) == n and (side > 0).sum() == n // 2 and ok["lev_" + nm][idx].all() and ok["badA_" + nm][idx].all()
        chi = ref["chi0_" + nm][idx]
        rel = chi / GX.THRESH - 1
        print("threshold", nm, "chi2 / thresh - 1:", " ".join("%+.4e" % r for r in rel), " margin / (MARGIN x bound): %.3g" % (np.abs(chi - GX.THRESH) / (GX.MARGIN * bnd["chi0_" + nm][idx])).min())
        assert np.allclose(rel, side * GX.REL, rtol=1e-3, atol=0)
        assert np.array_equal(ref["lev_" + nm][idx] == 1, side > 0) and np.array_equal(ref["badA_" + nm][idx], side > 0)
        assert (ref["dpos0_" + nm][idx] == 1).all()


# ---- the power of the rule ----------------------------------------------------------------------------------------------------------------
def _redecide(r64, w, thresh=GX.THRESH, use_depth=True, one_end=None):
    """the fp64 oracle's outputs with the gate's and cull (a)'s decisions taken anew by a defective rule"""
    bad = dict(r64)
    gp, gl = BX.levels(w)
    rp, rl = GX.depth_ratio(w)
    dp = {"pt": rp > 0, "ln": (rl > 0).all(axis=1) if one_end is None else rl[:, one_end] > 0}
    for nm, g0 in (("pt", gp), ("ln", gl)):
        d = dp[nm] if use_depth else np.ones(len(dp[nm]), bool)
        new = (r64["chi0_" + nm] > thresh) | ~d
        bad["lev_" + nm] = (g0 | new).astype(np.uint8)
        bad["badA_" + nm] = (r64["chiA_" + nm] > thresh) | ~d
    bad["gate"] = np.array([(bad["lev_pt"].astype(bool) & ~gp).sum(), (bad["lev_ln"].astype(bool) & ~gl).sum()])
    bad["cullA"] = np.array([bad["badA_pt"].sum(), bad["badA_ln"].sum()])
    return bad


def test_redeciding_with_the_right_rule_changes_nothing(pkg, orc):
    for name in GX.CASES:
        fx, w, wb, ref, noise, r64 = _case(pkg, orc, name)
        same = _redecide(r64, w)
        for k in ("lev_pt", "lev_ln", "badA_pt", "badA_ln", "gate", "cullA"):
            assert np.array_equal(np.asarray(same[k]).astype(np.int64), np.asarray(r64[k]).astype(np.int64)), (name, k)


@pytest.mark.parametrize("defect,case,sees", [("chi2_only", "behind", ("lev_pt", "lev_ln", "badA_pt", "badA_ln")),
                                               ("first_end_point_only", "behind", ("lev_ln", "badA_ln")),
                                               ("second_end_point_only", "behind", ("lev_ln", "badA_ln")),
                                               ("threshold_5.9911", "threshold", ("lev_pt", "lev_ln", "badA_pt", "badA_ln"))])
def test_the_rule_rejects_a_defective_decision(pkg, orc, defect, case, sees):
    fx, w, wb, ref, noise, r64 = _case(pkg, orc, case)
    bad = _redecide(r64, w, thresh=5.9911 if defect == "threshold_5.9911" else GX.THRESH, use_depth=defect != "chi2_only",
                    one_end={"first_end_point_only": 0, "second_end_point_only": 1}.get(defect))
    with pytest.raises(AssertionError) as ei:
        GX.hold(bad, ref, w, wb, noise, "corrupted", "%s %s" % (case, defect))
    failed = {q for q, _, _ in ei.value.args[0][2]}
    print(defect, "rejected on", sorted(failed))
    assert set(sees) <= failed and failed <= set(sees) | {"gate", "cullA"}


def test_greater_or_equal_is_not_the_decision():
    """an edge whose chi2 is the threshold exactly stays: the decision is >, not >="""
    chi = np.array([GX.THRESH, np.nextafter(GX.THRESH, 10.0), np.nextafter(GX.THRESH, 0.0)])
    assert list(GX.decide(chi, np.ones(3, np.uint8))) == [False, True, False]
    assert list(GX.decide(chi, np.zeros(3, np.uint8))) == [True, True, True]
    assert list(chi >= GX.THRESH) != list(GX.decide(chi, np.ones(3, np.uint8)))
