"""plba_bow_* on the device against tests/bow_ref.py.  Word ids, nnz and every decision computed from a given float column are compared for
equality; bag-of-words values and scores against the EXACT values within the derived tolerances of tests/bow_ref.py (the restatement itself
lies inside them on every scenario used here: tests/test_bow_cpu.py); decisions against the full restatement for equality where the
margins allow it (bow_ref.margins_ok, asserted to hold often enough by tests/test_bow_cpu.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from . import bow_ref as BR
from . import match_ref as MR
from . import relpose_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _opts(s, **over):
    o = dict(BR.DEFAULTS); o.update(s["opts"]); o.update(over)
    return o


def _load(p, s):
    """the scenario's vocabularies (setting one drops the database); an already loaded scenario only resets the database"""
    if getattr(p, "_bow_loaded", None) == s["name"]:
        p.bow_reset()
        return
    o = _opts(s)
    if o["mode"] != BR.LINES:
        p.bow_set_vocabulary(0, s["voc"][0], weighting=s["weighting"][0])
    if o["mode"] != BR.POINTS:
        p.bow_set_vocabulary(1, s["voc"][1], weighting=s["weighting"][1])
    p._bow_loaded = s["name"]


CAND = ("is_candidate", "kf_prev", "n_closest", "n_eligible", "best_score", "lc_min_score", "topk", "topk_score")


def _run(p, s, cuts=(), **over):
    """insert the scenario's keyframes, one call between two cuts (the removals are cuts); per keyframe a dict of its outputs"""
    o = _opts(s, **over)
    n = len(s["kfs"])
    cuts = sorted(set([0, n] + [a for a, _ in s["removed"] if a < n] + list(cuts)))
    rows = []
    for a, b in zip(cuts, cuts[1:]):
        for at, kf in s["removed"]:
            if at == a:
                p.bow_remove_keyframe(kf)
        out = p.bow_insert_keyframes(s["kfs"][a:b], cov=s["cov"][a:b], want_bow=True, **o)
        assert out["first_index"] == a
        for j in range(b - a):
            r = {k: out[k][j] for k in ("score_p", "score_l", "score", "score_f32")}
            r["cand"] = {k: out[k][j:j + 1] for k in CAND}
            for k, pre in enumerate(("pt", "ln")):
                if pre in out:
                    r["word%d" % k], r["id%d" % k], r["val%d" % k] = out[pre]["word"][j], out[pre]["bow_id"][j], out[pre]["bow_val"][j]
            rows.append(r)
    return rows


def _check(rows, s, **over):
    name = s["name"]
    ref, o = BR.reference(name), _opts(s, **over)
    worst = [0.0, 0.0]
    for idx, (h, r) in enumerate(zip(rows, ref)):
        for k in (0, 1):
            if (k == 0 and o["mode"] == BR.LINES) or (k == 1 and o["mode"] == BR.POINTS):
                continue
            assert np.array_equal(h["word%d" % k], r["word%d" % k]) and list(h["id%d" % k]) == r["id%d" % k], (idx, k)
            for v, x in zip(h["val%d" % k], r["xval%d" % k]):
                assert BR.exact_err(v, x) <= BR.tol_value(max(r["n"][k], 1)) * float(x), (idx, k)
        w = BR.column_errors(name, idx, h["score_p"], h["score_l"], h["score"])
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        assert w[0] < 1.0 and w[1] < 1.0, (idx, w)
        assert np.array_equal(h["score_f32"], h["score"].astype(np.float32), equal_nan=True), idx
        dead = np.flatnonzero(r["live"] == 0)
        assert not h["score"][dead].any() and not h["score_p"][dead].any() and not h["score_l"][dead].any(), idx
        # whatever the scores: the decision is lookForLoopCandidates of the device's own float column
        why = BR.same_decision(h["cand"], 0, BR.decide_ref(h["score_f32"][:idx], s["cov"][idx], r["live"], idx, **o))
        assert why is None, (idx, why)
        if not over and BR.margins_ok(name, idx):
            why = BR.same_decision(h["cand"], 0, r["cand"])
            assert why is None, (idx, why)
    print("%s: device / tolerance: single %.4f, chosen %.4f" % (name, worst[0], worst[1]))


# ---- the transform over the trees ------------------------------------------------------------------------------------------------------
def _transform_case(prob, voc, weighting, sets):
    prob.bow_set_vocabulary(0, voc, weighting=weighting)
    prob._bow_loaded = None
    out = prob.bow_transform(0, sets)
    v = BR.Voc(voc, weighting)
    for b, rows in enumerate(sets):
        words, ids, vals = v.transform(rows)
        _, _, xvals = v.transform(rows, exact=True)
        assert np.array_equal(out["word"][b], words) and list(out["bow_id"][b]) == ids, b
        for a, x in zip(out["bow_val"][b], xvals):
            assert BR.exact_err(a, x) <= BR.tol_value(max(len(rows), 1)) * float(x), b
    return out


def _sets(voc, sizes, seed):
    return [BR.make_keyframe(voc, None, n, 0, seed + i)["pdesc"] for i, n in enumerate(sizes)]


@pytest.mark.parametrize("k", [2, 3, 10, 11])
def test_transform_branching_and_depth(prob, k):
    for L in (1, 2, 3, 4):
        voc = BR.make_vocabulary(k, L, 500 + 10 * k + L)
        _transform_case(prob, voc, BR.TF_IDF, _sets(voc, (65, 0, 1, 30), 900 + L))


@pytest.mark.parametrize("name", ["ragged", "one_word", "one_word_hit", "root_128", "root_129", "root_300_ragged"])
def test_transform_special_trees(prob, name):
    if name == "ragged":
        voc = BR.make_vocabulary(5, 4, 77, ragged=True)
        assert len(set(np.bincount(voc["parent"][1:]))) > 2      # (the fan-out really varies, leaves above depth L)
    elif name == "one_word":
        voc = BR.make_vocabulary(1, 1, 78, zero_frac=0.0)
    elif name == "one_word_hit":      # all descriptors fall in one word: nnz = 1, a chain of 129 additions
        voc = BR.make_vocabulary(2, 1, 79, zero_frac=0.0)
        voc["desc"][2] = ~voc["desc"][1]
    elif name == "root_128":
        voc = BR.make_vocabulary(128, 1, 80)
    elif name == "root_129":
        voc = BR.make_vocabulary(129, 1, 81)
    else:
        voc = BR.make_vocabulary(300, 2, 82, ragged=True)
        voc["parent"] = voc["parent"].copy()
    sets = _sets(voc, (129, 64), 950)
    if name == "one_word_hit":
        rng = np.random.default_rng(5)
        sets = [np.array([BR.flip(voc["desc"][1], 3, rng) for _ in range(129)], np.uint8)]
    for w in (BR.TF_IDF, BR.BINARY):
        out = _transform_case(prob, voc, w, sets)
        if name in ("one_word", "one_word_hit"):
            assert [len(i) for i in out["bow_id"]] == [1] * len(sets) and all(v[0] == 1.0 for v in out["bow_val"])


# ---- the database ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BR.SCENARIOS))
def test_scenarios_against_the_reference(prob, name):
    """sizes: 0, 1, 63, 64, 65, 129 and 600 descriptors, empty kinds (NaN); big: 8192 once; db258: database sizes 0 .. 257; the three modes;
    the weightings; removed keyframes; topk 0, 1, 8, 16 with fewer eligible than topk"""
    s = BR.scenario(name)
    _load(prob, s)
    rows = _run(prob, s)
    _check(rows, s)
    db = prob.debug_get("bow_db")
    n = len(s["kfs"])
    assert db[0] == n and db[1] == n - len({kf for a, kf in s["removed"] if a < n}) and db[4] > 0
    assert db[2] == sum(len(r["id0"]) for r in rows if "id0" in r) and db[3] == sum(len(r["id1"]) for r in rows if "id1" in r)
    if name == "removed":
        for a, kf in s["removed"]:
            for idx in range(a, n):
                assert rows[idx]["score_f32"][kf] == 0 and kf not in rows[idx]["cand"]["topk"][0] and rows[idx]["cand"]["kf_prev"][0] != kf


def _same_bits(a, b):
    for idx, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if k == "cand":
                for c in CAND:
                    assert np.array_equal(x["cand"][c], y["cand"][c], equal_nan=True), (idx, c)
            else:
                assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (idx, k)


def test_one_call_of_258_or_258_calls_of_one(pkg, prob):
    """across the growth of the database's buffers: the same bits, and the same database"""
    s = BR.scenario("db258")
    _load(prob, s)
    one = _run(prob, s)
    db1 = prob.debug_get("bow_db")
    other = pkg.new_problem()
    try:
        _load(other, s)
        many = _run(other, s, cuts=range(258))
        db2 = other.debug_get("bow_db")
    finally:
        other.close()
    _same_bits(one, many)
    assert list(db1[:4]) == list(db2[:4])
    _load(prob, s)
    _same_bits(one, _run(prob, s, cuts=(1, 63, 64, 65, 200, 257)))


def test_two_runs_give_the_same_bits(prob):
    s = BR.scenario("loop80")
    _load(prob, s)
    a = _run(prob, s)
    _load(prob, s)
    _same_bits(a, _run(prob, s))


def test_options_at_the_decisions_boundaries(prob):
    """n_eligible == lc_kf_max_dist fails the strict test, one less passes it; n_closest == lc_nkf_closest - 1 fails, n_closest passes"""
    s = BR.scenario("loop80")
    ref = BR.reference("loop80")
    idx = 79
    assert BR.margins_ok("loop80", idx) and ref[idx]["cand"]["is_candidate"] == 1
    n_el = ref[idx]["cand"]["n_eligible"]
    seen = {}
    for tag, over in (("at", dict(lc_kf_max_dist=n_el, lc_nkf_closest=0)), ("below", dict(lc_kf_max_dist=n_el - 1, lc_nkf_closest=0))):
        _load(prob, s)
        rows = _run(prob, s, **over)
        _check(rows, s, **over)
        seen[tag] = rows[idx]["cand"]
    assert seen["at"]["n_eligible"][0] == n_el and seen["at"]["is_candidate"][0] == 0 and seen["below"]["is_candidate"][0] == 1
    n_cl = ref[idx]["cand"]["n_closest"]
    for tag, over in (("short", dict(lc_nkf_closest=n_cl + 1)), ("enough", dict(lc_nkf_closest=n_cl))):
        _load(prob, s)
        rows = _run(prob, s, **over)
        _check(rows, s, **over)
        seen[tag] = rows[idx]["cand"]
    assert seen["short"]["n_closest"][0] == n_cl and seen["short"]["is_candidate"][0] == 0 and seen["short"]["kf_prev"][0] == -1
    assert seen["enough"]["is_candidate"][0] == 1 and seen["enough"]["kf_prev"][0] == ref[idx]["cand"]["kf_prev"]


def test_planted_revisit_feeds_the_verification(prob):
    """descriptors -> BoW -> scores -> top-k -> plba_verify_loop_candidates: the new keyframe revisits keyframe 5 (a candidate pair of
    tests/match_ref.py); it is found as kf_prev, and its topk, handed on unchanged, verifies that pair as the direct call does"""
    kf0, kf1, want = MR.loop_runs("pass_40_24")
    rng = np.random.default_rng(603)
    feats = []
    for i in range(12):
        if i == 5:
            feats.append(kf0)
        else:
            n, m = int(rng.integers(40, 70)), int(rng.integers(20, 40))
            feats.append(dict(pdesc=rng.integers(0, 256, (n, 32), dtype=np.uint8), P3=rng.uniform(1.0, 5.0, (n, 3)), ldesc=rng.integers(0, 256, (m, 32), dtype=np.uint8),
                              sPeP=rng.uniform(1.0, 5.0, (m, 6))))

    # vocabularies as training makes them, from the map's own descriptors: here every stored descriptor is a word (660 / 330 children of the root)
    vp, vl = BR.flat_vocabulary(np.concatenate([f["pdesc"] for f in feats]), 601), BR.flat_vocabulary(np.concatenate([f["ldesc"] for f in feats]), 602)
    prob.bow_set_vocabulary(0, vp); prob.bow_set_vocabulary(1, vl); prob._bow_loaded = None

    def bow_kf(f):
        return dict(pdesc=f["pdesc"], pl=rng.uniform(0, 640, (len(f["pdesc"]), 2)), ldesc=f["ldesc"], spl_epl=rng.uniform(0, 640, (len(f["ldesc"]), 4)))
    cov = [np.full(i, 100, np.int32) for i in range(13)]
    o = dict(lc_kf_dist=2, lc_kf_max_dist=3, lc_nkf_closest=0, topk=3)
    prob.bow_insert_keyframes([bow_kf(f) for f in feats], cov=cov[:12], **o)
    out = prob.bow_insert_keyframes([bow_kf(kf1)], cov=cov[12:], **o)
    assert out["first_index"] == 12 and out["is_candidate"][0] == 1 and out["kf_prev"][0] == 5 and out["topk"][0][0] == 5
    top = [int(t) for t in out["topk"][0] if t >= 0]
    assert len(top) == 3
    res = prob.verify_loop_candidates([feats[t] for t in top], [kf1] * len(top), RC.CAM)
    direct = prob.verify_loop_candidates([kf0], [kf1], RC.CAM)
    assert res["ratio_ok"][0] == 1 == want["ratio_ok"] and res["relpose"]["accepted"][0] == 1 and list(res["ratio_ok"][1:]) == [0, 0]
    assert np.array_equal(res["relpose"]["T_inc"][0], direct["relpose"]["T_inc"][0]) and np.array_equal(res["pt_match"][0], direct["pt_match"][0])


def test_window_state_untouched_and_one_wait(pkg, hip):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    s = BR.scenario("few_eligible")
    res = []
    for with_call in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_call:
            _load(p, s)
            o = _opts(s)
            before = p.debug_get("host_waits")[0]
            p.bow_insert_keyframes(s["kfs"][:7], cov=s["cov"][:7], **o)
            assert p.debug_get("host_waits")[0] == before + 1
            p.bow_insert_keyframes(s["kfs"][7:], cov=s["cov"][7:], want_bow=True, **o)
            assert p.debug_get("host_waits")[0] == before + 2
            p.bow_transform(1, [k["ldesc"] for k in s["kfs"][:3]])
            assert p.debug_get("host_waits")[0] == before + 3
            p.bow_remove_keyframe(2)
            assert p.debug_get("host_waits")[0] == before + 3
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_refusals_leave_everything_unchanged(pkg, prob):
    abi = pkg.abi
    s = BR.scenario("few_eligible")
    _load(prob, s)
    o0 = _opts(s)
    prob.bow_insert_keyframes(s["kfs"][:4], cov=s["cov"][:4], **o0)
    db = list(prob.debug_get("bow_db"))
    kf = s["kfs"][4]
    ip, up, dp = abi._ip, abi._up, abi._dp
    ps, ls = np.array([0, len(kf["pdesc"])], np.int32), np.array([0, len(kf["ldesc"])], np.int32)
    dP, dL = np.ascontiguousarray(kf["pdesc"]), np.ascontiguousarray(kf["ldesc"])
    pl, se = np.ascontiguousarray(kf["pl"]), np.ascontiguousarray(kf["spl_epl"])
    cs, cv = np.array([0, 4], np.int32), np.ascontiguousarray(s["cov"][4], np.int32)

    def attempt(B=1, ps=ps, ls=ls, dP=dP, dL=dL, pl=pl, se=se, cs=cs, cv=cv, opt=True, res=True, cand=True, cap=5, **o):
        op = abi.BowOptions()
        prob.lib.fn["bow_default_options"](C.byref(op))
        for k, v in dict(o0, **o).items():
            setattr(op, k, v)
        sc, sf, w, nz = np.full(5, 77.0), np.full(5, 77.0, np.float32), np.full(max(int(ps[-1]), 1), 77, np.int32), np.full(2, 77, np.int32)
        cd = (abi.BowCandidate * 1)()
        cd[0].kf_prev = 77
        r = abi.BowResult()
        r.first_index = 77; r.score_cap = cap
        r.score_p, r.score, r.score_f32, r.pt_word, r.pt_nnz = dp(sc), dp(sc), sf.ctypes.data_as(C.POINTER(C.c_float)), ip(w), ip(nz)
        if cand:
            r.cand = cd
        rc = prob.lib.fn["bow_insert_keyframes"](prob._h, C.byref(op) if opt else None, B, ip(ps), up(dP), dp(pl), ip(ls), up(dL), dp(se), ip(cs), ip(cv), C.byref(r) if res else None)
        assert rc == -1, (rc, o)
        assert r.first_index == 77 and (sc == 77).all() and (sf == 77).all() and (w == 77).all() and (nz == 77).all() and cd[0].kf_prev == 77
        assert list(prob.debug_get("bow_db")) == db

    attempt(B=0)
    attempt(ps=np.array([1, len(dP)], np.int32))
    attempt(ls=np.array([3, 1], np.int32))
    attempt(dP=None)
    attempt(pl=None)
    attempt(se=None)
    attempt(opt=False)
    attempt(res=False)
    attempt(cand=False)
    attempt(cap=4)
    attempt(cs=np.array([0, 3], np.int32))
    attempt(cv=-np.ones(4, np.int32))
    attempt(mode=3)
    attempt(topk=17)
    attempt(topk=-1)
    for k in ("lc_kf_dist", "lc_kf_max_dist", "lc_nkf_closest", "min_lm_cov_graph", "min_kf_local_map"):
        attempt(**{k: -1})
    big = np.zeros((8193, 32), np.uint8)
    attempt(ps=np.array([0, 8193], np.int32), dP=big, pl=np.zeros((8193, 2)))
    # no vocabulary for a kind the mode uses, on a problem of its own
    other = pkg.new_problem()
    try:
        other.bow_set_vocabulary(0, s["voc"][0])
        with pytest.raises(abi.PlbaError, match="no vocabulary"):
            other.bow_insert_keyframes(s["kfs"][:1])
        assert other.bow_insert_keyframes(s["kfs"][:1], mode=BR.POINTS)["first_index"] == 0
        with pytest.raises(abi.PlbaError, match="no vocabulary"):
            other.bow_transform(1, [kf["ldesc"]])
        # a malformed tree, an unsupported scoring: refused, and the database stays
        bad = dict(s["voc"][0]); bad["parent"] = bad["parent"].copy(); bad["parent"][3] = 3
        dup = dict(s["voc"][0]); dup["word_id"] = dup["word_id"].copy(); lv = BR.leaf_rows(dup); dup["word_id"][lv[1]] = dup["word_id"][lv[0]]
        noid = dict(s["voc"][0]); noid["word_id"] = noid["word_id"].copy(); noid["word_id"][lv[0]] = -1
        for v, kw in ((bad, {}), (dup, {}), (noid, {}), (s["voc"][0], dict(scoring=1)), (s["voc"][0], dict(weighting=4))):
            with pytest.raises(abi.PlbaError):
                other.bow_set_vocabulary(0, v, **kw)
            assert other.debug_get("bow_db")[0] == 1
        with pytest.raises(abi.PlbaError):
            other.bow_remove_keyframe(1)
        other.bow_remove_keyframe(0)
        assert list(other.debug_get("bow_db")[:2]) == [1, 0]
        other.bow_reset()
        assert list(other.debug_get("bow_db")[:4]) == [0, 0, 0, 0]
        assert other.bow_insert_keyframes(s["kfs"][:1], mode=BR.POINTS)["first_index"] == 0      # the vocabulary stayed
    finally:
        other.close()
    # the transform's refusals
    w, i, v, nz = np.full(len(dP), 77, np.int32), np.full(len(dP), 77, np.int32), np.full(len(dP), 77.0), np.full(1, 77, np.int32)
    for args in ((2, 1, ip(ps), up(dP)), (0, 0, ip(ps), up(dP)), (0, 1, ip(np.array([1, 2], np.int32)), up(dP)), (0, 1, ip(ps), None)):
        assert prob.lib.fn["bow_transform"](prob._h, *args, ip(w), ip(i), dp(v), ip(nz)) == -1
        assert (w == 77).all() and (i == 77).all() and (v == 77).all() and (nz == 77).all()
    assert list(prob.debug_get("bow_db")) == db
