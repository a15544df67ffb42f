"""plba_match_descriptors and plba_verify_loop_candidates on the device against tests/match_ref.py.  Every comparison of the matcher is for
integer equality: matches_12, the counts and nn3.  The composed call is held bit for bit to the sequence it replaces (two match calls,
the gate and the gather on the host, one plba_relative_pose call), its counts and its gate to the reference exactly, and the accepted
candidates' poses to tests/relpose_ref.py under the rule tests/test_relpose.py uses: the planted pairs of a `pass` candidate ARE a case
of tests/relpose_cases.py (tests/test_match_cpu.py asserts it by the reference alone), so the yardstick is that case's shared runs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from . import match_ref as MR
from . import relpose_cases as RC
from . import relpose_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _call(prob, cases, nnr=0.9, best_lr=1, nnr_b=None):
    return prob.match_descriptors([c["d1"] for c in cases], [c["d2"] for c in cases], nnr_b=nnr_b, want_nn3=True, nnr=nnr, best_lr=best_lr)


def _same(out, b, ref, what):
    assert np.array_equal(out["matches_12"][b], ref["matches_12"]), what
    assert int(out["n_matches"][b]) == ref["n"], (what, int(out["n_matches"][b]), ref["n"])
    assert np.array_equal(out["nn3"][b], ref["nn3"]), what


@pytest.mark.parametrize("name", [n for n in sorted(MR.CASES) if n.startswith("size_")])
def test_sizes_around_the_tiles(prob, name):
    """0 .. 3 rows and the values around the wave, the query tile (64) and the train tile (128) on either side; 257 x 63, 65 x 257, 513 x 300"""
    c, ref = MR.runs(name)
    _same(_call(prob, [c]), 0, ref, name)


@pytest.mark.parametrize("name", ["float_pin", "tie_rule", "all_equal", "one_way"])
def test_boundary_cases(prob, name):
    c, ref = MR.runs(name)
    out = _call(prob, [c], c["nnr"], c["best_lr"])
    _same(out, 0, ref, name)
    if name == "float_pin":      # (4, 5) and (8, 10) at 0.8f: a double evaluation would match both
        assert list(out["matches_12"][0]) == [-1, -1] and [tuple(t) for t in out["nn3"][0]] == [(1, 4, 5), (3, 8, 10)]
    if name == "all_equal":
        assert (out["matches_12"][0] == -1).all() and (out["nn3"][0] == 0).all()


def test_per_problem_ratio(prob):
    names = ["size_65_63", "size_129_129", "size_3_65", "size_64_64", "float_pin"]
    nnr_b = [0.9, 0.7, 1.3, 0.8, 0.81]
    out = _call(prob, [MR.runs(n)[0] for n in names], nnr=0.5, nnr_b=nnr_b)
    for b, (n, r) in enumerate(zip(names, nnr_b)):
        c = MR.runs(n)[0]
        _same(out, b, MR.match(c["d1"], c["d2"], r, True), (n, r))
    assert out["n_matches"][4] == 2      # 5 x 0.81f is above 4 in float too: the pin case matches once the ratio leaves the boundary


SMALL = ["size_0_0", "size_1_1", "size_3_65", "size_65_3", "size_63_65", "size_64_64", "size_65_63", "size_65_64", "size_0_64", "size_64_0", "size_1_65",
         "size_2_2", "size_129_129", "all_equal"]


@pytest.fixture(scope="module")
def alone(prob):
    return {n: _call(prob, [MR.runs(n)[0]]) for n in SMALL}


@pytest.mark.parametrize("B", [1, 2, 65, 257])
def test_batch_is_the_problems_alone(prob, alone, B):
    """mixed sizes in one call, an empty problem and a one-row problem among them: every problem bit-identical to itself called alone, and
    to the reference"""
    names = [SMALL[(5 * b + b // 14) % len(SMALL)] for b in range(B)]
    if B >= 2:
        names[0], names[1] = "size_0_0", "size_1_1"
    out = _call(prob, [MR.runs(n)[0] for n in names])
    for b, n in enumerate(names):
        for k in ("matches_12", "nn3"):
            assert np.array_equal(out[k][b], alone[n][k][0]), (b, n, k)
        assert out["n_matches"][b] == alone[n]["n_matches"][0], (b, n)
        _same(out, b, MR.runs(n)[1], (b, n))


def test_two_calls_give_the_same_bits(prob):
    cases = [MR.runs(n)[0] for n in ("size_513_300", "size_257_63", "size_65_257")]
    a, b = _call(prob, cases), _call(prob, cases)
    for k in ("matches_12", "nn3"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k
    assert np.array_equal(a["n_matches"], b["n_matches"])


def _loop_call(prob, names, **opts):
    cands = [MR.loop_runs(n, **opts) for n in names]
    return cands, prob.verify_loop_candidates([c[0] for c in cands], [c[1] for c in cands], RC.CAM, **opts)


def test_window_state_untouched_and_one_wait(pkg, hip):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    res = []
    for with_call in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_call:
            before = p.debug_get("host_waits")[0]
            out = _call(p, [MR.runs("size_257_63")[0], MR.runs("size_0_0")[0]])
            assert p.debug_get("host_waits")[0] == before + 1
            _same(out, 0, MR.runs("size_257_63")[1], "size_257_63")
            _, lo = _loop_call(p, ["pass_40_24", "fail_points", "pass_129_70"])
            assert p.debug_get("host_waits")[0] == before + 2
            assert list(lo["ratio_ok"]) == [1, 0, 1] and list(lo["relpose"]["accepted"]) == [1, 0, 1]
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_refusals_leave_the_outputs_untouched(pkg, prob):
    abi = pkg.abi
    c = MR.runs("size_65_63")[0]
    dA, dB = np.ascontiguousarray(c["d1"]), np.ascontiguousarray(c["d2"])
    sa, sb = np.array([0, len(dA)], np.int32), np.array([0, len(dB)], np.int32)
    ip, up = abi._ip, abi._up
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))

    def attempt(B=1, sa=sa, sb=sb, dA=dA, dB=dB, nnr_b=None, opt=True, out=True, cnt=True, **o):
        op = abi.MatchOptions()
        prob.lib.fn["match_default_options"](C.byref(op))
        for k, v in o.items():
            setattr(op, k, v)
        m, n, nn = np.full(len(c["d1"]), 77, np.int32), np.full(2, 77, np.int32), np.full(3 * len(c["d1"]), 77, np.int32)
        rc = prob.lib.fn["match_descriptors"](prob._h, C.byref(op) if opt else None, B, ip(sa), up(dA), ip(sb), up(dB), fp(nnr_b), ip(m) if out else None,
                                              ip(n) if cnt else None, ip(nn))
        assert rc == -1, rc      # PLBA_ERR_INVALID
        assert (m == 77).all() and (n == 77).all() and (nn == 77).all()
    attempt(B=0)
    attempt(sa=np.array([0, -1], np.int32))
    attempt(sb=np.array([1, len(dB)], np.int32))
    attempt(B=2, sa=np.array([0, len(dA), len(dA) - 1], np.int32), sb=np.array([0, len(dB), len(dB)], np.int32))
    attempt(sa=None)
    attempt(dA=None)
    attempt(dB=None)
    attempt(out=False)
    attempt(cnt=False)
    attempt(opt=False)
    attempt(nnr=float("nan"))
    attempt(nnr=float("inf"))
    attempt(nnr=0.0)
    attempt(nnr=-0.9)
    attempt(nnr_b=np.array([0.0], np.float32))
    attempt(nnr_b=np.array([np.nan], np.float32))
    _same(_call(prob, [c]), 0, MR.runs("size_65_63")[1], "the handle still works")


def test_loop_refusals_leave_the_outputs_untouched(pkg, prob):
    abi = pkg.abi
    kf0, kf1, _ = MR.loop_runs("pass_40_24")
    f8 = lambda a: np.ascontiguousarray(a, np.float64)
    arr = dict(dPA=np.ascontiguousarray(kf0["pdesc"]), P3=f8(kf0["P3"]), dPB=np.ascontiguousarray(kf1["pdesc"]), uv=f8(kf1["uv"]),
               dLA=np.ascontiguousarray(kf0["ldesc"]), pq=f8(kf0["sPeP"]), dLB=np.ascontiguousarray(kf1["ldesc"]), l3=f8(kf1["l3"]))
    st = dict(pa=np.array([0, len(arr["dPA"])], np.int32), pb=np.array([0, len(arr["dPB"])], np.int32), la=np.array([0, len(arr["dLA"])], np.int32),
              lb=np.array([0, len(arr["dLB"])], np.int32))
    dp, ip, up = abi._dp, abi._ip, abi._up

    def attempt(B=1, opt=True, out=True, set_opt=None, **kw):
        a = dict(arr); s = dict(st)
        for k, v in kw.items():
            (a if k in a else s)[k] = v
        op = abi.LoopOptions()
        prob.lib.fn["loop_default_options"](C.byref(op))
        if set_opt:
            set_opt(op)
        res = (abi.LoopResult * 2)()
        C.memset(res, 0x5A, C.sizeof(res))
        mp, ml = np.full(len(arr["dPA"]), 77, np.int32), np.full(len(arr["dLA"]), 77, np.int32)
        qp, ql = np.full(len(arr["dPA"]), 7, np.uint8), np.full(len(arr["dLA"]), 7, np.uint8)
        rc = prob.lib.fn["verify_loop_candidates"](prob._h, C.byref(op) if opt else None, B, ip(s["pa"]), up(a["dPA"]), dp(a["P3"]), ip(s["pb"]), up(a["dPB"]), dp(a["uv"]),
                                                   ip(s["la"]), up(a["dLA"]), dp(a["pq"]), ip(s["lb"]), up(a["dLB"]), dp(a["l3"]), *[float(v) for v in RC.CAM],
                                                   ip(mp), ip(ml), up(qp), up(ql), res if out else None)
        assert rc == -1, rc
        assert bytes(res) == b"\x5a" * C.sizeof(res) and (mp == 77).all() and (ml == 77).all() and (qp == 7).all() and (ql == 7).all()
    bad = arr["uv"].copy(); bad[5, 1] = np.nan
    attempt(B=0)
    attempt(pa=np.array([1, len(arr["dPA"])], np.int32))
    attempt(lb=np.array([0, -2], np.int32))
    attempt(la=None)
    attempt(dPB=None)
    attempt(pq=None)
    attempt(uv=bad)
    attempt(out=False)
    attempt(opt=False)
    attempt(set_opt=lambda o: setattr(o.match_ln, "nnr", 0.0))
    attempt(set_opt=lambda o: setattr(o, "lc_inlier_ratio", float("nan")))
    attempt(set_opt=lambda o: setattr(o.relpose, "protocol", 2))
    attempt(set_opt=lambda o: setattr(o.relpose, "max_iters", -1))


# ---- plba_verify_loop_candidates -------------------------------------------------------------------------------------------------------------
RP_KEYS = ("T_inc", "pose_inc", "H", "e", "cov_eig", "t", "r", "n_inliers", "iters", "status", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot")


def _sequence(prob, cands, **opts):
    """what the composed call replaces: two plba_match_descriptors calls, the gate and the gather on the host (match_ref's), one
    plba_relative_pose call; results in the composed call's layout"""
    o = dict(MR.LOOP_DEFAULTS); o.update(opts)
    B = len(cands)
    rows = lambda k, key: MR._rows(k.get(key))
    none = lambda ks, key: dict(matches_12=[np.full(len(rows(k, key)), -1, np.int32) for k in ks], n_matches=np.zeros(B, np.int32))
    k0s, k1s = [c[0] for c in cands], [c[1] for c in cands]
    mp = prob.match_descriptors([rows(k, "pdesc") for k in k0s], [rows(k, "pdesc") for k in k1s], nnr=o["nnr_pt"], best_lr=o["best_lr"]) if o["use_points"] else none(k0s, "pdesc")
    ml = prob.match_descriptors([rows(k, "ldesc") for k in k0s], [rows(k, "ldesc") for k in k1s], nnr=o["nnr_ln"], best_lr=o["best_lr"]) if o["use_lines"] else none(k0s, "ldesc")
    out = dict(pt_match=mp["matches_12"], ln_match=ml["matches_12"], common_pt=np.asarray(mp["n_matches"], np.int32), common_ls=np.asarray(ml["n_matches"], np.int32),
               inl_ratio_pt=np.zeros(B), inl_ratio_ls=np.zeros(B), ratio_ok=np.zeros(B, np.int32), pt_inlier=[], ln_inlier=[])
    feats = []
    for b, (k0, k1) in enumerate(zip(k0s, k1s)):
        rp = MR.inlier_ratio(out["common_pt"][b], len(rows(k0, "pdesc")), len(rows(k1, "pdesc")))
        rl = MR.inlier_ratio(out["common_ls"][b], len(rows(k0, "ldesc")), len(rows(k1, "ldesc")))
        th = o["lc_inlier_ratio"]
        ok = (rp > th and rl > th) if (o["use_points"] and o["use_lines"]) else (rp > th) if o["use_points"] else (rl > th) if o["use_lines"] else False
        out["inl_ratio_pt"][b], out["inl_ratio_ls"][b], out["ratio_ok"][b] = rp, rl, int(ok)
        g = MR.gather(k0, k1, out["pt_match"][b], out["ln_match"][b])
        if not ok:      # handed over with no features
            g = dict(g, P3=np.zeros((0, 3)), uv=np.zeros((0, 2)), pq=np.zeros((0, 6)), l3=np.zeros((0, 3)))
        feats.append(g)
    rp_opts = {k: v for k, v in opts.items() if k not in MR.LOOP_DEFAULTS}
    r = prob.relative_pose([g["P3"] for g in feats], [g["uv"] for g in feats], [g["pq"] for g in feats], [g["l3"] for g in feats], RC.CAM, **rp_opts)
    out["relpose"] = {k: np.array(r[k]) for k in RP_KEYS}
    for b, g in enumerate(feats):
        pi, li = np.zeros(len(out["pt_match"][b]), bool), np.zeros(len(out["ln_match"][b]), bool)
        if out["ratio_ok"][b]:
            pi[g["ip"]] = r["pt_inlier"][b]; li[g["il"]] = r["ln_inlier"][b]
        else:      # the reference returns false without estimating: the composed call reports a zero result
            for k in RP_KEYS:
                out["relpose"][k][b] = 0
        out["pt_inlier"].append(pi); out["ln_inlier"].append(li)
    return out


def _assert_loop(name_list, cands, out, seq):
    for k in ("common_pt", "common_ls", "ratio_ok", "inl_ratio_pt", "inl_ratio_ls"):
        assert np.array_equal(out[k], seq[k], equal_nan=True), k
    for k in RP_KEYS:
        assert np.array_equal(out["relpose"][k], seq["relpose"][k], equal_nan=True), k
    for b, (n, (kf0, kf1, ref)) in enumerate(zip(name_list, cands)):
        for k in ("pt_match", "ln_match", "pt_inlier", "ln_inlier"):
            assert np.array_equal(out[k][b], seq[k][b]), (b, n, k)
        for k in ("common_pt", "common_ls", "ratio_ok"):      # against the reference, exactly
            assert int(out[k][b]) == ref[k], (b, n, k)
        for k in ("inl_ratio_pt", "inl_ratio_ls"):
            assert np.array_equal(out[k][b], ref[k], equal_nan=True), (b, n, k)
        assert np.array_equal(out["pt_match"][b], ref["pt_match"]) and np.array_equal(out["ln_match"][b], ref["ln_match"]), (b, n)
        if not ref["ratio_ok"]:
            assert all(not np.asarray(out["relpose"][k][b]).any() for k in RP_KEYS) and not out["pt_inlier"][b].any() and not out["ln_inlier"][b].any(), (b, n)


def _hold_pose(out, b, name, ref):
    """an accepted `pass` candidate against the reference runs of the relative-pose case its pairs are, under test_relpose.py's rule"""
    case, r64, rw = RC.runs(MR.LOOP[name][0])
    res = RC.as_result(dict(out["relpose"], pt_inlier=[out["pt_inlier"][b][ref["ip"]]] * (b + 1), ln_inlier=[out["ln_inlier"][b][ref["il"]]] * (b + 1)), b)
    RR.hold(res, r64, rw, "hip-loop", name)


LOOP_BATCH = {1: ["pass_129_70"], 3: ["pass_40_24", "fail_points", "boundary"],
              65: [sorted(MR.LOOP)[(3 * b + b // 8) % len(MR.LOOP)] for b in range(65)]}


@pytest.mark.parametrize("B", [1, 3, 65])
def test_loop_candidates_are_the_sequence_and_the_reference(prob, B):
    names = LOOP_BATCH[B]
    if B == 65:
        assert set(names) == set(MR.LOOP)      # a candidate that fails on points, one on lines, the boundary, keyframes without lines
    before = prob.debug_get("host_waits")[0]
    cands, out = _loop_call(prob, names)
    assert prob.debug_get("host_waits")[0] == before + 1
    seq = _sequence(prob, cands)
    _assert_loop(names, cands, out, seq)
    held = set()
    for b, n in enumerate(names):
        if n.startswith("pass_") and n not in held:
            assert out["ratio_ok"][b] == 1 and out["relpose"]["accepted"][b] == 1, (b, n)
            _hold_pose(out, b, n, cands[b][2])
            held.add(n)
    if B == 3:
        assert list(out["ratio_ok"]) == [1, 0, 0] and out["inl_ratio_pt"][2] == 30.0 and out["common_pt"][2] == 3


@pytest.mark.parametrize("opts", [dict(use_lines=0), dict(use_points=0), dict(best_lr=0, nnr_pt=0.8, nnr_ln=0.95), dict(lc_inlier_ratio=75.0, protocol=1)],
                         ids=["no_lines", "no_points", "one_way", "gate_75_p1"])
def test_loop_options(prob, opts):
    names = sorted(MR.LOOP)
    cands, out = _loop_call(prob, names, **opts)
    seq = _sequence(prob, cands, **opts)
    _assert_loop(names, cands, out, seq)
    b = names.index("no_lines_65")
    if opts.get("use_lines") == 0:      # the keyframes without line segments pass on their points alone, and those are the relative-pose case
        assert out["ratio_ok"][b] == 1 and (out["ln_match"][names.index("pass_40_24")] == -1).all()
        _hold_pose(out, b, "no_lines_65", cands[b][2])
    if opts.get("use_points") == 0:
        assert (out["common_pt"] == 0).all() and all((m == -1).all() for m in out["pt_match"]) and out["ratio_ok"][b] == 0
    if "lc_inlier_ratio" in opts:
        assert not out["ratio_ok"].any()


def test_two_loop_calls_give_the_same_bits(prob):
    names = ["pass_300_100", "pass_outliers", "fail_lines", "pass_40_24"]
    (_, a), (_, b) = _loop_call(prob, names), _loop_call(prob, names)
    for k in RP_KEYS:
        assert np.array_equal(a["relpose"][k], b["relpose"][k], equal_nan=True), k
    for k in ("pt_match", "ln_match", "pt_inlier", "ln_inlier"):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k
    # a candidate's result does not depend on its neighbours
    _, c = _loop_call(prob, ["pass_outliers"])
    for k in RP_KEYS:
        assert np.array_equal(a["relpose"][k][1], c["relpose"][k][0], equal_nan=True), k
    assert np.array_equal(a["pt_inlier"][1], c["pt_inlier"][0]) and np.array_equal(a["ln_inlier"][1], c["ln_inlier"][0])
