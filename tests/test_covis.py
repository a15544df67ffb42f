"""plba_covis_* on the device against the numpy reference (tests/covis_ref.py): CSR rows, the dense column, the edge list and the local-map
flags for exact equality on every map of covis_ref.CASES (degenerate maps, stride and tile boundaries, counter width, thresholds, dead
keyframes, a trajectory), the measurements inside the derived bound of the wide evaluation, the graph handed to
plba_optimize_pose_graph, the column handed to plba_bow_insert_keyframes, refusals, the number of blocking waits, and the rest of the
problem left alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from . import bow_ref as BR
from . import covis_ref as CR

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _set(p, m):
    return p.covis_set_map(m["K"], m["pt_start"], m["pt_kf"], m["ln_start"], m["ln_kf"], live=m["live"])


def _answers(p, m, q, opts, P):
    loops = np.asarray(q["loops"], np.int32).reshape(-1, 2)
    ei, ej, Z = p.covis_pose_graph(P[:q["nv"]], loop_ij=loops if len(loops) else None, loop_meas12=CR.loop_meas(P, loops) if len(loops) else None, **(opts or {}))
    return dict(rows=p.covis_rows(q["rows"], q["min_count"]), cov=p.covis_column(q["idx"]), ei=ei, ej=ej, meas=Z, local=p.covis_local_map(q["kf"], **(opts or {})))


@pytest.mark.parametrize("name", CR.CASES)
def test_against_the_reference(prob, name):
    from . import lba_ref
    m = CR.case(name)
    q = CR.queries(m, name)
    P = CR.poses(m["K"])
    info = _set(prob, m)
    Ep, El = len(m["pt_kf"]), len(m["ln_kf"])
    assert list(info[:5]) == [m["K"], int(CR.live_of(m).sum()), len(m["pts"]) + len(m["lns"]), Ep, El] and info[5] >= 8 * (Ep + El) + 5 * m["K"]
    assert np.array_equal(prob.debug_get("covis_map"), info)
    for opts in (CR.OPTION_SETS if m["K"] <= 400 else CR.OPTION_SETS[:1]):
        got = _answers(prob, m, q, opts, P)
        want = CR.expected(m, q, opts)
        assert CR.same(got, want) is None, (name, opts, CR.same(got, want))
        n_cov = len(got["ei"]) - len(q["loops"])
        if m["K"] <= 400 and n_cov:
            dt = lba_ref.wide()
            Zw = CR.relative_pose(P, got["ei"][:n_cov], got["ej"][:n_cov], dt)
            err = np.array(np.abs(got["meas"][:n_cov].astype(np.longdouble if dt != "mp" else object) - Zw), dtype=np.float64)
            bound = CR.meas_bound(P, got["ei"][:n_cov], got["ej"][:n_cov])
            print("%s: meas12 error / bound %.3f" % (name, (err / bound).max()))
            assert (err <= bound).all()
        if q["loops"]:
            assert np.array_equal(got["meas"][n_cov:], CR.loop_meas(P, q["loops"]))
    # the whole symmetric graph
    if m["K"] <= 400:
        rs, col, cnt = prob.covis_rows(np.arange(m["K"]))
        S = np.zeros((m["K"], m["K"]), np.int64)
        for r in range(m["K"]):
            S[r, col[rs[r]:rs[r + 1]]] = cnt[rs[r]:rs[r + 1]]
            assert np.all(np.diff(col[rs[r]:rs[r + 1]]) > 0)
        assert np.array_equal(S, CR.recount_dense(m))


def test_min_count_zero_one_and_above(prob):
    m = CR.case("thresholds")
    _set(prob, m)
    kf = np.arange(m["K"])[::-1]
    r0, r1, r75 = prob.covis_rows(kf, 0), prob.covis_rows(kf, 1), prob.covis_rows(kf, 75)
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b)
    for mc, got in ((0, r0), (75, r75), (150, prob.covis_rows(kf, 150)), (152, prob.covis_rows(kf, 152))):
        for a, b in zip(got, CR.rows_ref(m, kf, mc)):
            assert np.array_equal(a, b), mc
    assert len(r75[1]) == 2 * 7 and len(prob.covis_rows(kf, 152)[1]) == 2


def test_dead_keyframes(prob):
    m = CR.case("dead")
    _set(prob, m)
    K = m["K"]
    rs, col, cnt = prob.covis_rows(np.arange(K))
    dead = np.flatnonzero(m["live"] == 0)
    for k in dead:
        assert rs[k + 1] == rs[k] and k not in col and not prob.covis_column(k).any()
        loc = prob.covis_local_map(min(k + 1, K - 2))
        assert loc["kf_local"][k] == 0
        assert prob.covis_local_map(k)["counts"][0] == CR.local_map_ref(m, k)["counts"][0] and prob.covis_local_map(k)["kf_local"][k] == 0
    ei, ej, _ = prob.covis_pose_graph(CR.poses(K))
    assert not np.isin(ei, dead).any() and not np.isin(ej, dead).any()
    pairs = set(zip(ei.tolist(), ej.tolist()))
    assert (5, 6) in pairs and (6, 7) not in pairs and (7, 8) not in pairs and (19, 20) not in pairs and (20, 21) not in pairs and (21, 22) not in pairs
    assert prob.covis_column(K - 2)[dead[:-1]].tolist() == [0, 0, 0]


def test_order_permutation_and_repetition(prob):
    m = CR.case("traj200")
    kf = np.array(list(range(199, 150, -1)) + [170, 3, 3], np.int32)
    _set(prob, m)
    a = prob.covis_rows(kf, 10)
    b = prob.covis_rows(kf, 10)
    rng = np.random.default_rng(5)
    pts, lns = [m["pts"][i] for i in rng.permutation(len(m["pts"]))], [m["lns"][i] for i in rng.permutation(len(m["lns"]))]
    _set(prob, CR.make_map(m["K"], pts, lns))
    c = prob.covis_rows(kf, 10)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    P = CR.poses(m["K"])
    g1, g2 = prob.covis_pose_graph(P), prob.covis_pose_graph(P)
    for x, y in zip(g1, g2):
        assert np.array_equal(x, y)
    # row r of the answer is keyframe kf[r]'s, repeats included
    rs = a[0]
    r1, r2 = len(kf) - 2, len(kf) - 1
    assert np.array_equal(a[1][rs[r1]:rs[r1 + 1]], a[1][rs[r2]:rs[r2 + 1]]) and rs[r2 + 1] == len(a[1])


def test_pose_graph_is_consistent_with_its_poses(pkg, prob):
    """without loop edges the graph's chi2 at its own poses is at rounding level: 6 residuals an edge, each within 64 u max|pose|"""
    m = CR.case("traj60")
    _set(prob, m)
    P = CR.poses(m["K"])
    ei, ej, Z = prob.covis_pose_graph(P)
    want = CR.edge_loop(CR.recount_dense(m), CR.live_of(m), m["K"])
    assert np.array_equal(ei, want[0]) and np.array_equal(ej, want[1]) and len(ei) > 59
    fixed = np.zeros(m["K"], np.uint8); fixed[0] = 1
    _, st, _ = prob.pgo(P, ei, ej, Z, fixed=fixed, iters=0)
    bound = 36 * len(ei) * (64 * U) ** 2 * np.abs(P).max() ** 2
    print("chi2_initial %.3e, bound %.3e" % (st["chi2_initial"], bound))
    assert st["chi2_initial"] <= bound


def test_pose_graph_with_loop_edges_into_the_sparse_solver(pkg, hip):
    """the device-built graph and the reference-built one (literal double loop, float64 measurements) through pgo_solver = 1: the same
    iteration and trial counts, poses within the bar tests/test_pgo.py holds between two paths after a few iterations"""
    m = CR.case("traj60")
    K = m["K"]
    P = CR.poses(K)
    rng = np.random.default_rng(9)
    drift = P.copy()
    drift[:, 9:] += np.cumsum(rng.normal(size=(K, 3)) * 2e-3, axis=0)      # the drifted estimates the graph is built from
    loops = np.array([(0, K - 1), (1, K - 2), (3, K - 1)], np.int32)
    lm = CR.loop_meas(P, loops)      # the loop edges carry the undrifted relative poses
    p = pkg.new_problem(pgo_solver=1)
    try:
        _set(p, m)
        ei, ej, Z = p.covis_pose_graph(drift, loop_ij=loops, loop_meas12=lm)
        rei, rej = CR.edge_loop(CR.recount_dense(m), CR.live_of(m), K, None, [tuple(l) for l in loops])
        assert np.array_equal(ei, rei) and np.array_equal(ej, rej) and np.array_equal(ei[-3:], loops[:, 0]) and np.array_equal(ej[-3:], loops[:, 1])
        n_cov = len(ei) - 3
        rZ = np.concatenate([CR.relative_pose(drift, rei[:n_cov], rej[:n_cov]).astype(np.float64), lm])
        fixed = np.zeros(K, np.uint8); fixed[0] = 1
        Xa, sa, _ = p.pgo(drift, ei, ej, Z, fixed=fixed, iters=4, user_lambda=1e-10, initial_guess=True)
        Xb, sb, _ = p.pgo(drift, rei, rej, rZ, fixed=fixed, iters=4, user_lambda=1e-10, initial_guess=True)
        assert p.debug_get("pgo_sparse")[0] == 1
    finally:
        p.close()
    assert (sa["iterations"], sa["trials"]) == (sb["iterations"], sb["trials"]) and sa["iterations"] > 0
    assert sa["chi2_final"] < sa["chi2_initial"]
    print("poses: %.3e" % np.abs(Xa - Xb).max())
    assert np.abs(Xa - Xb).max() <= 1e-8


def test_nv_below_K(prob):
    m = CR.case("traj200")
    _set(prob, m)
    P = CR.poses(m["K"])
    for nv in (1, 2, 57):
        ei, ej, Z = prob.covis_pose_graph(P[:nv])
        want = CR.edge_loop(CR.recount_dense(m), CR.live_of(m), nv)
        assert np.array_equal(ei, want[0]) and np.array_equal(ej, want[1]) and (len(ei) == 0 or ej.max() < nv)


def test_column_into_bow(pkg, hip):
    """plba_covis_column handed to plba_bow_insert_keyframes: the candidate equals, field for field, the one from the numpy column"""
    s = BR.scenario("few_eligible")
    n = len(s["kfs"])
    m = CR.trajectory(n, 23, per_kf=60)
    assert any((CR.column_ref(m, idx) >= 75).any() for idx in range(n)) and any((CR.column_ref(m, idx) < 75).any() for idx in range(1, n))
    o = dict(BR.DEFAULTS); o.update(s["opts"])
    res = []
    for dev_col in (True, False):
        p = pkg.new_problem()
        try:
            p.bow_set_vocabulary(0, s["voc"][0], weighting=s["weighting"][0]); p.bow_set_vocabulary(1, s["voc"][1], weighting=s["weighting"][1])
            _set(p, m)
            outs = []
            for idx in range(n):
                col = p.covis_column(idx) if dev_col else CR.column_ref(m, idx)
                assert col.dtype == np.int32 and len(col) == idx
                outs.append(p.bow_insert_keyframes([s["kfs"][idx]], cov=[col], **o))
            res.append(outs)
        finally:
            p.close()
    for a, b in zip(*res):
        for k in ("is_candidate", "kf_prev", "n_closest", "n_eligible", "best_score", "lc_min_score", "topk", "topk_score"):
            assert np.array_equal(a[k], b[k]), k


def test_local_map_neighbours_and_an_older_keyframe(prob):
    m = CR.case("traj200")
    _set(prob, m)
    for kf in (199, 120, 0, 5):
        for opts in (None, dict(min_kf_local_map=0), dict(min_lm_cov_graph=20, min_kf_local_map=6)):
            got, want = prob.covis_local_map(kf, **(opts or {})), CR.local_map_ref(m, kf, opts)
            for k in want:
                assert np.array_equal(got[k], want[k]), (kf, opts, k)
    # neighbours in the index with no shared landmark are local all the same
    iso = CR.make_map(9, [[0, 8], [8, 0]], [[1, 2]])
    _set(prob, iso)
    got = prob.covis_local_map(4)
    assert got["kf_local"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0] and got["counts"].tolist() == [7, 0, 1]
    assert got["pt_local"].tolist() == [0, 0] and got["ln_local"].tolist() == [1]
    _set(prob, m)


def _raw(pkg, p):
    abi = pkg.abi
    return abi, p.lib.fn, p._h, abi._ip, abi._up, abi._dp


def test_refusals_change_nothing(pkg, prob):
    abi, fn, h, ip, up, dp = _raw(pkg, prob)
    INVALID, STATE = -1, -2
    prob.covis_reset()
    # a query before any map
    rs = np.full(2, -7, np.int32); col = np.full(4, -7, np.int32); cnt = np.full(4, -7, np.int32)
    kf1 = np.zeros(1, np.int32)
    o = abi.CovisOptions(); fn["covis_default_options"](C.byref(o))
    ne = C.c_int(-7)
    P = CR.poses(10)
    fk = np.full(10, 9, np.uint8); fp = np.full(1000, 9, np.uint8); c3 = np.full(3, -7, np.int32)
    assert fn["covis_rows"](h, 1, ip(kf1), 0, ip(rs), 4, ip(col), ip(cnt)) == STATE
    assert fn["covis_column"](h, 1, ip(col)) == STATE
    assert fn["covis_pose_graph"](h, C.byref(o), 2, dp(P), 0, None, None, 4, ip(col), ip(cnt), dp(np.zeros(48)), C.byref(ne)) == STATE
    assert fn["covis_local_map"](h, C.byref(o), 0, up(fk), up(fp), up(fp), ip(c3)) == STATE
    assert (rs == -7).all() and (col == -7).all() and (cnt == -7).all() and ne.value == -7 and (fk == 9).all() and (c3 == -7).all()
    assert not prob.debug_get("covis_map").any()

    m = CR.case("thresholds")
    info = _set(prob, m)
    kf_all = np.arange(m["K"], dtype=np.int32)
    before = prob.covis_rows(kf_all)
    w0 = prob.debug_get("host_waits")[0]
    ps, pk, ls, lk = m["pt_start"], m["pt_kf"], m["ln_start"], m["ln_kf"]
    inf6 = np.full(6, -7.0)

    def set_map(K, live, Np, ps_, pk_, Nl, ls_, lk_):
        return fn["covis_set_map"](h, K, up(live), Np, ip(ps_), ip(pk_), Nl, ip(ls_), ip(lk_), dp(inf6))
    Np = len(ps) - 1
    bad = pk.copy(); bad[3] = m["K"]
    assert set_map(m["K"], None, Np, ps, bad, 0, None, None) == INVALID
    bad = pk.copy(); bad[0] = -1
    assert set_map(m["K"], None, Np, ps, bad, 0, None, None) == INVALID
    bad = ps.copy(); bad[0] = 1
    assert set_map(m["K"], None, Np, bad, pk, 0, None, None) == INVALID
    bad = ps.copy(); bad[5] = bad[4] - 1
    assert set_map(m["K"], None, Np, bad, pk, 0, None, None) == INVALID
    assert set_map(0, None, Np, ps, pk, 0, None, None) == INVALID
    assert set_map(-3, None, Np, ps, pk, 0, None, None) == INVALID
    big_p, big_l = np.array([0, 2 ** 31 - 1], np.int32), np.array([0, 1], np.int32)      # 2^31 observations in all: refused before a list is read
    assert set_map(m["K"], None, 1, big_p, pk, 1, big_l, pk) == INVALID
    assert set_map(m["K"], None, Np, ps, None, 0, None, None) == INVALID      # a missing array with a non-zero count
    assert set_map(m["K"], None, Np, None, pk, 0, None, None) == INVALID
    assert (inf6 == -7).all()
    assert np.array_equal(prob.debug_get("covis_map"), info)
    after = prob.covis_rows(kf_all)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)      # the resident map is the earlier one

    # rows
    w0 = prob.debug_get("host_waits")[0]
    rs = np.full(m["K"] + 1, -7, np.int32); col = np.full(64, -7, np.int32); cnt = np.full(64, -7, np.int32)
    for bad_kf in (m["K"], -1):
        kfb = kf_all.copy(); kfb[2] = bad_kf
        assert fn["covis_rows"](h, m["K"], ip(kfb), 0, ip(rs), 64, ip(col), ip(cnt)) == INVALID
    assert fn["covis_rows"](h, m["K"], None, 0, ip(rs), 64, ip(col), ip(cnt)) == INVALID
    assert fn["covis_rows"](h, m["K"], ip(kf_all), -1, ip(rs), 64, ip(col), ip(cnt)) == INVALID
    assert (rs == -7).all() and (col == -7).all() and (cnt == -7).all()
    need = len(before[1])
    assert fn["covis_rows"](h, m["K"], ip(kf_all), 0, ip(rs), need - 1, ip(col), ip(cnt)) == INVALID      # a capacity too small: the needed count, nothing else
    assert rs[m["K"]] == need and (rs[:m["K"]] == -7).all() and (col == -7).all() and (cnt == -7).all()
    assert fn["covis_rows"](h, m["K"], ip(kf_all), 0, ip(rs), need, ip(col), ip(cnt)) == 0
    assert np.array_equal(rs, before[0]) and np.array_equal(col[:need], before[1]) and (col[need:] == -7).all()
    assert fn["covis_column"](h, m["K"], ip(col)) == INVALID and fn["covis_column"](h, -1, ip(col)) == INVALID

    # pose graph
    K = m["K"]
    P = CR.poses(K)
    ei = np.full(64, -7, np.int32); ej = np.full(64, -7, np.int32); Z = np.full((64, 12), -7.0); ne = C.c_int(-7)
    loops = np.array([[0, 5], [2, 9]], np.int32); lmz = CR.loop_meas(P, loops)

    def pg(opt, nv, pose, n_loop, lij, lmeas, cap):
        return fn["covis_pose_graph"](h, C.byref(opt), nv, dp(pose), n_loop, ip(lij), dp(lmeas), cap, ip(ei), ip(ej), dp(Z), C.byref(ne))
    Pbig = CR.poses(K + 1)
    assert pg(o, K + 1, Pbig, 0, None, None, 64) == INVALID
    assert pg(o, 0, P, 0, None, None, 64) == INVALID
    for bad_loop in ([[0, K]], [[-1, 3]], [[4, 4]]):
        assert pg(o, K, P, 1, np.array(bad_loop, np.int32), lmz[:1].copy(), 64) == INVALID
    assert pg(o, K - 1, P, 1, np.array([[0, K - 1]], np.int32), lmz[:1].copy(), 64) == INVALID      # the range is nv's, not K's
    for bad_val in (np.nan, np.inf):
        Pn = P.copy(); Pn[3, 4] = bad_val
        assert pg(o, K, Pn, 0, None, None, 64) == INVALID
    for field in ("min_lm_ess_graph", "min_lm_cov_graph", "min_kf_local_map"):
        ob = abi.CovisOptions(); fn["covis_default_options"](C.byref(ob)); setattr(ob, field, -1)
        assert pg(ob, K, P, 0, None, None, 64) == INVALID
        assert fn["covis_local_map"](h, C.byref(ob), 0, up(fk), up(fp), up(fp), ip(c3)) == INVALID
    assert pg(o, K, P, 2, loops, None, 64) == INVALID
    assert fn["covis_local_map"](h, C.byref(o), K, up(fk), up(fp), up(fp), ip(c3)) == INVALID
    assert fn["covis_local_map"](h, C.byref(o), -1, up(fk), up(fp), up(fp), ip(c3)) == INVALID
    assert (ei == -7).all() and (ej == -7).all() and (Z == -7).all() and ne.value == -7 and (fk == 9).all() and (fp == 9).all() and (c3 == -7).all()
    want = CR.edge_loop(CR.recount_dense(m), CR.live_of(m), K, None, [tuple(l) for l in loops])
    assert pg(o, K, P, 2, loops, lmz, len(want[0]) - 1) == INVALID
    assert ne.value == len(want[0]) and (ei == -7).all() and (ej == -7).all() and (Z == -7).all()
    assert pg(o, K, P, 2, loops, lmz, len(want[0])) == 0 and ne.value == len(want[0])
    assert np.array_equal(ei[:ne.value], want[0]) and np.array_equal(ej[:ne.value], want[1]) and (ei[ne.value:] == -7).all()
    assert np.array_equal(prob.debug_get("covis_map"), info)


def test_state_waits_and_the_rest_of_the_problem(pkg, hip):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    m = CR.case("traj60")
    P = CR.poses(m["K"])
    res = []
    for with_calls in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_calls:
            abi, fn, h, ip, up, dp = _raw(pkg, p)
            bow = list(p.debug_get("bow_db"))
            n = p.debug_get("host_waits")[0]
            _set(p, m)
            assert p.debug_get("host_waits")[0] == n + 1
            rs, col, cnt = p.covis_rows(np.arange(m["K"]), cap=200000)
            assert p.debug_get("host_waits")[0] == n + 2 and len(col) > 0
            p.covis_column(40)
            assert p.debug_get("host_waits")[0] == n + 3
            p.covis_pose_graph(P, edge_cap=20000)
            assert p.debug_get("host_waits")[0] == n + 4
            p.covis_local_map(30)
            assert p.debug_get("host_waits")[0] == n + 5
            r1 = np.zeros(2, np.int32)
            assert fn["covis_rows"](h, 1, ip(np.array([m["K"]], np.int32)), 0, ip(r1), 0, None, None) == -1      # refused: no wait
            p.debug_get("covis_map")
            assert p.debug_get("host_waits")[0] == n + 5
            p.covis_reset()
            assert p.debug_get("host_waits")[0] == n + 5 and not p.debug_get("covis_map").any()
            _set(p, m)
            assert list(p.debug_get("bow_db")) == bow
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
