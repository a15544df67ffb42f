"""plba_pose_graph_marginals on the device: the marginal covariances of a whole pose graph from the sparse factor (Takahashi's selected
inversion down the elimination tree, csrc/plba_pgo_cov.hip) against the extended-precision inverse of the device's own H
(tests/pgo_cov_ref.py), the exact properties the header states, determinism and isolation, failure and refusal, and a 20 000-keyframe
graph.

Bars.  Hard: E_sel <= 32 n u kappa_s (rule (b) of tests/marginals_exact.py).  Second: E_sel <= 8 x the largest E of the three fp64 CPU
inverses on the same entries (8 = the project's FACTOR for another summation order of the same sums)."""
import ctypes as C

import numpy as np
import pytest

from . import pgo_cov_ref as PC
from . import pgo_ref
from . import solver_ref as R

pytestmark = pytest.mark.gpu
DUMP = 32      # PLBA_DIAG_PGO_COV_DUMP
LAM = 1e-10


def _call(pkg, g, pairs=None, diag=DUMP, p=None, **opts):
    """(result dict, "pgo_cov" record, dumped Hblk)"""
    assert "pose_graph_marginals" in pkg.abi.SIGNATURES, "plba_pose_graph_marginals is missing"
    own = p is None
    if own:
        p = pkg.new_problem(diag=diag, **opts)
    try:
        out = p.pgo_marginals(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], pairs=pairs)
        return out, p.debug_get("pgo_cov").copy(), p.debug_get("pgo_cov_H").copy()
    finally:
        if own:
            p.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _exact_properties(g, pairs, out, fill):
    vs, ps, ns = PC.statuses(g, pairs, fill)
    assert np.array_equal(out["v_status"], vs) and np.array_equal(out["pair_status"], ps) and np.array_equal(out["n_status"], ns)
    V, Pc = out["v_cov"], out["pair_cov"]
    assert np.all(V[vs == 1] == 0) and np.all(np.isnan(V[vs == 2])) and np.all(np.isfinite(V[vs == 0]))
    assert np.all(Pc[ps == 1] == 0) and np.all(np.isnan(Pc[ps >= 2])) and np.all(np.isfinite(Pc[ps == 0]))
    assert np.array_equal(_bits(V[vs == 0]), _bits(np.swapaxes(V[vs == 0], 1, 2)))                 # exactly symmetric
    assert np.all(np.einsum("kii->ki", V[vs == 0]) > 0)
    where = {}
    for k, (i, j) in enumerate(pairs.tolist()):
        if ps[k] != 0:
            continue
        if (j, i) in where:
            assert np.array_equal(_bits(Pc[k]), _bits(Pc[where[(j, i)]].T)), (i, j)           # the bitwise transpose
        if (i, j) in where:
            assert np.array_equal(_bits(Pc[k]), _bits(Pc[where[(i, j)]])), (i, j)             # a repeated pair
        if i == j:
            assert np.array_equal(_bits(Pc[k]), _bits(V[i])), i                               # (i, i) is the vertex block
        where.setdefault((i, j), k)
    return vs, ps


def _entries(g, pairs, out, vs, ps, cols=None):
    """the reported blocks as (i rank, j rank, block), those with their column vertex's rank in `cols` when given"""
    fr, _ = PC.free_ranks(g)
    ent = [(int(fr[v]), int(fr[v]), out["v_cov"][v]) for v in np.flatnonzero(vs == 0)]
    ent += [(int(fr[i]), int(fr[j]), out["pair_cov"][k]) for k, (i, j) in enumerate(pairs.tolist()) if ps[k] == 0]
    return [e for e in ent if cols is None or e[1] in cols]


def _accuracy(name, g, pairs, out, Hb, vs, ps, cols=None):
    H = PC.dense_H(g, Hb)
    H64 = PC.dense_H(g)
    assert np.abs(H - H64).max() <= 1e-12 * np.abs(H64).max()              # the dump is the H of the graph, to assembly rounding
    n = H.shape[0] // 6
    ent = _entries(g, pairs, out, vs, ps, cols)
    ext = PC.exact_columns(H, range(n) if cols is None else cols)
    d = np.sqrt(np.diag(H))
    E = PC.e_sel(ent, ext, d)
    ks = R.kappa_s(H)
    bound = PC.bound(H.shape[0], ks)
    cpu = max(PC.e_cpu(H, [(i, j) for i, j, _ in ent], ext))
    print("%s: dims %d entries %d kappa_s %.3e E_sel %.3e bound %.3e E_cpu %.3e ratio %.2f" % (name, H.shape[0], len(ent), ks, E, bound, cpu, E / cpu))
    assert E <= bound, (E, bound)
    assert E <= PC.FACTOR * cpu, (E, cpu)


@pytest.mark.parametrize("name", PC.SMALL)
def test_accuracy_and_exact_properties(pkg, orc, hip, name):
    g = PC.graph(name)
    pairs, fill = PC.request(name, g)
    out, rec, Hb = _call(pkg, g, pairs)
    fr, free = PC.free_ranks(g)
    assert rec[0] == 1 and rec[1] == len(free) and rec[2] >= 1 and rec[3] >= 1 and rec[5] >= 6
    if name == "complete80":
        assert rec[2] == 1 and rec[5] == 6 * 79                              # one front, wider than LDS holds, a 10-row tile tail
    if name in ("chain16", "chain17"):
        assert rec[2] == (1 if name == "chain16" else 3)                     # either side of SP_LEAF
    vs, ps = _exact_properties(g, pairs, out, fill)
    _accuracy(name, g, pairs, out, Hb, vs, ps)


def test_accuracy_on_300_keyframes_sampled_columns(pkg, orc, hip):
    g = PC.graph("cov300")
    pairs, fill = PC.request("cov300", g)
    out, rec, Hb = _call(pkg, g, pairs)
    vs, ps = _exact_properties(g, pairs, out, fill)
    n = int(rec[1])
    assert n == 298 and rec[2] > 1 and rec[3] > 1
    _accuracy("cov300", g, pairs, out, Hb, vs, ps, cols=[0, n // 3, n // 2, n - 1])


def test_determinism_and_isolation(pkg, orc, hip):
    g = PC.graph("cov300")
    pairs, _ = PC.request("cov300", g)
    pose0 = g["pose"].copy()
    p = pkg.new_problem()
    a, rec, Hb = _call(pkg, g, pairs, p=p)
    assert Hb.size == 0                                                     # no dump without the diag bit
    b, _, _ = _call(pkg, g, pairs, p=p)
    p.close()
    c, _, Hc = _call(pkg, g, pairs)                                          # a fresh handle, with the dump: the same bits
    assert Hc.size == 36 * len(PC.block_list(g)[0])
    for k in ("v_cov", "pair_cov", "v_status", "pair_status", "n_status"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(c[k]).view(np.uint8)), k
    assert np.array_equal(g["pose"], pose0)
    # whatever options.pgo_solver says, an invalid value included
    for solver in (0, 2):
        e, rec_s, _ = _call(pkg, g, pairs, diag=0, pgo_solver=solver)
        assert rec_s[0] == 1 and np.array_equal(_bits(e["v_cov"]), _bits(a["v_cov"])) and np.array_equal(_bits(e["pair_cov"]), _bits(a["pair_cov"]))
    # the problem's window and a following pose-graph optimisation (the pattern of test_pgo_sparse.test_determinism_isolation_and_refusal)
    w = pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AA)
    gs = pgo_ref.cov_graph(60, seed=9)
    ps60, _ = PC.request("cov60", gs)
    res = []
    for with_cov in (False, True):
        for solver in (0, 1):
            p = pkg.new_problem(pgo_solver=solver)
            p.upload_window(w)
            p.optimize(3)
            if with_cov:
                m = p.pgo_marginals(gs["pose"], gs["ei"], gs["ej"], gs["meas"], info=gs["info"], fixed=gs["fixed"], pairs=ps60)
                assert p.debug_get("pgo_cov")[0] == 1 and np.all(np.isfinite(m["v_cov"][2:]))
            X, st, tr = p.pgo(gs["pose"], gs["ei"], gs["ej"], gs["meas"], info=gs["info"], fixed=gs["fixed"], iters=20, user_lambda=LAM)
            so = p.optimize(5)
            res.append((pkg.protocol.results(p), X, st["chi2_final"], tr, so.chi2_final))
            p.close()
    for x, y in ((res[0], res[2]), (res[1], res[3])):
        for k in x[0]:
            assert np.array_equal(np.asarray(x[0][k]), np.asarray(y[0][k])), k
        assert np.array_equal(_bits(x[1]), _bits(y[1])) and x[2] == y[2] and x[3] == y[3] and x[4] == y[4]


def test_the_optimiser_and_the_marginals_hold_the_same_plan(pkg, orc, hip):
    """one analysis and one device image of it behind both entry points: free vertices, fronts, levels, blocks of L and the largest front
    of the two records agree exactly (the bytes differ: each call counts its own buffers besides)"""
    g = pgo_ref.cov_graph(40, seed=3)
    p = pkg.new_problem(pgo_solver=1)
    try:
        p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], iters=1, user_lambda=LAM)
        opt = p.debug_get("pgo_sparse").copy()
        p.pgo_marginals(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"])
        cov = p.debug_get("pgo_cov").copy()
    finally:
        p.close()
    print("pgo_sparse", opt, "pgo_cov", cov)
    assert opt[0] == 1 and cov[0] == 1 and opt[1] == 38
    assert np.array_equal(opt[1:6], cov[1:6]), (opt, cov)
    assert opt[6] > 0 and cov[6] > 0


def test_the_call_blocks_once(pkg, orc, hip):
    """the header's count of blocking waits, by plba_debug_get("host_waits"): one read-back; one more for the dump; one more to name the
    front of a failed factorisation"""
    g = pgo_ref.cov_graph(60, seed=8)
    pairs = np.stack([g["ei"], g["ej"]], 1)
    bad = dict(g); bad["info"] = g["info"].copy(); bad["info"][20] = -1e7 * np.eye(6)
    for diag, graph, want in ((0, g, 1), (DUMP, g, 2), (0, PC.graph("fixed_hub"), 1), (0, bad, 2)):
        p = pkg.new_problem(diag=diag)
        for _ in range(2):      # (a first call and a call on a warm handle alike)
            h0 = p.debug_get("host_waits")[0]
            try:
                p.pgo_marginals(graph["pose"], graph["ei"], graph["ej"], graph["meas"], info=graph["info"], fixed=graph["fixed"], pairs=pairs if graph is not PC.graph("fixed_hub") else None)
                assert graph is not bad
            except pkg.abi.PlbaError:
                assert graph is bad
            assert p.debug_get("host_waits")[0] - h0 == want, (diag, want)
        p.close()


def _raw(pkg, p, g, want, pairs, v_cov=True, pair_cov=True, n_pairs=None, sentinel=-7.25):
    """the C entry itself on sentinel-filled buffers: (rc, buffers untouched?, record)"""
    abi = pkg.abi
    X = np.ascontiguousarray(g["pose"], np.float64).copy()
    fx = np.ascontiguousarray(g["fixed"], np.uint8); ei = np.ascontiguousarray(g["ei"], np.int32); ej = np.ascontiguousarray(g["ej"], np.int32)
    Z = np.ascontiguousarray(g["meas"], np.float64); om = np.ascontiguousarray(g["info"], np.float64)
    gr = abi.PoseGraph(len(X), abi._dp(X), abi._up(fx), len(ei), abi._ip(ei), abi._ip(ej), abi._dp(Z), abi._dp(om))
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    vc = np.full((len(X), 6, 6), sentinel); vs = np.full(len(X), 99, np.uint8)
    pc = np.full((max(len(pr), 1), 6, 6), sentinel); ps = np.full(max(len(pr), 1), 99, np.uint8)
    m = abi.PgoMarginals()
    m.want = want; m.n_pairs = len(pr) if n_pairs is None else n_pairs; m.pairs = abi._ip(pr) if len(pr) else None
    m.v_cov = abi._dp(vc) if v_cov else None; m.v_status = abi._up(vs)
    m.pair_cov = abi._dp(pc) if pair_cov else None; m.pair_status = abi._up(ps)
    for i in range(4):
        m.n_status[i] = -5
    rc = p.lib.fn["pose_graph_marginals"](p._h, C.byref(gr), C.byref(m))
    untouched = bool(np.all(vc == sentinel) and np.all(pc == sentinel) and np.all(vs == 99) and np.all(ps == 99) and list(m.n_status) == [-5] * 4)
    return rc, untouched and np.array_equal(_bits(X), _bits(g["pose"])), p.debug_get("pgo_cov").copy()      # (bits: a NaN pose compares equal to itself)


def test_failure_and_refusal(pkg, orc, hip):
    good = pgo_ref.cov_graph(60, seed=8)
    pairs = np.stack([good["ei"], good["ej"]], 1)
    p = pkg.new_problem()
    rc, untouched, rec = _raw(pkg, p, good, 3, pairs)
    assert rc == 0 and not untouched and rec[0] == 1 and rec[1] == 58
    # the failing factorisation of test_pgo_sparse.test_a_failing_factorisation_matches_the_dense_path
    bad = dict(good); bad["info"] = good["info"].copy(); bad["info"][20] = -1e7 * np.eye(6)
    rc, untouched, rec = _raw(pkg, p, bad, 3, pairs)
    assert rc == -4 and untouched and np.all(rec == 0), (rc, untouched, rec)          # PLBA_ERR_NUMERIC
    msg = p.lib.fn["last_error"](p._h).decode()
    print(msg)
    assert "front" in msg and "pivot" in msg, msg
    # the named front is the right one: edge 20 joins vertices 20 and 21, whose diagonal blocks alone carry the -1e7 I, so the first
    # failing pivot is one of the two, and the front that eliminates it lists it among its pivot vertices
    import re
    lo, hi = [int(x) for x in re.search(r"pivot vertices (\d+) \.\. (\d+)", msg).groups()]
    assert bad["ei"][20] == 20 and bad["ej"][20] == 21 and lo <= 21 and hi >= 20, (lo, hi)      # (a leaf's pivots ascend but need not be consecutive)
    rc, untouched, rec = _raw(pkg, p, good, 3, pairs)                                   # the handle goes on working
    assert rc == 0 and rec[0] == 1
    nv = good["nv"]
    refusals = [dict(want=0, pairs=pairs), dict(want=4, pairs=pairs), dict(want=3, pairs=pairs, n_pairs=-1), dict(want=3, pairs=[(0, nv)]),
                dict(want=3, pairs=[(-1, 2)]), dict(want=1, pairs=pairs, v_cov=False), dict(want=2, pairs=pairs, pair_cov=False),
                dict(want=3, pairs=pairs, pair_cov=False)]
    for kw in refusals:
        rc, untouched, rec = _raw(pkg, p, good, **kw)
        assert rc == -1 and untouched and np.all(rec == 0), kw
        rc, _, rec = _raw(pkg, p, good, 3, pairs)
        assert rc == 0 and rec[0] == 1
    for key, val in (("ei", np.where(np.arange(len(good["ei"])) == 5, nv, good["ei"]).astype(np.int32)), ("ej", good["ei"].copy()),
                     ("pose", np.where(np.arange(12 * nv).reshape(nv, 12) == 40, np.nan, good["pose"]))):
        g2 = dict(good); g2[key] = val
        rc, untouched, rec = _raw(pkg, p, g2, 3, pairs)                       # what plba_optimize_pose_graph refuses about the graph
        assert rc == -1 and untouched and np.all(rec == 0), key
    p.close()


def test_large_graph(pkg, orc, hip):
    nv = 20000
    g = pgo_ref.cov_graph(nv, seed=7, n_loops=3)
    pairs = np.stack([g["ei"], g["ej"]], 1)
    p = pkg.new_problem()
    a, rec, _ = _call(pkg, g, pairs, p=p)
    b, _, _ = _call(pkg, g, pairs, p=p)
    p.close()
    P = 6 * (nv - 2)
    assert rec[0] == 1 and rec[1] == nv - 2 and rec[2] > 1 and rec[3] > 1 and rec[4] >= nv - 2
    assert rec[6] < 0.02 * 8.0 * P * P
    assert np.array_equal(_bits(a["v_cov"]), _bits(b["v_cov"])) and np.array_equal(_bits(a["pair_cov"]), _bits(b["pair_cov"]))
    assert np.all(a["pair_status"] == np.where((pairs < 2).any(1), 1, 0)) and a["n_status"].tolist() == [nv - 2, 2, 0, 0]
    assert np.all(np.isfinite(a["v_cov"][2:])) and np.all(a["v_cov"][:2] == 0)
    # accuracy on 2 sampled vertices against sparse-LU columns refined with a long double residual, at the largest size whose bound
    # 32 n u kappa_s says something (kappa_s of the 20 000-keyframe chain behind two fixed vertices is ~1e11: the bound exceeds 1)
    for size in (20000, 5000, 2000, 1000):
        gg = g if size == nv else pgo_ref.cov_graph(size, seed=7, n_loops=3)
        ks = PC.kappa_s_sparse(PC.sparse_H(gg))
        bound = PC.bound(6 * (size - 2), ks)
        print("large: %d keyframes kappa_s %.3e bound %.3e%s" % (size, ks, bound, "" if bound <= 1e-3 else " > 1e-3: the graph is shrunk"))
        if bound <= 1e-3:
            break
    assert bound <= 1e-3
    pp = np.stack([gg["ei"], gg["ej"]], 1)
    out, rec2, Hb = (a, rec, None) if size == nv else _call(pkg, gg, pp)[:3]
    if Hb is None:
        out, rec2, Hb = _call(pkg, gg, pp)
    Hs = PC.sparse_H(gg, Hb)
    n = size - 2
    cols = [n // 3, n - 1]
    ext, om = PC.refined_sparse_columns(Hs, cols)
    assert om <= 1e-17, om
    vs, ps, _ = PC.statuses(gg, pp)
    ent = _entries(gg, pp, out, vs, ps, cols)
    E = PC.e_sel(ent, ext, np.sqrt(Hs.diagonal()))
    print("large: %d keyframes, %d entries in the columns of ranks %s: E_sel %.3e bound %.3e" % (size, len(ent), cols, E, bound))
    assert E <= bound
