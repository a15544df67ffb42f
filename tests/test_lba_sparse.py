"""plba_lba_visual with the sparse reduced-camera solve (plba_lba_options.solver = 1; csrc/plba_lba.hip: k_lba_sblk, csrc/plba_lba_sparse.h,
the multifrontal solve of csrc/plba_pgo_sparse.hip) against the extended-precision reference tests/lba_ref.py and against the dense device
path, on covisibility graphs that give each shape of elimination tree, on every entry count at which k_lba_sblk's wave loop changes, and on
one window of 1 000 local keyframes against tests/lba_sparse_ref.py.

Bars (DESIGN.md 9 / tests/test_lba_visual.py): poses 1e-9, landmarks 1e-8 absolute, lambda and err_first 1e-12 relative against the
reference's wide run; pass and update counts, solver_failed and the moved flags exactly, on windows whose decisions keep lba_ref.MARGIN x
the noise (tests/test_lba_sparse_cpu.py asserts that for every window here); the pose step of pass one under lba_ref.hold_pose_step.  The
8 x noise rule of lba_ref.hold belongs to the dense solve's summation order and is NOT asserted: error / noise is printed per quantity.
Every sparse call goes through _sparse(), which fails on a library without the option."""
import ctypes as C

import numpy as np
import pytest

from . import lba_cases as LC
from . import lba_ref as LR
from . import lba_sparse_cases as SC

STATS = ("iterations", "updates", "err_first", "err_last", "lam", "solver_failed")


def _args(w):
    return (w["T_kf_w"], w["kf_loc"], w["xyz"], w["pq"], w["po_pt"], w["po_kf"], w["uv"], w["lo_ln"], w["lo_kf"], w["l3"], w["cam"])


def _sparse(pkg, prob, w, **opts):
    assert "solver" in [f[0] for f in pkg.abi.LbaOptions._fields_], "this library has no plba_lba_options.solver"
    res = prob.lba_visual(*_args(w), solver=1, **opts)
    rec = prob.debug_get("lba_sparse")
    assert len(rec) == 8 and rec[0] == 1, rec
    return res


def _hold(res, r64, rw, who, name, opts=None):
    """the decisions exactly, every output within the fixed bars against the wide run; error / noise printed, not asserted"""
    assert r64["omega"] <= LR.SR.RESIDUAL_MAX and rw["omega"] <= LR.SR.RESIDUAL_MAX, (r64["omega"], rw["omega"])
    assert LR.decisions_have_margin(r64, rw, opts) >= LR.MARGIN, name
    for k in ("iterations", "updates", "solver_failed"):
        assert res[k] == rw[k] == r64[k], (name, k, res[k], rw[k], r64[k])
    assert np.array_equal(res["pt_moved"], rw["pt_moved"]) and np.array_equal(res["ln_moved"], rw["ln_moved"]), name
    _, noise = LR.tolerances(r64, rw)
    lim = dict(T=LR.LIMITS["T"], xyz=LR.LIMITS["xyz"], pq=LR.LIMITS["pq"], lam=LR.LIMITS["lam_rel"] * abs(rw["lam"]),
               err_first=LR.LIMITS["err_first_rel"] * abs(rw["err_first"]))
    bad = []
    for k in noise:
        e = float(np.abs(np.asarray(res[k], np.float64) - np.asarray(rw[k], np.float64)).max())
        print("%s %s %-9s error %.3e  noise %.3e  bar %.3e  error/noise %.2f" % (who, name, k, e, noise[k], lim[k], e / noise[k] if noise[k] > 0 else np.inf if e > 0 else 0.0))
        if not e <= lim[k]:
            bad.append((k, e, lim[k]))
    assert not bad, (who, name, bad)


def _close(a, b, name):
    """two device paths: the same decisions, the outputs within the same bars"""
    for k in ("iterations", "updates", "solver_failed"):
        assert a[k] == b[k], (name, k, a[k], b[k])
    assert np.array_equal(a["pt_moved"], b["pt_moved"]) and np.array_equal(a["ln_moved"], b["ln_moved"]), name
    assert np.abs(a["T"] - b["T"]).max() <= LR.LIMITS["T"] and np.abs(a["xyz"] - b["xyz"]).max(initial=0.0) <= LR.LIMITS["xyz"], name
    assert np.abs(a["pq"] - b["pq"]).max(initial=0.0) <= LR.LIMITS["pq"], name
    assert abs(a["lam"] - b["lam"]) <= LR.LIMITS["lam_rel"] * abs(b["lam"]) and abs(a["err_first"] - b["err_first"]) <= LR.LIMITS["err_first_rel"] * abs(b["err_first"]), name


def _hold_window(pkg, w, r64, rw, name, opts, plan=None):
    g = pkg.new_problem()
    try:
        for k in (1, None):
            o = dict(opts) if k is None else dict(opts, max_iters=k)
            res = _sparse(pkg, g, w, **o)
            rec = g.debug_get("lba_sparse")
            if plan is not None:
                assert tuple(int(v) for v in rec[1:4]) == plan, (name, rec)
            _hold(res, LR.at(r64, k), LR.at(rw, k), "sparse", "%s %s passes" % (name, k or "all"), o)
            dense = g.lba_visual(*_args(w), **o)
            assert not g.debug_get("lba_sparse").any()
            _close(res, dense, name)
            if k == 1:
                LR.hold_pose_step(res["T"], w, rw, "sparse", name)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("run", SC.RUNS, ids=SC.run_id)
def test_tree_shapes(pkg, hip, run):
    """one front; the first separator; three levels; a revisit joining two distant stretches; one front holding everything; two
    components; a vertex without neighbour — points only, with a fifth lines, the line pass at the map poses and at the iterate, and the
    40-keyframe band as the GBA variant"""
    w, r64, rw = SC.run_reference(run)
    _, nkf, fronts, levels = SC.SHAPES[run[0]]
    _hold_window(pkg, w, r64, rw, SC.run_id(run), run[2], plan=(nkf, fronts, levels))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SC.ENTRIES_N)
def test_entries_per_block(pkg, hip, n):
    """an off-diagonal block with exactly n pair entries (its keyframes' diagonal blocks: 30 + n): one lane, the last lane idle, every
    lane once, a second round of one lane, four full rounds, a fifth of one lane"""
    w, r64, rw = SC.entries_reference(n)
    _hold_window(pkg, w, r64, rw, "entries %d" % n, {})


@pytest.mark.gpu
def test_reproducible_bit_for_bit(pkg, hip):
    w = SC.SHAPES["revisit40"][0](True)
    g = pkg.new_problem()
    a, b = _sparse(pkg, g, w), _sparse(pkg, g, w)
    g.close()
    h = pkg.new_problem()
    c = _sparse(pkg, h, w)
    h.close()
    for x in (b, c):
        for k in ("T", "xyz", "pq", "pt_moved", "ln_moved"):
            assert np.array_equal(a[k], x[k]), k
        assert [a[k] for k in STATS] == [x[k] for k in STATS]


@pytest.mark.gpu
def test_all_keyframes_fixed_is_refused_as_by_the_dense_path(pkg, hip):
    """no local keyframe: nothing to solve; either solver refuses the call alike and leaves an all-zero record"""
    w = SC.all_fixed()
    g = pkg.new_problem()
    try:
        msgs = []
        for o in (dict(), dict(solver=1)):
            with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_INVALID.*no local keyframe") as e:
                g.lba_visual(*_args(w), **o)
            msgs.append(str(e.value))
            assert not g.debug_get("lba_sparse").any()
        assert msgs[0] == msgs[1]
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", [("point", LC.fail_unobserved_point), ("keyframe", LC.fail_unobserved_keyframe)])
def test_reports_the_numerical_failure_as_the_dense_path(pkg, hip, name, make):
    """a point without observation (a zero landmark block) / a local keyframe without observation (a zero diagonal block of S): solver_ok
    cleared, no update, the run stops"""
    w = make()
    g = pkg.new_problem()
    a, b = _sparse(pkg, g, w), g.lba_visual(*_args(w))
    g.close()
    for x in (a, b):
        assert (x["solver_failed"], x["updates"]) == (1, 0)
        assert np.array_equal(x["xyz"], w["xyz"]) and np.array_equal(x["pq"], w["pq"])
        assert np.abs(x["T"] - w["T_kf_w"]).max() <= 64 * LR.U * np.abs(w["T_kf_w"]).max()      # expmap(logmap(T)) of the local keyframes
    assert a["iterations"] == b["iterations"] and np.array_equal(a["T"], b["T"])


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [2, -1])
def test_unknown_solver_is_refused_with_outputs_untouched(pkg, hip, solver):
    w = SC.SHAPES["band12"][0](True)
    assert "solver" in [f[0] for f in pkg.abi.LbaOptions._fields_]
    g = pkg.new_problem()
    try:
        _sparse(pkg, g, w, max_iters=1)      # (a record to be cleared)
        o = pkg.abi.LbaOptions()
        g.lib.fn["lba_default_options"](C.byref(o))
        o.solver = solver
        f64 = lambda a: np.ascontiguousarray(a, np.float64)
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        T, xyz, pq = f64(w["T_kf_w"]).reshape(-1, 16).copy(), f64(w["xyz"]).copy(), f64(w["pq"]).copy()
        loc, po_pt, po_kf, lo_ln, lo_kf = i32(w["kf_loc"]), i32(w["po_pt"]), i32(w["po_kf"]), i32(w["lo_ln"]), i32(w["lo_kf"])
        uv, l3 = f64(w["uv"]), f64(w["l3"])
        Tout = np.full((len(T), 16), 7.0); pm = np.full(len(xyz), 9, np.uint8); lm = np.full(len(pq), 9, np.uint8)
        st = pkg.abi.LbaStats(); st.iterations = 77; st.lam = 5.0
        rc = g.lib.fn["lba_visual"](g._h, C.byref(o), len(T), dp(T), ip(loc), len(xyz), dp(xyz), len(pq), dp(pq), len(po_pt), ip(po_pt), ip(po_kf), dp(uv),
                                    len(lo_ln), ip(lo_ln), ip(lo_kf), dp(l3), *[float(c) for c in w["cam"]], dp(Tout), up(pm), up(lm), C.byref(st))
        assert rc == -1      # PLBA_ERR_INVALID
        assert (Tout == 7.0).all() and (pm == 9).all() and (lm == 9).all() and (st.iterations, st.lam) == (77, 5.0)
        assert np.array_equal(xyz, w["xyz"]) and np.array_equal(pq, w["pq"])
        assert not g.debug_get("lba_sparse").any()
    finally:
        g.close()


@pytest.mark.gpu
def test_a_thousand_keyframes(pkg, hip):
    """1 000 local keyframes, tracks over 2 .. 6 keyframes, 20 points + 4 lines first seen per keyframe, 3 revisits, about 1e5 observations:
    two passes against lba_sparse_ref; the pose system takes less than an eighth of the dense matrix's 36 * 8 * Nkf^2 bytes"""
    w, r64, rw = SC.scale_reference(pkg)
    g = pkg.new_problem()
    try:
        res = _sparse(pkg, g, w, **SC.SCALE_OPTS)
        rec = g.debug_get("lba_sparse")
    finally:
        g.close()
    print("lba_sparse record:", rec)
    assert rec[1] == SC.SCALE_N and rec[6] < 36 * 8 * SC.SCALE_N ** 2 / 8, rec
    _hold(res, r64, rw, "sparse", "1000 keyframes", SC.SCALE_OPTS)
