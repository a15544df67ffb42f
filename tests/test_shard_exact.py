"""The landmark-sharded path of plba_optimize (world > 1: launch_reduce / launch_reduce_n and launch_posediag ahead of
launch_lambda_init2, the structural exchange list of launch_list_pack, the chain elimination as a launch of its own behind the
exchange, k_lm_gather without the W^T W tiles, the trial launch without a riding decision, [chi2, scale] all-reduced, lambda and the
unit padding from one rank, pose-side edges on rank 0) at worlds of two, three and eight, against the quad-precision build of the
oracle under the rule of tests/build_exact.py, unchanged: the fixtures tests/golden/build_exact_<case>.npz, their noise, FACTOR = 8
(32 for the solution and the trial).  tests/shard_exact.py runs the W ranks as W threads of this process and merges their results
into the unsharded window's layout; tests/test_shard_exact_cpu.py holds that harness, and the fp64 oracle's own sharded mode, to the
same rule without a GPU.  Both the fused passes (lm_fused = 2) and the record-based ones (lm_fused = 0) run, and which one ran is
asserted.

Asserted bit-identical on every rank: chi2, maxdiag, Hschur, bschur, bp, the pose part of x and the first trace row (shard_exact.GLOBAL).

Measured on the MI355X (DESIGN.md 7a has the table per quantity): worst error / tolerance
  world 2   lm_fused = 2: 0.23 (bl_pt of prior13)        lm_fused = 0: 0.23 (bl_pt of prior13)
  world 3   lm_fused = 2: 0.23 (bl_pt of prior13)        lm_fused = 0: 0.30 (Hschur of points_only)
  world 3, explicit cuts   0.15 on both (hll_pt of k6; the two cuts with an empty rank run the record-based passes whatever is asked for)
  world 8   lm_fused = 2: 0.23 (bl_pt of prior13)        lm_fused = 0: 0.23 (bl_pt of prior13)
the figures of the single-GPU build (tests/test_build_exact.py).  Nothing was beyond its tolerance.  The first run of these tests found
several sharded ranks of one process dead-locked in prepare(): the asynchronous group-table fill kept the host worker pool's lock
across the co-observation all-reduce; prepare() now joins the fill first (finding 1)."""
import ctypes as C

import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC
from . import shard_exact as SX
from . import test_distributed as TD

pytestmark = pytest.mark.gpu

RUNS = [r for r in SX.RUNS if r not in SX.DROPPED]


def _probe(p):
    return dict(lm_fused=p.debug_get("lm_fused").copy(), solver_ok=int(p.debug_get("solver_ok")[0]))


@pytest.mark.parametrize("run", RUNS, ids=[SX.run_id(r) for r in RUNS])
def test_sharded_build_solution_and_first_trial(pkg, hip, run):
    name, W, label, kind = run
    fx, w = SX.load_case(pkg.window, name)
    case = BC.CASES[name]
    i = SX.lambda_index(name, label)
    lam = float(fx["lams"][i])
    ref, tq, _, noise, decided = BX.load(fx, w, i)
    cut = SX.edge_cut(pkg.window, w, kind) if kind else None
    failed, ran = [], set()
    for fused in (2, 0):
        if fused == 0 and 0 in ran:      # (a cut with an empty rank: the pass that asked for the fused passes ran the record-based ones already)
            continue
        per_rank, shards = SX.run_sharded(lambda **kw: pkg.new_problem(lm_fused=fused, **case["opts"], **kw), w, W, lam, cut=cut,
                                          window_module=pkg.window, distributed=pkg.distributed, probe=_probe)
        # which passes ran: the fused ones where they were asked for and every rank holds an observation (the vote of prepare() is global)
        want = 1 if fused and all(len(s["po_pt"]) + len(s["lo_ln"]) for s in shards) else 0
        if kind:
            assert (want == 1) == (fused == 2 and SX.EVERY_RANK_HAS_OBSERVATIONS[kind])
        ran.add(want)
        # wide groups exactly where they are meant: on the ranks that hold a landmark with more than eight observations (LMF_W; a track
        # that starts late in the window is cut short by its end, so a late stretch of a wide case may hold none), and the case is a
        # wide one exactly if some rank does
        wide = [max(np.bincount(s["po_pt"]).max(initial=0), np.bincount(s["lo_ln"]).max(initial=0)) > 8 for s in shards]
        assert any(wide) == case["wide"]
        for r, res in enumerate(per_rank):
            for pr in (res["probe"], res["probe_trial"]):
                assert pr["lm_fused"][0] == want and pr["solver_ok"] == 1, (fused, r, pr)
                if want:
                    assert pr["lm_fused"][1] > 0 and (pr["lm_fused"][3] > 0) == wide[r], (r, pr, wide)
        try:
            merged = SX.merge(per_rank, w, shards)
            BX.hold(merged, ref, noise, "world %d lm_fused=%d" % (W, fused), SX.run_id(run), trial=(merged["trial"], tq, decided))
        except AssertionError as e:      # (the other path's figures are printed before the test fails)
            failed.append(e)
    assert not failed, failed
    assert 0 in ran and (1 in ran) == (kind is None or SX.EVERY_RANK_HAS_OBSERVATIONS[kind])      # both passes, but for an empty rank


@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("win", [TD.WIN_SMALL, TD.WIN_PRIOR], ids=["small", "prior"])
@pytest.mark.parametrize("W", [3, 8])
def test_sharded_local_ba_equals_the_unsharded_device(pkg, orc, hip, W, win, fused):
    """protocol.local_ba (optimize, gate, optimize) on W in-process ranks against the same call on one unsharded device problem: the LM
    decisions and the summed gate counts exactly, the pose blocks bit-identical across the ranks, the states under the bars
    test_distributed._check uses"""
    w = TD._window(pkg, orc, win)
    one = pkg.new_problem(lm_fused=fused); one.upload_window(w)
    rr = pkg.protocol.local_ba(one, stage1=win[4], stage2=win[5])
    res = pkg.protocol.results(one)
    acc = [t["accepted"] for t in one.trace()]
    path = int(one.debug_get("lm_fused")[0])
    one.close()
    assert path == (1 if fused else 0)
    got = SX.local_ba_ranks(lambda **kw: pkg.new_problem(lm_fused=fused, **kw), pkg.protocol, w, W, win[4], win[5], pkg.window, pkg.distributed,
                            probe=lambda p: int(p.debug_get("lm_fused")[0]))
    for g in got:
        assert g["probe"] == path, "the sharded run took other landmark passes than the unsharded one"
        assert g["accepted"] == acc and g["counts"] == tuple((rr[k].iterations, rr[k].trials) for k in ("stage1", "stage2"))
        for k in ("P", "V", "q", "dbg", "dba"):
            assert g["results"][k].tobytes() == got[0]["results"][k].tobytes(), (k, g["shard"]["rank"])
        for k in ("P", "V", "q", "dbg"):
            assert np.abs(g["results"][k] - res[k]).max() < 1e-8, k
        pi, li = g["shard"]["pt_index"], g["shard"]["ln_index"]
        if len(pi):
            assert np.abs(g["results"]["points"] - res["points"][pi]).max() < 1e-7
        if len(li):
            assert np.abs(g["results"]["lines"] - res["lines"][li]).max() < 1e-7
        assert g["chi2_final"] == pytest.approx(rr["stage2"].chi2_final, rel=1e-8)
        assert g["chi2_final"] == got[0]["chi2_final"]
    assert tuple(sum(g["gated"][i] for g in got) for i in range(2)) == rr["gated"]


# ---- plba_set_shard and the entry points that refuse a sharded problem -------------------------------------------------------------------
def _run_bits(p, iters=3):
    st = p.optimize(iters)
    kf = p.get_keyframes()
    return (st.chi2_final, st.trials, [(t["accepted"], t["chi2_trial"], t["lam"]) for t in p.trace()]) + tuple(kf[k].tobytes() for k in sorted(kf)) + (
        p.get_points().tobytes(), p.get_lines().tobytes())


def test_set_shard_refusals_leave_the_problem_unsharded(pkg, hip):
    w = pkg.window.make_window(6, 80, 20, imu=True, seed=5)
    fresh = pkg.new_problem(); fresh.upload_window(w); want = _run_bits(fresh); fresh.close()
    p = pkg.new_problem(); p.upload_window(w)
    fn = lambda buf, n, op, stream: None      # noqa: E731
    for rank, world in ((2, 2), (3, 2), (0, 0), (0, -1), (-1, 2)):      # rank >= world, world < 1, rank < 0
        with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_INVALID"):
            p.set_shard(rank, world, fn)
    with pytest.raises(pkg.abi.PlbaError, match="needs an all-reduce callback"):      # world > 1 without a callback
        p.call("set_shard", 0, 2, C.cast(None, pkg.abi.ALLREDUCE_FN), None)
    assert _run_bits(p) == want      # (still world 1: no collective is attempted, and the bits are a fresh problem's)
    p.close()


def test_entry_points_that_refuse_a_sharded_problem_leave_the_window_untouched(pkg, hip):
    """plba_refine_landmarks, plba_slide_window, plba_marginalize_to_prior and plba_compute_marginals on the ranks of a two-rank problem:
    each is refused on every rank, before and after an optimize, and the optimize calls around them give the bits of a run without them"""
    Wm = pkg.window
    seq = Wm.make_sequence(8, 2, 160, 40, seed=0x51DE)
    w = Wm.window_at(seq, 0, 8)
    delta = Wm.slide_delta(w, Wm.window_at(seq, 1, 8, prev=w))
    E = pkg.abi.PlbaError

    def refused(p):
        with pytest.raises(E, match="PLBA_ERR_INVALID.*sharded"): p.refine_landmarks()
        with pytest.raises(E, match="PLBA_ERR_STATE.*sharded"): p.slide_window(delta)
        with pytest.raises(E, match="PLBA_ERR_STATE.*sharded"): p.marginalize_to_prior(0, 50)
        with pytest.raises(E, match="PLBA_ERR_STATE.*sharded"): p.marginals()

    def run(with_refusals):
        shards = SX.shards_of(Wm, w, 2)

        def body(r, attach):
            p = pkg.new_problem(); p.upload_window(shards[r]); attach(p)
            if with_refusals: refused(p)
            a = _run_bits(p, 2)
            if with_refusals: refused(p)
            b = _run_bits(p, 2)
            p.close()
            return a, b
        res, err = SX.run_ranks(2, body, pkg.distributed)
        assert not any(err), err
        return res
    assert run(True) == run(False)


@pytest.mark.parametrize("fail_at", [0, 1, 2, 6])
def test_a_callback_that_raises_on_every_rank(pkg, hip, fail_at, capfd):
    """the exchange hook of EVERY rank raises at the same collective (0, 1: the two of prepare(); 2: the first of the call; 6: inside the
    LM loop): every rank gets PLBA_ERR_EXCHANGE with the library's message — an error return, no rank is left waiting — and a fresh
    upload on the same handles with a working hook gives the bits of fresh handles"""
    w = pkg.window.make_window(6, 80, 20, imu=True, seed=5)
    W = 3
    shards = SX.shards_of(pkg.window, w, W)

    def body(r, attach):
        fresh = pkg.new_problem(); fresh.upload_window(shards[r]); attach(fresh)
        want = _run_bits(fresh, 2)
        fresh.close()
        p = pkg.new_problem(); p.upload_window(shards[r]); attach(p, failing=True)
        with pytest.raises(pkg.abi.PlbaError, match=r"PLBA_ERR_EXCHANGE.*all-reduce callback failed \(1\)"):
            p.optimize(2)
        p.upload_window(shards[r]); attach(p)
        got = _run_bits(p, 2)
        p.close()
        return want, got
    res, err = SX.run_ranks(W, body, pkg.distributed, fail_at=fail_at)
    assert not any(err), "\n".join(e for e in err if e)
    for want, got in res:
        assert got == want
    assert capfd.readouterr().err.count("fails at collective %d, as asked" % fail_at) == W      # (the trampoline prints each rank's exception)
