"""The fixed cost of a plba_optimize call (csrc/plba_kernels.hip: k_call_setup, diag_arrive, k_state_copy).

One set-up launch replaces the control-block kernel and three memsets in front of the first iteration and clears the IMU accumulator at
its STRUCTURAL positions only; lambda_init rides in the diagonal pass's last-arriving workgroup; save_state / restore_state are one
launch each.  None of it may change a bit of any result, so everything here is an equality: a handle whose accumulators a previous
call left dirty — in every way a call can end — against a fresh handle, across a structure change on a re-used handle, and the first
lambda against the CPU oracle and against the launch forms that keep lambda_init as a launch of its own (profile = 2, sharded).

The window is the smallest that has everything the set-up touches: 8 keyframes (first one fixed), 120 points, 24 lines, 7 IMU edges,
with and without a marginalization prior; lm_fused = 2 (fused landmark passes) and lm_fused = 0 (record-based passes)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = (8, 120, 24, 0xCA115E7)
COLS = ("iteration", "trial", "accepted", "solver_ok", "lam", "chi2_current", "chi2_trial", "scale", "rho")


def _make(pkg, orc, prior, seed=WIN[3], drop_imu=None, **kw):
    # tracks over 2 .. 4 keyframes: the prior left by marginalizing keyframe 0 then sits on keyframes 1 .. 3 and the rest of the window keeps
    # its chain segments — a prior on EVERY keyframe leaves none, and such a window takes the record-based passes whatever lm_fused says
    kw.setdefault("track", (2, 4))

    def base():
        w = pkg.window.make_window(WIN[0], WIN[1], WIN[2], imu=True, seed=seed, **kw)
        if drop_imu is not None:      # no IMU edge between two neighbours: another IMU topology (the chain falls apart there)
            im = dict(w["imu"]); keep = np.ones(WIN[0] - 1, bool); keep[drop_imu] = False
            for k in ("kf_i", "kf_j", "preint", "info_pvr", "info_bias"): im[k] = im[k][keep]
            w["imu"] = im
        return w
    w = base()
    if prior:      # the prior the ORACLE's marginalization of the same window's first BA leaves: deterministic, computed on the CPU
        o = orc.new_problem(); o.upload_window(w); pkg.protocol.local_ba(o, stage1=2, stage2=2); pr = o.marginalize(0, 50); o.close()
        w = base(); w["prior"] = pr
    return w


@pytest.fixture(scope="module")
def wins(pkg, orc):
    """the windows of this file, built once: plain | prior | another IMU topology with a prior on other keyframes | perturbed landmarks (10 keyframes)"""
    out = {False: _make(pkg, orc, False), True: _make(pkg, orc, True)}
    out["other"] = _make(pkg, orc, True, seed=WIN[3] + 1, drop_imu=3, track=(2, 3))
    assert set(out["other"]["prior"]["vid"].tolist()) != set(out[True]["prior"]["vid"].tolist()), "the second window's prior is meant to sit on other keyframes"
    # the window of tests/test_gpu_parity.py::test_rejected_trials_with_imu_edges (10 keyframes, points perturbed by a metre): with
    # lambda_init = 1e-6 its iteration 2 rejects six trials in a row, on every device path and in the quad-precision run
    # (tests/golden/fused_overshoot_quad.json, case rejected_small) — a rejection that does not hang on the last bits of a solve
    far = pkg.window.make_window(10, 150, 30, imu=True, seed=77)
    far["points"] = far["points"] + np.random.default_rng(1).normal(size=far["points"].shape) * 1.0
    out["far"] = far
    return out


def _snap(p):
    """everything a call leaves for its caller, as bytes: the LM trace (every column) and the states"""
    tr = np.array([[r[c] for c in COLS] for r in p.trace()], dtype=np.float64)
    kf = p.get_keyframes()
    return (tr.tobytes(), tuple(sorted((k, np.ascontiguousarray(v).tobytes()) for k, v in kf.items())), p.get_points().tobytes(), p.get_lines().tobytes())


def _run(p, n):
    p.optimize(n)
    return _snap(p)


def _fresh(pkg, w, n, fused, **opts):
    p = pkg.new_problem(lm_fused=fused, **opts); p.upload_window(w)
    s = _run(p, n)
    assert int(p.debug_get("lm_fused")[0]) == (1 if fused else 0)
    p.close()
    return s


@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("prior", [False, True])
def test_dirty_accumulators(pkg, orc, hip, wins, prior, fused):
    """optimize(3), restore_state(), optimize(3): the second call finds the accumulators as the first left them — the last accepted
    linearisation in one, a trial's in the other — and must reproduce the first call and a fresh handle bit for bit.  The same after
    optimize(1), which ends on the trial launch without Jacobians (nothing was swapped, the current accumulator still holds the call's
    first linearisation)."""
    w = wins[prior]
    ref = _fresh(pkg, w, 3, fused)
    g = pkg.new_problem(lm_fused=fused); g.upload_window(w)
    g.save_state()
    a = _run(g, 3)
    g.restore_state()
    b = _run(g, 3)
    assert a == ref and b == ref
    g.restore_state()
    g.optimize(1)
    g.restore_state()
    assert _run(g, 3) == ref
    g.close()


@pytest.mark.parametrize("fused", [2, 0])
def test_dirty_accumulators_after_a_rejected_last_trial(pkg, orc, hip, wins, fused):
    """points perturbed by a metre, lambda_init = 1e-6 (the window of tests/test_gpu_parity.py: test_rejected_trials_with_imu_edges) and two
    trials per iteration: two steps are accepted — the accumulators swap —, then both trials of iteration 2 are rejected and the call
    stops there, the last trial's Jacobians in the idle accumulator, never swapped in"""
    w = wins["far"]
    opts = dict(user_lambda_init=1e-6, max_trials=2)
    ref = _fresh(pkg, w, 6, fused, **opts)
    g = pkg.new_problem(lm_fused=fused, **opts); g.upload_window(w)
    a = _run(g, 6)
    tr = g.trace()
    assert [(r["iteration"], r["trial"], r["accepted"]) for r in tr] == [(0, 0, 1), (1, 0, 1), (2, 0, 0), (2, 1, 0)], "the scenario is meant to end on a rejected trial"
    g.restore_state()
    b = _run(g, 6)
    assert a == ref and b == ref
    g.close()


@pytest.mark.parametrize("fused", [2, 0])
def test_structure_change_on_a_reused_handle(pkg, orc, hip, wins, fused):
    """after a call, a window with another IMU topology and a prior on other keyframes (a structure-cache miss: both accumulators are
    re-created, zero everywhere), then the first window again (a miss once more: the cache holds one structure), then the first window
    uploaded a second time (a hit: the buffers stay and are cleared): each equal to a fresh handle's, bit for bit"""
    wa, wb = wins[True], wins["other"]
    ra, rb = _fresh(pkg, wa, 3, fused), _fresh(pkg, wb, 3, fused)
    g = pkg.new_problem(lm_fused=fused)
    for w, ref in ((wa, ra), (wb, rb), (wa, ra), (wa, ra), (wb, rb)):
        g.upload_window(w)
        assert _run(g, 3) == ref
    g.close()


@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("prior", [False, True])
def test_first_lambda_against_the_oracle(pkg, orc, hip, wins, prior, fused):
    """lambda_0 = tau * max |H_jj|: formed in the diagonal pass's last workgroup (fused) / by k_lambda_init (record-based)"""
    w = wins[prior]
    g = pkg.new_problem(lm_fused=fused); g.upload_window(w); g.optimize(1)
    o = orc.new_problem(); o.upload_window(w); o.optimize(1)
    lg, lo = g.trace()[0]["lam"], o.trace()[0]["lam"]
    print("first lambda: device %.17g oracle %.17g rel %.3e" % (lg, lo, abs(lg - lo) / abs(lo)))
    assert lg > 0 and abs(lg - lo) <= 1e-12 * abs(lo)
    g.close(); o.close()


@pytest.mark.parametrize("prior", [False, True])
def test_profile_2_keeps_its_own_launches_and_agrees(pkg, orc, hip, wins, prior):
    """profile = 2 (an event after every phase, no speculation, no riding decisions): lambda_init stays a launch of its own behind the
    diagonal pass — the same device function, so lambda_0 has the same bits — and the call takes the same steps"""
    w = wins[prior]
    g = pkg.new_problem(lm_fused=2); g.upload_window(w); g.optimize(3); tg = g.trace(); kg = g.get_keyframes(); g.close()
    h = pkg.new_problem(lm_fused=2, profile=2); h.upload_window(w); h.optimize(3); th = h.trace(); kh = h.get_keyframes(); h.close()
    assert th[0]["lam"] == tg[0]["lam"] and th[0]["chi2_current"] == tg[0]["chi2_current"]
    assert [tuple(r[c] for c in COLS) for r in th] == [tuple(r[c] for c in COLS) for r in tg]
    assert all(np.array_equal(kh[k], kg[k]) for k in kg)


def _shard_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    from oracle import oracle as orc
    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        w = _make(pkg, orc, True)
        torch.cuda.set_device(0)
        p = pkg.new_problem(lm_fused=2)
        p.upload_window(pkg.window.shard_window(w, rank, world))
        p.set_shard(rank, world, pkg.distributed.make_allreduce(dist, 0, None, via_host=True))
        p.optimize(3)
        out.put((rank, [tuple(r[c] for c in COLS) for r in p.trace()], int(p.debug_get("lm_fused")[0])))
        p.close()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:   # report instead of dead-locking the peer in a collective
        import traceback
        out.put(("error", rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
        out.close(); out.join_thread()
        os._exit(1)


def test_sharded_form_keeps_its_own_launches_and_agrees(pkg, orc, hip, wins):
    """two ranks on one GPU, all-reduce through gloo (the harness of tests/test_distributed.py): chi2, max |Hll_jj| and the pose diagonal
    are all-reduced before lambda_init, which stays a launch.  The ranks' partial sums are added in another order than on one GPU:
    lambda_0 is a maximum over sums of at most a few hundred non-negative terms (relative rounding difference <= n * 2^-53 ~ 1e-13), held
    to 1e-12 like the oracle's; the later rows to the sharded tests' own 1e-8."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in range(2):
            g = q.get(timeout=240)
            if g[0] == "error":
                raise AssertionError("rank %d failed:\n%s" % (g[1], g[2]))
            got.append(g)
    finally:
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
    got.sort(key=lambda g: g[0])
    assert got[0][1] == got[1][1] and got[0][2] == 1      # every rank: the same rows, on the fused passes
    one = pkg.new_problem(lm_fused=2); one.upload_window(wins[True]); one.optimize(3)
    t1 = [tuple(r[c] for c in COLS) for r in one.trace()]; one.close()
    ts = got[0][1]
    il = COLS.index("lam")
    assert abs(ts[0][il] - t1[0][il]) <= 1e-12 * abs(t1[0][il])
    assert [r[:4] for r in ts] == [r[:4] for r in t1]
    for a, b in zip(ts, t1):
        for c in ("lam", "chi2_current", "chi2_trial"):
            i = COLS.index(c)
            assert a[i] == pytest.approx(b[i], rel=1e-8), c
