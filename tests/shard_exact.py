"""The landmark-sharded path of plba_optimize (plba_set_shard, world > 1) run as W ranks in ONE process, and its results put back into
the unsharded window's layout, so that tests/build_exact.py's rule — the quad-precision fixtures, the diagonal-scaled norms, the
tolerance max(FACTOR x noise, m u) — holds a sharded build exactly as it holds the single-GPU one.  A sharded build is another
summation order of the same sums, which is what FACTOR is the project's figure for: no new tolerance.

Ranks.  W host threads, one problem each (include/plba.h: thread-compatible, one thread per problem).  The all-reduce hook of rank r
(Exchange.callback) views the buffer — device memory through distributed.as_tensor after a device synchronisation, as
make_allreduce(via_host=True) does, or host memory through distributed.host_array for an oracle problem — copies it into slot r,
waits on a threading.Barrier, reduces the W slots IN RANK ORDER (sum or max), so that every rank computes the same bits, waits again
so that no slot is overwritten early, and copies the result back.  The ranks must agree on the length and the operation of every
collective; a disagreement raises on all of them.  A broken or timed-out barrier raises inside the hook, which Problem.set_shard's
trampoline turns into PLBA_ERR_EXCHANGE; a worker that raises aborts the barrier: a failure ends the run, it does not hang it.
No torch.distributed, no sockets, no child processes.

Why threads cannot dead-lock the device (read in csrc/plba_mailbox.h, plba_problem.h and the sharded branches of plba_api.hip before
the first run).  The problems of one process share the library's one non-blocking stream per device, so the ranks' launches
interleave on it in whatever order the threads issue them.  No launch of the sharded path waits for the host: the only in-launch
wait, k_lm_trial's pose-side blocks (lead_wait), is for chain segments of the SAME launch and is bounded (Ctrl::sync_fail).  The
host waits — mail_wait polling the mapped mailbox k_decide writes, plba_stream_wait, and the hook's device synchronisation — wait for
work already in the stream, each rank for its own mailbox (a Mailbox per problem, HostCtx::h_mail).  prepare() itself holds two
collectives per upload (the fused-path vote, the co-observation map) and debug_build / optimize the ones listed below; a rank
reaches each only through calls every rank makes, which is why the ranks step through the same call sequence here.

What the exchange makes global (read in enqueue_linearize, enqueue_solve, lm_enqueue_first, lm_enqueue_system and the accept loop):
chi2 (sum) and max |H_jj| (max) and the pose diagonal (sum) ahead of launch_lambda_init2, hence `chi2` and `maxdiag`; the structural
entries of the reduced system and its two right-hand-side rows (launch_list_pack, npk doubles), hence `Hschur`, `bschur` and `bp`;
the solve runs on that system on every rank, hence the pose part of `x`; [chi2, scale] of the trial, hence the whole trace row.
GLOBAL lists them; merge() asserts them BIT-IDENTICAL on every rank.  Per landmark (hll_*, bl_*, the landmark part of x) and per
observation (err_pt, err_ln) a rank returns its shard's; the IMU and prior residuals are rank 0's (owns_pose_edges), and every other
rank must return zeros of the same shape: its buffers are cleared at upload and no launch of its writes them before the solve.

No buffer that build_exact.read() takes is overwritten by the sharded solve: the chain elimination behind the exchange writes its
own W (ChainView), k_chain_schur writes dd.sys, the factorisation Lfac — d.sys, bpg, hll, bl stay as built.  The one exception is
the one read_device() already handles on one GPU: debug_build(lam, True) ends in a trial launch that re-evaluates the IMU / prior
edges (on every rank: it passes with_pose_edges = true), so err_pvr, err_bias and err_prior are read after debug_build(lam, False)."""
import os
import threading
import traceback

import numpy as np

from . import build_exact as BX
from . import build_exact_cases as BC

GLOBAL = ("chi2", "maxdiag", "Hschur", "bschur", "bp")      # + x[:P] and the first trace row
RANK0 = BX.AT_THE_STATE
TIMEOUT = 30.0


class Exchange:
    """the in-process all-reduce of W ranks; `fail_at` = k: the k-th collective (from 0) raises on every rank instead of reducing"""
    def __init__(self, W, distributed, fail_at=None, timeout=TIMEOUT):
        self.W, self.D, self.fail_at = W, distributed, fail_at
        self.barrier = threading.Barrier(W, timeout=timeout)
        self.slots, self.meta = [None] * W, [None] * W
        self.calls = [0] * W

    def callback(self, r, on_device):
        D = self.D
        if on_device:
            import torch

        def fn(ptr, n, op, _stream):
            k = self.calls[r]; self.calls[r] += 1
            if self.fail_at is not None and k == self.fail_at:
                raise RuntimeError("the exchange of rank %d fails at collective %d, as asked" % (r, k))
            if on_device:
                t = D.as_tensor(ptr, n, torch.cuda.current_device())
                torch.cuda.synchronize()
                self.slots[r] = t.cpu().numpy().copy()
            else:
                a = D.host_array(ptr, n)
                self.slots[r] = a.copy()
            self.meta[r] = (int(n), int(op), k)
            self.barrier.wait()
            if any(m != self.meta[0] for m in self.meta):
                raise RuntimeError("the ranks disagree on a collective (length, op, number): %r" % (self.meta,))
            out = self.slots[0].copy()
            for s in self.slots[1:]:
                out = out + s if op == 0 else np.maximum(out, s)
            self.barrier.wait()
            if on_device:
                t.copy_(torch.from_numpy(out))
                torch.cuda.synchronize()
            else:
                a[:] = out
        return fn


def on_device(p):
    return p.lib.backend_name().startswith("hip")


def run_ranks(W, body, distributed, fail_at=None):
    """body(r, attach) on W threads; attach(problem) = set_shard with the in-process exchange, attach(problem, failing=True) with one
    whose collective number `fail_at` raises on every rank.  Returns ([result per rank], [error per rank]) — errors as text, None
    where the rank finished.  Never hangs: a rank that raises aborts the barriers for the others."""
    ex, exf = Exchange(W, distributed), Exchange(W, distributed, fail_at)
    res, err = [None] * W, [None] * W

    def worker(r):
        try:
            res[r] = body(r, lambda p, failing=False: p.set_shard(r, W, (exf if failing else ex).callback(r, on_device(p))))
        except BaseException as e:      # noqa: BLE001
            err[r] = "".join(traceback.format_exception(type(e), e, e.__traceback__))
            ex.barrier.abort(); exf.barrier.abort()
    th = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for t in th: t.start()
    for t in th: t.join()
    return res, err


def shards_of(Wm, w, W, cut=None, by="time"):
    """the W shards of a window: window.shard_window's, or the explicit [(point indices, line indices)] of `cut`"""
    if cut is None:
        return [Wm.shard_window(w, r, W, by=by) for r in range(W)]
    assert len(cut) == W
    return [Wm.shard_cut(w, np.sort(np.asarray(pi, np.int64)), np.sort(np.asarray(li, np.int64)), r, W) for r, (pi, li) in enumerate(cut)]


def run_sharded(make_problem, w, W, lam, cut=None, window_module=None, distributed=None, probe=None):
    """The sequence of build_exact.read_device and the first trial of optimize(1), on every rank of a W-rank run of `w`:
    ([per rank: raw arrays of read() + "trial" (the first trace row) + what probe(problem) returns after the build], shards).
    make_problem(**options) gives a problem of the implementation under test (device or oracle)."""
    shards = shards_of(window_module, w, W, cut)

    def body(r, attach):
        p = make_problem(); p.upload_window(shards[r]); attach(p)
        p.debug_build(lam, False)
        at = {k: p.debug_get(k).copy() for k in RANK0}
        p.debug_build(lam, True)
        out = BX.read(p)
        out.update(at)
        if probe is not None:
            out["probe"] = probe(p)
        p.close()
        t = make_problem(user_lambda_init=lam); t.upload_window(shards[r]); attach(t)
        t.optimize(1)
        out["trial"] = BX.first_trial(t)
        if probe is not None:
            out["probe_trial"] = probe(t)
        t.close()
        return out
    res, err = run_ranks(W, body, distributed)
    assert not any(err), "\n".join("rank %d:\n%s" % (r, e) for r, e in enumerate(err) if e)
    return res, shards


def obs_selection(w, shard):
    """the window's observation numbers (points, lines) that went to a shard, in the shard's order"""
    out = []
    for lm, ob, key in (("points", "po_pt", "pt_index"), ("lines", "lo_ln", "ln_index")):
        m = np.zeros(len(w[lm]), bool); m[shard["shard"][key]] = True
        out.append(np.flatnonzero(m[w[ob]]) if len(w[ob]) else np.zeros(0, np.int64))
    return out


def merge(per_rank, w, shards):
    """one result in the unsharded window's layout (the raw arrays of build_exact.read() and "trial").  Asserts: the quantities of GLOBAL,
    the pose part of x and the trace row bit-identical on every rank; the residuals of the IMU and prior edges zero on every rank but
    rank 0; every landmark and observation of the window filled by exactly one rank."""
    lay = BX.layout(w)
    r0 = per_rank[0]
    P = int(r0["P"])
    out = {"P": P}
    for r, res in enumerate(per_rank):
        assert int(res["P"]) == P, ("pose_dim", r, res["P"], P)
        for k in GLOBAL:
            assert np.asarray(res[k]).tobytes() == np.asarray(r0[k]).tobytes(), "%s differs between rank 0 and rank %d" % (k, r)
        assert np.asarray(res["x"][:P]).tobytes() == np.asarray(r0["x"][:P]).tobytes(), "the pose part of x differs between rank 0 and rank %d" % r
        if "trial" in r0:
            assert np.asarray(res["trial"]).tobytes() == np.asarray(r0["trial"]).tobytes(), "the first trace row differs between rank 0 and rank %d: %r %r" % (r, res["trial"], r0["trial"])
        for k in RANK0:
            assert np.asarray(res[k]).shape == np.asarray(r0[k]).shape, (k, r)
            if r:
                assert not np.asarray(res[k]).any(), "%s of rank %d, which owns no pose-side edge, is not zero" % (k, r)
    for k in GLOBAL + RANK0:
        out[k] = np.asarray(r0[k]).copy()
    if "trial" in r0:
        out["trial"] = np.asarray(r0["trial"]).copy()
    sel = [obs_selection(w, s) for s in shards]
    tables = (("err_pt", 2, len(w["po_pt"]), [s[0] for s in sel]), ("err_ln", 3, len(w["lo_ln"]), [s[1] for s in sel]),
              ("hll_pt", 9, lay["Np"], [s["shard"]["pt_index"] for s in shards]), ("bl_pt", 3, lay["Np"], [s["shard"]["pt_index"] for s in shards]),
              ("hll_ln", 36, lay["Nl"], [s["shard"]["ln_index"] for s in shards]), ("bl_ln", 6, lay["Nl"], [s["shard"]["ln_index"] for s in shards]))
    for k, n, N, idx in tables:
        full, cnt = np.full((N, n), np.nan), np.zeros(N, np.int64)
        for r, res in enumerate(per_rank):
            a = np.asarray(res[k])
            assert a.size == n * len(idx[r]), (k, r, a.size, n, len(idx[r]))
            full[idx[r]] = a.reshape(-1, n); cnt[idx[r]] += 1
        assert (cnt == 1).all(), "%s: %d entries of the window filled by no rank or by more than one" % (k, int((cnt != 1).sum()))
        out[k] = full.ravel()
    parts, offs = [np.asarray(r0["x"][:P])], [P] * len(per_rank)
    for free, n, key in ((lay["free_pt"], 3, "pt_index"), (lay["free_ln"], 6, "ln_index")):
        slot = np.cumsum(free) - 1
        full, cnt = np.full((int(free.sum()), n), np.nan), np.zeros(int(free.sum()), np.int64)
        for r, res in enumerate(per_rank):
            idx = np.asarray(shards[r]["shard"][key], np.int64)
            idx = idx[free[idx]] if len(idx) else idx
            x = np.asarray(res["x"])
            blocks = x[offs[r]:offs[r] + n * len(idx)]
            assert blocks.size == n * len(idx), ("x", key, r, len(x), offs[r], n, len(idx))
            offs[r] += blocks.size
            full[slot[idx]] = blocks.reshape(-1, n); cnt[slot[idx]] += 1
        assert (cnt == 1).all(), ("x", key)
        parts.append(full.ravel())
    for r, res in enumerate(per_rank):
        assert offs[r] == len(res["x"]), ("x of rank %d has %d entries, its free landmarks account for %d" % (r, len(res["x"]), offs[r]))
    out["x"] = np.concatenate(parts)
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def load_case(window_module, name):
    """(fixture, window) of a case of build_exact_cases; loaded once, shared, never written"""
    if name not in _CACHE:
        with np.load(os.path.join(GOLDEN, "build_exact_%s.npz" % name)) as z:
            fx = {k: z[k] for k in z.files}
        w = BC.CASES[name]["make"](window_module, BX.prior_of(fx))
        assert BC.window_sha(w) == str(fx["sha"]), "the window generator gives another window here than where the fixture was made"
        _CACHE[name] = (fx, w)
    return _CACHE[name]


# ---- the runs of tests/test_shard_exact.py and, on the oracle, of tests/test_shard_exact_cpu.py ------------------------------------------
def lambda_index(name, label):
    return [l for l in BC.CASES[name]["lambdas"] if (name, l) not in BC.DROPPED].index(label)


def _split(order, W):
    return [np.sort(order[(len(order) * r) // W:(len(order) * (r + 1)) // W]) for r in range(W)]


def _by_time(Wm, w, kind):
    lm, ob, kf = (("points", "po_pt", "po_kf"), ("lines", "lo_ln", "lo_kf"))[kind]
    first = Wm._first_kf(w[ob].astype(np.int64), w[kf].astype(np.int64), len(w[lm]))
    return np.argsort(first, kind="stable"), first


def edge_cut(Wm, w, kind):
    """the explicit three-rank cuts: [(point indices, line indices)] per rank"""
    none = np.zeros(0, np.int64)
    po, pfirst = _by_time(Wm, w, 0)
    lo, _ = _by_time(Wm, w, 1)
    if kind == "empty_rank":            # rank 1 holds no landmark at all
        p2, l2 = _split(po, 2), _split(lo, 2)
        return [(p2[0], l2[0]), (none, none), (p2[1], l2[1])]
    if kind == "rank0_empty":           # rank 0 holds the pose-side edges only
        p2, l2 = _split(po, 2), _split(lo, 2)
        return [(none, none), (p2[0], l2[0]), (p2[1], l2[1])]
    if kind == "lines_on_one_rank":     # rank 1 holds every line and no point
        p2 = _split(po, 2)
        return [(p2[0], none), (none, np.arange(len(w["lines"]))), (p2[1], none)]
    if kind == "one_bucket":            # rank 1 holds the points of one first-keyframe bucket only (the fullest one) and no line
        k = int(np.bincount(pfirst[pfirst < len(w["kf"]["vid_pvr"])]).argmax())      # (an unobserved landmark's first keyframe is 1 << 30)
        mine = np.flatnonzero(pfirst == k)
        rest = po[pfirst[po] != k]
        p2, l2 = _split(rest, 2), _split(lo, 2)
        return [(p2[0], l2[0]), (mine, none), (p2[1], l2[1])]
    raise KeyError(kind)


EDGE_KINDS = ("empty_rank", "one_bucket", "lines_on_one_rank", "rank0_empty")
EVERY_RANK_HAS_OBSERVATIONS = {"empty_rank": False, "one_bucket": True, "lines_on_one_rank": True, "rank0_empty": False}
# (a rank without an observation votes "does not fit" in prepare()'s fused-path vote — lm_structure_fits wants E > 0 — and the vote is
# global: every rank of such a window takes the record-based passes, whatever lm_fused asks for.  The tests assert exactly that.)

# (case, world, lambda label, edge cut or None)
RUNS = [(name, 3, 5.0, None) for name in BC.OLD]      # the twelve windows as uploaded (the gated cases of DESIGN.md 9l carry levels, which a shard cut does not)
for _W in (2, 8):
    RUNS += [("k6", _W, "init", None), ("k6", _W, 5.0, None), ("k6", _W, 0.05, None)]
    RUNS += [(name, _W, 5.0, None) for name in ("prior13", "fixed8", "noimu7", "k14_lines")]
RUNS += [(name, 3, 5.0, kind) for name in ("k6", "steps3") for kind in EDGE_KINDS]
# Left out by the verdict of tests/test_shard_exact_cpu.py (the sharded fp64 oracle against the same fixtures, before any device ran):
# {(case, world, lambda label, cut): why}.  At most two, and no case at every world.
DROPPED = {}


def run_id(run):
    name, W, label, kind = run
    return "%s-w%d-%s%s" % (name, W, label, "-" + kind if kind else "")


def local_ba_ranks(make_problem, protocol, w, W, stage1, stage2, window_module, distributed, cut=None, probe=None):
    """protocol.local_ba on every rank of a W-rank run: [per rank dict(results, gated, chi2_final, accepted, probe, shard)]"""
    shards = shards_of(window_module, w, W, cut)

    def body(r, attach):
        p = make_problem(); p.upload_window(shards[r]); attach(p)
        o = protocol.local_ba(p, stage1=stage1, stage2=stage2)
        out = dict(results=protocol.results(p), gated=o["gated"], chi2_final=o["stage2"].chi2_final, accepted=[t["accepted"] for t in p.trace()],
                   counts=tuple((o[k].iterations, o[k].trials) for k in ("stage1", "stage2")),
                   probe=probe(p) if probe is not None else None, shard=shards[r]["shard"])
        p.close()
        return out
    res, err = run_ranks(W, body, distributed)
    assert not any(err), "\n".join("rank %d:\n%s" % (r, e) for r, e in enumerate(err) if e)
    return res
