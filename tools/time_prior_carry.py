"""The marginalization prior carried on the device (plba_marginalize_to_prior) against the host round trip (plba_marginalize -> slide ->
plba_set_prior), per keyframe of a sliding sequence, the two forms alternating in one process after a warm-up.

Each form runs blocks of --block keyframes back to back on a stream of its own, the blocks of the two forms alternating.  Nothing
synchronises inside a block: a marginalization the device form leaves queued is waited for by whatever needs it next (the next keyframe's
plba_optimize resolves it), and the stream synchronisation at the block's end — the last marginalization's completion — is counted in the
block.  Per-keyframe figures are block time / block length.

Shapes: the reference's own 12-keyframe window (bench.py realistic_leg's, cut from make_sequence(..., track=(6, 12))) and configs[3]
(50 KF / 20k points / 4k lines + IMU + prior).  Per form, medians over --kf keyframes of
  marg_host_ms    host time inside the marginalization call
  marg_device_ms  device time of the marginalization (events on the problem's stream around the call)
  ba_ms           the slid local BA call alone (protocol.local_ba without the marginalization, host wall)
  kf_ms           slide + local_ba + results() + marginalization, back to back (the write-back does not depend on the marginalization and
                  goes first: on the problem's stream it would wait for the enqueued one)
  kf_gap_ms       the same with a fixed host gap (--gap-ms, busy, no synchronisation) before each keyframe — the mapping thread's other
                  work, during which a queued marginalization may run — not counted
The host round trip's set_prior is part of its slide step.  One JSON line per shape; with --out, also written there.

  python tools/time_prior_carry.py [--kf 30] [--block 5] [--warm 1] [--gap-ms 3] [--shapes 12kf,cfg3] [--forms device,host_round_trip] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402  (before the library: one HSA runtime, as in __graft_entry__.build())
import numpy as np  # noqa: E402
import __graft_entry__ as g  # noqa: E402

SHAPES = {
    "12kf": dict(K=12, Np=2000, Nl=400, kw=dict(kf_dt=0.1, track=(6, 12), revisit=0.2)),
    "cfg3": dict(K=50, Np=20000, Nl=4000, kw={}),
}


class Carry:
    """one handle sliding through the sequence with one form of the prior's carry"""

    def __init__(self, pkg, seq, K, device, stream):
        self.pkg, self.seq, self.K, self.device, self.stream = pkg, seq, K, device, stream
        self.p = pkg.new_problem()
        self.p.set_stream(stream.cuda_stream)
        self.w = pkg.window.window_at(seq, 0, K)
        self.p.upload_window(self.w)
        self.prior, self.i = None, 0

    def cut(self, n):
        """the next n windows and their deltas, cut from the sequence before a block (outside the timed span)"""
        prev, self.nxt = self.w, []
        for i in range(self.i, self.i + n):
            if i:
                w = self.pkg.window.window_at(self.seq, i, self.K, prev=prev)
                self.nxt.append((w, self.pkg.window.slide_delta(prev, w)))
                prev = w
            else:
                self.nxt.append(None)

    def step(self):
        """one keyframe, nothing waited for at its end; returns (marg_host_ms, ba_ms, marg_event_pair)"""
        pkg, p = self.pkg, self.p
        nxt = self.nxt.pop(0)
        if nxt is not None:
            w, delta = nxt
            p.slide_window(delta)
            for kind, d in w["huber"].items():
                p.set_robust(kind, True, d)
            if not self.device:
                p.set_prior(self.prior)
            self.w = w
        tb = time.perf_counter()
        pkg.protocol.local_ba(p)
        tm = time.perf_counter()
        pkg.protocol.results(p)      # (the write-back first: it would otherwise queue behind the enqueued marginalization on the stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t1 = time.perf_counter()
        e0.record(self.stream)
        if self.device:
            p.marginalize_to_prior(0, pkg.protocol.MARG_NUM)
        else:
            self.prior = p.marginalize(0, pkg.protocol.MARG_NUM)
        t2 = time.perf_counter()
        e1.record(self.stream)
        self.i += 1
        return (t2 - t1) * 1e3, (tm - tb) * 1e3, (e0, e1)


def measure(pkg, shape, n_kf, block, warm, gap_ms, which=("device", "host_round_trip")):
    s = SHAPES[shape]
    nblk = max(1, n_kf // block)
    nwin = 2 * (warm + nblk) * block + 1
    seq = pkg.window.make_sequence(s["K"], nwin, s["Np"], s["Nl"], seed=0x9A1DC0, **s["kw"])
    streams = {f: torch.cuda.Stream() for f in which}
    forms = {f: Carry(pkg, seq, s["K"], f == "device", streams[f]) for f in which}
    torch.cuda.synchronize()
    rows = {f: dict(marg_host_ms=[], marg_device_ms=[], ba_ms=[], kf_ms=[], kf_gap_ms=[], prior_n=0) for f in forms}
    events = {f: [] for f in forms}
    for phase, gap in (("kf_ms", 0.0), ("kf_gap_ms", gap_ms)):
        for b in range(warm + nblk):
            for f, c in forms.items():      # (alternating blocks)
                r, total = rows[f], 0.0
                c.cut(block)
                for _ in range(block):
                    if gap:
                        t = time.perf_counter() + gap * 1e-3
                        while time.perf_counter() < t:
                            pass
                    t0 = time.perf_counter()
                    mh, ba, ev = c.step()
                    total += time.perf_counter() - t0
                    if b >= warm and phase == "kf_ms":
                        r["marg_host_ms"].append(mh); r["ba_ms"].append(ba); events[f].append(ev)
                t0 = time.perf_counter()
                streams[f].synchronize()      # the block's last marginalization, counted
                total += time.perf_counter() - t0
                if b >= warm:
                    r[phase].append(total * 1e3 / block)
    torch.cuda.synchronize()
    out = dict(shape=shape, K=s["K"], Np=s["Np"], Nl=s["Nl"], keyframes=nblk * block, block=block, warmup_blocks=warm, gap_ms=gap_ms)
    for f, c in forms.items():
        r = rows[f]
        r["marg_device_ms"] = [e0.elapsed_time(e1) for e0, e1 in events[f]]
        r["prior_n"] = int(c.p.dims.get("n_prior", 0))
        out[f] = {k: (float(np.median(v)) if isinstance(v, list) else v) for k, v in r.items()}
        c.p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=30)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1, help="warm-up blocks per form and phase")
    ap.add_argument("--gap-ms", type=float, default=3.0)
    ap.add_argument("--shapes", default="12kf,cfg3")
    ap.add_argument("--forms", default="device,host_round_trip", help="one of them alone: e.g. a trace of one form")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = g.load_package()
    res = []
    for shape in a.shapes.split(","):
        r = measure(pkg, shape, a.kf, a.block, a.warm, a.gap_ms, tuple(a.forms.split(",")))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
