"""Time of plba_match_descriptors and plba_verify_loop_candidates per call for B = 1, 8, 64 keyframe pairs of 600 point + 200 line
descriptors each, against the plain-C++ drop-in of include/plba_g2o/match.h on one core (built -O2 without sanitizers from
csrc/plba_match_hostcheck.cpp, timed inside the program so that process start and file I/O stay out), and against the sequence the
composed call replaces: two match calls, the gate and the gather on the host (numpy over the flat arrays), one plba_relative_pose call.
The device calls are timed at the C ABI on arrays laid out beforehand: best of `reps` wall-clock calls after a warm-up; the host column is
the mean of `reps` batches.  A keyframe pair: 420 + 140 planted pairs (70 %), the planted geometry that of relpose_cases.make.
python tools/time_match.py [reps]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import match_ref as MR  # noqa: E402
from tests import relpose_cases as RC  # noqa: E402

pkg = ge.load_package()
abi = pkg.abi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
exe = MR.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_match_hostcheck"), sanitize=False)
p = pkg.new_problem()
fn = p.lib.fn
dp, ip, up = abi._dp, abi._ip, abi._up


def best(f):
    f()
    wall = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); f(); wall = min(wall, time.perf_counter() - t0)
    return wall * 1e3


def pair(seed):
    """600 + 200 rows a side, 420 + 140 planted"""
    c = RC.make(420, 140, seed=seed)
    return MR.loop_candidate(c, extra_pt=(3 / 7, 3 / 7), extra_ln=(3 / 7, 3 / 7), seed=seed)


res = {}
with tempfile.TemporaryDirectory() as tmp:
    for B in (1, 8, 64):
        kfs = [pair(1000 + b) for b in range(B)]
        k0s, k1s = [k[0] for k in kfs], [k[1] for k in kfs]
        cat = lambda ks, key, dt: np.ascontiguousarray(np.concatenate([k[key] for k in ks]), dtype=dt)
        st = lambda ks, key: MR._starts([k[key] for k in ks])
        pa, pb, la, lb = st(k0s, "pdesc"), st(k1s, "pdesc"), st(k0s, "ldesc"), st(k1s, "ldesc")
        dPA, dPB, dLA, dLB = (cat(ks, key, np.uint8) for ks, key in ((k0s, "pdesc"), (k1s, "pdesc"), (k0s, "ldesc"), (k1s, "ldesc")))
        P3, uv, pq, l3 = cat(k0s, "P3", np.float64), cat(k1s, "uv", np.float64), cat(k0s, "sPeP", np.float64), cat(k1s, "l3", np.float64)
        mo = abi.MatchOptions(); fn["match_default_options"](C.byref(mo))
        lo = abi.LoopOptions(); fn["loop_default_options"](C.byref(lo))
        ro = abi.RelposeOptions(); fn["relpose_default_options"](C.byref(ro))
        mp, ml = np.zeros(pa[-1], np.int32), np.zeros(la[-1], np.int32)
        cp, cl = np.zeros(B, np.int32), np.zeros(B, np.int32)

        def ok(rc):
            if rc != 0:
                raise RuntimeError("a call returned %d" % rc)

        def match_pt():
            ok(fn["match_descriptors"](p._h, C.byref(mo), B, ip(pa), up(dPA), ip(pb), up(dPB), None, ip(mp), ip(cp), None))

        def match_ln():
            ok(fn["match_descriptors"](p._h, C.byref(mo), B, ip(la), up(dLA), ip(lb), up(dLB), None, ip(ml), ip(cl), None))
        g = {}

        def gather():
            """the gate per candidate and the matched pairs of the passing ones, ascending i1, over the flat arrays"""
            n = lambda s: np.diff(s).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rp = np.maximum(100.0 * cp / n(pa), 100.0 * cp / n(pb)); rl = np.maximum(100.0 * cl / n(la), 100.0 * cl / n(lb))
            gate = (rp > 30.0) & (rl > 30.0)
            kp = (mp >= 0) & np.repeat(gate, np.diff(pa)); kl = (ml >= 0) & np.repeat(gate, np.diff(la))
            ipt, iln = np.flatnonzero(kp), np.flatnonzero(kl)
            g["P3"] = P3[ipt]; g["uv"] = uv[mp[ipt] + np.repeat(pb[:-1], np.diff(pa))[ipt]]
            g["pq"] = pq[iln]; g["l3"] = l3[ml[iln] + np.repeat(lb[:-1], np.diff(la))[iln]]
            g["ps"] = np.concatenate([[0], np.cumsum(np.where(gate, cp, 0))]).astype(np.int32)
            g["ls"] = np.concatenate([[0], np.cumsum(np.where(gate, cl, 0))]).astype(np.int32)
        rr = (abi.RelposeResult * B)()

        def relpose():
            ok(fn["relative_pose"](p._h, C.byref(ro), B, ip(g["ps"]), dp(g["P3"]), dp(g["uv"]), ip(g["ls"]), dp(g["pq"]), dp(g["l3"]), *[float(v) for v in RC.CAM],
                                   None, None, None, rr))
        lr = (abi.LoopResult * B)()
        mp2, ml2 = np.zeros(pa[-1], np.int32), np.zeros(la[-1], np.int32)

        def composed():
            ok(fn["verify_loop_candidates"](p._h, C.byref(lo), B, ip(pa), up(dPA), dp(P3), ip(pb), up(dPB), dp(uv), ip(la), up(dLA), dp(pq), ip(lb), up(dLB), dp(l3),
                                            *[float(v) for v in RC.CAM], ip(mp2), ip(ml2), None, None, lr))

        def sequence():
            match_pt(); match_ln(); gather(); relpose()
        t = dict(match_pt=best(match_pt), match_ln=best(match_ln), gather=best(gather), relpose=best(relpose), sequence=best(sequence), composed=best(composed))
        assert np.array_equal(mp, mp2) and np.array_equal(ml, ml2)
        assert all(bytes(a.relpose) == bytes(b) for a, b in zip(lr, rr))      # the composed call is the sequence, bit for bit
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        MR.write_match_batch(fin, [dict(d1=a["pdesc"], d2=b["pdesc"]) for a, b in kfs])
        host_pt = float(subprocess.check_output([exe, "match", fin, fout, "1", str(max(reps, 2))]).split()[0])
        MR.write_match_batch(fin, [dict(d1=a["ldesc"], d2=b["ldesc"]) for a, b in kfs])
        host_ln = float(subprocess.check_output([exe, "match", fin, fout, "1", str(max(reps, 2))]).split()[0])
        MR.write_loop_batch(fin, k0s, k1s)
        host_loop = float(subprocess.check_output([exe, "loop", fin, fout, str(max(reps, 2))]).split()[0])
        res["B=%d" % B] = dict(B=B, ms_match_points=round(t["match_pt"], 4), ms_match_lines=round(t["match_ln"], 4), ms_host_match_points=round(host_pt, 4),
                               ms_host_match_lines=round(host_ln, 4), ms_verify_composed=round(t["composed"], 4), ms_sequence=round(t["sequence"], 4),
                               ms_sequence_gather=round(t["gather"], 4), ms_sequence_relpose=round(t["relpose"], 4), ms_host_is_loop_closure=round(host_loop, 4),
                               matched_points=int(cp.sum()), matched_lines=int(cl.sum()), gate_passed=int(sum(r.ratio_ok for r in lr)),
                               accepted=int(sum(r.relpose.accepted for r in lr)))
        print("B=%d" % B, json.dumps(res["B=%d" % B]), flush=True)
p.close()
print(json.dumps(res))
