"""Time of the plba_covis_* calls on synthetic trajectories of 300 / 1 000 / 5 000 / 20 000 keyframes (about 120 observations a
keyframe, three quarters points and one quarter lines, tracks of 2 - 12 consecutive observers, one track in twenty revisiting an earlier
keyframe): plba_covis_set_map, the whole graph through plba_covis_rows (n = K), plba_covis_pose_graph over all keyframes, one
plba_covis_column (the newest keyframe's) and plba_covis_local_map (the newest keyframe's).  Wall clock per call at the C ABI on arrays
laid out beforehand, capacities exact, best of `reps` after a warm-up; beside them the same queries through include/plba_g2o/covis.h on
one core (csrc/plba_covis_hostcheck.cpp built -O2 without sanitizers, timed inside the program, best of `host_reps`).  Also printed: the
bytes the reference's dense full_graph would take (4 K^2) and the device bytes of the resident map.
python tools/time_covis.py [reps] [host_reps]"""
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

from tests import covis_ref as CR  # noqa: E402

pkg = ge.load_package()
abi = pkg.abi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
host_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SIZES = (300, 1000, 5000, 20000)
exe = CR.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_covis_hostcheck"), sanitize=False)


def trajectory(K, seed):
    """(start, kf) per kind, vectorised: 17 tracks begin at every keyframe"""
    rng = np.random.default_rng(seed)
    out = []
    for per_kf in (13, 4):
        first = np.repeat(np.arange(K), per_kf)
        ln = np.minimum(rng.integers(2, 13, len(first)), K - first)
        revisit = (rng.random(len(first)) < 0.05) & (first > 20)
        tot = ln + revisit
        start = np.zeros(len(first) + 1, np.int64); start[1:] = np.cumsum(tot)
        kf = np.repeat(first, tot) + (np.arange(start[-1]) - np.repeat(start[:-1], tot))
        back = (rng.random(int(revisit.sum())) * (first[revisit] - 10)).astype(np.int64)
        kf[start[1:][revisit] - 1] = back      # the revisiting track's last entry: an earlier keyframe
        out += [start.astype(np.int32), kf.astype(np.int32)]
    return out


def best(call, n):
    call()
    b = 1e9
    for _ in range(n):
        t0 = time.perf_counter()
        rc = call()
        b = min(b, time.perf_counter() - t0)
        assert rc == 0, rc
    return b * 1e3


p = pkg.new_problem()
fn, dp, ip, up = p.lib.fn, abi._dp, abi._ip, abi._up
res = {}
with tempfile.TemporaryDirectory() as tmp:
    for K in SIZES:
        ps, pk, ls, lk = trajectory(K, 100 + K)
        Np, Nl = len(ps) - 1, len(ls) - 1
        info = np.zeros(6)
        t_set = best(lambda: fn["covis_set_map"](p._h, K, None, Np, ip(ps), ip(pk), Nl, ip(ls), ip(lk), dp(info)), reps)
        kf = np.arange(K, dtype=np.int32)
        rs, col, cnt = p.covis_rows(kf)      # (sizes the arrays)
        nnz = len(col)
        col, cnt = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.int32)
        t_rows = best(lambda: fn["covis_rows"](p._h, K, ip(kf), 0, ip(rs), nnz, ip(col), ip(cnt)), reps)
        o = abi.CovisOptions(); fn["covis_default_options"](C.byref(o))
        P = CR.poses(K)
        ei, ej, Z = p.covis_pose_graph(P)
        ne = len(ei)
        Z = np.zeros((ne, 12)); n_out = C.c_int(0)
        t_pg = best(lambda: fn["covis_pose_graph"](p._h, C.byref(o), K, dp(P), 0, None, None, ne, ip(ei), ip(ej), dp(Z), C.byref(n_out)), reps)
        cov = np.zeros(K, np.int32)
        t_col = best(lambda: fn["covis_column"](p._h, K - 1, ip(cov)), reps)
        fk, fp, fl, c3 = np.zeros(K, np.uint8), np.zeros(Np, np.uint8), np.zeros(Nl, np.uint8), np.zeros(3, np.int32)
        t_lm = best(lambda: fn["covis_local_map"](p._h, C.byref(o), K - 1, up(fk), up(fp), up(fl), ip(c3)), reps)
        m = dict(K=K, pts=range(Np), lns=range(Nl), pt_start=ps, pt_kf=pk, ln_start=ls, ln_kf=lk, live=None)
        q = dict(rows=kf, min_count=0, idx=K - 1, nv=K, loops=[], kf=K - 1)
        pin = os.path.join(tmp, "in.bin")
        CR.write_host_input(pin, m, q, None, P)
        host = [float(v) for v in subprocess.check_output([exe, pin, "-", str(host_reps)]).split()]
        res[K] = dict(observations=int(info[3] + info[4]), landmarks=Np + Nl, nnz=nnz, edges=ne, local=[int(v) for v in c3], dense_bytes=4 * K * K, device_bytes=int(info[5]),
                      device_ms=dict(set_map=round(t_set, 4), rows=round(t_rows, 4), pose_graph=round(t_pg, 4), column=round(t_col, 4), local_map=round(t_lm, 4)),
                      host_ms=dict(zip(("set_map", "rows", "pose_graph", "column", "local_map"), (round(v, 4) for v in host))))
        print("K %6d: %8d obs, nnz %8d, %7d edges | device ms set %.3f rows %.3f graph %.3f column %.3f local %.3f | covis.h ms set %.3f rows %.3f graph %.3f column %.3f "
              "local %.3f | dense %.1f MB, resident %.2f MB" % ((K, res[K]["observations"], nnz, ne, t_set, t_rows, t_pg, t_col, t_lm) + tuple(host)
                                                                + (4e-6 * K * K, info[5] / 1e6)), flush=True)
p.close()
print(json.dumps(dict(what="covisibility graph, ~120 observations a keyframe", reps=reps, host_reps=host_reps, sizes=res)))
