"""Wall time of plba_optimize_pose_graph (100 iterations, lambda = 1e-10) on loopClosureOptimizationCovGraphG2O-shaped graphs
(tests/pgo_ref.cov_graph) of 80, 300 and 1000 keyframes, next to the facade's host path on the same graphs (tools/localba_harness.cpp
essgraph: VertexSE3 / EdgeSE3 through SparseOptimizer::optimizeHost, identity information as that harness sets it), per iteration:
python tools/time_pgo.py [reps] [--once]
--once: one device call per size and no facade runs, for a separate  rocprofv3 --kernel-trace --stats -- python tools/time_pgo.py 1 --once"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, '.')
sys.path.insert(0, 'tools')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import pgo_ref  # noqa: E402

pkg = ge.load_package()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 3
once = "--once" in sys.argv


def log6(orc, X):
    """SE3Quat(R, t).log() through the oracle's restatement (what the harness's SE3Quat::exp inverts)"""
    import ctypes as C
    lib = orc.lib().cdll
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    R = np.ascontiguousarray(X[:9]); t = np.ascontiguousarray(X[9:12]); q = np.zeros(4); x = np.zeros(6)
    lib.orc_R_to_quat(dp(R), dp(q))
    q = q / np.linalg.norm(q) * (1.0 if q[3] >= 0 else -1.0)
    lib.orc_se3_log(dp(q), dp(t), dp(x))
    return x


def facade_s_per_iter(g, iters_list):
    """seconds per iteration of the facade's host loop: wall time of the harness at two iteration counts, differenced"""
    from harness_io import build_harness
    from oracle import oracle as orc
    orc.build()
    exe = build_harness()
    nv = g["nv"]
    est = np.array([log6(orc, x) for x in g["pose"]]); meas = np.array([log6(orc, z) for z in g["meas"]])
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for it in iters_list:
            fin, fout = os.path.join(td, "p.bin"), os.path.join(td, "p.out")
            with open(fin, "wb") as f:
                np.array([nv, len(g["ei"]), 0, it, 0], np.int32).tofile(f)
                np.arange(nv, dtype=np.int32).tofile(f); g["fixed"].astype(np.int32).tofile(f); est.tofile(f)
                g["ei"].astype(np.int32).tofile(f); g["ej"].astype(np.int32).tofile(f); meas.tofile(f)
            t0 = time.perf_counter()
            subprocess.check_call([exe, "pgo", fin, fout], timeout=3600)
            out[it] = time.perf_counter() - t0
            r = np.fromfile(fout, np.float64)
            out["done_%d" % it] = int(r[6 * nv + 2])
    a, b = iters_list
    return (out[b] - out[a]) / max(out["done_%d" % b] - out["done_%d" % a], 1), out


res = {}
for nv, fac_iters in ((80, (1, 6)), (300, (1, 4)), (1000, (1, 2))):
    g = pgo_ref.cov_graph(nv, seed=7)
    p = pkg.new_problem()
    best, st = 1e9, None
    for _ in range(1 if once else reps + 1):
        t0 = time.perf_counter()
        _, st, _ = p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], iters=100, user_lambda=1e-10)
        best = min(best, time.perf_counter() - t0)
    p.close()
    row = dict(nv=nv, ne=int(len(g["ei"])), P=6 * (nv - 2), device_ms=round(1e3 * best, 2), iterations=st["iterations"], trials=st["trials"],
               device_ms_per_trial=round(1e3 * best / max(st["trials"], 1), 3))
    if not once:
        gi = dict(g); gi["info"] = None
        _, sti, _ = pkg.new_problem().pgo(gi["pose"], gi["ei"], gi["ej"], gi["meas"], fixed=gi["fixed"], iters=100, user_lambda=1e-10)
        s_it, raw = facade_s_per_iter(gi, fac_iters)
        row.update(facade_ms_per_iter=round(1e3 * s_it, 2), facade_raw=raw, device_identity_info=dict(iterations=sti["iterations"], trials=sti["trials"], ms=round(sti["ms_total"], 2)))
    res[nv] = row
    print(json.dumps(row), flush=True)
