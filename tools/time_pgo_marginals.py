"""plba_pose_graph_marginals on loopClosureOptimizationCovGraphG2O-shaped graphs (tests/pgo_ref.cov_graph) of 300, 1 000, 5 000 and
20 000 keyframes: every vertex block plus every edge as a pair.  One JSON line per size: the whole call in ms (best of --reps after a
warm-up call: host analysis, uploads, linearisation, factorisation, selected inversion, read-back), the "pgo_cov" record (free
vertices, fronts, tree levels, blocks of L, largest front, device bytes, host ms of the analysis), and, from the same run on the same
graph, the ms per trial of plba_optimize_pose_graph with options.pgo_solver = 1 (whole call / trials, as tools/time_pgo_sparse.py).
python tools/time_pgo_marginals.py [--reps R] [--sizes NV ...]"""
import argparse
import json
import sys
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

import numpy as np  # noqa: E402

from tests import pgo_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="*", default=[300, 1000, 5000, 20000])
a = ap.parse_args()
pkg = ge.load_package()

for nv in a.sizes:
    g = pgo_ref.cov_graph(nv, seed=7)
    pairs = np.stack([g["ei"], g["ej"]], 1)
    p = pkg.new_problem(pgo_solver=1)
    best = 1e30
    for _ in range(a.reps + 1):      # (the first call warms the allocator up)
        t0 = time.perf_counter()
        out = p.pgo_marginals(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], pairs=pairs)
        best = min(best, time.perf_counter() - t0)
    rec = p.debug_get("pgo_cov")
    tb, st = 1e30, None
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        _, st, _ = p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], iters=100, user_lambda=1e-10)
        tb = min(tb, time.perf_counter() - t0)
    p.close()
    print(json.dumps(dict(nv=nv, P=6 * (nv - 2), pairs=len(pairs), call_ms=round(1e3 * best, 2), analysis_ms=round(rec[7], 2),
                          pgo_cov=[int(rec[0]), int(rec[1]), int(rec[2]), int(rec[3]), int(rec[4]), int(rec[5]), int(rec[6]), round(rec[7], 2)],
                          device_mb=round(rec[6] / 2 ** 20, 1), status=[int(x) for x in out["n_status"]],
                          pgo_sparse_trial_ms=round(1e3 * tb / max(st["trials"], 1), 3), pgo_sparse_call_ms=round(1e3 * tb, 2), pgo_sparse_trials=st["trials"])),
          flush=True)
