"""Dense against sparse pose-graph solver (options.pgo_solver 0 / 1) of plba_optimize_pose_graph on loopClosureOptimizationCovGraphG2O-
shaped graphs (tests/pgo_ref.cov_graph, lambda = 1e-10): whole-call wall time and wall time per LM trial at 300, 1000 and 5000 keyframes,
the sparse solver alone at 20 000 (and at a larger size if asked), with the structure the sparse analysis reports (plba_debug_get
"pgo_sparse": fronts, tree levels, nonzero 6 x 6 blocks of L, largest front, device bytes, host ms of the analysis).  One JSON line per run.
python tools/time_pgo_sparse.py [--reps R] [--big NV ...] [--once]
The dense path at 5000 keyframes runs DENSE_5000_ITERS iterations only (its per-trial cost grows as P^3).  --once: one call per
configuration, for a  rocprofv3 --kernel-trace --stats -- python tools/time_pgo_sparse.py --once  run."""
import argparse
import json
import sys
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import pgo_ref  # noqa: E402

DENSE_5000_ITERS = 2

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--big", type=int, nargs="*", default=[20000])
ap.add_argument("--once", action="store_true")
a = ap.parse_args()
pkg = ge.load_package()


def run(g, solver, iters):
    p = pkg.new_problem(pgo_solver=solver)
    best, st = 1e30, None
    for _ in range(1 if a.once else a.reps + 1):      # (the first call warms the allocator up)
        t0 = time.perf_counter()
        _, st, _ = p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], info=g["info"], fixed=g["fixed"], iters=iters, user_lambda=1e-10)
        best = min(best, time.perf_counter() - t0)
    info = p.debug_get("pgo_sparse")
    p.close()
    row = dict(nv=g["nv"], P=6 * (g["nv"] - 2), solver="sparse" if solver else "dense", iters_asked=iters, iterations=st["iterations"],
               trials=st["trials"], call_ms=round(1e3 * best, 2), ms_per_trial=round(1e3 * best / max(st["trials"], 1), 3),
               chi2_initial=st["chi2_initial"], chi2_final=st["chi2_final"])
    if solver:
        row.update(fronts=int(info[2]), levels=int(info[3]), nnz_blocks_L=int(info[4]), max_front=int(info[5]),
                   device_mb=round(info[6] / 2 ** 20, 1), analysis_ms=round(info[7], 2))
    print(json.dumps(row), flush=True)
    return row


for nv in (300, 1000, 5000):
    g = pgo_ref.cov_graph(nv, seed=7)
    it = DENSE_5000_ITERS if nv >= 5000 else 100
    run(g, 0, it)
    run(g, 1, it)
    if it != 100:
        run(g, 1, 100)
for nv in a.big:
    run(pgo_ref.cov_graph(nv, seed=7), 1, 100)
