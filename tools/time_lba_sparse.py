"""Dense against sparse reduced-camera solver (plba_lba_options.solver 0 / 1) of plba_lba_visual on whole-map windows
(window.make_map_window: 20 points + 4 lines first seen per keyframe, tracks over 2 .. 6 consecutive keyframes, a few revisits) at 100, 400,
1 000 and 3 000 local keyframes, called as globalBundleAdjustment calls it (variant = 1, machine epsilon for both thresholds: every pass
runs).  Per size and solver: wall time of a call of PASSES[0] and of PASSES[1] passes, their difference per pass (the set-up of a call
-- lists, analysis, uploads -- cancels), the device bytes of the pose system (sparse: plba_debug_get "lba_sparse"[6]; dense: the system
and its factor, 2 x (Ppad + 64) x Ppad doubles) and the structure the analysis reports.  The dense leg is skipped above --dense-max local
keyframes.  One JSON line per run.
python tools/time_lba_sparse.py [--sizes N ...] [--dense-max N] [--reps R]
Run it under a time limit of its own, e.g.  timeout 600 python tools/time_lba_sparse.py"""
import argparse
import json
import sys
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

PASSES = (2, 6)
EPS = 2.0 ** -52

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="*", default=[100, 400, 1000, 3000])
ap.add_argument("--dense-max", type=int, default=1000)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
pkg = ge.load_package()


def run(w, n, solver):
    p = pkg.new_problem()
    args = (w["T_kf_w"], w["kf_loc"], w["xyz"], w["pq"], w["po_pt"], w["po_kf"], w["uv"], w["lo_ln"], w["lo_kf"], w["l3"], w["cam"])
    best, res = {}, None
    for passes in PASSES:
        best[passes] = 1e30
        for _ in range(a.reps + 1):      # (the first call warms the allocator up)
            t0 = time.perf_counter()
            res = p.lba_visual(*args, variant=1, min_error=EPS, min_error_change=EPS, max_iters=passes, solver=solver)
            best[passes] = min(best[passes], time.perf_counter() - t0)
        assert res["iterations"] == passes and not res["solver_failed"], res
    info = p.debug_get("lba_sparse")
    p.close()
    ppad = (6 * n + 63) // 64 * 64
    row = dict(keyframes=n, observations=len(w["po_pt"]) + len(w["lo_ln"]), solver="sparse" if solver else "dense",
               call_ms={k: round(1e3 * v, 2) for k, v in best.items()}, ms_per_pass=round(1e3 * (best[PASSES[1]] - best[PASSES[0]]) / (PASSES[1] - PASSES[0]), 3),
               device_mb=round(info[6] / 2 ** 20, 2) if solver else round(2 * (ppad + 64) * ppad * 8 / 2 ** 20, 2), err_last=res["err_last"], lam=res["lam"])
    if solver:
        row.update(fronts=int(info[2]), levels=int(info[3]), nnz_blocks_L=int(info[4]), max_front=int(info[5]), analysis_ms=round(info[7], 2))
    print(json.dumps(row), flush=True)


for n in a.sizes:
    w = pkg.window.make_map_window(n, revisits=max(3, n // 100))
    if n <= a.dense_max:
        run(w, n, 0)
    run(w, n, 1)
