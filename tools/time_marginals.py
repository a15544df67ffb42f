"""Wall time of plba_compute_marginals (keyframe blocks + every point / line) on the 12-keyframe reference-shaped window and on
BASELINE configs[2] and configs[4] (0-based: window.make_config(3) and (5), both with IMU edges — a window
without them leaves every velocity unconstrained, and the call then refuses it with PLBA_ERR_NUMERIC), after the two-stage local BA, next to one optimize(10) on the same state:
python tools/time_marginals.py [reps]"""
import json
import sys
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

pkg = ge.load_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
windows = {"k12": lambda: pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AA, track=(6, 12)),
           "configs[2]": lambda: pkg.window.make_config(3), "configs[4]": lambda: pkg.window.make_config(5)}
res = {}
for name, mk in windows.items():
    w = mk()
    p = pkg.new_problem()
    p.upload_window(w)
    pkg.protocol.local_ba(p)
    p.save_state()
    m = p.marginals()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); p.marginals(); best = min(best, time.perf_counter() - t0)
    ba = 1e9
    for _ in range(3):
        p.restore_state()
        t0 = time.perf_counter(); p.optimize(10); ba = min(ba, time.perf_counter() - t0)
    res[name] = dict(P=int(p.debug_get("pose_dim")[0]), K=len(m["kf"]), Np=len(m["pt"]), Nl=len(m["ln"]), n_excluded=m["n_excluded"],
                     ms_marginals=round(best * 1e3, 3), ms_optimize10=round(ba * 1e3, 3))
    print(name, json.dumps(res[name]), flush=True)
    p.close()
print(json.dumps(res))
