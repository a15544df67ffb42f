"""Time of plba_relative_pose per call for B = 1, 8, 64 candidates of 300 points + 100 lines each (default options, protocol 0), against
the plain-C++ host function of include/plba_g2o/relative_pose.h on the same candidates (one lane, built -O2 without sanitizers from
csrc/plba_relpose_hostcheck.cpp, timed inside the program so that process start and file I/O stay out): best of `reps` wall-clock calls
after a warm-up on the device, the mean of `reps` batches on the host.  A single candidate is a launch-bound call:
python tools/time_relpose.py [reps]"""
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import relpose_cases as RC  # noqa: E402

pkg = ge.load_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
exe = RC.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_relpose_hostcheck"), sanitize=False)
p = pkg.new_problem()
res = {}
with tempfile.TemporaryDirectory() as tmp:
    for B in (1, 8, 64):
        cases = [RC.make(300, 100, seed=1000 + b) for b in range(B)]
        args = ([c["P3"] for c in cases], [c["uv"] for c in cases], [c["pq"] for c in cases], [c["l3"] for c in cases], RC.CAM)
        out = p.relative_pose(*args)      # warm-up
        wall = 1e9
        for _ in range(reps):
            t0 = time.perf_counter(); out = p.relative_pose(*args); wall = min(wall, time.perf_counter() - t0)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        RC.write_batch(fin, cases, {})
        host_ms = float(subprocess.check_output([exe, fin, fout, "1", str(max(reps, 2))]).split()[0])
        res["B=%d" % B] = dict(B=B, ms_device_call=round(wall * 1e3, 4), ms_host_function=round(host_ms, 4), accepted=int(out["accepted"].sum()),
                               passes=int(out["iters"].sum()))
        print("B=%d" % B, json.dumps(res["B=%d" % B]), flush=True)
p.close()
print(json.dumps(res))
