"""Time of plba_track_pose per call for B = 1, 8, 64 problems of 300 points + 100 lines each (default options), against the plain-C++
host function of include/plba_g2o/track_pose.h on the same problems (one lane, built -O2 without sanitizers from
csrc/plba_track_hostcheck.cpp, timed inside the program so that process start and file I/O stay out): best of `reps` wall-clock calls
after a warm-up on the device, the mean of `reps` batches on the host.  A single problem is a launch-bound call:
python tools/time_track.py [reps]"""
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import track_cases as TC  # noqa: E402

pkg = ge.load_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
exe = TC.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_track_hostcheck"), sanitize=False)
p = pkg.new_problem()
res = {}
with tempfile.TemporaryDirectory() as tmp:
    for B in (1, 8, 64):
        cases = [TC.make(300, 100, seed=1000 + b) for b in range(B)]
        out = TC.call(p, cases, {})      # warm-up
        wall = 1e9
        for _ in range(reps):
            t0 = time.perf_counter(); out = TC.call(p, cases, {}); wall = min(wall, time.perf_counter() - t0)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        TC.write_batch(fin, cases, {})
        host_ms = float(subprocess.check_output([exe, fin, fout, "1", str(max(reps, 2))]).split()[0])
        res["B=%d" % B] = dict(B=B, ms_device_call=round(wall * 1e3, 4), ms_host_function=round(host_ms, 4), good=int(out["good"].sum()),
                               passes=int(out["iters"].sum()), paths=sorted(set(int(v) for v in out["path"])))
        print("B=%d" % B, json.dumps(res["B=%d" % B]), flush=True)
p.close()
print(json.dumps(res))
