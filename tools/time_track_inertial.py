"""Time of plba_track_inertial per call for B = 1, 8, 64 problems of 300 points + 100 lines each (default options: 4 rounds of up to 10
iterations), with the anchor fixed and with it free, against the plain-C++ host function of include/plba_g2o/track_inertial.h on the same
problems (one lane on one core, built -O2 without sanitizers from csrc/plba_vitrack_hostcheck.cpp, timed inside the program so that
process start and file I/O stay out): best of `reps` wall-clock calls after a warm-up on the device, the mean of `reps` batches on the host.

As context, `parent`: ONE fixed-anchor problem by the only device route there was before this entry, a two-keyframe window with every
landmark flagged fixed through upload + per round plba_optimize(iters) + plba_gate_outliers, with and without the upload in the time.
That route cannot batch, has no free anchor with an EdgeNavStatePrior and returns no marginal information; its Huber / gate protocol is
the BA's (kernels on in every round here), so it is a cost figure, not the same computation.
python tools/time_track_inertial.py [reps] [--no-parent]"""
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

from tests import vitrack_cases as VC  # noqa: E402
from tests import vitrack_ref as VR  # noqa: E402

pkg = ge.load_package()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 20
exe = VC.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_vitrack_hostcheck"), sanitize=False)
p = pkg.new_problem()
res = {}
with tempfile.TemporaryDirectory() as tmp:
    for free in (False, True):
        for B in (1, 8, 64):
            cases = [VC.frame(1000 + b, 300, 100, free=free) for b in range(B)]
            out = VC.call(p, cases, {})      # warm-up
            wall = 1e9
            for _ in range(reps):
                t0 = time.perf_counter(); out = VC.call(p, cases, {}); wall = min(wall, time.perf_counter() - t0)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            VC.write_batch(fin, cases, {})
            host_ms = float(subprocess.check_output([exe, fin, fout, "1", str(max(reps, 2))]).split()[0])
            key = "%s B=%d" % ("free" if free else "fixed", B)
            res[key] = dict(B=B, anchor_free=int(free), ms_device_call=round(wall * 1e3, 4), ms_host_function=round(host_ms, 4), ok=int((out["status"] == VR.OK).sum()),
                            iterations=int(out["iterations"].sum()), trials=int(out["trials"].sum()))
            print(key, json.dumps(res[key]), flush=True)
p.close()

if "--no-parent" not in sys.argv:
    c = VC.frame(1000, 300, 100)
    o = dict(VR.DEFAULTS)
    st = lambda k: np.stack([np.asarray(c["si"], np.float64)[k], np.asarray(c["sj"], np.float64)[k]])
    Np, Nl = len(c["Pw"]), len(c["pq"])
    w = dict(cam=dict(fx=c["cam"][0], fy=c["cam"][1], cx=c["cam"][2], cy=c["cam"][3], Rbc=np.asarray(c["Rbc"], np.float64), Pbc=np.asarray(c["Pbc"], np.float64)), gw=c["gw"],
             kf=dict(vid_pvr=np.array([0, 2], np.int32), vid_bias=np.array([1, 3], np.int32), P=st(slice(0, 3)), V=st(slice(3, 6)), q=st(slice(6, 10)), bg=st(slice(10, 13)),
                     ba=st(slice(13, 16)), dbg=st(slice(16, 19)), dba=st(slice(19, 22)), fixed_pvr=np.array([1, 0], np.uint8), fixed_bias=np.array([1, 0], np.uint8)),
             points=c["Pw"], point_fixed=np.ones(Np, np.uint8), lines=c["pq"], line_fixed=np.ones(Nl, np.uint8),
             po_pt=np.arange(Np, dtype=np.int32), po_kf=np.ones(Np, np.int32), po_uv=c["uv"], po_w=c["pt_w"],
             lo_ln=np.arange(Nl, dtype=np.int32), lo_kf=np.ones(Nl, np.int32), lo_l=c["l3"], lo_w=c["ln_w"],
             imu=dict(kf_i=np.array([0], np.int32), kf_j=np.array([1], np.int32), preint=np.asarray(c["pre"]).reshape(1, 142), info_pvr=np.asarray(c["ipvr"]).reshape(1, 81),
                      info_bias=np.asarray(c["ibias"]).reshape(1, 36)),
             prior=None, huber={pkg.abi.EDGE_POINT: o["huber_pt"], pkg.abi.EDGE_LINE: o["huber_ln"]})
    q = pkg.new_problem()

    def route(upload):
        if upload:
            q.upload_window(w)
        else:
            q.restore_state()
            q.set_levels(pkg.abi.EDGE_POINT, np.zeros(Np, np.uint8)); q.set_levels(pkg.abi.EDGE_LINE, np.zeros(Nl, np.uint8))
        its = 0
        for _ in range(o["rounds"]):
            its += q.optimize(o["iters"]).iterations
            q.gate_outliers(o["chi2_pt"])
        return its
    route(True)      # warm-up: allocations, the structure build
    t_up, t_res = 1e9, 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); its = route(True); t_up = min(t_up, time.perf_counter() - t0)
    q.upload_window(w); q.recompute_errors(); q.save_state()
    for _ in range(reps):
        t0 = time.perf_counter(); its = route(False); t_res = min(t_res, time.perf_counter() - t0)
    q.close()
    res["parent"] = dict(B=1, ms_upload_optimize_gate=round(t_up * 1e3, 4), ms_restore_optimize_gate=round(t_res * 1e3, 4), iterations=int(its))
    print("parent", json.dumps(res["parent"]), flush=True)
print(json.dumps(res))
