"""Time of plba_refine_landmarks (every landmark, default options: 5 iterations, 10 trials) on the 12-keyframe window, BASELINE
configs[2] and configs[4], from a freshly uploaded window (the state a slide leaves its added landmarks in): best of `reps` after a
warm-up, HIP events on the problem's stream next to the wall clock; the landmarks are put back before every repetition
(plba_restore_state).  As the only available yardstick the same run prints the cost of one LM iteration of the same window the way
bench.py takes it (stage 1 + gating, then stage 2 replayed from the saved state, wall time / iterations):
python tools/time_refine.py [reps]"""
import json
import sys
import time

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402  (torch's HIP runtime first, as in the tests)

pkg = ge.load_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
windows = {"k12": lambda: pkg.window.make_window(12, 500, 100, imu=True, seed=0x5EED0A01),
           "configs[2]": lambda: pkg.window.make_config(3), "configs[4]": lambda: pkg.window.make_config(5)}
stream = torch.cuda.Stream()
res = {}
for name, mk in windows.items():
    w = mk()
    p = pkg.new_problem()
    p.set_stream(stream.cuda_stream)
    p.upload_window(w)
    p.save_state()
    got = p.refine_landmarks()      # warm-up (and the structure build)
    wall, dev = 1e9, 1e9
    for _ in range(reps):
        p.restore_state()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter(); got = p.refine_landmarks(); t1 = time.perf_counter()
        e1.record(stream)
        torch.cuda.synchronize()
        wall, dev = min(wall, t1 - t0), min(dev, e0.elapsed_time(e1) * 1e-3)
    # one joint LM iteration of the same window, as bench.py measures it
    p.restore_state()
    p.optimize(pkg.protocol.STAGE1_ITERS); p.gate_outliers(pkg.window.CHI2_GATE); p.save_state()
    p.restore_state(); p.optimize(10)
    torch.cuda.synchronize()
    done, t0 = 0, time.perf_counter()
    while done < 30:
        p.restore_state()
        st = p.optimize(10)
        done += max(st.iterations, 1)
    torch.cuda.synchronize()
    ms_step = (time.perf_counter() - t0) / done * 1e3
    m = w["meta"]
    res[name] = dict(K=m["K"], Np=m["Np"], Nl=m["Nl"], E=m["Ep"] + m["El"], ms_refine_wall=round(wall * 1e3, 3), ms_refine_events=round(dev * 1e3, 3),
                     lm_iterations=int(got["iterations"]), lm_trials=int(got["trials"]), n_exhausted=got["n_exhausted"],
                     chi2_before=got["chi2_before"], chi2_after=got["chi2_after"], ms_per_step_joint_lm=round(ms_step, 3))
    print(name, json.dumps(res[name]), flush=True)
    p.close()
print(json.dumps(res))
