"""g2o::StructureOnlySolver<3> / <6> of the facade (include/plba_g2o/g2o_compat.h): calc() refines the listed landmark vertices on the
device — tools/localba_harness.cpp `structonly` — to the C ABI's result bit for bit; a vertex that is no landmark is refused loudly."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from harness_io import build_harness, write_window  # noqa: E402

@pytest.mark.gpu
def test_calc_moves_the_selected_landmarks_to_the_c_abi_result(pkg, hip, tmp_path):
    w = pkg.window.make_window(12, 120, 30, imu=True, seed=77)
    K, Np, Nl = 12, len(w["points"]), len(w["lines"])
    exe = build_harness()
    win, res = str(tmp_path / "w.bin"), str(tmp_path / "r.bin")
    write_window(w, win)
    subprocess.check_call([exe, "structonly", win, res], timeout=120)
    with open(res, "rb") as f:
        P, q = np.fromfile(f, np.float64, 3 * K).reshape(K, 3), np.fromfile(f, np.float64, 4 * K).reshape(K, 4)
        pts, lns = np.fromfile(f, np.float64, 3 * Np).reshape(Np, 3), np.fromfile(f, np.float64, 6 * Nl).reshape(Nl, 6)
    # the same graph through the C ABI: keyframes only (no bias vertices, no IMU edges), as the harness holds them
    w2 = dict(w)
    w2["kf"] = dict(w["kf"], P=P, q=q, vid_bias=np.full(K, -1, np.int32))
    w2["imu"] = None
    w2["huber"] = {0: w["huber"][0], 1: w["huber"][1]}
    sp, sl = np.arange(Np) % 2 == 0, np.arange(Nl) % 2 == 0
    g = pkg.new_problem(); g.upload_window(w2)
    g.refine_landmarks(select_point=sp, select_line=np.zeros(Nl, bool), max_iters=3)       # calc<3>(points), then calc<6>(lines)
    g.refine_landmarks(select_point=np.zeros(Np, bool), select_line=sl, max_iters=3)
    rp, rl = g.get_points(), g.get_lines()
    g.close()
    assert np.array_equal(pts, rp) and np.array_equal(lns, rl)
    assert np.all(np.any(pts[sp] != w["points"][sp], 1)) and np.all(np.any(lns[sl] != w["lines"][sl], 1)), "a selected landmark came back unchanged"
    assert np.array_equal(pts[~sp], w["points"][~sp]) and np.array_equal(lns[~sl], w["lines"][~sl])


def test_calc_on_a_keyframe_vertex_fails_loudly(pkg, tmp_path):
    """(refused before anything is uploaded: needs no device)"""
    w = pkg.window.make_window(12, 40, 10, imu=True, seed=78)
    exe = build_harness()
    win = str(tmp_path / "w.bin")
    write_window(w, win)
    r = subprocess.run([exe, "structonly_bad", win, str(tmp_path / "r.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "[plba g2o facade]" in r.stderr and "VertexLMPointXYZ" in r.stderr
