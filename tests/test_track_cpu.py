"""plba_track_pose without a GPU: the numpy reference (tests/track_ref.py) against itself in a wide type, against numeric derivatives,
numpy.sort and a brute-force projection; the device's arithmetic compiled for the host (csrc/plba_track_hostcheck.cpp: 64 emulated lanes
in the kernel's reduction order, and one lane = include/plba_g2o/track_pose.h) under the tolerance rule the GPU tests use; the ABI surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import lba_ref as LR
from . import relpose_ref as RR
from . import track_cases as TC
from . import track_ref as TR

ROOT = TC.ROOT


def _numeric(fn, h=1e-6):
    d = np.zeros(6)
    for k in range(6):
        e = np.zeros(6); e[k] = h
        d[k] = (fn(e) - fn(-e)) / (2 * h)
    return d


def _moved(T, delta, left=False):
    """T inverse(exp(delta)), or inverse(exp(delta)) T"""
    R, t = LR.se3_inv(*LR.se3_exp(np.asarray(delta, np.float64), np.float64))
    if left:
        return R @ T[:3, :3], R @ T[:3, 3] + t
    return T[:3, :3] @ R, T[:3, :3] @ t + T[:3, 3]


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_reference_has_margin_and_float64_agrees_with_wide(name):
    """every case, by the reference alone: each comparison of the wide run (exit tests, err > err_prev, isGoodSolution's four tests, the
    overlap branch and lambda tests, r < 2 stdv, the cut, the clamp of s, the log-determinant) lies 1000 x the noise of the compared
    quantity away from its threshold, the MAD lies that far from a float rounding boundary, the float64 run made the same comparisons,
    and masks, counts, path, status and good agree"""
    case, r64, rw = TC.runs(name)
    TR.hold(r64, r64, rw, "float64", name)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_reference_noise_sample_is_representative(name):
    """every case, by the reference alone: it serves its purpose (track_cases.EXPECT), and the float64 reference with its features in 12
    other orders stays within HALF the rule's tolerance of the wide run with every discrete output unchanged (see tests/test_relpose_cpu.py)"""
    case, r64, rw = TC.runs(name)
    assert TC.EXPECT[name](rw), name
    worst = TC.reference_is_stable(case, r64, rw)
    print("%s: reordered float64 reference, largest error / tolerance %.3f" % (name, worst))
    assert worst <= 0.5, (name, worst)


def test_cases_cover_the_paths_and_exits():
    """what the cases are for, as properties of the wide runs taken together"""
    runs = {n: TC.runs(n)[2] for n in TC.CASES}
    assert {r["path"] for r in runs.values()} == {TR.REFINED, TR.ROBUST, TR.FEW_BEFORE, TR.FEW_AFTER}
    exits = {(s, w) for r in runs.values() for s, w in r["exits"]}
    assert {(1, "gt"), (2, "negdet"), (0, "limit"), (2, "limit")} <= exits, exits
    assert set().union(*[r["branches"] for r in runs.values()]) == {0, 1, 2} and set().union(*[r["outcomes"] for r in runs.values()]) == {0, 1, 2, 3, 4}
    assert runs["outliers_t0"]["started_from"] is not None and np.array_equal(runs["outliers_t0"]["started_from"][0], TC.runs("outliers_t0")[0]["T0"][:3, :3])
    # the err = -1 return of :435 needs err > 999999999.9 on the first pass.  Every term of e is r^2 w = r^2 / (1 + r^2) < 1 times an
    # overlap in [0, 1], so e < 1 for finite input and the return cannot be reached; no case can take it
    assert all(w != "minus1" for _, w in exits)


@pytest.mark.parametrize("kind", ["point", "line"])
def test_jacobian_times_sqrt_sigma2_is_minus_the_derivative_of_the_residual(kind):
    """r = |err| sqrt(sigma2) against a central difference: H x = g with g = sum J r w is a Gauss-Newton step of the scaled residual when
    J_aux sqrt(sigma2) = -dr / d delta.  The text leaves sqrt(sigma2) out of J_aux (:615, :683), which this project reproduces: the
    identity holds for sigma2 = 1 and is off by sqrt(sigma2) otherwise; both are asserted.  Through T inverse(exp(delta)) at T = identity
    and through inverse(exp(delta)) T at a general T, as tests/test_relpose_cpu.py explains; fx = fy."""
    cam = np.array([458.654, 458.654, 367.215, 248.375])
    th = 1e-7
    k = TC.make(6, 6, seed=3)
    Tg = k["T_true"] @ np.linalg.inv(TC._offset(np.eye(4), [0.01, -0.02, 0.01], [0.01, 0.02, -0.01]))
    for T, left in ((np.eye(4), False), (Tg, True)):
        for i in range(6):
            if kind == "point":
                X, z, s2 = k["P3"][i], k["uv"][i], k["pt_s2"][i]
                res = lambda d: RR.point_err(cam, *_moved(T, d, left), X, z)[3] * np.sqrt(s2)
                n, J = RR.point_obs(cam, th, T[:3, :3], T[:3, 3], X, z)
            else:
                X, z, s2 = k["pq"][i], k["l3"][i], k["ln_s2"][i]
                res = lambda d: RR.line_err(cam, *_moved(T, d, left), X, z)[4] * np.sqrt(s2)
                n, J = RR.line_obs(cam, th, T[:3, :3], T[:3, 3], X, z)
            fd = _numeric(res)
            assert n > 1e-3 and np.allclose(J * np.sqrt(s2), -fd, rtol=0, atol=1e-7 * np.abs(fd).max()), (kind, i, left, J, fd)
            if s2 != 1.0:
                assert not np.allclose(J, -fd, rtol=0, atol=1e-3 * np.abs(fd).max())


@pytest.fixture(scope="module")
def hostcheck():
    return TC.build_hostcheck(os.path.join(ROOT, "tools", "_build_track_hostcheck"), sanitize=True)


@pytest.mark.parametrize("lanes", [64, 1])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_selection_is_numpy_sort(hostcheck, tmp_path, n, lanes):
    """track::select, every k, against numpy.sort: distinct values, ties, all values equal, a zero, a denormal, and a flagged subset"""
    rng = np.random.default_rng(n)
    lists = [rng.uniform(0, 50, n), np.round(rng.uniform(0, 4, n)), np.full(n, 0.731), np.concatenate([[0.0, 5e-324], rng.uniform(0, 1e-300, n)])[:n],
             np.float32(rng.uniform(0, 3, n)).astype(np.float64)]
    for v in lists:
        assert np.array_equal(TC.host_select(hostcheck, str(tmp_path), v, None, lanes), np.sort(v))
        m = rng.uniform(size=n) < 0.6
        assert np.array_equal(TC.host_select(hostcheck, str(tmp_path), v, m, lanes), np.sort(v[m]))


def _brute_overlap(so, eo, sp, ep):
    """the length, in units of the observed segment, of what the projected segment covers of it: orthogonal projection on the observed line"""
    l = eo - so
    lam = sorted([float((sp - so) @ l / (l @ l)), float((ep - so) @ l / (l @ l))])
    return max(0.0, min(lam[1], 1.0) - max(lam[0], 0.0))


def test_overlap_against_a_brute_force_projection():
    """lineSegmentOverlap in each of its three branches and all five lambda outcomes.  On an exactly vertical or horizontal observed
    segment its branch formula is the orthogonal projection; the general branch is it for every direction"""
    rng = np.random.default_rng(1)
    seen = set()
    for branch, direction in ((0, np.array([0.0, 1.0])), (1, np.array([1.0, 0.0])), (2, np.array([0.6, 0.8])), (2, np.array([-0.8, 0.6]))):
        for a, b in TC.SLIDES:
            for _ in range(4):
                s = rng.uniform(100, 300, 2)
                e = s + direction * rng.uniform(40, 120) * rng.choice([-1.0, 1.0])
                so, eo = s + a * (e - s), s + b * (e - s)
                sp, ep = s + rng.normal(size=2) * 0.5, e + rng.normal(size=2) * 0.5
                chk = []
                ov, br, k = TR.line_overlap(so, eo, sp, ep, lambda l, v, t: (chk.append(l), bool(v < t))[1])
                ref = _brute_overlap(so, eo, sp, ep)
                assert br == branch and abs(float(ov) - ref) <= 1e-12, (branch, a, b, ov, ref)
                seen.add((br, k))
    assert seen == {(br, k) for br in range(3) for k in range(5)}, seen
    # nearly vertical (|dx| < 1): the vertical branch is taken and uses the y coordinates alone
    so, eo = np.array([200.0, 100.0]), np.array([200.6, 180.0])
    ov, br, k = TR.line_overlap(so, eo, np.array([230.0, 120.0]), np.array([170.0, 160.0]), lambda l, v, t: bool(v < t))
    assert br == 0 and k == 4 and abs(float(ov) - 0.5) <= 1e-15


@pytest.mark.parametrize("lanes", [64, 1])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_host_check_holds_the_rule(hostcheck, tmp_path, name, lanes):
    """the device's arithmetic on the CPU, built with the address and undefined-behaviour sanitizers and run directly: 64 emulated lanes
    in the kernel's reduction order, and one lane, which is include/plba_g2o/track_pose.h as a caller uses it.  The same rule as the GPU
    tests: 8 x the float64 reference's own noise against the wide run, everything discrete exactly."""
    case, r64, rw = TC.runs(name)
    res = TC.host_run(hostcheck, str(tmp_path), [case], case["opts"], lanes)[0]
    TR.hold(res, r64, rw, "host%d" % lanes, name)


def test_host_check_batch_is_the_problems_alone(hostcheck, tmp_path):
    cases = [TC.runs(n)[0] for n in TC.DEFAULT_OPTS]
    batch = TC.host_run(hostcheck, str(tmp_path), cases, {}, 64)
    for n, c, b in zip(TC.DEFAULT_OPTS, cases, batch):
        alone = TC.host_run(hostcheck, str(tmp_path), [c], {}, 64)[0]
        for k in TR.QUANT + TR.EXACT + ("pt_in", "ln_in"):
            assert np.array_equal(np.asarray(alone[k]), np.asarray(b[k]), equal_nan=True), (n, k)


def test_abi_surface(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct sizes as a C compiler lays out include/plba.h, and the defaults of the reference's configuration"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    assert hasattr(lib, "plba_track_pose") and hasattr(lib, "plba_track_default_options")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(plba_track_options), '
                   'sizeof(plba_track_result), offsetof(plba_track_result, n_inliers_pt), offsetof(plba_track_options, homog_th)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    so, sr, off_n, off_h = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert (so, sr) == (C.sizeof(abi.TrackOptions), C.sizeof(abi.TrackResult)) == (48, 952)
    assert off_n == abi.TrackResult.n_inliers_pt.offset and off_h == abi.TrackOptions.homog_th.offset
    o = abi.TrackOptions()
    f = lib.plba_track_default_options
    f.restype = None; f.argtypes = [C.POINTER(abi.TrackOptions)]
    f(C.byref(o))
    assert (o.max_iters, o.max_iters_ref, o.min_features, o.homog_th, o.min_error, o.min_error_change, o.inlier_k) == (5, 10, 10, 1e-7, 1e-7, 1e-7, 4.0)
    assert {k: getattr(o, k) for k in TR.DEFAULTS} == TR.DEFAULTS
    assert {"track_pose", "track_default_options"} <= set(abi.SIGNATURES) and {"track_pose", "track_default_options"} <= abi.PRODUCT_ONLY
    assert (abi.TRACK_OK, abi.TRACK_NONFINITE, abi.TRACK_RANK) == (TR.OK, TR.NONFINITE, TR.RANK)
    assert (abi.TRACK_REFINED, abi.TRACK_ROBUST, abi.TRACK_FEW_BEFORE, abi.TRACK_FEW_AFTER) == (TR.REFINED, TR.ROBUST, TR.FEW_BEFORE, TR.FEW_AFTER)
