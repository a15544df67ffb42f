"""plba_relative_pose without a GPU: the numpy reference (tests/relpose_ref.py) against itself in a wide type, against numeric derivatives
and numpy's linear algebra; the device's arithmetic compiled for the host (csrc/plba_relpose_hostcheck.cpp: 64 emulated lanes in the
kernel's reduction order, and one lane = include/plba_g2o/relative_pose.h) under the tolerance rule the GPU tests use; the ABI surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import lba_ref as LR
from . import relpose_cases as RC
from . import relpose_ref as RR

ROOT = RC.ROOT
U = RR.U


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_reference_has_margin_and_float64_agrees_with_wide(name):
    """every case, by the reference alone: each comparison of the wide run (exit tests, the cut, the decisions) lies 1000 x the noise of
    the compared quantity away from its threshold, the float64 run made the same comparisons, and masks, counts and bits agree"""
    case, r64, rw = RC.runs(name)
    RR.hold(r64, r64, rw, "float64", name)


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_reference_noise_sample_is_representative(name):
    """every case, by the reference alone: it serves its purpose (relpose_cases.EXPECT), and the float64 reference with its features in
    12 other orders stays within HALF the rule's tolerance of the wide run with every discrete output unchanged.  The iteration of the
    text does not contract, so one sample |float64 - wide| can by chance be tens of times smaller than the next one
    (a 12-point candidate with cond(H) 1e9: 1.2e-9 .. 1.2e-7 in T over six orders); a case whose sample is such a chance is no yardstick
    for another evaluation in double precision, whatever its order of summation.  The seeds in use are the first that pass this and the
    margin test above (relpose_cases.pick_seed)."""
    case, r64, rw = RC.runs(name)
    assert RC.EXPECT[name](rw), name
    worst = RC.reference_is_stable(case, r64, rw)
    print("%s: reordered float64 reference, largest error / tolerance %.3f" % (name, worst))
    assert worst <= 0.5, (name, worst)


def _numeric(fn, h=1e-6, h_rot=None):
    d = np.zeros(6)
    for k in range(6):
        hk = h_rot if (h_rot is not None and k >= 3) else h
        e = np.zeros(6); e[k] = hk
        d[k] = (fn(e) - fn(-e)) / (2 * hk)
    return d


def _moved(T, delta, left=False):
    """T inverse(exp(delta)), or inverse(exp(delta)) T"""
    R, t = LR.se3_inv(*LR.se3_exp(np.asarray(delta, np.float64), np.float64))
    if left:
        return R @ T[:3, :3], R @ T[:3, 3] + t
    return T[:3, :3] @ R, T[:3, :3] @ t + T[:3, 3]


@pytest.mark.parametrize("kind", ["point", "line"])
def test_jacobian_is_minus_the_derivative_of_the_error_norm(kind):
    """J_aux against a central difference of the error norm: H x = g with g = sum J n w is a Gauss-Newton step when J_aux = -dn / d delta.
    Through T inverse(exp(delta)), the update the text applies (:3548), that holds at T = identity, where the reference starts.  At a
    general T the rows are written in the coordinates of the TRANSFORMED point (gx, gy, gz = T P, :3449-3451), so they are the derivative
    through inverse(exp(delta)) T — the perturbation on the other side of T_inc; both are asserted (SURVEY App. B-Q10 notes the mismatch,
    which this project reproduces).  The text uses fx for both image axes (:3453): the identity needs fx = fy, which this test sets.
    Away from the homog_th floors first, then once on each floor."""
    cam = np.array([458.654, 458.654, 367.215, 248.375])
    th = 1e-7
    k = RC.make(6, 6, seed=3)
    Tg = k["T_true"] @ np.linalg.inv(RC._offset(np.eye(4), [0.01, -0.02, 0.01], [0.01, 0.02, -0.01]))
    for T, left in ((np.eye(4), False), (np.eye(4), True), (Tg, True)):
        for i in range(6):
            if kind == "point":
                X, z = k["P3"][i], k["uv"][i]
                norm = lambda d: RR.point_err(cam, *_moved(T, d, left), X, z)[3]
                n, J = RR.point_obs(cam, th, T[:3, :3], T[:3, 3], X, z)
            else:
                X, z = k["pq"][i], k["l3"][i]
                norm = lambda d: RR.line_err(cam, *_moved(T, d, left), X, z)[4]
                n, J = RR.line_obs(cam, th, T[:3, :3], T[:3, 3], X, z)
            fd = _numeric(norm)
            assert n > 1e-3 and np.allclose(J, -fd, rtol=0, atol=1e-7 * np.abs(fd).max()), (kind, i, left, J, fd)
    # the floor of gz^2: a feature 1e-4 in front of the camera, J_aux = (gz^2 / homog_th) x the unclamped row
    s = 1e-4 / 4.0
    if kind == "point":
        X, z = np.array([0.3, -0.2, 4.0]) * s, np.array([400.0, 230.0])
        norm = lambda d: RR.point_err(cam, *_moved(np.eye(4), d), X, z)[3]
        n, J = RR.point_obs(cam, th, np.eye(3), np.zeros(3), X, z)
    else:
        X, z = np.array([0.3, -0.2, 4.0, 0.5, 0.1, 4.0]) * s, np.array([0.6, 0.8, -430.0])
        norm = lambda d: RR.line_err(cam, *_moved(np.eye(4), d), X, z)[4]
        n, J = RR.line_obs(cam, th, np.eye(3), np.zeros(3), X, z)
    fd = _numeric(norm, h=1e-10, h_rot=1e-5)      # (a rotation below 1e-6 rad is the identity to expmap_se3; a translation must stay far below the depth)
    assert np.allclose(J[:3], -fd[:3] * (1e-4 ** 2 / th), rtol=1e-5, atol=0) and np.allclose(J[3:], -fd[3:] * (1e-4 ** 2 / th), rtol=0, atol=1e-5 * np.abs(fd[3:]).max()), (kind, J, fd)
    # the floor of the norm: an error of 9e-8 px, J_aux homog_th = the row before the division = -d (n^2 / 2) / d delta
    if kind == "point":
        X = np.array([0.3, -0.2, 4.0])
        g = X
        z = np.array([cam[2] + cam[0] * g[0] / g[2] + 5.4e-8, cam[3] + cam[1] * g[1] / g[2] - 7.2e-8])
        half = lambda d: RR.point_err(cam, *_moved(np.eye(4), d), X, z)[3] ** 2 / 2
        n, J = RR.point_obs(cam, th, np.eye(3), np.zeros(3), X, z)
    else:
        X = np.array([0.3, -0.2, 4.0, 0.5, 0.1, 5.0])
        su, sv = RR._project(cam, X[:3]); eu, ev = RR._project(cam, X[3:])
        l = np.cross([su, sv, 1.0], [eu, ev, 1.0]); l /= np.hypot(l[0], l[1]); z = l + np.array([0, 0, 6e-8])
        half = lambda d: RR.line_err(cam, *_moved(np.eye(4), d), X, z)[4] ** 2 / 2
        n, J = RR.line_obs(cam, th, np.eye(3), np.zeros(3), X, z)
    assert n < th
    # h above the 1e-6 rad below which expmap_se3 returns the identity; the central difference's own error is h^2 |J J''|, about
    # 4e-12 x 1e4 against rows of 1e-5: a few parts in a thousand
    fd = _numeric(half, h=2e-6)
    assert np.allclose(J * th, -fd, rtol=0, atol=2e-2 * np.abs(J * th).max()), (kind, J * th, fd)


def _pass_system(name):
    case = RC.CASES[name]()
    cam = np.array(case["cam"])
    n, J = RR.point_obs(cam, 1e-7, np.eye(3), np.zeros(3), case["P3"], case["uv"])
    if len(case["pq"]):
        n2, J2 = RR.line_obs(cam, 1e-7, np.eye(3), np.zeros(3), case["pq"], case["l3"])
        n, J = np.concatenate([n, n2]), np.concatenate([J, J2])
    w = 1 / (1 + n * n)
    return (J[:, :, None] * J[:, None, :] * w[:, None, None]).sum(0), (J * (n * w)[:, None]).sum(0)


def test_qr_solve_against_numpy_and_the_rank_rule():
    for name in ("size_40_24_p0", "size_300_100_p0", "size_63_0_p0"):
        H, g = _pass_system(name)
        x, rank, _ = RR.qr_solve(H, g, np.float64)
        ref = np.linalg.solve(H, g)
        assert rank == 6 and np.abs(x - ref).max() <= 64 * U * np.linalg.cond(H) * np.abs(ref).max(), name
    # three collinear points and no line: three scalar residuals, a rank-3 H; the deficient part of the solution is zero and what is
    # left solves the system (g lies in the range of H)
    H, g = _pass_system("collinear3")
    x, rank, piv = RR.qr_solve(H, g, np.float64)
    assert rank == 3 and np.count_nonzero(x) == 3
    assert np.abs(H @ x - g).max() <= 1e-9 * np.abs(g).max()
    xw, rankw, _ = RR.qr_solve(LR.cast(H, LR.wide()), LR.cast(g, LR.wide()), LR.wide())
    assert rankw == 3 and np.array_equal(LR.f64(xw) != 0, x != 0)


def test_cov_eig_against_numpy():
    for name in ("size_40_24_p0", "size_300_100_p0", "outliers_p0", "fail_unc", "size_65_0_p1"):
        _, r64, rw = RC.runs(name)
        ref = np.linalg.eigvalsh(np.linalg.inv(rw["H"]))
        k = np.linalg.cond(rw["H"])
        assert np.abs(rw["cov_eig"] - ref).max() <= 64 * U * k * np.abs(ref).max(), (name, rw["cov_eig"], ref)
        assert np.all(np.diff(rw["cov_eig"]) >= 0)


@pytest.fixture(scope="module")
def hostcheck():
    return RC.build_hostcheck(os.path.join(ROOT, "tools", "_build_relpose_hostcheck"), sanitize=True)


@pytest.mark.parametrize("lanes", [64, 1])
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_host_check_holds_the_rule(hostcheck, tmp_path, name, lanes):
    """the device's arithmetic on the CPU, built with the address and undefined-behaviour sanitizers and run directly: 64 emulated lanes
    in the kernel's reduction order, and one lane, which is include/plba_g2o/relative_pose.h as a caller uses it.  The same rule as the
    GPU tests: 8 x the float64 reference's own noise against the wide run, everything discrete exactly."""
    case, r64, rw = RC.runs(name)
    res = RC.host_run(hostcheck, str(tmp_path), [case], case["opts"], lanes)[0]
    RR.hold(res, r64, rw, "host%d" % lanes, name)
    assert res["returned"] == rw["accepted"]
    if rw["accepted"]:
        assert np.array_equal(res["pose_out"], res["pose_inc"])
    else:
        assert not res["pose_out"].any()      # a refused candidate leaves pose_inc alone


def test_host_check_batch_is_the_candidates_alone(hostcheck, tmp_path):
    cases = [RC.runs(n)[0] for n in RC.DEFAULT_OPTS]
    batch = RC.host_run(hostcheck, str(tmp_path), cases, {}, 64)
    for n, c, b in zip(RC.DEFAULT_OPTS, cases, batch):
        alone = RC.host_run(hostcheck, str(tmp_path), [c], {}, 64)[0]
        for k in ("T", "pose_inc", "H", "e", "cov_eig", "iters", "status", "pt_in", "ln_in"):
            assert np.array_equal(np.asarray(alone[k]), np.asarray(b[k]), equal_nan=True), (n, k)


def test_abi_surface(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct sizes as a C compiler lays out include/plba.h, and the defaults of the reference's configuration"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    assert hasattr(lib, "plba_relative_pose") and hasattr(lib, "plba_relpose_default_options")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(plba_relpose_options), '
                   'sizeof(plba_relpose_result), offsetof(plba_relpose_result, n_inliers), offsetof(plba_relpose_options, lc_res)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    so, sr, off_n, off_res = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert (so, sr) == (C.sizeof(abi.RelposeOptions), C.sizeof(abi.RelposeResult)) == (72, 576)
    assert off_n == abi.RelposeResult.n_inliers.offset and off_res == abi.RelposeOptions.lc_res.offset
    o = abi.RelposeOptions()
    f = lib.plba_relpose_default_options
    f.restype = None; f.argtypes = [C.POINTER(abi.RelposeOptions)]
    f(C.byref(o))
    assert (o.max_iters, o.max_iters_ref, o.homog_th, o.chi2_th, o.protocol) == (5, 10, 1e-7, 7.815, 0)
    assert (o.lc_res, o.lc_unc, o.lc_inl, o.lc_trs, o.lc_rot) == (1.0, 0.01, 0.3, 1.5, 35.0)
    assert {"relative_pose", "relpose_default_options"} <= set(abi.SIGNATURES) and {"relative_pose", "relpose_default_options"} <= abi.PRODUCT_ONLY
    assert (abi.RELPOSE_OK, abi.RELPOSE_EMPTY, abi.RELPOSE_NONFINITE, abi.RELPOSE_RANK) == (RR.OK, RR.EMPTY, RR.NONFINITE, RR.RANK)
