"""Synthetic loop-closure candidates for the relative-pose tests (tests/test_relpose_cpu.py, tests/test_relpose.py): matched stereo points
and line segments 2 - 15 m ahead of kf0, observed in kf1 through a true increment of a few cm and a few degrees, EuRoC intrinsics as
tests/lba_cases.py uses, pixel noise 0.5.  Both reference runs of a case (float64 and wide) are computed once and shared."""
import functools
import os
import shutil
import subprocess

import numpy as np

from . import lba_ref as LR
from . import relpose_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (458.654, 457.296, 367.215, 248.375)


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _proj(g):
    return np.stack([CAM[2] + CAM[0] * g[:, 0] / g[:, 2], CAM[3] + CAM[1] * g[:, 1] / g[:, 2]], -1)


def make(n_pt, n_ln, seed, trans=0.05, rot_deg=3.0, noise=0.5, outliers=0.0, gross=30.0, depth=(2.0, 15.0), spread=1.0, collinear=False):
    """one candidate: dict(P3, uv, pq, l3, cam, T_true)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    T = np.eye(4); T[:3, :3] = _rot(a * np.deg2rad(rot_deg)); T[:3, 3] = d * trans

    def cloud(n):
        z = rng.uniform(depth[0], depth[1], n)
        return np.stack([rng.uniform(-0.6, 0.6, n) * z * spread, rng.uniform(-0.4, 0.4, n) * z * spread, z], -1)
    P = cloud(n_pt)
    if collinear and n_pt:
        P = np.array([0.3, -0.2, 4.0]) + np.outer(np.linspace(0.0, 2.0, n_pt), np.array([0.5, 0.2, 1.0]))
    uv = _proj(P @ T[:3, :3].T + T[:3, 3]) + rng.normal(size=(n_pt, 2)) * noise
    bad = rng.permutation(n_pt)[:int(round(outliers * n_pt))]
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    uv[bad] += gross * np.stack([np.cos(ang), np.sin(ang)], -1)
    s = cloud(n_ln)
    q = s + rng.normal(size=(n_ln, 3)) * np.array([0.6, 0.6, 0.3])
    q[:, 2] = np.maximum(q[:, 2], 1.0)
    su = _proj(s @ T[:3, :3].T + T[:3, 3]) + rng.normal(size=(n_ln, 2)) * noise
    qu = _proj(q @ T[:3, :3].T + T[:3, 3]) + rng.normal(size=(n_ln, 2)) * noise
    l = np.cross(np.concatenate([su, np.ones((n_ln, 1))], -1), np.concatenate([qu, np.ones((n_ln, 1))], -1))
    l /= np.hypot(l[:, 0], l[:, 1])[:, None]                      # le: the normalised line through the two observed end points
    bad = rng.permutation(n_ln)[:int(round(outliers * n_ln))]
    l[bad, 2] += gross * rng.choice([-1.0, 1.0], len(bad))
    return dict(P3=P, uv=uv, pq=np.concatenate([s, q], -1), l3=l, cam=CAM, T_true=T)


def _with(case, T0=None, **opts):
    case = dict(case)
    if T0 is not None:
        case["T0"] = T0
    case["opts"] = opts
    return case


def _offset(T, trans, w):
    D = np.eye(4); D[:3, :3] = _rot(np.asarray(w, float)); D[:3, 3] = trans
    return T @ D


SIZES = ((3, 0), (0, 4), (63, 0), (64, 0), (65, 0), (40, 24), (129, 70), (300, 100))
# BUILD[name](seed) makes the case; SEED[name] is the seed in use: the first of 0, 1, 2, ... (pick_seed below) for which the REFERENCE ALONE
# serves the case's purpose (EXPECT), has (a) the decision margin of relpose_ref.decisions_have_margin and (b) a noise sample that is representative: the iteration of the text does not contract, so the rounding a float64
# evaluation ends with depends on the order of its sums, and one sample |float64 - wide| can by chance be tens of times smaller than the
# next; the rule's tolerance is only meaningful where the float64 reference itself, with its features in REORDER other orders, stays
# within half of it (reference_is_stable).  tests/test_relpose_cpu.py asserts both for every case.  No seed was chosen by what the library gives.
BUILD = {}
for _np, _nl in SIZES:      # feature counts around the wave, both protocols
    for _pr in (0, 1):
        BUILD["size_%d_%d_p%d" % (_np, _nl, _pr)] = (lambda seed, a=_np, b=_nl, c=_pr: _with(make(a, b, seed=seed), protocol=c))
for _pr in (0, 1):          # 20 % gross outliers in points and in lines
    BUILD["outliers_p%d" % _pr] = (lambda seed, c=_pr: _with(make(129, 70, seed=seed, outliers=0.2), protocol=c))
# start increments: a general one, an exactly-identity rotation, a rotation below 1e-6 rad (the small-angle branches of expmap / logmap)
BUILD["t0_general"] = lambda seed: (lambda k: _with(k, T0=_offset(k["T_true"], [0.02, -0.01, 0.015], [0.01, -0.02, 0.005])))(make(65, 20, seed=seed))
BUILD["t0_identity_rotation"] = lambda seed: (lambda k: _with(k, T0=_offset(np.eye(4), [0.01, 0.0, -0.01], [0, 0, 0])))(make(65, 20, seed=seed))
BUILD["t0_tiny_rotation"] = lambda seed: (lambda k: _with(k, T0=_offset(np.eye(4), [0.0, 0.01, 0.0], [3e-7, -2e-7, 4e-7])))(make(65, 20, seed=seed))
BUILD["t0_tiny_rotation_eval"] = lambda seed: (lambda k: _with(k, T0=_offset(np.eye(4), [0.0, 0.01, 0.0], [3e-7, -2e-7, 4e-7]), max_iters=0, max_iters_ref=0, protocol=1))(make(65, 20, seed=seed, trans=0.01, rot_deg=0.0))
# iteration limits, from a start near the true increment so that the cut of an evaluation-only stage keeps the inliers
_near = lambda k: _offset(k["T_true"], [0.004, -0.003, 0.002], [0.002, -0.001, 0.0015])
BUILD["iters_0_first"] = lambda seed: (lambda k: _with(k, T0=_near(k), max_iters=0))(make(70, 30, seed=seed))
BUILD["iters_0_ref"] = lambda seed: (lambda k: _with(k, T0=_near(k), max_iters_ref=0))(make(70, 30, seed=seed))
BUILD["iters_0_both"] = lambda seed: (lambda k: _with(k, T0=_near(k), max_iters=0, max_iters_ref=0))(make(70, 30, seed=seed))
BUILD["iters_1_only"] = lambda seed: (lambda k: _with(k, T0=_near(k), max_iters=1, max_iters_ref=0))(make(70, 30, seed=seed))
BUILD["iters_0_p1"] = lambda seed: (lambda k: _with(k, T0=_near(k), max_iters=0, protocol=1))(make(70, 30, seed=seed))
# decisions: one candidate per failing bit, one that passes all.  lc_res and lc_unc fail against thresholds of their own: with Cauchy weights
# every term of e is below 1, so lc_res = 1.0 cannot fail; and a candidate whose covariance exceeds 0.01 has an H of condition 1e9, on which
# no float64 evaluation is stable (criterion (b)), so lc_unc is set below the covariance of an ordinary candidate instead
BUILD["fail_res"] = lambda seed: _with(make(80, 20, seed=seed, noise=1.5), lc_res=0.3)
BUILD["fail_unc"] = lambda seed: _with(make(80, 20, seed=seed), lc_unc=1e-5)
BUILD["fail_trs"] = lambda seed: (lambda k: _with(k, T0=k["T_true"]))(make(80, 20, seed=seed, trans=2.0))
BUILD["fail_rot"] = lambda seed: (lambda k: _with(k, T0=k["T_true"]))(make(80, 20, seed=seed, rot_deg=40.0))
BUILD["fail_inl_p1"] = lambda seed: (lambda k: _with(k, T0=k["T_true"], protocol=1))(make(80, 20, seed=seed, outliers=0.75))
BUILD["pass_all_p1"] = lambda seed: _with(make(80, 20, seed=seed), protocol=1)
# degenerate candidates
BUILD["empty"] = lambda seed: _with(make(0, 0, seed=seed))
BUILD["collinear3"] = lambda seed: _with(make(3, 0, seed=seed, collinear=True))
# noise of 1e-7 px and room for 20 first-stage passes: the iteration converges until e (1e-10, held there by the homog_th floor of the norm)
# stalls far below its own size, so the |e - err_prev| exit is clearly taken by the first stage and again by the FIRST pass of the
# refinement, because err_prev is carried over (a reset err_prev would cost the refinement a second pass)
BUILD["stall"] = lambda seed: _with(make(40, 24, seed=seed, noise=1e-7), max_iters=20)
# what a case is for, as a property of the wide run (a seed must have it too)
_bits = lambda r: "".join(str(r[k]) for k in ("lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot"))
EXPECT = {n: (lambda r: True) for n in BUILD}
for _n in BUILD:
    if _n.startswith("size_") and not _n.startswith(("size_3_0", "size_0_4")) or _n.startswith(("t0_general", "t0_identity", "t0_tiny_rotation")) and not _n.endswith("eval") or _n in ("iters_0_first", "iters_0_ref", "iters_1_only", "pass_all_p1"):
        EXPECT[_n] = lambda r: r["accepted"] == 1
EXPECT["size_3_0_p0"] = EXPECT["size_3_0_p1"] = EXPECT["size_0_4_p0"] = EXPECT["size_0_4_p1"] = EXPECT["collinear3"] = lambda r: r["status"] == RR.RANK
EXPECT["outliers_p0"] = EXPECT["outliers_p1"] = lambda r: r["accepted"] == 1 and 140 <= r["n_inliers"] <= 165
EXPECT["fail_res"] = lambda r: r["status"] == RR.OK and _bits(r) == "01111"
EXPECT["fail_unc"] = lambda r: r["status"] == RR.OK and _bits(r) == "10111"
EXPECT["fail_trs"] = lambda r: r["status"] == RR.OK and _bits(r) == "11101"
EXPECT["fail_rot"] = lambda r: r["status"] == RR.OK and _bits(r) == "11110"
EXPECT["fail_inl_p1"] = lambda r: r["status"] == RR.OK and _bits(r) == "11011"
EXPECT["empty"] = lambda r: r["status"] == RR.EMPTY
EXPECT["stall"] = lambda r: r["accepted"] == 1 and r["iters"][0] < 20 and r["iters"][1] == 1
SEED = {'size_3_0_p0': 3, 'size_3_0_p1': 1, 'size_0_4_p0': 0, 'size_0_4_p1': 0, 'size_63_0_p0': 1, 'size_63_0_p1': 1, 'size_64_0_p0': 1, 'size_64_0_p1': 1,
        'size_65_0_p0': 2, 'size_65_0_p1': 2, 'size_40_24_p0': 2, 'size_40_24_p1': 1, 'size_129_70_p0': 0, 'size_129_70_p1': 1, 'size_300_100_p0': 0,
        'size_300_100_p1': 2, 'outliers_p0': 0, 'outliers_p1': 0, 't0_general': 2, 't0_identity_rotation': 1, 't0_tiny_rotation': 0, 't0_tiny_rotation_eval': 0,
        'iters_0_first': 1, 'iters_0_ref': 1, 'iters_0_both': 0, 'iters_1_only': 0, 'iters_0_p1': 0, 'fail_res': 1, 'fail_unc': 0, 'fail_trs': 0, 'fail_rot': 2,
        'fail_inl_p1': 1, 'pass_all_p1': 3, 'empty': 0, 'collinear3': 11, 'stall': 21}      # {n: pick_seed(n) for n in BUILD}
CASES = {n: (lambda n=n: BUILD[n](SEED[n])) for n in BUILD}
DEFAULT_OPTS = [n for n in ("size_3_0_p0", "size_0_4_p0", "size_63_0_p0", "size_64_0_p0", "size_65_0_p0", "size_40_24_p0", "size_129_70_p0", "size_300_100_p0",
                            "outliers_p0", "empty", "collinear3")]
REORDER = 12


def reordered(case, k):
    """the case with its points and its lines in the k-th other order (masks follow their features)"""
    rng = np.random.default_rng(7000 + k)
    pp, pl = rng.permutation(len(case["P3"])), rng.permutation(len(case["pq"]))
    c = dict(case)
    c["P3"], c["uv"], c["pq"], c["l3"] = case["P3"][pp], case["uv"][pp], case["pq"][pl], case["l3"][pl]
    if case.get("pt_in") is not None:
        c["pt_in"] = np.asarray(case["pt_in"])[pp]
    if case.get("ln_in") is not None:
        c["ln_in"] = np.asarray(case["ln_in"])[pl]
    return c


def reference_is_stable(case, r64, rw):
    """criterion (b): the largest error / tolerance, over the quantities of the rule, of the float64 reference against the wide run with the
    features in REORDER other orders; stable means at most 1/2.  A reordering that changes a discrete output counts as unstable."""
    tol, _ = RR.tolerances(r64, rw)
    worst = 0.0
    for k in range(REORDER):
        r = RR.run(reordered(case, k), np.float64, **case["opts"])
        if any(not np.array_equal(np.asarray(r[q]), np.asarray(rw[q])) for q in RR.EXACT):
            return np.inf
        for q in tol:
            worst = max(worst, float(np.abs(np.asarray(r[q], np.float64) - np.asarray(rw[q], np.float64)).max()) / tol[q] if tol[q] > 0 else 0.0)
    return worst


def pick_seed(name, start=0, tries=400):
    """the first seed from `start` on with (a) and (b), by the reference alone: how SEED was made"""
    for seed in range(start, start + tries):
        case = BUILD[name](seed)
        r64, rw = RR.run(case, np.float64, **case["opts"]), RR.run(case, LR.wide(), **case["opts"])
        if EXPECT[name](rw) and RR.decisions_have_margin(r64, rw) >= RR.MARGIN and reference_is_stable(case, r64, rw) <= 0.5:
            return seed
    raise RuntimeError("no seed for %s" % name)


@functools.lru_cache(maxsize=None)
def runs(name):
    """(case, float64 run, wide run) of the named case, computed once and shared"""
    case = CASES[name]()
    return case, RR.run(case, np.float64, **case["opts"]), RR.run(case, LR.wide(), **case["opts"])


HOSTCHECK_SRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc", "plba_relpose_hostcheck.cpp")


def build_hostcheck(out_dir, sanitize=True):
    """the stand-alone host program (csrc/plba_relpose_hostcheck.cpp), with the host sanitizers unless told otherwise; returns its path"""
    exe = os.path.join(out_dir, "plba_relpose_hostcheck" + ("_san" if sanitize else ""))
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    deps = [HOSTCHECK_SRC, os.path.join(ROOT, "pl-inertial-slam_amd", "csrc", "plba_relpose_dev.h"), os.path.join(ROOT, "include", "plba_g2o", "relative_pose.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    os.makedirs(out_dir, exist_ok=True)
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Wall"] + flags +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pl-inertial-slam_amd", "csrc"), HOSTCHECK_SRC, "-o", exe])
    return exe


def write_batch(path, cases, opts):
    """the host program's input file for a batch of cases under one set of options"""
    o = dict(RR.DEFAULTS); o.update(opts)
    B = len(cases)
    has_T0 = any(c.get("T0") is not None for c in cases)
    has_m = any(c.get("pt_in") is not None or c.get("ln_in") is not None for c in cases)
    ps = np.zeros(B + 1, np.int32); ps[1:] = np.cumsum([len(np.asarray(c["P3"]).reshape(-1, 3)) for c in cases])
    ls = np.zeros(B + 1, np.int32); ls[1:] = np.cumsum([len(np.asarray(c["pq"]).reshape(-1, 6)) for c in cases])
    cam = cases[0]["cam"]
    with open(path, "wb") as f:
        np.array([B, o["protocol"], o["max_iters"], o["max_iters_ref"], int(has_T0), int(has_m)], np.int32).tofile(f)
        np.array([o["homog_th"], o["chi2_th"], o["lc_res"], o["lc_unc"], o["lc_inl"], o["lc_trs"], o["lc_rot"]] + list(cam), np.float64).tofile(f)
        ps.tofile(f); ls.tofile(f)
        for k, wd in (("P3", 3), ("uv", 2), ("pq", 6), ("l3", 3)):
            np.concatenate([np.asarray(c[k], np.float64).reshape(-1, wd) for c in cases]).tofile(f)
        if has_T0:
            np.stack([np.eye(4) if c.get("T0") is None else np.asarray(c["T0"], np.float64) for c in cases]).tofile(f)
        if has_m:
            for k, st in (("pt_in", ps), ("ln_in", ls)):
                np.concatenate([np.ones(st[b + 1] - st[b], np.uint8) if c.get(k) is None else np.asarray(c[k]).astype(np.uint8) for b, c in enumerate(cases)] + [np.zeros(0, np.uint8)]).tofile(f)
    return ps, ls


def host_run(exe, tmp, cases, opts, lanes=None):
    """the batch through the host program (or, lanes = None, through `localba_harness relpose`, which writes the same file); a list of
    results in the layout of relpose_ref.run (plus `returned` and `pose_out`)"""
    fin, fout = os.path.join(tmp, "relpose_in.bin"), os.path.join(tmp, "relpose_out.bin")
    ps, ls = write_batch(fin, cases, opts)
    subprocess.check_call([exe, "relpose", fin, fout] if lanes is None else [exe, fin, fout, str(lanes)])
    B = len(cases)
    with open(fout, "rb") as f:
        od = np.fromfile(f, np.float64, 73 * B).reshape(B, 73)
        oi = np.fromfile(f, np.int32, 11 * B).reshape(B, 11)
        pm = np.fromfile(f, np.uint8, int(ps[-1])); lm = np.fromfile(f, np.uint8, int(ls[-1]))
    res = []
    for b in range(B):
        r = dict(T=od[b, :16].reshape(4, 4), pose_inc=od[b, 16:22], H=od[b, 22:58].reshape(6, 6), e=float(od[b, 58]), cov_eig=od[b, 59:65], t=od[b, 65], r=od[b, 66],
                 pose_out=od[b, 67:73], iters=[int(oi[b, 1]), int(oi[b, 2])], pt_in=pm[ps[b]:ps[b + 1]].astype(bool), ln_in=lm[ls[b]:ls[b + 1]].astype(bool), returned=int(oi[b, 10]))
        for i, k in enumerate(("n_inliers", None, None, "status", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot")):
            if k:
                r[k] = int(oi[b, i])
        res.append(r)
    return res


def as_result(out, b):
    """candidate b of Problem.relative_pose's dict in the layout of relpose_ref.run"""
    r = dict(T=out["T_inc"][b], pose_inc=out["pose_inc"][b], H=out["H"][b], e=float(out["e"][b]), cov_eig=out["cov_eig"][b], iters=[int(v) for v in out["iters"][b]],
             pt_in=np.asarray(out["pt_inlier"][b], bool), ln_in=np.asarray(out["ln_inlier"][b], bool))
    for k in ("status", "n_inliers", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot"):
        r[k] = int(out[k][b])
    return r
