"""plba_match_descriptors and plba_verify_loop_candidates without a GPU: the numpy reference (tests/match_ref.py) against scipy's Hamming
distance and its own case conditions; the device's arithmetic compiled for the host (csrc/plba_match_hostcheck.cpp: plba_match_dev.h in
the kernels' tile order, and include/plba_g2o/match.h) built with the address and undefined-behaviour sanitizers and run directly,
against the reference for EQUALITY — everything here is an integer or one rounded operation, there is no tolerance; the ABI surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import match_ref as MR
from . import relpose_cases as RC

ROOT = MR.ROOT
NAMES = sorted(MR.CASES)


def test_reference_distances_equal_scipy():
    from scipy.spatial.distance import cdist
    for name in ("size_65_63", "size_129_257", "float_pin", "tie_rule"):
        c, _ = MR.runs(name)
        bits = lambda d: np.unpackbits(d, axis=1)
        ref = cdist(bits(c["d1"]), bits(c["d2"]), "hamming") * 256
        D = MR.distances(c["d1"], c["d2"])
        assert np.array_equal(D, np.rint(ref).astype(np.int32)) and np.abs(ref - np.rint(ref)).max() < 1e-9, name


def test_the_tiles_are_the_header_s():
    txt = open(os.path.join(ROOT, "pl-inertial-slam_amd", "csrc", "plba_match_dev.h")).read()
    assert int(re.search(r"QUERY_TILE = (\d+)", txt).group(1)) == MR.QUERY_TILE and int(re.search(r"TRAIN_TILE = (\d+)", txt).group(1)) == MR.TRAIN_TILE
    sizes = set(MR.SIZES)
    for t in (MR.QUERY_TILE, MR.TRAIN_TILE):      # tile - 1, tile, tile + 1, 2 tiles + 1 on either side
        for n in (t - 1, t, t + 1, 2 * t + 1):
            assert any(n in s for s in sizes), n
    assert {(257, 63), (65, 257), (513, 300)} <= sizes


def test_case_conditions_by_the_reference_alone():
    """every case: at least half of the planted pairs matched; some case loses a match to the mutual check; some case has a row whose
    best distance is tied; the prototype's sizes behave as the recipe's prototype did"""
    lost, tied = [], []
    for name in NAMES:
        c, r = MR.runs(name)
        hit = sum(int(r["matches_12"][a] == b) for a, b in c["pairs"])
        assert 2 * hit >= len(c["pairs"]), (name, hit, len(c["pairs"]))
        assert r["n"] == int((r["matches_12"] >= 0).sum()) <= r["one_way"]
        if c["best_lr"] and r["n"] < r["one_way"]:
            lost.append(name)
        if len(r["nn3"]) and ((r["nn3"][:, 1] == r["nn3"][:, 2]) & (r["nn3"][:, 1] >= 0)).any():
            tied.append(name)
    assert lost and tied
    for name in MR.PROTOTYPE:
        assert name in tied and name in lost, name
    print("cases that lose a match to the mutual check: %d, with a tied best: %d of %d" % (len(lost), len(tied), len(NAMES)))


def test_float_pin_passes_in_double_and_fails_in_float():
    c, r = MR.runs("float_pin")
    assert [tuple(t) for t in r["nn3"]] == [(1, 4, 5), (3, 8, 10)]
    assert list(r["matches_12"]) == [-1, -1] and r["n"] == 0
    assert list(MR.match(c["d1"], c["d2"], c["nnr"], False, dt=np.float64)["matches_12"]) == [1, 3]
    # at 0.9f no pair of distances tells the two apart
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    keep = d0 <= d1
    assert np.array_equal(MR.ratio_ok(d0[keep], d1[keep], 0.9), MR.ratio_ok(d0[keep], d1[keep], 0.9, np.float64))
    assert not np.array_equal(MR.ratio_ok(d0[keep], d1[keep], 0.6), MR.ratio_ok(d0[keep], d1[keep], 0.6, np.float64))


def test_tie_rule_lower_index_wins():
    c, r = MR.runs("tie_rule")
    D = MR.distances(c["d1"], c["d2"])
    seen = 0
    for i1 in range(len(D)):
        d0 = D[i1].min()
        first = np.flatnonzero(D[i1] == d0)
        if len(first) >= 2 and d0 > 0:
            assert r["matches_12"][i1] == first[0] and r["nn3"][i1, 0] == first[0] and r["nn3"][i1, 1] == r["nn3"][i1, 2] == d0
            seen += 1
    assert seen >= 10
    c, r = MR.runs("all_equal")
    assert (r["matches_12"] == -1).all() and (r["nn3"] == [0, 0, 0]).all()


@pytest.fixture(scope="module")
def hostcheck():
    return MR.build_hostcheck(os.path.join(ROOT, "tools", "_build_match_hostcheck"), sanitize=True)


def _same(got, ref, what, nn3=True):
    assert np.array_equal(got["matches_12"], ref["matches_12"]) and got["n"] == ref["n"], what
    if nn3:
        assert np.array_equal(got["nn3"], ref["nn3"]), what


def _by_options(names):
    groups = {}
    for n in names:
        c = MR.runs(n)[0]
        groups.setdefault((float(c["nnr"]), int(c["best_lr"])), []).append(n)
    return groups


def test_host_check_equals_the_reference(hostcheck, tmp_path):
    """the shared header in the kernels' tile order, under the sanitizers: matches_12, the counts and nn3 of every case, alone"""
    for (nnr, lr), names in _by_options(NAMES).items():
        for n in names:
            got = MR.host_match(hostcheck, str(tmp_path), [MR.runs(n)[0]], 0, nnr, lr)[0]
            _same(got, MR.runs(n)[1], n)


def test_host_check_batch_is_the_problems_alone(hostcheck, tmp_path):
    names = [n for n in NAMES if n.startswith("size_")] + ["all_equal"]
    got = MR.host_match(hostcheck, str(tmp_path), [MR.runs(n)[0] for n in names], 0)
    for n, g in zip(names, got):
        _same(g, MR.runs(n)[1], n)
    # one ratio per problem
    names = ["size_65_63", "size_129_129", "size_3_65", "size_64_64"]
    nnr_b = [0.9, 0.7, 1.3, 0.8]
    got = MR.host_match(hostcheck, str(tmp_path), [MR.runs(n)[0] for n in names], 0, nnr_b=nnr_b)
    for n, r, g in zip(names, nnr_b, got):
        c = MR.runs(n)[0]
        _same(g, MR.match(c["d1"], c["d2"], r, True), (n, r))


def test_drop_in_equals_the_host_check(hostcheck, tmp_path):
    """plba_g2o::match of include/plba_g2o/match.h"""
    for (nnr, lr), names in _by_options(NAMES).items():
        cases = [MR.runs(n)[0] for n in names]
        a = MR.host_match(hostcheck, str(tmp_path), cases, 0, nnr, lr)
        b = MR.host_match(hostcheck, str(tmp_path), cases, 1, nnr, lr)
        for n, x, y in zip(names, a, b):
            _same(y, x, n, nn3=False)
            _same(y, MR.runs(n)[1], n, nn3=False)


@pytest.mark.parametrize("opts", [{}, dict(use_lines=0), dict(use_points=0), dict(best_lr=0, nnr_pt=0.8)], ids=["default", "no_lines", "no_points", "one_way"])
def test_is_loop_closure_equals_the_reference(hostcheck, tmp_path, opts):
    """plba_g2o::is_loop_closure: the gate, the counts and the index lists exactly as the reference's; the pose bit for bit that of
    include/plba_g2o/relative_pose.h (the relative-pose host check with one lane) on the pairs the REFERENCE gathers"""
    names = sorted(MR.LOOP)
    cands = [MR.loop_runs(n, **opts) for n in names]
    got = MR.host_loop(hostcheck, str(tmp_path), [c[0] for c in cands], [c[1] for c in cands], **opts)
    rp_exe = RC.build_hostcheck(os.path.join(ROOT, "tools", "_build_relpose_hostcheck"), sanitize=True)
    passed = [(n, c[2]) for n, c in zip(names, cands) if c[2]["ratio_ok"]]
    assert len(passed) >= (4 if not opts else 1)
    poses = RC.host_run(rp_exe, str(tmp_path), [dict(P3=r["P3"], uv=r["uv"], pq=r["pq"], l3=r["l3"], cam=RC.CAM) for _, r in passed], {}, 1) if passed else []
    poses = dict(zip([n for n, _ in passed], poses))
    for n, (kf0, kf1, ref), g in zip(names, cands, got):
        for k in ("common_pt", "common_ls", "ratio_ok"):
            assert g[k] == ref[k], (n, k)
        for k in ("inl_ratio_pt", "inl_ratio_ls"):
            assert np.array_equal(g[k], ref[k], equal_nan=True), (n, k)
        assert np.array_equal(g["pt_match"], ref["pt_match"]) and np.array_equal(g["ln_match"], ref["ln_match"]), n
        if not ref["ratio_ok"]:
            assert g["returned"] == 0 and not g["pose_out"].any() and not g["pt_kept"].any() and not g["ln_kept"].any(), n
            continue
        p = poses[n]
        assert np.array_equal(g["pose_inc"], p["pose_inc"]) and np.array_equal(g["T"], p["T"]) and g["e"] == p["e"] and g["returned"] == p["returned"], n
        assert np.array_equal(g["pose_out"], p["pose_out"]), n
        if p["returned"]:      # the compacted index lists: the matched rows whose pair survived the cut
            assert np.array_equal(np.flatnonzero(g["pt_kept"]), ref["ip"][p["pt_in"]]) and np.array_equal(np.flatnonzero(g["ln_kept"]), ref["il"][p["ln_in"]]), n


def test_loop_candidates_by_the_reference_alone():
    """what each candidate is for (match_ref.LOOP), and that a `pass` candidate's gathered pairs are its relative-pose case, whose reference
    runs tests/test_relpose_cpu.py holds"""
    for n, (rc_name, _, want) in MR.LOOP.items():
        kf0, kf1, ref = MR.loop_runs(n)
        assert want(ref, RC.runs(rc_name)[0]), n
    assert MR.loop_runs("no_lines_65", use_lines=0)[2]["ratio_ok"] == 1
    assert MR.inlier_ratio(3, 10, 10) == 30.0 and np.isnan(MR.inlier_ratio(0, 0, 5)) and MR.inlier_ratio(0, 5, 0) == 0.0


def test_abi_surface(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct sizes as a C compiler lays out include/plba.h, and the defaults of the reference's configuration"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    names = ("match_default_options", "match_descriptors", "loop_default_options", "verify_loop_candidates")
    for n in names:
        assert hasattr(lib, "plba_" + n), n
    assert set(names) <= set(abi.SIGNATURES) and set(names) <= abi.PRODUCT_ONLY
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(plba_match_options), '
                   'sizeof(plba_loop_options), sizeof(plba_loop_result), offsetof(plba_loop_options, relpose), offsetof(plba_loop_result, relpose)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sm, so, sr, off_o, off_r = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert (sm, so, sr) == (C.sizeof(abi.MatchOptions), C.sizeof(abi.LoopOptions), C.sizeof(abi.LoopResult))
    assert off_o == abi.LoopOptions.relpose.offset and off_r == abi.LoopResult.relpose.offset
    o = abi.LoopOptions()
    f = lib.plba_loop_default_options
    f.restype = None; f.argtypes = [C.POINTER(abi.LoopOptions)]
    f(C.byref(o))
    assert (o.match_pt.nnr, o.match_pt.best_lr, o.match_ln.nnr, o.match_ln.best_lr) == (np.float32(0.9), 1, np.float32(0.9), 1)
    assert (o.use_points, o.use_lines, o.lc_inlier_ratio, o.relpose.max_iters, o.relpose.chi2_th) == (1, 1, 30.0, 5, 7.815)
    assert hasattr(abi.Problem, "match_descriptors") and hasattr(abi.Problem, "verify_loop_candidates")


def test_calls_fail_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        # with a device the refusal is the library's: a null handle is an error, not a fallback
        lib = pkg.hip_lib()
        o = pkg.abi.MatchOptions()
        lib.fn["match_default_options"](C.byref(o))
        assert lib.fn["match_descriptors"](None, C.byref(o), 1, None, None, None, None, None, None, None, None) != 0
        return
    with pytest.raises(pkg.abi.PlbaError, match="no HIP device|no CPU fallback"):
        pkg.new_problem().match_descriptors([np.zeros((2, 32), np.uint8)], [np.zeros((2, 32), np.uint8)])
