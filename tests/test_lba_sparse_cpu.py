"""CPU-side checks of the sparse reduced-camera solve of plba_lba_visual (plba_lba_options.solver = 1): the option and its default, the host
side's block list (csrc/plba_lba_sparse.h) under the host sanitizers against a brute-force enumeration, the sparse numpy reference the GPU
tests hold the large window with (tests/lba_sparse_ref.py) against lba_ref.run where both run, and the decision margins of every window
tests/test_lba_sparse.py uses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import lba_ref as LR
from . import lba_sparse_cases as SC
from . import lba_sparse_ref as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_lba_sparse_hostcheck.cpp")
WINDOWS = ("band12", "band17", "band40", "revisit40", "full20", "components", "lonely", "duplicate", "unobserved", "all_fixed", "no_landmark")


def test_the_option_exists_and_the_default_is_dense(pkg, hip_lib_path):
    assert pkg.abi.LbaOptions._fields_[-1][0] == "solver"                 # appended: the older fields keep their offsets
    assert pkg.abi.Options._fields_[-1][0] == "pgo_solver"                # plba_options is as it was
    lib = C.CDLL(hip_lib_path)
    o = pkg.abi.LbaOptions()
    o.solver = 7
    lib.plba_lba_default_options(C.byref(o))
    assert o.solver == 0


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """csrc/plba_lba_sparse_hostcheck.cpp, a stand-alone program, built with the host sanitizers and run directly"""
    exe = os.path.join(str(tmp_path_factory.mktemp("lba_sparse_hostcheck")), "plba_lba_sparse_hostcheck_san")
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOSTCHECK_SRC, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_the_host_program_runs_clean_under_the_sanitizers(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr == "", report.stderr      # a sanitizer report goes to stderr


@pytest.mark.parametrize("window", WINDOWS)
def test_block_list_equals_the_brute_force_enumeration(report, window):
    assert "ok %s" % window in report.stdout.splitlines(), report.stdout + report.stderr


def test_the_host_header_is_standard_library_only():
    incs = [line.split()[1] for line in open(os.path.join(CSRC, "plba_lba_sparse.h")).read().splitlines() if line.startswith("#include")]
    assert incs and all(i.startswith("<") for i in incs), incs


@pytest.mark.parametrize("run", SC.RUNS[::3], ids=SC.run_id)
def test_sparse_reference_agrees_with_the_dense_one(run):
    """lba_sparse_ref.run against lba_ref.run(form="elim"), both types: the decisions exactly, the outputs within the project's bars"""
    w, r64, rw = SC.run_reference(run)
    for dt, r in ((np.float64, r64), (LR.wide(), rw)):
        s = LS.run(w, dt, **run[2])
        assert s["omega"] <= LR.SR.RESIDUAL_MAX, s["omega"]
        for k in ("iterations", "updates", "solver_failed"):
            assert s[k] == r[k], (k, s[k], r[k])
        assert np.array_equal(s["pt_moved"], r["pt_moved"]) and np.array_equal(s["ln_moved"], r["ln_moved"])
        eT, ex, eq = np.abs(s["T"] - r["T"]).max(), np.abs(s["xyz"] - r["xyz"]).max(), np.abs(s["pq"] - r["pq"]).max(initial=0.0)
        print("%s: T %.2e xyz %.2e pq %.2e" % (SC.run_id(run), eT, ex, eq))
        assert eT <= LR.LIMITS["T"] and ex <= LR.LIMITS["xyz"] and eq <= LR.LIMITS["pq"]
        assert abs(s["lam"] - r["lam"]) <= LR.LIMITS["lam_rel"] * abs(r["lam"])
        assert abs(s["err_first"] - r["err_first"]) <= LR.LIMITS["err_first_rel"] * abs(r["err_first"])


@pytest.mark.parametrize("run", SC.RUNS, ids=SC.run_id)
def test_decisions_have_margin_on_the_tree_shapes(run):
    _, r64, rw = SC.run_reference(run)
    assert (r64["solver_failed"], rw["solver_failed"]) == (0, 0)
    assert LR.decisions_have_margin(r64, rw, run[2]) >= LR.MARGIN


@pytest.mark.parametrize("n", SC.ENTRIES_N)
def test_decisions_have_margin_on_the_entry_count_windows(n):
    w, r64, rw = SC.entries_reference(n)
    loc = w["kf_loc"][w["po_kf"]]
    both = np.bincount(w["po_pt"][loc == 0], minlength=len(w["xyz"])) * np.bincount(w["po_pt"][loc == 2], minlength=len(w["xyz"]))
    assert both.sum() == n      # the block of the local keyframes (0, 2) has exactly n pair entries
    assert LR.decisions_have_margin(r64, rw) >= LR.MARGIN


def test_decisions_have_margin_on_the_scale_window(pkg):
    """the 1 000-keyframe window of the GPU test, two passes of lba_sparse_ref in both types"""
    w, r64, rw = SC.scale_reference(pkg)
    assert (w["kf_loc"] >= 0).sum() == SC.SCALE_N and 9e4 <= len(w["po_pt"]) + len(w["lo_ln"]) <= 1.1e5
    assert max(r64["omega"], rw["omega"]) <= LR.SR.RESIDUAL_MAX
    assert LR.decisions_have_margin(r64, rw, SC.SCALE_OPTS) >= LR.MARGIN
    tol, noise = LR.tolerances(r64, rw)
    print("scale window noise:", noise)
    for k, lim in (("T", LR.LIMITS["T"]), ("xyz", LR.LIMITS["xyz"]), ("pq", LR.LIMITS["pq"])):
        assert LR.FACTOR * noise[k] < lim, (k, noise[k])      # the reference's own fp64 evaluation is well inside the bars
