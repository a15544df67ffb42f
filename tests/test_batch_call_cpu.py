"""The HIP-free part of the batched calls' scaffold (csrc/plba_batch_conv.h: the block layout, the CSR start check, the pose / 6 x 6 / mask
conversions) without a GPU: csrc/plba_batch_call_hostcheck.cpp, a stand-alone program with its own main, built with the host compiler
under the address and undefined-behaviour sanitizers and run directly.  Everything it checks is exact: offsets, refusals, bit patterns."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_batch_call_hostcheck.cpp")
GROUPS = ("layout", "starts", "poses", "sym6", "masks")


def build_hostcheck(out_dir):
    """csrc/plba_batch_call_hostcheck.cpp with the host sanitizers; returns its path"""
    exe = os.path.join(out_dir, "plba_batch_call_hostcheck_san")
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOSTCHECK_SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = build_hostcheck(str(tmp_path_factory.mktemp("batch_call_hostcheck")))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r


def test_the_host_program_runs_clean_under_the_sanitizers(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr == "", report.stderr      # a sanitizer report goes to stderr


@pytest.mark.parametrize("group", GROUPS)
def test_group(report, group):
    assert "ok %s" % group in report.stdout.splitlines(), report.stdout + report.stderr


def test_the_header_has_no_hip_dependency():
    txt = open(os.path.join(CSRC, "plba_batch_conv.h")).read()
    incs = [line.split()[1] for line in txt.splitlines() if line.startswith("#include")]
    assert incs and all(i.startswith("<c") for i in incs), incs      # the C++ standard library's C headers only
