"""The two HIP-free contracts of the host side without a GPU: csrc/plba_dense_work.h (the dense solver's padding rule, the element counts of
its workspace, when the explicit inverse is kept) and the mailbox overlay of csrc/plba_mailbox.h.  csrc/plba_dense_work_hostcheck.cpp, a
stand-alone program with its own main, is built with the host compiler under the address and undefined-behaviour sanitizers and run
directly.  Everything it checks is exact: the counts are the ones the call sites computed by hand before the header existed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_dense_work_hostcheck.cpp")
GROUPS = ("ppad", "counts", "overlay")


def build_hostcheck(out_dir):
    """csrc/plba_dense_work_hostcheck.cpp with the host sanitizers; returns its path"""
    exe = os.path.join(out_dir, "plba_dense_work_hostcheck_san")
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOSTCHECK_SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = build_hostcheck(str(tmp_path_factory.mktemp("dense_work_hostcheck")))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r


def test_the_host_program_runs_clean_under_the_sanitizers(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr == "", report.stderr      # a sanitizer report goes to stderr


@pytest.mark.parametrize("group", GROUPS)
def test_group(report, group):
    assert "ok %s" % group in report.stdout.splitlines(), report.stdout + report.stderr


def _includes(name):
    txt = open(os.path.join(CSRC, name)).read()
    return [line.split()[1] for line in txt.splitlines() if line.startswith("#include")]


def test_the_header_has_no_hip_dependency():
    incs = _includes("plba_dense_work.h")
    assert incs and all(i.startswith("<c") for i in incs), incs      # the C++ standard library's C headers only


def test_the_mailbox_header_has_no_hip_dependency():
    incs = _includes("plba_mailbox.h")
    assert incs and all(i.startswith("<c") or i == '"plba.h"' for i in incs), incs      # ... and the C ABI, which includes <stddef.h> / <stdint.h>
    assert all(i in ("<stddef.h>", "<stdint.h>") for i in
               [line.split()[1] for line in open(os.path.join(ROOT, "include", "plba.h")).read().splitlines() if line.startswith("#include")])
