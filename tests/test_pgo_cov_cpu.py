"""CPU-side checks of plba_pose_graph_marginals: the ABI surface, the host side (csrc/plba_pgo_cov.h) under the host sanitizers —
places against a brute-force search, the long double walk of the whole computation against a dense inverse —, and the reference of
tests/pgo_cov_ref.py under its own rule on every graph tests/test_pgo_cov.py uses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import marginals_exact as MX
from . import pgo_cov_ref as PC
from . import pgo_ref
from . import solver_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_pgo_cov_hostcheck.cpp")
GRAPHS = ("chain1", "chain2", "chain16", "chain17", "chain40", "star", "fixed_hub", "two_components", "clique3", "clique4", "clique6", "clique9", "band300")


def test_abi_surface(pkg, tmp_path):
    """the symbol, the struct as a C compiler lays out include/plba.h, the diag bit, and plba_options as it was"""
    abi = pkg.abi
    assert "pose_graph_marginals" in abi.SIGNATURES and "pose_graph_marginals" in abi.PRODUCT_ONLY
    assert abi.Options._fields_[-1][0] == "pgo_solver"                # plba_options gains no field
    assert hasattr(pkg.abi.Problem, "pgo_marginals")
    src = tmp_path / "layout.c"
    fields = ("want", "n_pairs", "pairs", "v_cov", "v_status", "pair_cov", "pair_status", "n_status")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %d", sizeof(plba_pgo_marginals), sizeof(plba_options), PLBA_DIAG_PGO_COV_DUMP);\n'
                   + "".join('printf(" %%zu", offsetof(plba_pgo_marginals, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("gcc") or shutil.which("cc") or "/opt/rocm/lib/llvm/bin/clang", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(abi.PgoMarginals) and out[1] == C.sizeof(abi.Options) and out[2] == 32
    assert out[3:] == [getattr(abi.PgoMarginals, f).offset for f in fields]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plba.h")).read(), flags=re.S)
    assert re.search(r"int\s+plba_pose_graph_marginals\s*\(\s*plba_problem\*\s*p,\s*const\s+plba_pose_graph\*\s*g,\s*plba_pgo_marginals\*\s*m\s*\)", hdr)


def test_the_library_exports_the_entry(hip_lib_path):
    assert hasattr(C.CDLL(hip_lib_path), "plba_pose_graph_marginals")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """csrc/plba_pgo_cov_hostcheck.cpp, a stand-alone program, built with the host sanitizers and run directly"""
    exe = os.path.join(str(tmp_path_factory.mktemp("pgo_cov_hostcheck")), "plba_pgo_cov_hostcheck_san")
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, HOSTCHECK_SRC, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_the_host_program_runs_clean_under_the_sanitizers(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr == "", report.stderr      # a sanitizer report goes to stderr


@pytest.mark.parametrize("graph", GRAPHS)
def test_places_and_the_long_double_walk(report, graph):
    assert "ok %s" % graph in report.stdout.splitlines(), report.stdout + report.stderr


def test_the_host_header_is_standard_library_only():
    for header in ("plba_pgo_cov.h", "plba_pgo_sparse.h"):
        incs = [line.split()[1] for line in open(os.path.join(CSRC, header)).read().splitlines() if line.startswith("#include")]
        assert incs and all(i.startswith("<") for i in incs), (header, incs)


# ---- the reference under its own rule, and the bound of every graph the GPU tests use ----------------------------------------------------
_H = {}


def _dense(name):
    if name not in _H:
        g = PC.graph(name)
        H = PC.dense_H(g)
        _H[name] = (g, H, R.kappa_s(H))
    return _H[name]


@pytest.mark.parametrize("name", PC.SMALL + ["cov300"])
def test_every_gpu_graph_is_well_inside_the_rule(name):
    """32 n u kappa_s <= 1e-6: the hard bar of tests/test_pgo_cov.py says something on each of them"""
    g, H, ks = _dense(name)
    b = PC.bound(H.shape[0], ks)
    print("%s: n %d kappa_s %.3e bound %.3e" % (name, H.shape[0], ks, b))
    assert b <= 1e-6


@pytest.mark.parametrize("name", ["cov20", "cov40", "cov300", "star", "fixed_hub", "two_components", "one_free", "complete80"])
def test_the_cpu_inverses_stay_inside_the_rule(name):
    """the three fp64 inverses of marginals_exact.cpu_inverses against the extended-precision columns, in the E_sel measure, on the
    entries a call reports (every vertex block and every edge block; the 300-keyframe graph on 4 sampled vertices' columns)"""
    g, H, ks = _dense(name)
    fr, free = PC.free_ranks(g)
    n = len(free)
    cols = list(range(n)) if n <= 80 else [0, n // 3, n // 2, n - 1]
    ext = PC.exact_columns(H, cols)
    a, b = fr[g["ei"]], fr[g["ej"]]
    both = (a >= 0) & (b >= 0)
    sel = [(i, i) for i in cols] + [(int(x), int(y)) for x, y in zip(a[both], b[both]) if y in cols] + [(int(y), int(x)) for x, y in zip(a[both], b[both]) if x in cols]
    each = PC.e_cpu(H, sel, ext)
    print("%s: E_cpu %s bound %.3e" % (name, ["%.2e" % e for e in each], PC.bound(H.shape[0], ks)))
    assert max(each) <= PC.bound(H.shape[0], ks)


def test_kappa_by_eigsh_agrees_with_the_dense_one():
    g, H, ks = _dense("cov300")
    ke = PC.kappa_s_sparse(PC.sparse_H(g))
    assert np.array_equal(PC.sparse_H(g).toarray(), H)
    assert abs(ke - ks) <= 0.01 * ks, (ke, ks)


def test_status_rules():
    g = PC.graph("two_components")
    pairs, fill = PC.request("two_components", g)
    vs, ps, ns = PC.statuses(g, pairs, fill)
    assert set(np.flatnonzero(vs == 1)) == {0, 30} and set(np.flatnonzero(vs == 2)) == set(range(25, 30)) | set(range(56, 60))
    ne = len(g["ei"])
    assert np.all(ps[:2 * ne][(vs[pairs[:2 * ne, 0]] == 0) & (vs[pairs[:2 * ne, 1]] == 0)] == 0)
    assert ps[-1] == 2 and ps[-2] == 2 and ps[-3] == 1 and ps[-4] == 1 and ns.tolist() == [(vs == 0).sum(), 2, 9, 0]
    g = PC.graph("chain17")
    pairs, fill = PC.request("chain17", g)
    assert PC.statuses(g, pairs, fill)[1][-2:].tolist() == [3, 3] and PC.statuses(g, pairs, fill)[2][3] == 2
    g = PC.graph("chain16")
    pairs, fill = PC.request("chain16", g)
    assert PC.statuses(g, pairs, fill)[1][-2:].tolist() == [0, 0]
