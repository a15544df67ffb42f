"""The marginalization step of csrc/plba_marg.hip — k_marg_factors (the point, line and IMU rows, the copied rows of an old prior, the
column layout, the factor selection), A = J^T J, the block-wise and the dense pseudo-inverse Schur elimination, marg_kept_block's three
eigen-solvers, J0 / r0 / x0 — against a reference built without the device: the quad-precision oracle's stacked factors taken through
the step at 50 digits.  tests/marg_quad.py is the rule, tests/marg_quad_cases.py the windows; the references are the fixtures
tests/golden/marg_quad_<case>.npz (tests/golden/make_marg_quad.py; tests/test_marg_quad_cpu.py holds them to their conditions without a
GPU).  Only the fixtures, the package and numpy are used here; every test is one upload and one marginalization.

Measured on the MI355X (DESIGN.md 6d has every figure): the rows of J and r, the layout, the factor selection, x0 and r0^T r0 pass the
rule on every window and option set (worst error / tolerance 0.84, a line residual), and so does everything on m15 and noimu.  The first
run found the certificate of marg_exact = 1 taking the block-wise form on `once` (landmarks seen once), where A' then missed even the
1e-10 max norm in use (1.35e-9; the dense path: 3.4e-13): the certificate now also asks that every kept landmark eigenvalue be resolved
by its formed block (finding 1), which sends `once` and `lines_only` down the dense path.  Open: A' misses the rule on 16
of the 18 windows where it is compared (error / tolerance 1.1 .. 3.8e4), J0^T J0 on 15 (4 .. 1.2e6), J0^T r0 on 12 (1.8 .. 3.4e5), b' on
6 (1.2 .. 410), and the row count of J0 is off by 1 to 3 on points_only, lines_only and cap3: the device, like the reference and the
fp64 oracle, forms A = J^T J and diagonalises the formed blocks, so in the diagonal-scaled norm a weak row (velocity, bias) carries
u |A| of the strong ones.  Those quantities keep the max-norm assertion they had, which holds on every window
(tests/marg_quad_known.py lists each with the measured excess; DESIGN.md 6d lists them as open)."""
import os

import numpy as np
import pytest

from . import marg_quad as MQ
from . import marg_quad_cases as MC
from .marg_quad_known import KNOWN, PATH_KNOWN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DUMP, NO_PREROTATE = 2, 8      # PLBA_DIAG_MARG_DUMP, PLBA_DIAG_NO_MARG_PREROTATE
NEAR = ("far1", "k12full")
KEPT_BLOCK_PATHS = ("full11", "k12full", "full15", "full16")      # n = 96, 105, 132, 141: marg_kept_block's paths
_CACHE = {}


def _case(pkg, name):
    if name not in _CACHE:
        fx, ref = MQ.load(name, GOLDEN)
        w = MC.CASES[name]["make"](pkg.window, ref.prior)
        assert MC.window_sha(w) == str(fx["sha_window"]), "the window generator gives another window here than where the fixture was made"
        _CACHE[name] = (ref, w)
    return _CACHE[name]


def _path_ok(name, ref, path):
    """marg_path[0]: 1 (dense) where the block-wise form is not the reference's (MC.DENSE) or a landmark block's formed J_b^T J_b does not
    resolve a kept eigenvalue (marg_quad.unresolved_blocks, from the reference's J: `once`, `lines_only`), otherwise 0.  Open (PATH_KNOWN,
    DESIGN.md 6d): on `noimu` the certificate declines the block-wise form although it would pass the rule there — the dense path does."""
    want = 1 if name in MC.DENSE or MQ.unresolved_blocks(ref) else 0
    if int(path[0]) != want and PATH_KNOWN.get(name) == int(path[0]):
        print("%s marg_path %s: KNOWN EXCESS, %d expected" % (name, list(path), want))
        return True
    return int(path[0]) == want


@pytest.mark.parametrize("name", list(MC.CASES))
def test_marginalize_default_options(pkg, hip, name):
    """plba_marginalize with the dump: every quantity of the rule, J and r included, and the path the certificate chose"""
    ref, w = _case(pkg, name)
    res = MQ.run(pkg.new_problem, w, MC.CASES[name], diag=DUMP)
    assert _path_ok(name, ref, res["path"]), list(res["path"])
    assert name not in MC.N_EXPECT or res["n"] == MC.N_EXPECT[name]
    fig = MQ.hold(res, ref, "marginalize", name, known=KNOWN.get((name, "marginalize")))
    assert "J_pvr" in fig or name == "noimu"


@pytest.mark.parametrize("name", list(MC.CASES))
def test_marginalize_to_prior_default_options(pkg, hip, name):
    """plba_marginalize_to_prior + plba_get_prior without the dump (which would force a read-back): the prior that stays on the device"""
    ref, w = _case(pkg, name)
    res = MQ.run(pkg.new_problem, w, MC.CASES[name], to_prior=True)
    assert _path_ok(name, ref, res["path"]), list(res["path"])
    fig = MQ.hold(res, ref, "to_prior", name, known=KNOWN.get((name, "to_prior")))
    assert "J0tJ0" in fig or not ref.decided_r or ref.yard("J0tJ0") is None


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", MC.FAR + NEAR)
def test_forced_paths(pkg, hip, name, mode):
    """marg_exact = 2 (always dense) is held to the rule everywhere; marg_exact = 0 (always block-wise) where every discarded direction is
    a block-local null space (the near windows) — on the far-landmark windows it is asserted to miss it, as
    tests/test_gpu_parity.py::test_marginalization_forced_paths does"""
    ref, w = _case(pkg, name)
    res = MQ.run(pkg.new_problem, w, MC.CASES[name], marg_exact=mode, diag=DUMP)
    assert int(res["path"][0]) == (1 if mode == 2 else 0)
    if mode == 0 and name in MC.FAR:
        err = MQ.errors(res, ref, exact=False)
        print("marg_exact=0 %s Ar error %.3e tolerance %.3e" % (name, err["Ar"], ref.tol("Ar")))
        assert not err["Ar"] <= ref.tol("Ar"), (name, err["Ar"], ref.tol("Ar"))
    else:
        MQ.hold(res, ref, "marg_exact=%d" % mode, name, known=KNOWN.get((name, "marg_exact=%d" % mode)))


@pytest.mark.parametrize("name", KEPT_BLOCK_PATHS)
def test_kept_block_paths_without_prerotation(pkg, hip, name):
    """PLBA_DIAG_NO_MARG_PREROTATE: the eigen-solver of the kept block from a cold start, one window per path of marg_kept_block"""
    ref, w = _case(pkg, name)
    res = MQ.run(pkg.new_problem, w, MC.CASES[name], diag=DUMP | NO_PREROTATE)
    assert res["n"] == MC.N_EXPECT[name]
    MQ.hold(res, ref, "no_prerotate", name, known=KNOWN.get((name, "no_prerotate")))
