"""plba_track_inertial without a GPU: the numpy reference (tests/vitrack_ref.py) against itself in a wide type and against numeric
derivatives through IncSmall; the information it hands to the next frame against the Schur complement it came from; the device's
arithmetic compiled for the host (csrc/plba_vitrack_hostcheck.cpp: 64 emulated lanes in the kernel's reduction order, and one lane =
include/plba_g2o/track_inertial.h) under the tolerance rule the GPU tests use; the same graph built from the g2o facade's classes and run
through SparseOptimizer::optimizeHost (tools/vitrack_facade_harness.cpp); the ABI surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import lba_ref as LR
from . import vitrack_cases as VC
from . import vitrack_ref as VR

ROOT = VC.ROOT
NAMES = sorted(VC.CASES) + ["chain_2"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_has_margin_and_float64_agrees_with_wide(name):
    """every case, by the reference alone: each decision of the wide run (a trial's accept / reject, every gate comparison, every depth
    sign, every Cholesky pivot's sign) lies 1000 x the noise of the compared quantity away from its threshold, the float64 run made the
    same decisions, and masks, counts, iterations, trials, stop reasons and status agree.  (vitrack_cases.SKIP: the pivots of the
    `singular` case's S, which is zero but for rounding in every precision, have no margin to ask for; its verdict is still compared.)"""
    case, r64, rw = VC.runs(name)
    VR.hold(r64, r64, rw, "float64", name, skip=VC.SKIP.get(name, ()))


@pytest.mark.parametrize("name", NAMES)
def test_reference_noise_sample_is_representative(name):
    """every case, by the reference alone: it serves its purpose (vitrack_cases.EXPECT), and the float64 reference with its features in 12
    other orders stays within HALF the rule's tolerance of the wide run with every discrete output unchanged"""
    case, r64, rw = VC.runs(name)
    assert VC.EXPECT["chain_1" if name == "chain_2" else name](rw), name
    worst = VC.reference_is_stable(case, r64, rw)
    print("%s: reordered float64 reference, largest error / tolerance %.3f" % (name, worst))
    assert worst <= 0.5, (name, worst)


def test_cases_cover_both_anchors_a_rejection_a_readmission_and_singular():
    runs = {n: VC.runs(n) for n in NAMES}
    assert {int(c["anchor_free"]) for c, _, _ in runs.values()} == {0, 1}
    assert runs["reject"][2]["events"]["rejected"] >= 1 and runs["reject"][2]["events"]["accepted"] >= 1
    for n in ("gate", "gate_free"):
        assert runs[n][2]["events"]["dropped"] >= 1 and runs[n][2]["events"]["readmitted"] >= 1
    assert runs["singular"][2]["status"] == VR.SINGULAR and {r["status"] for n, (_, _, r) in runs.items() if n != "singular"} == {VR.OK}
    assert any(l == "depth" and not t for l, _, _, t, _ in runs["depth"][2]["checks"])
    assert runs["chain_2"][0]["pinfo"].any() and np.array_equal(runs["chain_2"][0]["pst"], runs["chain_1"][1]["state_j"])
    sizes = {(len(c["Pw"]), len(c["pq"])) for n, (c, _, _) in runs.items() if n.startswith("fixed_")}
    assert sizes == set(VC.SIZES)


# ---- the Jacobians against central differences through IncSmall (step and tolerance of tests/test_track_cpu.py) ----------------------------
def _numeric(fn, n=15, h=1e-6):
    cols = []
    for k in range(n):
        e = np.zeros(n); e[k] = h
        cols.append((np.asarray(fn(e), np.float64) - np.asarray(fn(-e), np.float64)) / (2 * h))
    return np.stack(cols, -1)


def _close(J, fd):
    return np.allclose(J, fd, rtol=0, atol=1e-7 * np.abs(fd).max())


def _visual_case():
    c = VC.frame(3, 6, 6)
    a = lambda k, s: np.asarray(c[k], np.float64).reshape(s)
    return c, [float(v) for v in c["cam"]], a("Rbc", (3, 3)).T, a("Pbc", (3,))


@pytest.mark.parametrize("kind", ["point", "line"])
def test_visual_jacobians_are_the_derivatives_under_incsmall(kind):
    """both rows of a point edge and of a line edge with respect to (dP, dPhi) of j, and zero with respect to dV and the biases.  For
    the line edge this pins the position block to the true derivative (fix_line_position_jacobian = 1): the world-frame block of the
    BA's edge (SURVEY B-Q1) is asserted NOT to pass"""
    c, cam, Rcb, Pbc = _visual_case()
    sj = np.asarray(c["sj"], np.float64)
    for i in range(6):
        if kind == "point":
            X, z = c["Pw"][i:i + 1], c["uv"][i:i + 1]
            res = lambda d: VR.point_edges(VR.oplus(sj, d, np.float64), X, z, cam, Rcb, Pbc, False)[0][0]
            J = VR.point_edges(sj, X, z, cam, Rcb, Pbc, True)[2][0]
        else:
            X, z = c["pq"][i:i + 1], c["l3"][i:i + 1]
            res = lambda d: VR.line_edges(VR.oplus(sj, d, np.float64), X, z, cam, Rcb, Pbc, False)[0][0]
            J = VR.line_edges(sj, X, z, cam, Rcb, Pbc, True)[2][0]
        fd = _numeric(res)
        assert _close(J, fd[:, VR.VIS_COLS]), (kind, i, J, fd)
        assert not fd[:, [3, 4, 5, 9, 10, 11, 12, 13, 14]].any()
        if kind == "line":      # B-Q1's block: -l12^T Jpi M with M = Rcb Rwb^T, the derivative with respect to a WORLD-frame step
            wrong = J.copy(); wrong[:, :3] = J[:, :3] @ VR.q2R(sj[6:10]).T
            assert not _close(wrong, fd[:, VR.VIS_COLS])


def test_imu_edge_jacobians_with_respect_to_both_states():
    c = VC.frame(5, 0, 0, free=True, start=3.0)
    a = lambda k, s: np.asarray(c[k], np.float64).reshape(s)
    si, sj, pre, gw = a("si", (22,)), a("sj", (22,)), a("pre", (142,)), a("gw", (3,))
    e = VR.imu_error(si, sj, pre, gw, np.float64)
    Ji, Jj = VR.imu_jacobians(si, sj, pre, gw, e, np.float64)
    fi = _numeric(lambda d: VR.imu_error(VR.oplus(si, d, np.float64), sj, pre, gw, np.float64))
    fj = _numeric(lambda d: VR.imu_error(si, VR.oplus(sj, d, np.float64), pre, gw, np.float64))
    assert np.abs(e[6:9]).max() > 1e-3      # the rotation residual is not small: JrInv is not the identity
    assert _close(Ji, fi) and _close(Jj, fj), (np.abs(Ji - fi).max(), np.abs(Jj - fj).max())


def test_prior_jacobian():
    c = VC.frame(5, 0, 0, free=True, start=3.0)
    si, pst = np.asarray(c["si"], np.float64), np.asarray(c["pst"], np.float64)
    e = VR.prior_error(pst, si)
    fd = _numeric(lambda d: VR.prior_error(pst, VR.oplus(si, d, np.float64)))
    assert np.abs(e[6:9]).max() > 1e-3 and _close(VR.prior_jacobian(si, e, np.float64), fd)


@pytest.mark.parametrize("name", ["fixed_70_30", "free_70_30", "free_300_100", "gate_free", "chain_2"])
def test_next_prior_reproduces_the_schur_complement(name):
    """in the wide type: an EdgeNavStatePrior at state_j with the information handed on has J^T Omega J = S.  Omega = J^-T S J^-1 and the
    product back are four products of 15 terms with the entries of J and of J^-1 at most 1 in size and their absolute row sums at most
    sqrt(3), plus the cofactor inverse of R (a dozen operations): 4 x 15 x 3 + 16 = 196 roundings of size u max|S| bound every entry"""
    dt = LR.wide()
    case, r64, rw = VC.runs(name)
    with LR._prec(dt):
        S, sj = rw["wide"]["S"], rw["wide"]["sj"]
        D = -LR.cast(np.eye(15), dt)
        D[0:3, 0:3] = -LR._inv3(VR.q2R(sj[6:10]))
        D[6:9, 6:9] = LR.cast(np.eye(3), dt)
        Om = LR._mm(LR._tr(D), LR._mm(S, D))
        J = VR.prior_jacobian(sj, LR._zeros((15,), dt), dt)
        back = LR._mm(LR._tr(J), LR._mm(Om, J))
        u = 2.0 ** -136 if isinstance(dt, str) else float(np.finfo(dt).eps) / 2
        err, bound = float(abs(back - S).max()), 196 * u * float(abs(S).max())
        print("%s: |J^T Omega J - S| %.3e, bound %.3e" % (name, err, bound))
        assert err <= bound
        # and what the call returns is that Omega rounded to double
        assert np.abs(LR.f64(Om) - rw["next_prior"]).max() <= 4 * np.finfo(np.float64).eps * np.abs(rw["next_prior"]).max()


# ---- the device's arithmetic on the host -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostcheck():
    return VC.build_hostcheck(os.path.join(ROOT, "tools", "_build_vitrack_hostcheck"), sanitize=True)


def _host(hostcheck, tmp, name, lanes):
    """the named case through the host program; chain_2 from the program's own frame 1"""
    if name == "chain_2":
        c1 = VC.runs("chain_1")[0]
        case = VC.chain_2(VC.CHAIN_SEED, VC.host_run(hostcheck, tmp, [c1], c1["opts"], lanes)[0])
    else:
        case = VC.runs(name)[0]
    return VC.host_run(hostcheck, tmp, [case], case["opts"], lanes)[0]


@pytest.mark.parametrize("lanes", [64, 1])
@pytest.mark.parametrize("name", NAMES)
def test_host_check_holds_the_rule(hostcheck, tmp_path, name, lanes):
    """the device's arithmetic on the CPU, built with the address and undefined-behaviour sanitizers and run directly: 64 emulated lanes
    in the kernel's reduction order, and one lane, which is include/plba_g2o/track_inertial.h as a caller uses it.  The same rule as the
    GPU tests: 8 x the float64 reference's own noise against the wide run, everything discrete exactly."""
    case, r64, rw = VC.runs(name)
    res = _host(hostcheck, str(tmp_path), name, lanes)
    VR.hold(res, r64, rw, "host%d" % lanes, name, skip=VC.SKIP.get(name, ()))
    assert np.array_equal(res["H"], res["H"].T) and np.array_equal(res["next_prior"], res["next_prior"].T)
    if not case["anchor_free"]:
        assert np.array_equal(res["state_i"], np.asarray(case["si"], np.float64)) and not res["H"][:15].any()
    if name in ("rounds_0", "iters_0"):      # the states bit for bit, H still reported
        assert np.array_equal(res["state_i"], case["si"]) and np.array_equal(res["state_j"], case["sj"]) and res["H"][15:, 15:].any()


BATCH = ["fixed_70_30", "free_70_30", "fixed_0_0", "fixed_65_0", "free_300_100"]


def test_host_check_batch_is_the_problems_alone(hostcheck, tmp_path):
    cases = [VC.runs(n)[0] for n in BATCH]
    batch = VC.host_run(hostcheck, str(tmp_path), cases, VC.OPTS, 64)
    for n, c, b in zip(BATCH, cases, batch):
        alone = VC.host_run(hostcheck, str(tmp_path), [c], VC.OPTS, 64)[0]
        for k in VR.QUANT + VR.EXACT + ("pt_in", "ln_in"):
            assert np.array_equal(np.asarray(alone[k]), np.asarray(b[k]), equal_nan=True), (n, k)


# ---- the same graph from the facade's classes, through optimizeHost ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade(hip_lib_path):
    out_dir = os.path.join(ROOT, "tools", "_build_vitrack_facade")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "vitrack_facade_harness")
    pkgdir = os.path.dirname(hip_lib_path)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pkgdir, "csrc"),
                    os.path.join(ROOT, "tools", "vitrack_facade_harness.cpp"), "-o", exe, "-L", pkgdir, "-lplba_hip", "-Wl,-rpath," + pkgdir], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("singular",)])
def test_facade_graph_through_optimize_host_holds_the_rule(facade, tmp_path, name):
    """VertexNavState, EdgeNavState, EdgeNavStatePrior, EdgeNavStatePointXYZOnlyPose and EdgeNavStateLineOnlyPose in a SparseOptimizer, the
    rounds through optimize() (optimizeHost: its own dense system and LL^T), the kernels and the gate as a call site writes them: states
    and chi2 within the rule's tolerance of the wide run, iterations, trials, failures and masks equal.  (`singular` has nothing for this
    route to compute: it runs no round, and the facade has no marginal.)"""
    case, r64, rw = VC.runs(name)
    tol, noise = VR.tolerances(r64, rw)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")

    def through(c):
        ps, ls = VC.write_batch(fin, [c], c["opts"])
        subprocess.check_call([facade, fin, fout])
        with open(fout, "rb") as f:
            od, oi = np.fromfile(f, np.float64, 46), np.fromfile(f, np.int32, 10)
            pm, lm = np.fromfile(f, np.uint8, int(ps[-1])), np.fromfile(f, np.uint8, int(ls[-1]))
        return od, oi, pm, lm
    if name == "chain_2":      # frame 1 by this route has no marginal to hand on: the float64 chain's frame 2 is the input
        case = VC.runs("chain_2")[0]
    od, oi, pm, lm = through(case)
    got = dict(state_i=od[:22], state_j=od[22:44], chi2_initial=od[44], chi2_final=od[45])
    assert list(oi[:8]) == rw["iterations"] and oi[8] == rw["trials"] and oi[9] == rw["solver_failures"], (oi, rw["iterations"], rw["trials"])
    assert np.array_equal(pm.astype(bool), rw["pt_in"]) and np.array_equal(lm.astype(bool), rw["ln_in"])
    for k, v in got.items():
        e = float(np.abs(np.asarray(v) - np.asarray(rw[k], np.float64)).max())
        print("facade %s %-12s error %.3e  noise %.3e  tolerance %.3e" % (name, k, e, noise[k], tol[k]))
        assert e <= tol[k], (name, k, e, tol[k])


def test_abi_structs(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct sizes and offsets as a C compiler lays out include/plba.h, and the defaults"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    assert hasattr(lib, "plba_track_inertial") and hasattr(lib, "plba_vitrack_default_options")
    src = tmp_path / "sz.c"
    fields = ["H900", "next_prior_info225", "chi2_initial", "iterations", "stop_reason", "trials", "n_inliers_pt", "status"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu", sizeof(plba_vitrack_options), '
                   'sizeof(plba_vitrack_result), offsetof(plba_vitrack_options, tau), offsetof(plba_vitrack_options, chi2_ln));\n' +
                   "".join('printf(" %%zu", offsetof(plba_vitrack_result, %s));\n' % k for k in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert (v[0], v[1]) == (C.sizeof(abi.VitrackOptions), C.sizeof(abi.VitrackResult)) == (72, 9464)
    assert v[2] == abi.VitrackOptions.tau.offset and v[3] == abi.VitrackOptions.chi2_ln.offset
    py = {"H900": "H900", "next_prior_info225": "next_prior_info225"}
    for k, off in zip(fields, v[4:]):
        assert off == getattr(abi.VitrackResult, py.get(k, k)).offset, k
    assert np.dtype(VC.RESULT_DT).itemsize == 9464
    o = abi.VitrackOptions()
    f = lib.plba_vitrack_default_options
    f.restype = None; f.argtypes = [C.POINTER(abi.VitrackOptions)]
    f(C.byref(o))
    assert {k: getattr(o, k) for k in VR.DEFAULTS} == VR.DEFAULTS
    assert o.huber_pt == float(np.float32(np.sqrt(5.991))) and (o.rounds, o.iters, o.max_trials, o.robust_rounds) == (4, 10, 10, 2)
    assert {"track_inertial", "vitrack_default_options"} <= set(abi.SIGNATURES) and {"track_inertial", "vitrack_default_options"} <= abi.PRODUCT_ONLY
    assert (abi.VITRACK_OK, abi.VITRACK_NONFINITE, abi.VITRACK_SINGULAR) == (VR.OK, VR.NONFINITE, VR.SINGULAR)
