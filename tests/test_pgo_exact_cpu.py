"""The extended-precision reference of the pose graph (tests/pgo_exact.py) and its cases (tests/pgo_exact_cases.py), on the CPU:
its Jacobians against central differences of its own error under its own oplus, the conditions every case has to meet by the reference
alone, the other restatements (tests/pgo_ref.py, the oracle, the facade) and the device formula (csrc/plba_pgo_dev.h, compiled for the
host with the sanitizers as csrc/plba_pgo_hostcheck.cpp) held to the wide run under the rule of pgo_exact.py."""
import os

import numpy as np
import pytest

from . import lba_ref as LR
from . import pgo_cov_ref as PCR
from . import pgo_exact as PX
from . import pgo_exact_cases as C
from . import pgo_ref
from . import solver_ref as SR

ROOT = C.ROOT
COMPARED = [n for n in C.NAMES if n not in C.NOT_COMPARED]


@pytest.fixture(scope="module")
def hostcheck():
    return C.build_hostcheck(os.path.join(ROOT, "tools", "_build_pgo_hostcheck"), sanitize=True)


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------
def _branch_pair(branch, flip, seed, dt):
    """(Xi, Xj, Zi) in dt whose error rotation takes the given R_to_q branch, with q.w < 0 before the flip when asked for: the rotation
    of E is by 2.6 rad about the +-axis of the branch (branch 0: 0.7 rad about a general axis, w > 0 always)"""
    rng = np.random.default_rng(seed)
    pose = lambda s: pgo_ref.join(pgo_ref._rot(rng.normal(size=3) * s)[None], rng.normal(size=(1, 3)) * 2)[0]
    Xi, Z = pose(0.8), pose(0.8)
    w = rng.normal(size=3) * 0.4 if branch == 0 else np.eye(3)[branch - 1] * (2.6 if not flip else -2.6) + rng.normal(size=3) * 0.05
    Xj = C._turn(pgo_ref.iso_mul(Xi, Z), w); Xj[9:] += rng.normal(size=3) * 0.3
    return PX.cast(Xi, dt), PX.cast(Xj, dt), PX.iso_inv(PX.cast(Z, dt))


@pytest.mark.parametrize("branch,flip", [(0, False), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True)])
def test_jacobians_equal_central_differences_of_the_own_error(branch, flip):
    """The bound.  e(u) is smooth in the update u; a central difference with step h has truncation h^2 / 6 x the third derivative.  The
    quaternion rows are q_E (u, sqrt(1 - |u|^2)): odd derivatives of the even square root vanish at 0, so they are exact to O(h^4).  The
    translation rows are R(u) t with R's entries 2 (xy -+ wz), 1 - 2 (y^2 + z^2): the third derivative of 2 z sqrt(1 - z^2) at 0 is -6, so
    the truncation is at most h^2 |t| per entry (|t| the translation the rotation acts on: t_B for vertex 0, none for vertex 1), and the
    rounding is 2 eps |e| / (2 h).  Held to FACTOR x that: 8 (h^2 (1 + |t_B|) + eps max|e| / h), h = 1e-6: 3e-11 at |t_B| = 3 in long double."""
    dt = LR.wide()
    h = 1e-6
    with LR._prec(dt):
        eps = float(np.finfo(np.longdouble).eps) if not isinstance(dt, str) else 2.0 ** -135
        for seed in range(3):
            Xi, Xj, Zi = _branch_pair(branch, flip, 40 + seed, dt)
            e0, info = PX.edge_error(Xi[None], Xj[None], Zi[None])
            assert int(info["branch"][0]) == branch and bool(info["flip"][0]) == flip
            J0, J1 = PX.edge_jacobians(Xi[None], Xj[None], Zi[None], dt)
            _, tB = PX.split(PX.iso_mul(PX.iso_inv(Xi), Xj))
            bound = PX.FACTOR * (h * h * (1 + float(np.abs(PX.f64(tB)).max()) * 3 ** 0.5) + eps * float(np.abs(PX.f64(e0)).max()) / h)
            for which, J in ((0, J0[0]), (1, J1[0])):
                N = np.zeros((6, 6))
                for c in range(6):
                    ev = []
                    for sgn in (1, -1):
                        u = PX.cast(np.zeros((1, 6)), dt); u[0, c] = PX.cast(sgn * h, dt)[()]
                        Xp, _, _, _ = PX.oplus((Xi if which == 0 else Xj)[None], u, np.zeros(1, np.int64), dt)
                        e, i2 = PX.edge_error(Xp if which == 0 else Xi[None], Xj[None] if which == 0 else Xp, Zi[None])
                        assert int(i2["branch"][0]) == branch and bool(i2["flip"][0]) == flip
                        ev.append(e[0])
                    N[:, c] = PX.f64((ev[0] - ev[1]) / (2 * PX.cast(h, dt)[()]))
                err = float(np.abs(PX.f64(J) - N).max())
                print("branch %d flip %d vertex %d: |J - central differences| %.3e  bound %.3e" % (branch, flip, which, err, bound))
                assert err <= bound


def test_the_oplus_counter_and_the_identity_rotation_branch():
    dt = LR.wide()
    with LR._prec(dt):
        rng = np.random.default_rng(3)
        R = pgo_ref._rot(rng.normal(size=3)) @ (np.eye(3) + 1e-3 * rng.normal(size=(3, 3)))      # off the orthogonal matrices by 1e-3
        X = PX.cast(np.concatenate([R.ravel(), [1.0, 2.0, 3.0]])[None], dt)
        u = PX.cast(np.array([[0.1, -0.2, 0.3, 0.01, 0.02, -0.03]]), dt)
        Xa, ca, w2, fa = PX.oplus(X, u, np.array([999]), dt)
        Xb, cb, _, fb = PX.oplus(X, u, np.array([1000]), dt)
        assert ca[0] == 1000 and not fa[0] and cb[0] == 0 and fb[0]
        Ra, Rb = PX.f64(PX.split(Xa)[0][0]), PX.f64(PX.split(Xb)[0][0])
        off = lambda M: np.abs(M.T @ M - np.eye(3)).max()
        assert off(Rb) < 10 * off(Ra) ** 2 and off(Ra) > 1e-4      # one step of the iteration squares the distance
        big = PX.cast(np.array([[0.1, -0.2, 0.3, 0.8, 0.5, 0.4]]), dt)      # |u_r|^2 = 1.05
        Xc, _, w2c, _ = PX.oplus(X, big, np.array([0]), dt)
        assert float(w2c[0]) < 0 and np.array_equal(PX.f64(PX.split(Xc)[0]), PX.f64(PX.split(X)[0]))      # X (I, t): the rotation untouched
        assert np.abs(PX.f64(PX.split(Xc)[1][0]) - (R @ [0.1, -0.2, 0.3] + [1, 2, 3])).max() < 1e-15


# ---- the conditions of every case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_conditions_hold_by_the_reference_alone(name):
    case, r64, rw, T = C.runs(name)
    assert C.EXPECT[name](r64) and C.EXPECT[name](rw), name
    assert r64["omega"] <= SR.RESIDUAL_MAX and rw["omega"] <= SR.RESIDUAL_MAX, (r64["omega"], rw["omega"])
    if name in C.NOT_COMPARED:
        assert T == 0, (name, T)      # the rule leaves nothing: not a choice
        return
    assert T >= 1, name
    assert T == C.TRIALS[name], (name, T)      # the trial up to which the case is compared, as the file states it
    tol, noise, lim = PX.tolerances(case, r64, rw, T)
    tight = PX.tolerances_tighten(tol, noise, lim)
    _, margins = PX.horizon(r64, rw)
    stable = C.reference_is_stable(case, r64, rw, T)
    print("%s: compared over %d of %d trials; (a) 8 noise / today's bar %.3g  (b) smallest margin / noise %.3g  (c) reordered error / tolerance %.3g" % (
        name, T, rw["trials"], tight, min(margins), stable))
    assert tight < 1.0 and min(margins) >= PX.MARGIN and stable <= 0.5


def test_h_readable_lists_the_cases_whose_undamped_factorisation_has_margin():
    assert C.H_READABLE == [n for n in C.NAMES if C.undamped_pivot_margin(C.runs(n)[2]) >= PX.MARGIN]


def test_the_census_of_each_case_is_what_its_name_says():
    for a, b in (("x", 1), ("y", 2), ("z", 3)):
        _, r64, rw, T = C.runs("branch_" + a)
        for r in (r64, rw):
            n, f = C._census(r, b)
            assert n >= 2 and f >= 1, (a, n, f)
    for name, acc in (("big_step", 1), ("big_step_rejected", 0)):
        _, r64, rw, T = C.runs(name)
        assert [i for i in C._w2neg(rw, acc) if i < T] and C._w2neg(r64, acc) == C._w2neg(rw, acc), name
    rank = lambda g: PCR.free_ranks(g)[0]
    g = C.runs("reversed")[0]; fr = rank(g)
    assert np.all(g["ei"] > g["ej"]) and np.any((fr[g["ei"]] >= 0) & (fr[g["ej"]] >= 0))
    g = C.runs("relabelled")[0]
    assert np.all(g["ei"] > g["ej"])
    g = C.runs("mixed")[0]
    assert np.all((g["ei"] > g["ej"]) == (np.arange(len(g["ei"])) % 2 == 1))
    g = C.runs("dup_both_ways")[0]; fr = rank(g)
    start, src, _, row, col, _ = C.host_blocks(g)
    assert any({2, 3} <= {int(s) & 3 for s in src[start[q]:start[q + 1]]} for q in range(len(row)))      # one block, both kinds of source
    for n in (63, 64, 65, 255, 256, 257, 513):
        g = C.runs("edges_%d" % n)[0]
        assert len(g["ei"]) == n and int(g["fixed"].sum()) == 2
    for n in (63, 64, 65):
        g, _, rw, _ = C.runs("free_%d" % n)
        assert rw["n"] == n and len(C.host_blocks(g)[3]) % 4 == C.NBLK_MOD4["free_%d" % n] and len(C.host_blocks(g)[3]) == C.nblk_of(g)
    g, _, rw, _ = C.runs("hub_300")
    deg = np.bincount(np.concatenate([g["ei"], g["ej"]]), minlength=g["nv"])
    start, src, diag, row, col, _ = C.host_blocks(g)
    assert deg.max() == 300 and (np.diff(start)).max() == 300 and int((g["ei"] == 150).sum()) == 150 and int((g["ej"] == 150).sum()) == 150
    assert {int(s) & 3 for s in src} == {0, 1} and rw["n"] == 1 and len(row) == 1
    g = C.runs("info_none")[0]
    assert g["info"] is None
    g = C.runs("info_scaled")[0]
    a = np.abs(g["info"][g["info"] != 0])
    assert a.max() / np.median(np.abs(np.einsum("kii->ki", g["info"]))) > 1e2 and a.max() > 1e5 and np.einsum("kii->ki", g["info"]).min() < 1e-1
    g, _, rw, _ = C.runs("init_guess")
    assert rw["init_inverse"] >= 1 and int(g["fixed"].sum()) == 2 and g["opts"]["initial"]
    for name in C.NAMES:
        if name.startswith("near_pi"):
            g, _, rw, _ = C.runs(name)
            hot = rw["ev0"]["branch"] > 0
            d = 10.0 ** -int(name[-1])
            assert np.all(np.abs(PX.f64(rw["ev0"]["w"])[hot]) < d) and np.all(np.abs(PX.f64(rw["ev0"]["w"])[hot]) > d / 4)      # w = sin(delta / 2)


# These seven have SEED 0, pick_seed's first candidate, and test_conditions_hold_by_the_reference_alone asserts at that seed the very predicate
# pick_seed tests (EXPECT on both runs, (a), (b) over TRIALS >= 1, (c)): that they are reproduced follows from it and is not run twice.
SLOW_TO_PICK = ("edges_255", "edges_256", "edges_257", "edges_513", "free_63", "free_64", "free_65")


@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in C.SHARED and n not in SLOW_TO_PICK] + ["shared"])
def test_pick_seed_reproduces_the_seed(name):
    assert all(C.SEED[n] == 0 for n in SLOW_TO_PICK)
    if name == "shared":
        assert C.pick_shared_seed() == C.SEED["base12"] and all(C.SEED[n] == C.SEED["base12"] for n in C.SHARED)
    else:
        assert C.pick_seed(name) == C.SEED[name]


def test_relabelling_gives_the_unrelabelled_chi2_and_h():
    """`relabelled` (vertex v named nv - 1 - v, measurements untouched): the same chi2 and the same H, blocks renumbered and transposed, under
    the rule"""
    gb, b64, bw, _ = C.runs("base12")
    gr, r64, rw, _ = C.runs("relabelled")
    tol, noise, _ = PX.tolerances(gb, b64, bw, 0)
    bad = []
    PX.hold("relabelled", "chi2_initial", rw["chi2_initial"], bw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    n = bw["n"]
    Hb, Hr = PX.f64(bw["first"]["H"]).reshape(n, 6, n, 6), PX.f64(rw["first"]["H"]).reshape(n, 6, n, 6)
    rows, cols, _ = PX.block_sources(gb)
    for k, (a, c) in enumerate(zip(rows, cols)):
        PX.hold("relabelled", "H[%d,%d]" % (a, c), Hr[n - 1 - a, :, n - 1 - c, :], Hb[a, :, c, :], tol["H"][k], noise["H"][k], bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["reversed", "mixed"])
def test_a_reversed_edge_has_the_conjugated_inverse_error(name):
    """An edge (i, j, Z) given as (j, i, W), W the fp64 inverse of Z, has the error isometry E' = W^-1 Xj^-1 Xi = W^-1 E^-1 Z^-1 (= Z E^-1 Z^-1
    for an exact W): the inverse of E conjugated by the measurement.  Its error vector is no function of e alone (the rotation of E acts on
    t_Z), so neither chi2 nor H of a reversed graph equals the unreversed graph's, to rounding or to any order in e; what is exact is the
    relation between the isometries.  slam3d_detail::inv inverts a rotation by transposing it, and the fp64 rotations of the inputs are
    orthogonal to `defect` = max |R^T R - I| only, so the relation is asserted in the wide type to 64 (eps + defect) x the largest entry
    (five transposed inverses and four products of three terms an entry)."""
    gb = C.runs("base12")[0]
    g = C.runs(name)[0]
    dt = LR.wide()
    with LR._prec(dt):
        eps = float(np.finfo(np.longdouble).eps) if not isinstance(dt, str) else 2.0 ** -135
        X, Z, W = PX.cast(gb["pose"], dt), PX.cast(gb["meas"], dt), PX.cast(g["meas"], dt)
        E = PX.edge_isometry(X[gb["ei"]], X[gb["ej"]], PX.iso_inv(Z))
        E2 = PX.edge_isometry(X[g["ei"]], X[g["ej"]], PX.iso_inv(W))
        rev = g["ei"] != gb["ei"]
        assert rev.sum() == (len(rev) if name == "reversed" else len(rev) // 2) and np.array_equal(g["ei"][rev], gb["ej"][rev])
        want = PX.iso_mul(PX.iso_mul(PX.iso_inv(W), PX.iso_inv(E)), PX.iso_inv(Z))
        err = float(np.abs(PX.f64(E2[rev] - want[rev])).max())
        defect = max(float(np.abs(PX.f64(PX._mm(PX._tr(PX.split(A)[0]), PX.split(A)[0]) - PX.cast(np.eye(3), dt))).max()) for A in (X, Z, W))
        bound = 64 * (eps + defect) * float(np.abs(PX.f64(want)).max())
        same = float(np.abs(PX.f64(E2[~rev] - E[~rev])).max()) if (~rev).any() else 0.0
        e, _ = PX.edge_error(X[gb["ei"]], X[gb["ej"]], PX.iso_inv(Z))
        e2, _ = PX.edge_error(X[g["ei"]], X[g["ej"]], PX.iso_inv(W))
        print("%s: |E' - W^-1 E^-1 Z^-1| %.3e  bound %.3e;  max|e' + e| %.3e at max|e| %.3e: no equality of the error vectors (defect %.1e)" % (
            name, err, bound, float(np.abs(PX.f64(e2 + e))[rev].max()), float(np.abs(PX.f64(e)).max()), defect))
        assert err <= bound and same == 0.0


# ---- the other restatements ---------------------------------------------------------------------------------------------------------------
def _as_ref(r):
    return dict(poses=r["poses"], chi2_initial=r["chi2_initial"], trace=r["trace"], iterations=r["iterations"], trials=r["trials"])


@pytest.mark.parametrize("name", COMPARED)
def test_pgo_ref_is_held_to_the_wide_run(name):
    case, r64, rw, T = C.runs(name)
    o = case["opts"]
    bad = []
    for k in (1, 2, 3):
        r = pgo_ref.optimize(case["pose"], case["ei"], case["ej"], case["meas"], case["info"], case["fixed"], iters=k, user_lambda=o["user_lambda"], initial=o["initial"])
        bad += PX.hold_run("pgo_ref %s iters %d" % (name, k), case, _as_ref(r), r64, rw, T, k)
    g0 = dict(case, pose=PX.f64(rw["X_start"]))
    tol, noise, _ = PX.tolerances(case, r64, rw, T)
    B = PCR.blocks_from_graph(g0)
    Bw = PX.h_blocks(case, rw)
    for q in range(len(B)):
        e = float(np.abs(B[q] - Bw[q]).max())
        if not e <= tol["H"][q]:
            bad.append(("H", q, e, tol["H"][q]))
    print("pgo_ref %s H: worst error / tolerance %.3f over %d blocks" % (name, float((np.abs(B - Bw).reshape(len(B), -1).max(-1) / tol["H"]).max()), len(B)))
    assert not bad, bad


def _dp(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.mark.parametrize("name", ["branch_x", "branch_y", "branch_z", "near_pi_ring_9", "big_step", "reversed", "info_scaled"])
def test_oracle_edge_error_and_oplus_are_held_to_the_wide_run(orc, name):
    case, r64, rw, T = C.runs(name)
    lib = orc.lib().cdll
    X = np.ascontiguousarray(PX.f64(rw["X_start"]))
    ne = len(case["ei"])
    e = np.zeros((ne, 6))
    for k in range(ne):
        lib.orc_se3_edge_error(_dp(np.ascontiguousarray(X[case["ei"][k]])), _dp(np.ascontiguousarray(X[case["ej"][k]])), _dp(np.ascontiguousarray(case["meas"][k])), _dp(e[k]))
    bad = []
    n_e, t_e = PX._noise_tol(r64["first"]["e"], rw["first"]["e"], 64)
    PX.hold("oracle " + name, "edge errors", e, rw["first"]["e"], t_e, n_e, bad)
    # the first trial's oplus
    x = np.ascontiguousarray(PX.f64(rw["trace"][0]["x"]).reshape(-1, 6))
    free = PCR.free_ranks(case)[1]
    Xn = X.copy()
    for r, v in enumerate(free):
        out = np.zeros(12)
        lib.orc_se3_vertex_oplus(_dp(np.ascontiguousarray(X[v])), _dp(x[r]), _dp(out))
        Xn[v] = out
    dt = LR.wide()
    with LR._prec(dt):
        Xw, _, _, _ = PX.oplus(PX.cast(X[free], dt), PX.cast(x, dt), np.zeros(len(free), np.int64), dt)
    X6, _, _, _ = PX.oplus(X[free], x, np.zeros(len(free), np.int64), np.float64)
    n_x, t_x = PX._noise_tol(X6, Xw, 64)
    PX.hold("oracle " + name, "oplus", Xn[free], Xw, t_x, n_x, bad)
    assert not bad, bad


@pytest.mark.parametrize("name", ["base12", "edges_64", "info_scaled"])
def test_oracle_pose_graph_keeps_its_bars_against_the_wide_run(orc, name):
    """orc_pgo differentiates numerically: test_host_graphs' bars between numeric and analytic Jacobians (chi2_initial 1e-9 relative — held
    under the rule here, it has no Jacobian in it —, the trial sequence, chi2_final 1e-5 relative, poses 1e-6), against the wide run"""
    from .test_pgo_cpu import _orc_pgo
    case, r64, rw, T = C.runs(name)
    g = dict(nv=case["nv"], pose=case["pose"], ei=case["ei"], ej=case["ej"], meas=case["meas"], fixed=np.ascontiguousarray(case["fixed"], np.int32))
    info = np.tile(np.eye(6), (len(case["ei"]), 1, 1)) if case["info"] is None else case["info"]
    pose, st = _orc_pgo(orc, g, 3, 0, info=np.ascontiguousarray(info))
    tol, noise, _ = PX.tolerances(case, r64, rw, T)
    bad = []
    PX.hold("orc_pgo " + name, "chi2_initial", st[0], rw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    assert not bad, bad
    assert int(st[2]) == rw["iterations"] and int(st[3]) == rw["trials"]
    assert st[1] == pytest.approx(float(rw["chi2_final"]), rel=1e-5)
    assert np.abs(pose - PX.f64(rw["poses"])).max() < 1e-6


def _log_exp_round_trip(orc, X):
    """poses through SE3Quat::log and SE3Quat::exp in fp64, as the harness writes an estimate and the test reads it (the oracle's restatement of
    IMU/se3quat.h, as test_host_graphs._pgo_problem and _se3_exp use it)"""
    from .test_host_graphs import _pose12, _se3_exp
    lib = orc.lib().cdll
    out = []
    for x in np.ascontiguousarray(X, np.float64):
        R, t, q, v = np.ascontiguousarray(x[:9]), np.ascontiguousarray(x[9:]), np.zeros(4), np.zeros(6)
        lib.orc_R_to_quat(_dp(R), _dp(q))
        q = np.ascontiguousarray(q / np.linalg.norm(q) * (1.0 if q[3] >= 0 else -1.0))
        lib.orc_se3_log(_dp(q), _dp(t), _dp(v))
        out.append(_pose12(*_se3_exp(orc, v)))
    return np.array(out)


def test_facade_is_held_to_the_wide_run(pkg, orc, tmp_path):
    """the facade's host Levenberg loop through the harness (analytic Jacobians, identity information) on test_host_graphs' 24-vertex graph,
    under the rule: chi2 of the start and of the end, the same trials, the poses.  The harness writes each estimate as SE3Quat::log and the
    test reads it back through SE3Quat::exp: one more fp64 operation behind the optimiser, whose noise is measured as the rule measures
    any: the wide run's poses through the same log and exp in fp64, against themselves.  The poses are held to the rule's tolerance plus
    FACTOR x that noise (the operation runs once on the facade's poses and its rounding there is of the same size, not the same value)."""
    from .test_host_graphs import _pgo_problem, _run_pgo
    from .test_pgo import _from_log6
    g = _pgo_problem(pkg, orc)
    o = _run_pgo(pkg, orc, tmp_path, g, "pgo", 0, iters=3)
    case = C._from(dict(_from_log6(orc, g), info=None))
    r64, rw = PX.run(case, np.float64, **case["opts"]), PX.run(case, LR.wide(), **case["opts"])
    T, _ = PX.horizon(r64, rw)
    assert T == rw["trials"]
    tol, noise, _ = PX.tolerances(case, r64, rw, T)
    bad = []
    PX.hold("facade", "chi2_initial", o["chi0"], rw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    PX.hold("facade", "chi2_final", o["chi1"], rw["chi2_final"], tol[("chi2_trial", T - 1)], noise[("chi2_trial", T - 1)], bad)
    assert o["done"] == rw["iterations"] and o["trials"] == rw["trials"]
    Xw = PX.f64(rw["poses"])
    rt = float(np.abs(_log_exp_round_trip(orc, Xw) - Xw).max())
    print("facade: log / exp round trip of the wide run's poses in fp64: %.3e" % rt)
    PX.hold("facade", "poses after 3", o["got"], rw["poses"], tol[("poses", 3)] + PX.FACTOR * rt, noise[("poses", 3)] + rt, bad)
    assert not bad, bad


# ---- the device formula on the host ---------------------------------------------------------------------------------------------------------
def _hold_host(name, case, r64, rw, o, label="host"):
    """the host program's linearisation and first update against the wide run under the rule; the list of misses"""
    tol, noise, _ = PX.tolerances(case, r64, rw, 1)
    bad = []
    ne = len(case["ei"])
    rec = o["erec"]
    parts = dict(A00=rec[:, 0:36].reshape(ne, 6, 6), A11=rec[:, 36:72].reshape(ne, 6, 6), A10=rec[:, 72:108].reshape(ne, 6, 6), g0=rec[:, 108:114], g1=rec[:, 114:120])
    worst = {}
    for q, (p6, pw) in zip(("A00", "A11", "A10", "g0", "g1"), zip(r64["first"]["blocks"], rw["first"]["blocks"])):
        a6, aw, got = PX.f64(p6).reshape(ne, -1), PX.f64(pw).reshape(ne, -1), parts[q].reshape(ne, -1)
        nz = np.abs(a6 - aw).max(-1)
        t = np.maximum(PX.FACTOR * nz, 36 * PX.U * np.abs(aw).max(-1))      # per edge, in the block's maximum norm; 36 products an entry
        e = np.abs(got - aw).max(-1)
        worst[q] = float((e / t).max())
        for k in np.flatnonzero(~(e <= t)):
            bad.append((q, int(k), float(e[k]), float(t[k])))
    print("%s %s per-edge record: worst error / tolerance %s" % (label, name, {q: "%.3f" % v for q, v in worst.items()}))
    c6, cw = r64["first"]["e"], rw["first"]["e"]
    G6 = PX.Graph(case, np.float64)
    chi6 = PX.chi2_edges(PX.f64(c6), G6.om)
    with LR._prec(LR.wide()):
        Gw = PX.Graph(case, LR.wide())
        chiw = PX.chi2_edges(cw, Gw.om)
    nz, t = PX._noise_tol(chi6, chiw, 36)
    PX.hold(label + " " + name, "chi2 per edge", o["echi"], chiw, t, nz, bad)
    PX.hold(label + " " + name, "chi2_initial", o["echi"].sum(), rw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    Bw = PX.h_blocks(case, rw)
    e = np.abs(o["Hblk"] - Bw).reshape(len(Bw), -1).max(-1)
    print("%s %s H blocks: worst error / tolerance %.3f over %d blocks, worst error / noise %.2f" % (
        label, name, float((e / tol["H"]).max()), len(Bw), float(np.max(e / np.where(noise["H"] > 0, noise["H"], np.inf)))))
    for q in np.flatnonzero(~(e <= tol["H"])):
        bad.append(("H", int(q), float(e[q]), float(tol["H"][q])))
    _, _, cnt = PX.block_sources(case)
    nz, t = PX._noise_tol(r64["first"]["b"], rw["first"]["b"], 6 * int(cnt.max()))
    PX.hold(label + " " + name, "b", o["b"], rw["first"]["b"], t, nz, bad)
    return bad


def _first_update(case, rw):
    """(the step given to the host program, the wide and the fp64 reference's poses behind it, the wide chi2 there)"""
    X = PX.f64(rw["X_start"])
    x = PX.f64(rw["trace"][0]["x"]).reshape(-1, 6)
    free = PCR.free_ranks(case)[1]
    dt = LR.wide()
    with LR._prec(dt):
        Xf, _, _, _ = PX.oplus(PX.cast(X[free], dt), PX.cast(x, dt), np.zeros(len(free), np.int64), dt)
        Xw = PX.cast(X, dt); Xw[free] = Xf
        chiw = PX.Graph(case, dt).chi2(Xw)[0]
    X6 = X.copy(); X6[free] = PX.oplus(X[free], x, np.zeros(len(free), np.int64), np.float64)[0]
    chi6 = PX.Graph(case, np.float64).chi2(X6)[0]
    return x, Xw, X6, chiw, chi6


@pytest.mark.parametrize("name", COMPARED)
def test_device_formula_on_the_host_is_held_to_the_wide_run(hostcheck, tmp_path, name):
    case, r64, rw, T = C.runs(name)
    x, Xw, X6, chiw, chi6 = _first_update(case, rw)
    o = C.host_run(hostcheck, str(tmp_path), case, PX.f64(rw["X_start"]), x)
    bad = _hold_host(name, case, r64, rw, o)
    nz, t = PX._noise_tol(X6, Xw, 64)
    PX.hold("host " + name, "updated poses", o["X"], Xw, t, nz, bad)
    nz, t = PX._noise_tol(chi6, chiw, 6 * len(case["ei"]))
    PX.hold("host " + name, "chi2 of the trial", o["echi_trial"].sum(), chiw, t, nz, bad)
    fx = ~np.isin(np.arange(case["nv"]), PCR.free_ranks(case)[1])
    assert np.array_equal(o["X"][fx], PX.f64(rw["X_start"])[fx]) and np.all(o["cnt"][~fx] == 1) and np.all(o["cnt"][fx] == 0)
    assert not bad, bad


@pytest.mark.parametrize("name", ["base12", "branch_x", "hub_300"])
def test_reorthogonalisation_on_the_host_is_held_to_the_wide_run(hostcheck, tmp_path, name):
    """the counter preset to 1000, so that this oplus is the 1001st: k_pgo_update's re-orthogonalisation, which no single call of the C
    entry reaches.  The rotations are moved 1e-3 off the orthogonal matrices first, or the correction would be rounding noise itself."""
    case, r64, rw, T = C.runs(name)
    rng = np.random.default_rng(11)
    X = PX.f64(rw["X_start"]).copy()
    R = X[:, :9].reshape(-1, 3, 3) @ (np.eye(3) + 1e-3 * rng.normal(size=(len(X), 3, 3)))
    X[:, :9] = R.reshape(-1, 9)
    x = PX.f64(rw["trace"][0]["x"]).reshape(-1, 6)
    free = PCR.free_ranks(case)[1]
    o = C.host_run(hostcheck, str(tmp_path), case, X, x, cnt0=1000)
    dt = LR.wide()
    with LR._prec(dt):
        Xw, cw, _, fw = PX.oplus(PX.cast(X[free], dt), PX.cast(x, dt), np.full(len(free), 1000), dt)
        Xplain, _, _, _ = PX.oplus(PX.cast(X[free], dt), PX.cast(x, dt), np.zeros(len(free), np.int64), dt)
    X6, _, _, f6 = PX.oplus(X[free], x, np.full(len(free), 1000), np.float64)
    assert fw.all() and f6.all() and np.all(cw == 0) and np.all(o["cnt"][free] == 0)
    moved = float(np.abs(PX.f64(Xw) - PX.f64(Xplain)).max())
    bad = []
    nz, t = PX._noise_tol(X6, Xw, 64)
    PX.hold("host " + name, "re-orthogonalised", o["X"][free], Xw, t, nz, bad)
    print("the re-orthogonalisation moved the entries by up to %.3e" % moved)
    assert moved > 1e-4 and not bad, bad
