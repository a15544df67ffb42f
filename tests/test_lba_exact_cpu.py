"""The pre-init visual-only local BA against an extended-precision reference, without a GPU: tests/lba_ref.py (written from the
reference's text) against the 40-digit single-observation fixture, its two forms of the damped step against each other, its point
rows against numeric derivatives, and the fp64 oracle against it under the tolerance rule of lba_ref.tolerances."""
import json
import os

import numpy as np
import pytest

from . import lba_cases as LC
from . import lba_ref as LR
from . import solver_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "lba_obs_exact.json")) as f:
    FIX = json.load(f)


def _orc(orc, w, **o):
    p = orc.new_problem()
    r = p.lba_visual(w["T_kf_w"], w["kf_loc"], w["xyz"], w["pq"], w["po_pt"], w["po_kf"], w["uv"], w["lo_ln"], w["lo_kf"], w["l3"], w["cam"], **o)
    p.close()
    return r


def _pair(w, **o):
    return LR.run(w, np.float64, **o), LR.run(w, LR.wide(), **o)


def _wide_of_string(s, dt):
    if isinstance(dt, str):
        import mpmath
        return mpmath.mpf(s)
    return dt(s)


@pytest.mark.parametrize("dt", [np.float64, np.longdouble, "mp"], ids=["float64", "longdouble", "mpmath"])
@pytest.mark.parametrize("case", FIX["cases"], ids=[c["name"] for c in FIX["cases"]])
def test_reference_observation_matches_the_40_digit_fixture(case, dt):
    """n, w, Jp, Jl of one observation.  The residual is a difference of pixel coordinates of size |z|: its rounding error eps |z| is
    RELATIVE eps |z| / n in n and in every row (each is linear in the error vector, then divided by max(homog_th, n)), so the tolerance
    is 64 eps (1 + |proj| / max(n, tiny)) relative to the row's largest entry, eps that of the working type (2^-53, 2^-64; 1e-29 for mpmath: the fixture is written with 30 digits).  The clamp by homog_th is pinned
    by the two `below_homog_th` cases (n = 4e-8, 5e-8: nine digits left in fp64); `point_residual_of_rounding_only` (n = 3e-14, nothing
    but the rounding of uv) can pin only w and that the rows stay finite and small: its relative tolerance on n and the rows is 1e5."""
    with LR._prec(dt):
        eps = 1e-29 if isinstance(dt, str) else float(np.finfo(dt).eps) / 2
        c = lambda v: LR.cast(np.asarray(v, np.float64), dt)
        T = np.asarray(case["T"]); Ri, ti = LR.se3_inv(c(T[:3, :3])[None], c(T[:3, 3])[None])
        cam = [c(v)[()] for v in FIX["cam"]]
        fn = LR.point_obs if case["kind"] == "point" else LR.line_obs
        n, w, Jp, Jl = fn(cam, c(FIX["homog_th"])[()], Ri, ti, c(case["X"])[None], c(case["z"])[None])
        ex = case["expected"]
        n_ex = float(ex["n"])
        size = max(abs(FIX["cam"][2]), abs(FIX["cam"][3])) * 2 if case["kind"] == "point" else 1000.0      # |u|, |v|; l . (u, v, 1) terms
        rel = 64 * eps * (1 + size / max(n_ex, 1e-300))
        for got, want in ((n[None], [ex["n"]]), (Jp[0], ex["Jp"]), (Jl[0], ex["Jl"])):
            want = [_wide_of_string(s, dt) for s in want]
            scale = max(abs(float(v)) for v in want)
            for g, v in zip(np.ravel(got), want):
                assert abs(float(g - v)) <= rel * scale + 1e-300, (case["name"], float(g), float(v), rel)
        assert abs(float(w[0] - _wide_of_string(ex["w"], dt))) <= 64 * eps + rel * min(1.0, 2 * n_ex * n_ex)      # dw = -2 n^2 w^2 (dn / n)
        if case["fixed"]:      # kf_idx_loc == -1 (:1522-1527): nothing of the observation reaches the pose blocks
            part = (np.zeros(1, np.int64), np.full(1, -1), n, w, Jp, Jl, 1, Jl.shape[-1])
            _, Hpp, gp, lm = LR.blocks([part], 1, dt)
            assert not LR.f64(Hpp).any() and not LR.f64(gp).any() and LR.f64(lm[0][0]).any()


def test_fixture_generator_reproduces_the_committed_file(tmp_path):
    import subprocess
    import sys
    import shutil
    gen = tmp_path / "make_lba_obs_exact.py"
    shutil.copy(os.path.join(HERE, "golden", "make_lba_obs_exact.py"), gen)
    subprocess.check_call([sys.executable, str(gen)], stdout=subprocess.DEVNULL)
    with open(tmp_path / "lba_obs_exact.json") as f:
        assert json.load(f) == FIX


def test_mpmath_fallback_runs_the_whole_function():
    """the "mp" type through blocks, both forms of the step, the solve and the update, where long double is extended too: two passes on
    the duplicate-observation window against the long-double run (1e-15: the wider of the two is exact at this level)"""
    w = LC.edge_duplicate()
    for form in ("elim", "dense"):
        a, b = LR.run(w, "mp", form=form, max_iters=2), LR.run(w, np.longdouble if SR.LD_IS_EXTENDED else np.float64, form=form, max_iters=2)
        tol = 1e-15 if SR.LD_IS_EXTENDED else 1e-9
        assert a["omega"] <= SR.RESIDUAL_MAX and (a["iterations"], a["updates"]) == (b["iterations"], b["updates"]) == (2, 2)
        for q in ("T", "xyz", "pq"):
            assert np.abs(a[q] - b[q]).max() <= tol * max(1.0, np.abs(a[q]).max()), (form, q)
        assert abs(a["lam"] - b["lam"]) <= tol * abs(a["lam"]) and abs(a["err_first"] - b["err_first"]) <= tol * a["err_first"]


SMALL = dict(duplicate=LC.edge_duplicate, fixed_only=LC.edge_fixed_only, exact_uv=LC.edge_exact_uv, boundary_127_2=lambda: LC.block_boundary(127, 2),
             chunk_65_lines=lambda: LC.three_keyframes(65, True))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_eliminated_form_is_the_dense_form(name):
    """(b) against (a) in the wide type, N <= ~900, three passes: both solve the same wide system, so they agree to the wide type's
    rounding amplified by the conditioning: 1e-15 absolute (the fp64 noise of these windows is 1e-14 and more)"""
    w = SMALL[name]()
    a, b = LR.run(w, LR.wide(), form="dense", max_iters=3), LR.run(w, LR.wide(), form="elim", max_iters=3)
    assert a["omega"] <= SR.RESIDUAL_MAX and b["omega"] <= SR.RESIDUAL_MAX
    assert (a["iterations"], a["updates"]) == (b["iterations"], b["updates"]) == (3, 3)
    for k in (1, 2, 3):
        x, y = LR.at(a, k), LR.at(b, k)
        for q in ("T", "xyz", "pq"):
            assert np.abs(x[q] - y[q]).max() <= 1e-15 * max(1.0, np.abs(x[q]).max()), (name, k, q)
        assert x["lam"] == y["lam"] and x["err_first"] == y["err_first"]


def test_reference_point_rows_are_the_derivative_of_the_norm_residual():
    """points only: the reference's first step is the damped, weighted Gauss-Newton step on r = |e| from NUMERIC derivatives under
    T <- T expmap(dx)^-1 (central differences, h = 1e-6 in long double: truncation h^2, rounding eps / h, both below 1e-9 relative)"""
    w = LC.from_tracks(4, 1, [[0, 1, 2, 3] if k % 3 else [1, 2] for k in range(30)], [], 5)
    dt = LR.wide()
    o = dict(LR.DEFAULTS)
    with LR._prec(dt):
        win = LR.Window(w, dt, o)
        Nkf, Np = win.Nkf, win.Np

        def resid(dx):
            v = LR.Window(w, dt, o)
            LR.apply_step(v, dx[:6 * Nkf].reshape(Nkf, 6), [dx[6 * Nkf:].reshape(Np, 3), None])
            Ri, ti = LR.se3_inv(*v.poses(True))
            return LR.point_obs(v.cam, v.th, Ri[v.po_kf], ti[v.po_kf], v.xyz[v.po_pt], v.uv)[0]
        N = 6 * Nkf + 3 * Np
        z = LR.cast(np.zeros(N), dt)
        r0 = resid(z)
        h = LR.cast(1e-6, dt)[()]
        J = []
        for c in range(N):
            d = z.copy(); d[c] = h
            J.append((resid(d) - resid(-d)) / (2 * h))
        J = np.stack(J, 1)
        W = 1 / (1 + r0 * r0)
        H = LR.f64((J * W[:, None]).T @ J) if not isinstance(dt, str) else LR.f64(LR._mm((J * W[:, None]).T, J))
        g = LR.f64((J * (W * r0)[:, None]).sum(0))
    lam = 1e-5 * np.abs(np.diag(H)).max()
    r = LR.run(w, dt, form="dense", max_iters=1)
    assert r["lam"] == pytest.approx(lam, rel=1e-8)
    # the update is applied with the sign of the reference: DX = solve(H, +g), T <- T expmap(dx)^-1, X += dx, with g = J^T W r of the
    # ANALYTIC rows; the numeric J above is d r / d(applied dx), whose sign the analytic rows carry reversed
    dx = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
    p = r["passes"][0]
    got = np.concatenate([LR.f64(p["dxp"]).ravel(), (r["xyz"] - w["xyz"]).ravel()])
    assert np.abs(got - dx).max() <= 1e-7 * np.abs(dx).max()


CHUNKS = [(n, lines) for n in LC.CHUNK_N for lines in (False, True)]


@pytest.mark.parametrize("n,lines", CHUNKS)
def test_oracle_one_pass_on_the_chunk_windows(orc, n, lines):
    w = LC.three_keyframes(n, lines)
    r64, rw = _pair(w, max_iters=1)
    name = "chunk n=%d%s 1 pass" % (n, " lines" if lines else "")
    res = _orc(orc, w, max_iters=1)
    LR.hold(res, r64, rw, "oracle", name)
    LR.hold_pose_step(res["T"], w, rw, "oracle", name)


EDGE_RUNS = [(k, it, {}) for k in sorted(LC.EDGES) for it in (0, 1)] + [("duplicate", 0, dict(variant=1, min_error=2.0 ** -52, min_error_change=2.0 ** -52, max_iters=6))]
EDGE_OPTS = dict(identity=dict(lambda_lm=1e-9))      # see test_lba_exact.py: keeps the keyframe out of the ill-conditioned acos range after its first update


@pytest.mark.parametrize("edge,iterate,extra", EDGE_RUNS, ids=["%s-%d%s" % (k, it, "-gba" if e else "") for k, it, e in EDGE_RUNS])
def test_oracle_on_the_structure_edges(orc, edge, iterate, extra):
    """one, two, three passes and the full run"""
    w = LC.EDGES[edge]()
    o = dict(EDGE_OPTS.get(edge, {}), use_iterate_poses=iterate, **extra)
    r64, rw = _pair(w, **o)
    for k in (1, 2, 3, None):
        ok = dict(o) if k is None else dict(o, max_iters=k)
        LR.hold(_orc(orc, w, **ok), LR.at(r64, k), LR.at(rw, k), "oracle", "%s iterate=%d %s passes" % (edge, iterate, k or "all"), ok)


@pytest.mark.parametrize("Np,Nl", [(127, 2), (128, 1)])
def test_oracle_on_the_block_boundaries(orc, Np, Nl):
    w = LC.block_boundary(Np, Nl)
    r64, rw = _pair(w)
    for k in (1, 2, 3, None):
        ok = {} if k is None else dict(max_iters=k)
        LR.hold(_orc(orc, w, **ok), LR.at(r64, k), LR.at(rw, k), "oracle", "boundary %d+%d %s passes" % (Np, Nl, k or "all"), ok)


def test_oracle_one_pass_on_the_generated_multi_chunk_window(pkg, orc):
    w = pkg.window.make_visual_window(K=3, Np=400, Nl=100, n_fixed=1, seed=3, track=3)
    r64, rw = _pair(w, max_iters=1)
    LR.hold(_orc(orc, w, max_iters=1), r64, rw, "oracle", "generated 400+100 1 pass")


@pytest.mark.parametrize("name,make", [("point", LC.fail_unobserved_point), ("keyframe", LC.fail_unobserved_keyframe)])
def test_oracle_and_reference_report_the_numerical_failure(orc, name, make):
    w = make()
    r = LR.run(w, LR.wide())
    o = _orc(orc, w)
    for x in (r, o):
        assert (x["solver_failed"], x["updates"], x["iterations"]) == (1, 0, 0)
        assert np.array_equal(x["xyz"], w["xyz"]) and np.array_equal(x["pq"], w["pq"]) and np.abs(x["T"] - w["T_kf_w"]).max() <= 64 * LR.U * np.abs(w["T_kf_w"]).max()


def test_larger_windows_meet_the_conditions_of_the_gpu_tests(pkg):
    """(i)-(iii) on the two windows only the device runs (the oracle's dense N^2 does not fit): the seeds are chosen here, without a GPU"""
    for name, w in (("257 blocks", LC.blocks_257()), ("K=20", pkg.window.make_visual_window(K=20, Np=6000, Nl=1200, n_fixed=2, seed=21))):
        r64, rw = _pair(w)
        for k in (1, 2, 3, None):
            LR.hold(LR.at(r64, k), LR.at(r64, k), LR.at(rw, k), "fp64 reference", "%s %s passes" % (name, k or "all"))
