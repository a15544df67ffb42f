"""Reference of the loop-closure verification step, MapHandler::computeRelativePoseRobustGN / computeRelativePoseGN (numpy only).

Written from the reference's text, not from csrc/plba_relpose_dev.h:
    src/mapHandler.cpp:3411-3673     computeRelativePoseGN        (protocol 1: one stage, outlier cut, lc_inl applied)
    src/mapHandler.cpp:3675-4066     computeRelativePoseRobustGN  (protocol 0: stage, cut, refinement; err_prev carried over; lc_inl forced)
    stvo-pl/src/auxiliar.cpp:113-173 inverse_se3 / expmap_se3 / logmap_se3 (tests/lba_ref.py),  :556-559 robustWeightCauchy
    stvo-pl/src/pinholeStereoCamera.cpp:239-245 projection
The 6 x 6 solve restates the documented algorithm of Eigen's ColPivHouseholderQR: Householder QR with column pivoting by
the largest remaining column norm, rank = pivots above eps 6 |largest pivot|, zeros for the deficient part of the solution.

Every function takes a working type `dt` as tests/lba_ref.py does: np.float64, np.longdouble or "mp" (lba_ref.wide() names the wide one).
The thresholds of the text (numeric_limits<double>::epsilon(), sqrt(7.815), the lc_* values) are the same doubles in every type.

run() returns the outputs of plba_relative_pose as doubles plus, for the tolerance rule, `checks`: every comparison the control and the
decisions made, as (label, value in the working type, threshold, taken).
"""
import numpy as np

from . import lba_ref as LR
from .lba_ref import cast, f64, se3_exp, se3_inv, se3_log, _b, _clamp, _mm, _mv, _prec, _project, _sqrt, _zeros

U = LR.U
EPS = float(np.finfo(np.float64).eps)
OK, EMPTY, NONFINITE, RANK = 0, 1, 2, 3
DEFAULTS = dict(max_iters=5, max_iters_ref=10, homog_th=1e-7, chi2_th=7.815, protocol=0, lc_res=1.0, lc_unc=0.01, lc_inl=0.3, lc_trs=1.5, lc_rot=35.0)
FACTOR, MARGIN = LR.FACTOR, LR.MARGIN


def _s(v):
    return _sqrt(np.asarray(v))[()]


# ---- the observations (:3444-3475, :3484-3533) ------------------------------------------------------------------------------------------
def _jac6(g, a, b, fx, th):
    gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
    f = fx / _clamp(gz * gz, th)
    return np.stack([f * a * gz, f * b * gz, -f * (gx * a + gy * b), -f * (gx * gy * a + gy * gy * b + gz * gz * b),
                     f * (gx * gx * a + gz * gz * a + gx * gy * b), f * (gx * gz * b - gy * gz * a)], -1)


def point_err(cam, R, t, P, uv):
    g = _mv(R, P) + t
    pu, pv = _project(cam, g)
    dx, dy = pu - uv[..., 0], pv - uv[..., 1]
    return g, dx, dy, _sqrt(dx * dx + dy * dy)


def point_obs(cam, th, R, t, P, uv):
    """(n, J_aux[.., 6]) of :3444-3464"""
    g, dx, dy, n = point_err(cam, R, t, P, uv)
    return n, _jac6(g, dx, dy, cam[0], th) / _clamp(n, th)[..., None]


def line_err(cam, R, t, PQ, l3):
    gs, ge = _mv(R, PQ[..., :3]) + t, _mv(R, PQ[..., 3:]) + t
    su, sv = _project(cam, gs)
    eu, ev = _project(cam, ge)
    ds = l3[..., 0] * su + l3[..., 1] * sv + l3[..., 2]
    de = l3[..., 0] * eu + l3[..., 1] * ev + l3[..., 2]
    return gs, ge, ds, de, _sqrt(ds * ds + de * de)


def line_obs(cam, th, R, t, PQ, l3):
    """(n, J_aux[.., 6]) of :3484-3525"""
    gs, ge, ds, de, n = line_err(cam, R, t, PQ, l3)
    Js, Je = _jac6(gs, l3[..., 0], l3[..., 1], cam[0], th), _jac6(ge, l3[..., 0], l3[..., 1], cam[0], th)
    return n, (Js * ds[..., None] + Je * de[..., None]) / _clamp(n, th)[..., None]


# ---- ColPivHouseholderQR, by its documented algorithm -----------------------------------------------------------------------------------
def qr_solve(H, g, dt):
    """(x, rank, |pivots|) of H x = g"""
    A, c = H.copy(), g.copy()
    n = A.shape[0]
    perm, piv = list(range(n)), []
    for k in range(n):
        norms = [(A[k:, j] * A[k:, j]).sum() for j in range(k, n)]
        j = max(range(k, n), key=lambda q: (norms[q - k], -q))      # the first of the largest
        if j != k:
            A[:, [k, j]] = A[:, [j, k]]
            perm[k], perm[j] = perm[j], perm[k]
        x = A[k:, k]
        nx = _s((x * x).sum())
        if not _b(nx > 0):
            piv.append(nx * 0)
            continue
        alpha = -nx if _b(x[0] >= 0) else nx
        v = x.copy(); v[0] = v[0] - alpha
        beta = 2 / (v * v).sum()
        A[k:, k:] = A[k:, k:] - v[:, None] * (beta * (v[:, None] * A[k:, k:]).sum(0))[None, :]
        c[k:] = c[k:] - v * (beta * (v * c[k:]).sum())
        piv.append(abs(alpha))
    big = max(piv)
    thr = EPS * n * big
    rank = int(sum(1 for p in piv if _b(p > thr)))
    y = _zeros(n, dt)
    for i in range(rank - 1, -1, -1):
        y[i] = (c[i] - (A[i, i + 1:rank] * y[i + 1:rank]).sum()) / A[i, i]
    x = _zeros(n, dt)
    for i in range(rank):
        x[perm[i]] = y[i]
    return x, rank, piv


def sym_eig(A, dt, sweeps=12):
    """eigenvalues (ascending) of a symmetric matrix by cyclic Jacobi with a fixed number of sweeps"""
    A = A.copy()
    n = A.shape[0]
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                if not _b(abs(A[p, q]) > 0):
                    continue
                th = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = (1 if _b(th >= 0) else -1) / (abs(th) + _s(th * th + 1))
                c = 1 / _s(t * t + 1); s = t * c
                Ap, Aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
                Ap, Aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * Ap - s * Aq, s * Ap + c * Aq
    d = np.array([A[i, i] for i in range(n)], dtype=A.dtype)
    return d[np.argsort(f64(d), kind="stable")]


# ---- the protocol -----------------------------------------------------------------------------------------------------------------------
def run(case, dt=np.float64, **opts):
    """case: dict(P3 (Np, 3), uv (Np, 2), pq (Nl, 6), l3 (Nl, 3), cam (fx, fy, cx, cy)[, T0 (4, 4), pt_in (Np,), ln_in (Nl,)])"""
    o = dict(DEFAULTS); o.update(opts)
    with _prec(dt), np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = lambda v: cast(v, dt)[()]
        cam = [c(v) for v in case["cam"]]
        th = c(o["homog_th"])
        P, uv = cast(np.asarray(case["P3"], np.float64).reshape(-1, 3), dt), cast(np.asarray(case["uv"], np.float64).reshape(-1, 2), dt)
        PQ, l3 = cast(np.asarray(case["pq"], np.float64).reshape(-1, 6), dt), cast(np.asarray(case["l3"], np.float64).reshape(-1, 3), dt)
        Np, Nl = len(P), len(PQ)
        pin = np.ones(Np, bool) if case.get("pt_in") is None else np.asarray(case["pt_in"]).astype(bool).copy()
        lin = np.ones(Nl, bool) if case.get("ln_in") is None else np.asarray(case["ln_in"]).astype(bool).copy()
        T0 = np.eye(4) if case.get("T0") is None else np.asarray(case["T0"], np.float64).reshape(4, 4)
        R, t = cast(T0[:3, :3], dt), cast(T0[:3, 3], dt)
        H, g, e = _zeros((6, 6), dt), _zeros(6, dt), c(0.0)
        err_prev = c(999999999.9)
        eps, cut = c(EPS), _s(c(o["chi2_th"]))
        checks, iters, status, n_feat = [], [0, 0], OK, 0

        def check(label, value, thr, m=64):
            taken = bool(_b(value < thr))
            checks.append((label, value, float(thr), taken, m))
            return taken

        def a_pass():
            n_p, J_p = point_obs(cam, th, R, t, P[pin], uv[pin])
            n_l, J_l = line_obs(cam, th, R, t, PQ[lin], l3[lin])
            n, J = np.concatenate([n_p, n_l]), np.concatenate([J_p, J_l])
            w = 1 / (1 + n * n)                                            # robustWeightCauchy
            Hs = (J[:, :, None] * J[:, None, :] * w[:, None, None]).sum(0)
            gs = (J * (n * w)[:, None]).sum(0)
            return Hs, gs, (n * n * w).sum() / len(n), len(n)

        def a_cut():
            _, _, _, n = point_err(cam, R, t, P[pin], uv[pin])
            for i, v in zip(np.flatnonzero(pin), n):
                if not check("cut", -v, -cut, 8):       # err_i.norm() > sqrt(7.815)
                    continue
                pin[i] = False
            _, _, _, _, n = line_err(cam, R, t, PQ[lin], l3[lin])
            for i, v in zip(np.flatnonzero(lin), n):
                if not check("cut", -v, -cut, 8):
                    continue
                lin[i] = False

        stages = (o["max_iters"], o["max_iters_ref"]) if o["protocol"] == 0 else (o["max_iters"],)
        for st, lim in enumerate(stages):
            if pin.sum() + lin.sum() == 0:
                status = EMPTY
                break
            for _ in range(lim):
                H, g, e, n_feat = a_pass()
                iters[st] += 1
                if not np.isfinite(float(e)):
                    status = NONFINITE
                    break
                if check("de", abs(e - err_prev), eps, n_feat) | check("e", e, eps, n_feat):
                    break
                x, _, _ = qr_solve(H, g, dt)
                Rd, td = se3_inv(*se3_exp(x, dt))
                R, t = _mm(R, Rd), _mv(R, td) + t
                if check("dx", _s((x * x).sum()), eps):
                    break
                err_prev = e
            if status != OK:
                break
            if st == 0:
                a_cut()
        n_inl = int(pin.sum() + lin.sum())
        res = dict(status=status, iters=list(iters), n_inliers=n_inl, pt_in=pin.copy(), ln_in=lin.copy(), checks=checks, n_feat=max(n_feat, 1))
        T = np.eye(4); T[:3, :3] = f64(R); T[:3, 3] = f64(t)
        res.update(T=T, H=f64(H), e=float(e))
        bits = dict(lc_res=0, lc_unc=0, lc_inl=0, lc_trs=0, lc_rot=0)
        res.update(pose_inc=np.zeros(6), cov_eig=np.full(6, np.inf), t=0.0, r=0.0)
        if status == OK:
            x = se3_log(R, t, dt)
            if o["protocol"] == 0:
                pose = se3_log(*se3_inv(*se3_exp(x, dt)), dt)               # :4060
            else:
                pose = se3_log(*se3_inv(R, t), dt)                         # :3667
            tn, rn = _s((x[:3] * x[:3]).sum()), _s((x[3:] * x[3:]).sum()) * c(180.0) / c(np.pi)
            res.update(pose_inc=f64(pose), t=float(tn), r=float(rn))
            bits["lc_res"] = int(check("lc_res", e, o["lc_res"], n_feat))
            _, rank, _ = qr_solve(H, g * 0, dt)
            if rank < 6:
                res["status"] = RANK
            else:
                ev = sym_eig(H, dt)
                cov = (1 / ev)[::-1]
                res["cov_eig"] = f64(cov)
                bits["lc_unc"] = int(check("lc_unc", cov[5], o["lc_unc"], n_feat))
            N = Np + Nl
            bits["lc_inl"] = 1 if o["protocol"] == 0 else int(check("lc_inl", -(c(n_inl) / c(max(N, 1))), -o["lc_inl"]))      # ratio > lcInl
            bits["lc_trs"] = int(check("lc_trs", tn, o["lc_trs"]))
            bits["lc_rot"] = int(check("lc_rot", rn, o["lc_rot"]))
        res.update(bits)
        res["accepted"] = int(res["status"] == OK and all(bits.values()))
        return res


# ---- the tolerance rule (lba_ref.hold's, for this entry's outputs) ----------------------------------------------------------------------
QUANT = ("T", "pose_inc", "H", "e", "cov_eig")
EXACT = ("status", "iters", "n_inliers", "accepted", "lc_res", "lc_unc", "lc_inl", "lc_trs", "lc_rot")


def tolerances(r64, rw):
    """per quantity max(8 noise, m u |value|): noise = |fp64 run - wide run| of this reference in the maximum norm of the quantity,
    m = the inlier features of the last pass (the terms of its sums)"""
    tol, noise = {}, {}
    m = max(64, rw["n_feat"])
    for k in QUANT:
        a, b = np.asarray(r64[k], np.float64), np.asarray(rw[k], np.float64)
        if not np.isfinite(b).all():
            continue
        noise[k] = float(np.abs(a - b).max())
        tol[k] = max(FACTOR * noise[k], m * U * float(np.abs(b).max()))
    return tol, noise


def decisions_have_margin(r64, rw):
    """every comparison of the wide run (exit tests, the cut, the decisions) lies MARGIN x the noise of the compared quantity away from
    its threshold, and the fp64 run made the same comparisons with the same outcome; returns the smallest margin / noise ratio"""
    if len(r64["checks"]) != len(rw["checks"]):
        return 0.0
    worst = np.inf
    for (l6, v6, t6, k6, _), (lw, vw, tw, kw, m) in zip(r64["checks"], rw["checks"]):
        if l6 != lw or k6 != kw:
            return 0.0
        v, v6 = float(vw), float(v6)
        if not np.isfinite(v):
            continue
        noise = max(abs(v - v6), m * U * abs(v))
        worst = min(worst, abs(v - tw) / noise if noise > 0 else np.inf)
    return worst


def hold(res, r64, rw, who, name, exact=True):
    """the reference's own conditions, then every output of `res` against the wide run; prints each figure before it asserts"""
    tol, noise = tolerances(r64, rw)
    if exact:
        margin = decisions_have_margin(r64, rw)
        print("%s %s: smallest decision margin / noise %.3g" % (who, name, margin))
        assert margin >= MARGIN, (name, margin)
        for k in EXACT:
            assert np.array_equal(np.asarray(res[k]), np.asarray(rw[k])) and np.array_equal(np.asarray(r64[k]), np.asarray(rw[k])), (name, k, res[k], rw[k], r64[k])
        assert np.array_equal(res["pt_in"], rw["pt_in"]) and np.array_equal(res["ln_in"], rw["ln_in"]), name
    bad = []
    for k in QUANT:
        a, b = np.asarray(res[k], np.float64), np.asarray(rw[k], np.float64)
        if k not in tol:
            assert np.array_equal(a, b) or (np.isnan(a) == np.isnan(b)).all(), (who, name, k, a, b)
            continue
        e = float(np.abs(a - b).max())
        print("%s %s %-8s error %.3e  noise %.3e  tolerance %.3e  error/noise %.2f" % (who, name, k, e, noise[k], tol[k], e / noise[k] if noise[k] > 0 else np.inf if e > 0 else 0.0))
        if not e <= tol[k]:
            bad.append((k, e, tol[k]))
    assert not bad, (who, name, bad)
