"""Reference of the tracker's pose estimator, StereoFrameHandler::optimizePose, mode 0 (numpy only).

Written from the reference's text, not from csrc/plba_track_dev.h:
    stvo-pl/src/stereoFrameHandler.cpp:319-332   isGoodSolution
    stvo-pl/src/stereoFrameHandler.cpp:334-419   optimizePose (the start pose is given: the motion-model decision is the caller's)
    stvo-pl/src/stereoFrameHandler.cpp:421-458   gaussNewtonOptimization          :460-507  gaussNewtonOptimizationRobust
    stvo-pl/src/stereoFrameHandler.cpp:576-721   optimizeFunctions                :723-989  optimizeFunctionsRobust
    stvo-pl/src/stereoFrameHandler.cpp:1015-1094 removeOutliers
    stvo-pl/src/stereoFrame.cpp:521-627          lineSegmentOverlap
    stvo-pl/src/auxiliar.cpp:387-430, :444-460   vector_mean_stdv_mad, vector_stdv_mad (fabsf: the deviations are rounded to float)
The observation bodies (J_aux), the pivoted QR and the Jacobi eigenvalues are those of tests/relpose_ref.py: the same text.  The
deviations are the ones include/plba.h states: a non-finite e ends the run (NONFINITE); a final H that is rank deficient by the QR's rule
is RANK and not good, a first-stage one is not good; cov_eig are the reciprocals of the eigenvalues of H; a stage with no pass reports
H = 0, e = 0.

Every function takes a working type `dt` as tests/lba_ref.py does.  The rounding of the deviations to float is applied in every type.
run() returns the outputs of plba_track_pose as doubles plus `checks`: every comparison made, as (label, value in the working type,
threshold, taken, terms), including for every float rounding that reaches an output (the MAD) its distance from the rounding boundary.
"""
import numpy as np

from . import lba_ref as LR
from . import relpose_ref as RR
from .lba_ref import cast, f64, se3_exp, se3_inv, se3_log, _b, _elementwise, _mm, _mv, _prec, _project, _sqrt, _zeros

U = LR.U
OK, NONFINITE, RANK = 0, 2, 3
REFINED, ROBUST, FEW_BEFORE, FEW_AFTER = 0, 1, 2, 3
DEFAULTS = dict(max_iters=5, max_iters_ref=10, min_features=10, homog_th=1e-7, min_error=1e-7, min_error_change=1e-7, inlier_k=4.0)
FACTOR, MARGIN = LR.FACTOR, LR.MARGIN
_log = _elementwise("log", np.log)


def _s(v):
    return _sqrt(np.asarray(v))[()]


def to_float(v, dt):
    """fabsf's argument: the value rounded to float, back in the working type"""
    a = np.asarray(v)
    r = np.float32(f64(a)) if a.dtype == object else a.astype(np.float32)
    return cast(r.astype(np.float64), dt)


def float_boundary(x):
    """the float rounding boundary (midpoint of two neighbouring floats) nearest to the double x"""
    f = np.float32(x)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    cands = [(float(f) + float(lo)) / 2, (float(f) + float(hi)) / 2]
    return min(cands, key=lambda c: abs(c - float(x)))


def overlap_of(ls, le, check):      # stereoFrame.cpp:541-553
    lmin, lmax = (ls, le) if _b(ls < le) else (le, ls)
    a, b, c, d = check("lmin<0", lmin, 0.0), check("lmax>1", -lmax, -1.0), check("lmax<0", lmax, 0.0), check("lmin>1", -lmin, -1.0)
    if a and b:
        return lmin * 0 + 1, 0
    if c or d:
        return lmin * 0, 1
    if a:
        return lmax, 2
    if b:
        return 1 - lmin, 3
    return lmax - lmin, 4


def line_overlap(so, eo, sp, ep, check):
    """(overlap, branch 0 vertical / 1 horizontal / 2 general, outcome 0..4) of lineSegmentOverlap(spl_obs, epl_obs, spl_proj, epl_proj)"""
    lx, ly = eo[0] - so[0], eo[1] - so[1]
    if check("vertical", abs(so[0] - eo[0]), 1.0):
        ov, k = overlap_of((sp[1] - so[1]) / ly, (ep[1] - so[1]) / ly, check)
        return ov, 0, k
    if check("horizontal", abs(so[1] - eo[1]), 1.0):
        ov, k = overlap_of((sp[0] - so[0]) / lx, (ep[0] - so[0]) / lx, check)
        return ov, 1, k
    a, b, c = so[1] - eo[1], eo[0] - so[0], so[0] * eo[1] - eo[0] * so[1]
    lxy = 1 / (a * a + b * b)
    sx = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy
    ex = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy
    ov, k = overlap_of((sx - so[0]) / lx, (ex - so[0]) / lx, check)
    return ov, 2, k


def select(v, k):
    """element k of the sorted list"""
    return np.sort(v)[k]


def stdv_mad(v, dt, check):
    """(1.4826 MAD, median) of vector_stdv_mad; 0 for an empty list"""
    n = len(v)
    if n == 0:
        return cast(0.0, dt)[()], cast(0.0, dt)[()]
    med = select(v, n // 2)
    d = v - med
    # rounding to float is monotone, so element n / 2 of the rounded deviations is the rounding of element n / 2 of the deviations: that
    # one rounding is the only one that reaches an output, and the only one whose distance from a rounding boundary is recorded (a
    # deviation of 1e-3 px has float neighbours 1e-10 apart, 1000 x the noise of a residual: no case could keep every deviation clear)
    x = float(f64(select(abs(d), n // 2)))
    check("f32", x, float_boundary(x), 1)
    dev = abs(to_float(d, dt))
    return cast(1.4826, dt)[()] * select(dev, n // 2), med


def mean_stdv_mad(v, dt, check):
    """(mean, stdv) of vector_mean_stdv_mad (auxiliar.cpp:387-430)"""
    n = len(v)
    stdv, _ = stdv_mad(v, dt, check)
    best = np.array([check("best", x, 2 * stdv, 1) for x in v], bool)
    if best.sum() >= int(0.2 * n):
        return v[best].sum() / int(best.sum()), stdv
    return v.sum() / n, stdv


def run(case, dt=np.float64, **opts):
    """case: dict(P3 (Np, 3), uv (Np, 2), pt_s2 (Np,), pq (Nl, 6), l3 (Nl, 3), se (Nl, 4), ln_s2 (Nl,), cam[, T0 (4, 4), pt_in, ln_in])"""
    o = dict(DEFAULTS); o.update(opts)
    with _prec(dt), np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = lambda v: cast(v, dt)[()]
        cam = [c(v) for v in case["cam"]]
        th = c(o["homog_th"])
        arr = lambda k, wd: cast(np.asarray(case[k], np.float64).reshape((-1, wd) if wd else (-1,)), dt)
        P, uv, s2p, PQ, l3, SE, s2l = arr("P3", 3), arr("uv", 2), arr("pt_s2", 0), arr("pq", 6), arr("l3", 3), arr("se", 4), arr("ln_s2", 0)
        Np, Nl = len(P), len(PQ)
        pin = np.ones(Np, bool) if case.get("pt_in") is None else np.asarray(case["pt_in"]).astype(bool).copy()
        lin = np.ones(Nl, bool) if case.get("ln_in") is None else np.asarray(case["ln_in"]).astype(bool).copy()
        T0 = np.eye(4) if case.get("T0") is None else np.asarray(case["T0"], np.float64).reshape(4, 4)
        R0, t0 = cast(T0[:3, :3], dt), cast(T0[:3, 3], dt)
        me, mec = o["min_error"], o["min_error_change"]
        checks, iters, exits = [], [0, 0, 0], []
        branches, outcomes = set(), set()
        st = dict(n_feat=1)

        def check(label, value, thr, m=None):
            taken = bool(_b(value < thr))
            checks.append((label, value, float(thr), taken, st["n_feat"] if m is None else m))
            return taken

        def residuals(R, t, scaled, pm, lm):
            """|err| (sqrt(sigma2)) of the selected points and lines"""
            _, _, _, n_p = RR.point_err(cam, R, t, P[pm], uv[pm])
            _, _, _, _, n_l = RR.line_err(cam, R, t, PQ[lm], l3[lm])
            return (n_p * _sqrt(s2p[pm]), n_l * _sqrt(s2l[lm])) if scaled else (n_p, n_l)

        def a_pass(R, t, robust):
            n_p, J_p = RR.point_obs(cam, th, R, t, P[pin], uv[pin])
            n_l, J_l = RR.line_obs(cam, th, R, t, PQ[lin], l3[lin])
            st["n_feat"] = max(len(n_p) + len(n_l), 1)
            if robust:
                r_p, r_l = n_p, n_l
                s = []
                for v in (r_p, r_l):
                    sk = stdv_mad(v, dt, check)[0]
                    if check("s<min", sk, 0.0001, 1):
                        sk = c(0.0001)
                    if check("s>max", -sk, -np.sqrt(7.815), 1):
                        sk = c(np.sqrt(7.815))
                    s.append(sk)
                x_p, x_l = r_p / s[0], r_l / s[1]
            else:
                r_p, r_l = n_p * _sqrt(s2p[pin]), n_l * _sqrt(s2l[lin])
                x_p, x_l = r_p, r_l
            w_p, w_l = 1 / (1 + x_p * x_p), 1 / (1 + x_l * x_l)
            if len(n_l):
                gs, ge = _mv(R, PQ[lin][:, :3]) + t, _mv(R, PQ[lin][:, 3:]) + t
                su, sv = _project(cam, gs)
                eu, ev = _project(cam, ge)
                ov = []
                for i, se in enumerate(SE[lin]):
                    v, br, k = line_overlap(se[:2], se[2:], (su[i], sv[i]), (eu[i], ev[i]), lambda a, b, d: check(a, b, d, 1))
                    branches.add(br); outcomes.add(k)
                    ov.append(v)
                w_l = w_l * np.array(ov, dtype=w_l.dtype)
            r, J, w = np.concatenate([r_p, r_l]), np.concatenate([J_p, J_l]), np.concatenate([w_p, w_l])
            H = (J[:, :, None] * J[:, None, :] * w[:, None, None]).sum(0)
            g = (J * (r * w)[:, None]).sum(0)
            return H, g, (r * r * w).sum() / len(r)

        def step(R, t, x):
            Rd, td = se3_inv(*se3_exp(x, dt))
            return _mm(R, Rd), _mv(R, td) + t

        def gn(R, t, lim, stage):
            """gaussNewtonOptimization: (R, t, H, err_, how); how: 'ok', 'minus1' (:435) or 'nonfinite'"""
            H, e, err_prev = _zeros((6, 6), dt), c(0.0), c(999999999.9)
            why = "limit"
            for it in range(lim):
                H, g, e = a_pass(R, t, False)
                iters[stage] += 1
                if not np.isfinite(float(e)):
                    return R, t, H, e, "nonfinite"
                if check("gt", -e, -err_prev):
                    if it > 0:
                        why = "gt"
                        break
                    exits.append((stage, "minus1"))
                    return R, t, H, c(-1.0), "minus1"
                if check("e", e, me) | check("de", abs(e - err_prev), mec):
                    why = "small"
                    break
                x, _, _ = RR.qr_solve(H, g, dt)
                R, t = step(R, t, x)
                if check("dxt", _s((x[:3] * x[:3]).sum()), mec, 1) & check("dxr", _s((x[3:] * x[3:]).sum()), mec, 1):
                    why = "step"
                    break
                err_prev = e
            exits.append((stage, why))
            return R, t, H, e, "ok"

        def gnr(R, t, lim):
            """gaussNewtonOptimizationRobust: (R, t, H, err_, how); how: 'ok', 'negdet' (:502-504) or 'nonfinite'"""
            Rs, ts = R, t
            H, e, err_prev = _zeros((6, 6), dt), c(0.0), c(999999999.9)
            why = "limit"
            for it in range(lim):
                H, g, e = a_pass(R, t, True)
                iters[2] += 1
                if not np.isfinite(float(e)):
                    return R, t, H, e, "nonfinite"
                if check("de", abs(e - err_prev), mec) | check("e", e, me):
                    why = "small"
                    break
                x, _, piv = RR.qr_solve(H, g, dt)
                if any(not _b(p > 0) for p in piv):
                    lad = c(-np.inf)
                else:
                    lad = sum(_log(np.asarray(p))[()] for p in piv)
                if check("lad", lad, 0.0):
                    exits.append((2, "negdet"))
                    return Rs, ts, H, c(-1.0), "negdet"
                R, t = step(R, t, x)
                if check("dx", _s((x * x).sum()), mec, 1):
                    why = "step"
                    break
                err_prev = e
            exits.append((2, why))
            return R, t, H, e, "ok"

        def is_good(H, err, R, t):
            """(verdict, cov_eig): verdict 1 good, 0 not good, -1 H rank deficient"""
            _, rank, _ = RR.qr_solve(H, H[0] * 0, dt)
            if rank < 6:
                return -1, None
            ev = RR.sym_eig(H, dt)
            ce = (1 / ev)[::-1]
            bad = [check("ce0", ce[0], 0.0), check("ce5", -ce[5], -1.0), check("err<0", err, 0.0), check("err>1", -err, -1.0),
                   not (np.isfinite(f64(R)).all() and np.isfinite(f64(t)).all())]
            return (0 if any(bad) else 1), ce

        def cut(R, t):
            r_p, r_l = residuals(R, t, True, np.ones(Np, bool), np.ones(Nl, bool))
            stat = [c(0.0)] * 4
            for k, (r, m) in enumerate(((r_p, pin), (r_l, lin))):
                if len(r) == 0:
                    continue
                mean, stdv = mean_stdv_mad(r, dt, check)
                stat[2 * k], stat[2 * k + 1] = mean, stdv
                thr = c(o["inlier_k"]) * stdv
                for i in np.flatnonzero(m):
                    if check("cut", -abs(r[i] - mean), -thr, 1):
                        m[i] = False
            return stat

        status, path, negdet = OK, REFINED, False
        R, t = R0, t0
        H, err = _zeros((6, 6), dt), c(-1.0)
        stat = [c(0.0)] * 4
        started_from = None
        if pin.sum() + lin.sum() < o["min_features"]:
            path = FEW_BEFORE
            R, t = cast(np.eye(3), dt), cast(np.zeros(3), dt)
        else:
            R1, t1, H, err, how = gn(R0, t0, o["max_iters"], 0)
            if how == "nonfinite":
                status = NONFINITE
                R, t = R1, t1
            elif how == "ok" and is_good(H, err, R1, t1)[0] == 1:
                stat = cut(R1, t1)
                if pin.sum() + lin.sum() >= o["min_features"]:
                    started_from = f64(R0), f64(t0)
                    R, t, H2, err2, how = gn(R0, t0, o["max_iters_ref"], 1)      # :374: from DT, not DT_
                    H = H2                                                       # (after :435, DT_cov stays the first stage's: never used)
                    err = err2
                    if how == "nonfinite":
                        status = NONFINITE
                else:
                    path = FEW_AFTER
                    R, t = cast(np.eye(3), dt), cast(np.zeros(3), dt)
            else:
                path = ROBUST
                R, t, H, err, how = gnr(R0, t0, o["max_iters_ref"])
                negdet = how == "negdet"
                if how == "nonfinite":
                    status = NONFINITE
        good, cov_eig = 0, np.zeros(6)
        cov = np.zeros((6, 6))
        if negdet:
            cov = np.eye(6)
        elif status == OK and path != FEW_BEFORE:
            v, ce = is_good(H, err, R, t)
            if v < 0:
                status = RANK
            else:
                cov = f64(np.stack([RR.qr_solve(H, cast(np.eye(6)[j], dt), dt)[0] for j in range(6)], -1))
                if v == 1 and not (np.array_equal(f64(R), np.eye(3)) and np.array_equal(f64(t), np.zeros(3))):
                    good, cov_eig = 1, f64(ce)
        T = np.eye(4); T[:3, :3] = f64(R); T[:3, 3] = f64(t)
        DT = np.eye(4)
        if good:
            Rd, td = se3_exp(se3_log(*se3_inv(R, t), dt), dt)
            DT[:3, :3] = f64(Rd); DT[:3, 3] = f64(td)
        return dict(DT=DT, T_opt=T, H=f64(H), cov=cov, cov_eig=cov_eig, err=float(err) if good else -1.0,
                    pt_mean=float(stat[0]), pt_stdv=float(stat[1]), ln_mean=float(stat[2]), ln_stdv=float(stat[3]),
                    n_inliers_pt=int(pin.sum()), n_inliers_ln=int(lin.sum()), iters=list(iters), path=path, status=status, good=good,
                    pt_in=pin.copy(), ln_in=lin.copy(), checks=checks, n_feat=st["n_feat"], exits=exits, branches=branches, outcomes=outcomes,
                    started_from=started_from)


# ---- the tolerance rule (lba_ref.hold's, for this entry's outputs) ----------------------------------------------------------------------
QUANT = ("DT", "T_opt", "H", "cov", "cov_eig", "err", "pt_mean", "pt_stdv", "ln_mean", "ln_stdv")
EXACT = ("status", "path", "good", "iters", "n_inliers_pt", "n_inliers_ln")


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
    """every comparison of the wide run lies MARGIN x the noise of the compared quantity away from its threshold, and the fp64 run made
    the same comparisons with the same outcome; returns the smallest margin / noise ratio"""
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
