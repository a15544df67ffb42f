"""Reference of plba_track_inertial: the motion-only visual-inertial optimisation of two consecutive states (numpy only).

Written from the issue's statement of the graph and the protocol (include/plba.h repeats it) and from the reference's text, not from
csrc/plba_vitrack_dev.h or csrc/plba_math.h:
    IMU/NavState.cpp:69-121          IncSmallPVR / IncSmallBias (IncSmall is the two in turn)
    IMU/g2otypes.cpp:458-526         EdgeNavStatePrior: computeError, linearizeOplus
    IMU/g2otypes.cpp:849-1093        EdgeNavState: computeError, linearizeOplus
    IMU/g2otypes.h:617-690, .cpp:1162-1212   EdgeNavStatePointXYZOnlyPose
    IMU/g2otypes.cpp:1306-1359       EdgeNavStateLine's two rows, the line held; the position block is the true derivative under IncSmall
    IMU/so3.cpp:32-89, 199-280       JacobianR, JacobianRInv, log, exp
    g2o OptimizationAlgorithmLevenberg::solve as SURVEY App. A.2 / A.3 restate it; RobustKernelHuber

Every function takes a working type `dt` as tests/lba_ref.py does (np.float64, np.longdouble or "mp").  run() returns the outputs of
plba_track_inertial as doubles plus `checks`: every decision made — a trial's accept / reject (the sign of rho, which is also the loop's
rho < 0 and its rho == 0), every gate comparison, every depth sign, every Cholesky pivot's sign — as (label, value in the working type,
threshold, taken, terms); qmax is an integer count and has no noise.  The min / max that clamp the damping factor and Huber's two
branches are continuous in their argument and are not decisions.
"""
import numpy as np

from . import lba_ref as LR
from .lba_ref import cast, f64, _b, _elementwise, _inv3, _mm, _mv, _prec, _skew, _sqrt, _sin, _cos, _tr, _zeros

U = LR.U
FACTOR, MARGIN = LR.FACTOR, LR.MARGIN
OK, NONFINITE, SINGULAR = 0, 2, 3
STOP_ITERS, STOP_TRIALS, STOP_RHO0, STOP_LAMBDA, STOP_NONFINITE = range(5)
HUBER = float(np.float32(np.sqrt(5.991)))
DEFAULTS = dict(rounds=4, iters=10, max_trials=10, robust_rounds=2, tau=1e-5, user_lambda_init=0.0, huber_pt=HUBER, huber_ln=HUBER, huber_imu=0.0,
                chi2_pt=5.991, chi2_ln=5.991)
DBL_MAX = float(np.finfo(np.float64).max)
_atan = _elementwise("atan", np.arctan)
VIS_COLS = np.array([0, 1, 2, 6, 7, 8])


def _s(v):
    return _sqrt(np.asarray(v))[()]


def _fin(v):
    return bool(np.isfinite(float(v)))


# ---- quaternions (x, y, z, w) and SO(3), IMU/so3.cpp ----------------------------------------------------------------------------------------
def qnorm(q):
    return q / _s((q * q).sum())


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=a.dtype)


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=q.dtype)


def q2R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=q.dtype)


def R2q(R):      # Eigen's Quaterniond(Matrix3d)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if _b(t > 0):
        r = _s(t + 1)
        return np.array([(R[2, 1] - R[1, 2]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r), (R[1, 0] - R[0, 1]) / (2 * r), r / 2], dtype=R.dtype)
    i = int(np.argmax([float(R[0, 0]), float(R[1, 1]), float(R[2, 2])]))
    j, k = (i + 1) % 3, (i + 2) % 3
    r = _s(R[i, i] - R[j, j] - R[k, k] + 1)
    q = [None] * 4
    q[i] = r / 2
    q[3] = (R[k, j] - R[j, k]) / (2 * r)
    q[j] = (R[j, i] + R[i, j]) / (2 * r)
    q[k] = (R[k, i] + R[i, k]) / (2 * r)
    return np.array(q, dtype=R.dtype)


def so3_exp(w, dt):      # so3.cpp:257-280
    th = _s((w * w).sum())
    if _b(th < 1e-10):
        imag = cast(0.5, dt)[()] - th * th / 48 + th * th * th * th / 3840
    else:
        imag = _sin(np.asarray(th / 2))[()] / th
    return qnorm(np.array([imag * w[0], imag * w[1], imag * w[2], _cos(np.asarray(th / 2))[()]], dtype=w.dtype))


def so3_log(q):      # so3.cpp:206-247
    n = _s((q[:3] * q[:3]).sum())
    w = q[3]
    f = (2 / w - 2 * n * n / (w * w * w)) if _b(n < 1e-10) else 2 * _atan(np.asarray(n / w))[()] / n
    return q[:3] * f


def so3_Jr(w, dt):      # so3.cpp:32-49
    th = _s((w * w).sum())
    I = cast(np.eye(3), dt)
    if _b(th < 0.00001):
        return I
    K = _skew(w / th)
    return I - K * ((1 - _cos(np.asarray(th))[()]) / th) + _mm(K, K) * (1 - _sin(np.asarray(th))[()] / th)


def so3_JrInv(w, dt):      # so3.cpp:50-68
    th = _s((w * w).sum())
    I = cast(np.eye(3), dt)
    if _b(th < 0.00001):
        return I
    K = _skew(w / th)
    return I + _skew(w) / 2 + _mm(K, K) * (1 - (1 + _cos(np.asarray(th))[()]) * th / (2 * _sin(np.asarray(th))[()]))


# ---- the state: 22 numbers P3 V3 q4 bg3 ba3 dbg3 dba3 ------------------------------------------------------------------------------------
def oplus(s, u, dt):      # NavState::IncSmall
    q = qnorm(s[6:10])
    o = s.copy()
    o[0:3] = s[0:3] + _mv(q2R(q), u[0:3])
    o[3:6] = s[3:6] + u[3:6]
    o[6:10] = qnorm(qmul(q, so3_exp(u[6:9], dt)))
    o[16:22] = s[16:22] + u[9:15]
    return o


def imu_error(si, sj, pre, gw, dt):      # g2otypes.cpp:849-919
    qi, qj = qnorm(si[6:10]), qnorm(sj[6:10])
    RiT = _tr(q2R(qi))
    dT = pre[141]
    dbg, dba = si[16:19], si[19:22]
    M = lambda k: pre[k:k + 9].reshape(3, 3)
    rP = _mv(RiT, sj[0:3] - si[0:3] - si[3:6] * dT - gw * (dT * dT / 2)) - (pre[0:3] + _mv(M(15), dbg) + _mv(M(24), dba))
    rV = _mv(RiT, sj[3:6] - si[3:6] - gw * dT) - (pre[3:6] + _mv(M(33), dbg) + _mv(M(42), dba))
    dR = qmul(qnorm(R2q(M(6))), so3_exp(_mv(M(51), dbg), dt))
    rPhi = so3_log(qnorm(qmul(qmul(qconj(qnorm(dR)), qconj(qi)), qj)))
    rbg = (sj[10:13] + sj[16:19]) - (si[10:13] + si[16:19])
    rba = (sj[13:16] + sj[19:22]) - (si[13:16] + si[19:22])
    return np.concatenate([rP, rV, rPhi, rbg, rba])


def imu_jacobians(si, sj, pre, gw, e, dt):      # g2otypes.cpp:936-1093; Get_RotMatrix: the stored rotation
    Ri, Rj = q2R(si[6:10]), q2R(sj[6:10])
    RiT = _tr(Ri)
    dT = pre[141]
    M = lambda k: pre[k:k + 9].reshape(3, 3)
    I = cast(np.eye(3), dt)
    Ji, Jj = _zeros((15, 15), dt), _zeros((15, 15), dt)
    JrInv = so3_JrInv(e[6:9], dt)
    Ji[0:3, 0:3] = -I
    Ji[0:3, 3:6] = -RiT * dT
    Ji[0:3, 6:9] = _skew(_mv(RiT, sj[0:3] - si[0:3] - si[3:6] * dT - gw * (dT * dT / 2)))
    Ji[0:3, 9:12] = -M(15)
    Ji[0:3, 12:15] = -M(24)
    Ji[3:6, 3:6] = -RiT
    Ji[3:6, 6:9] = _skew(_mv(RiT, sj[3:6] - si[3:6] - gw * dT))
    Ji[3:6, 9:12] = -M(33)
    Ji[3:6, 12:15] = -M(42)
    ExpT = q2R(qconj(so3_exp(e[6:9], dt)))
    Ji[6:9, 6:9] = -_mm(JrInv, _mm(_tr(Rj), Ri))
    Ji[6:9, 9:12] = -_mm(_mm(_mm(JrInv, ExpT), so3_Jr(_mv(M(51), si[16:19]), dt)), M(51))
    Ji[9:15, 9:15] = -cast(np.eye(6), dt)
    Jj[0:3, 0:3] = _mm(RiT, Rj)
    Jj[3:6, 3:6] = RiT
    Jj[6:9, 6:9] = JrInv
    Jj[9:15, 9:15] = cast(np.eye(6), dt)
    return Ji, Jj


def prior_error(p, s):      # g2otypes.cpp:458-495
    w = so3_log(qnorm(qmul(qconj(qnorm(p[6:10])), qnorm(s[6:10]))))
    return np.concatenate([p[0:6] - s[0:6], w, (p[10:13] + p[16:19]) - (s[10:13] + s[16:19]), (p[13:16] + p[19:22]) - (s[13:16] + s[19:22])])


def prior_jacobian(s, e, dt):      # g2otypes.cpp:497-526
    J = -cast(np.eye(15), dt)
    J[0:3, 0:3] = -q2R(s[6:10])
    J[6:9, 6:9] = so3_JrInv(e[6:9], dt)
    return J


# ---- the visual edges on j, vectorised over the features -------------------------------------------------------------------------------------
def _cam_points(sj, X, Rcb, Pbc):
    """(Pc, Paux) of world points X (n, 3): Pc = Rcb Rwb^T (Pw - Pwb) - Rcb Pbc"""
    Paux = _mv(_mm(Rcb, _tr(q2R(sj[6:10]))), X - sj[0:3])
    return Paux - _mv(Rcb, Pbc), Paux


def _jpi(cam, Pc):
    """(n, 2, 3): [[fx, 0, -x / z fx], [0, fy, -y / z fy]] / z"""
    x, y, z = Pc[:, 0], Pc[:, 1], Pc[:, 2]
    zero = x * 0
    return np.stack([np.stack([cam[0] / z, zero, -x / z * cam[0] / z], -1), np.stack([zero, cam[1] / z, -y / z * cam[1] / z], -1)], -2)


def point_edges(sj, X, uv, cam, Rcb, Pbc, jac):
    """(e (n, 2), depth z (n,), J (n, 2, 6) over (dP, dPhi) or None)"""
    Pc, Paux = _cam_points(sj, X, Rcb, Pbc)
    e = np.stack([uv[:, 0] - (Pc[:, 0] / Pc[:, 2] * cam[0] + cam[2]), uv[:, 1] - (Pc[:, 1] / Pc[:, 2] * cam[1] + cam[3])], -1)
    if not jac:
        return e, Pc[:, 2], None
    Jpi = _jpi(cam, Pc)
    JdP = _mm(Jpi, Rcb)                              # -Jpi (-Rcb)
    JdR = -_mm(Jpi, _mm(_skew(Paux), Rcb))
    return e, Pc[:, 2], np.concatenate([JdP, JdR], -1)


def line_edges(sj, PQ, l3, cam, Rcb, Pbc, jac):
    """(e (n, 2), the smaller end-point depth (n,), J (n, 2, 6) or None): row k is l . (proj(P_k), 1)"""
    es, Js, zs = [], [], []
    for k in (0, 3):
        Pc, Paux = _cam_points(sj, PQ[:, k:k + 3], Rcb, Pbc)
        es.append(l3[:, 0] * (Pc[:, 0] / Pc[:, 2] * cam[0] + cam[2]) + l3[:, 1] * (Pc[:, 1] / Pc[:, 2] * cam[1] + cam[3]) + l3[:, 2])
        zs.append(Pc[:, 2])
        if jac:
            u = (l3[:, :2, None] * _jpi(cam, Pc)).sum(-2)      # l12^T Jpi, (n, 3)
            Js.append(np.concatenate([-_mv(_tr(Rcb), u), (u[:, :, None] * _mm(_skew(Paux), Rcb)).sum(-2)], -1))
    z = np.where(_b(zs[0] < zs[1]), zs[0], zs[1])
    return np.stack(es, -1), z, (np.stack(Js, -2) if jac else None)


def huber(chi, delta):
    """(rho0, rho1) of g2o's RobustKernelHuber for arrays"""
    d2 = delta * delta
    big = _b(chi > d2)
    s = _sqrt(np.where(big, chi, chi * 0 + 1))
    return np.where(big, 2 * s * delta - d2, chi), np.where(big, delta / s, chi * 0 + 1)


def chol(A, dt, check, label):
    """the lower factor of A by LL^T, column by column, or None at the first pivot that is not > 0"""
    n = A.shape[0]
    L = _zeros((n, n), dt)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not check(label, -d, 0.0):
            return None
        L[j, j] = _s(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - (L[j + 1:, :j] * L[j, :j]).sum(-1)) / L[j, j]
    return L


def lower_solve(L, B, dt):
    """L^-1 B for a matrix or a vector B"""
    Y = _zeros(B.shape, dt)
    for k in range(L.shape[0]):
        Y[k] = (B[k] - (L[k, :k].reshape((-1,) + (1,) * (B.ndim - 1)) * Y[:k]).sum(0)) / L[k, k]
    return Y


def upper_solve(L, y, dt):
    """L^-T y"""
    n = L.shape[0]
    x = _zeros(y.shape, dt)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - (L[k + 1:, k] * x[k + 1:]).sum()) / L[k, k]
    return x


def run(case, dt=np.float64, **opts):
    """case: dict(anchor_free, si, sj (22), pre (142), ipvr (9, 9), ibias (6, 6), [pst (22), pinfo (15, 15)], gw (3), cam (4), Rbc (3, 3), Pbc (3),
    Pw (Np, 3), uv (Np, 2), pt_w (Np,), pq (Nl, 6), l3 (Nl, 3), ln_w (Nl,)[, pt_in, ln_in])"""
    o = dict(DEFAULTS); o.update(opts)
    with _prec(dt), np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = lambda v: cast(v, dt)[()]
        arr = lambda k, shape: cast(np.asarray(case[k], np.float64).reshape(shape), dt)
        cam = [c(v) for v in case["cam"]]
        Rcb, Pbc, gw = _tr(arr("Rbc", (3, 3))), arr("Pbc", (3,)), arr("gw", (3,))
        X, uv, wp, PQ, l3, wl = arr("Pw", (-1, 3)), arr("uv", (-1, 2)), arr("pt_w", (-1,)), arr("pq", (-1, 6)), arr("l3", (-1, 3)), arr("ln_w", (-1,))
        Np, Nl = len(X), len(PQ)
        pin = np.ones(Np, bool) if case.get("pt_in") is None else np.asarray(case["pt_in"]).astype(bool).copy()
        lin = np.ones(Nl, bool) if case.get("ln_in") is None else np.asarray(case["ln_in"]).astype(bool).copy()
        free = bool(case["anchor_free"])
        si, sj, pre = arr("si", (22,)), arr("sj", (22,)), arr("pre", (142,))
        Om = _zeros((15, 15), dt)
        Om[:9, :9] = arr("ipvr", (9, 9)); Om[9:, 9:] = arr("ibias", (6, 6))
        if free:
            pst, Op = arr("pst", (22,)), arr("pinfo", (15, 15))
        o0 = 0 if free else 15
        hp, hl, hi = c(o["huber_pt"]), c(o["huber_ln"]), c(o["huber_imu"])
        checks = []
        st = dict(n_feat=1)
        events = dict(rejected=0, dropped=0, readmitted=0, accepted=0)

        def check(label, value, thr, m=None):
            taken = bool(_b(value < thr))
            checks.append((label, value, float(thr), taken, st["n_feat"] if m is None else m))
            return taken

        def edge_chi(e, Omega):      # g2o's chi2(): sum_i e_i (Omega e)_i
            return (e * _mv(Omega, e)).sum()

        def system(si, sj, robust, jac):
            """(chi2, H 30 x 30, b 30) of the active edges; H, b None without jac"""
            st["n_feat"] = max(int(pin.sum() + lin.sum()), 1)
            H, b = (_zeros((30, 30), dt), _zeros((30,), dt)) if jac else (None, None)
            chi = c(0.0)
            for kind, (edges, sel, w, delta) in enumerate(((lambda: point_edges(sj, X[pin], uv[pin], cam, Rcb, Pbc, jac), pin, wp, hp),
                                                           (lambda: line_edges(sj, PQ[lin], l3[lin], cam, Rcb, Pbc, jac), lin, wl, hl))):
                if not sel.any():
                    continue
                e, _, J = edges()
                ch = w[sel] * (e * e).sum(-1)
                rho0, rho1 = huber(ch, delta) if robust else (ch, ch * 0 + 1)
                chi = chi + rho0.sum()
                if jac:
                    wt = rho1 * w[sel]
                    cols = 15 + VIS_COLS
                    H[np.ix_(cols, cols)] += (J[:, :, :, None] * J[:, :, None, :] * wt[:, None, None, None]).sum((0, 1))
                    b[cols] -= (J * (e * wt[:, None])[:, :, None]).sum((0, 1))
            e = imu_error(si, sj, pre, gw, dt)
            ci = edge_chi(e, Om)
            wi = c(1.0)
            if o["huber_imu"] > 0:
                r0, r1 = huber(np.asarray(ci), hi)
                ci, wi = r0[()], r1[()]
            chi = chi + ci
            if jac:
                Ji, Jj = imu_jacobians(si, sj, pre, gw, e, dt)
                J = np.concatenate([Ji, Jj], -1)
                H += _mm(_tr(J), _mm(Om, J)) * wi
                b -= _mv(_tr(J), _mv(Om, e)) * wi
            if free:
                e = prior_error(pst, si)
                chi = chi + edge_chi(e, Op)
                if jac:
                    J = prior_jacobian(si, e, dt)
                    H[:15, :15] += _mm(_tr(J), _mm(Op, J))
                    b[:15] -= _mv(_tr(J), _mv(Op, e))
            if jac:
                H[:o0] = 0; H[:, :o0] = 0; b[:o0] = 0
                H = (H + _tr(H)) / 2
            return chi, H, b

        def gate(sj):
            for kind, (e, z, w, th, m) in enumerate(((point_edges(sj, X, uv, cam, Rcb, Pbc, False)[:2] + (wp, o["chi2_pt"], pin)),
                                                     (line_edges(sj, PQ, l3, cam, Rcb, Pbc, False)[:2] + (wl, o["chi2_ln"], lin)))):
                ch = w * (e * e).sum(-1)
                for i in range(len(ch)):
                    over = check("gate", -ch[i], -th, 1)
                    front = check("depth", -z[i], 0.0, 1)
                    new = (not over) and front
                    if m[i] and not new:
                        events["dropped"] += 1
                    if new and not m[i]:
                        events["readmitted"] += 1
                    m[i] = new

        status, trials, failures = OK, 0, 0
        iterations, stops = [0] * 8, [0] * 8
        lam = c(0.0)
        chi_initial, _, _ = system(si, sj, 0 < o["robust_rounds"], False)
        chi_final = chi_initial
        if not _fin(chi_initial):
            status = NONFINITE
        for r in range(o["rounds"]):
            if status != OK:
                break
            robust = r < o["robust_rounds"]
            ni = c(2.0)
            done, stop = 0, STOP_ITERS
            for it in range(o["iters"]):
                chi, H, b = system(si, sj, robust, True)
                if not _fin(chi):
                    status, stop, chi_final = NONFINITE, STOP_NONFINITE, chi
                    break
                if it == 0:
                    lam = c(o["user_lambda_init"]) if o["user_lambda_init"] > 0 else c(o["tau"]) * abs(np.diagonal(H)[o0:]).max()
                    ni = c(2.0)
                rho, qmax = c(0.0), 0
                while True:
                    A = H[o0:, o0:].copy()
                    k = np.arange(30 - o0)
                    A[k, k] = A[k, k] + lam
                    L = chol(A, dt, check, "pivot")
                    x = _zeros((30,), dt)
                    temp = c(DBL_MAX)
                    if L is None:
                        failures += 1
                    else:
                        x[o0:] = upper_solve(L, lower_solve(L, b[o0:], dt), dt)
                        ci_, cj_ = (oplus(si, x[:15], dt) if free else si), oplus(sj, x[15:], dt)
                        temp, _, _ = system(ci_, cj_, robust, False)
                    scale = c(1e-3) + (x * (lam * x + b)).sum()
                    rho = (chi - temp) / scale
                    trials += 1
                    accept = L is not None and check("rho", -rho, 0.0) and _fin(temp)
                    if accept:
                        t = 2 * rho - 1
                        alpha = 1 - t * t * t
                        alpha = alpha if _b(alpha < c(2.0) / 3) else c(2.0) / 3
                        lam = lam * (alpha if _b(alpha > c(1.0) / 3) else c(1.0) / 3)
                        ni = c(2.0)
                        chi, si, sj = temp, ci_, cj_
                        events["accepted"] += 1
                    else:
                        events["rejected"] += 1
                        lam = lam * ni; ni = ni * 2
                        if not _fin(lam):
                            break
                    qmax += 1
                    if not (_b(rho < 0) and qmax < o["max_trials"]):
                        break
                done += 1
                chi_final = chi
                if qmax == o["max_trials"]:
                    stop = STOP_TRIALS
                elif _b(rho == 0):
                    stop = STOP_RHO0
                elif not _fin(lam):
                    stop = STOP_LAMBDA
                if stop != STOP_ITERS:
                    break
            iterations[r], stops[r] = done, stop
            if status == OK:
                gate(sj)
        H30, Onext = np.zeros((30, 30)), np.zeros((15, 15))
        S_out = None
        if status == OK:
            last = max(o["rounds"] - 1, 0)
            chi_final, H, _ = system(si, sj, last < o["robust_rounds"], True)
            if not _fin(chi_final):
                status = NONFINITE
            else:
                H30 = f64(H)
                S = H[15:, 15:]
                ok = True
                if free:
                    L = chol(H[:15, :15], dt, check, "pivot_ii")
                    ok = L is not None
                    if ok:
                        Y = lower_solve(L, H[:15, 15:], dt)
                        S = S - _mm(_tr(Y), Y)
                        S = (S + _tr(S)) / 2
                if ok and chol(S, dt, check, "pivot_S") is not None:
                    D = -cast(np.eye(15), dt)
                    D[0:3, 0:3] = -_inv3(q2R(sj[6:10]))
                    D[6:9, 6:9] = cast(np.eye(3), dt)
                    On = _mm(_tr(D), _mm(S, D))
                    Onext = f64((On + _tr(On)) / 2)
                    S_out = S
                else:
                    status = SINGULAR
        return dict(state_i=f64(si), state_j=f64(sj), H=H30, next_prior=Onext, chi2_initial=float(chi_initial), chi2_final=float(chi_final), lambda_final=float(lam),
                    iterations=iterations, stop_reason=stops, trials=trials, solver_failures=failures, n_inliers_pt=int(pin.sum()), n_inliers_ln=int(lin.sum()),
                    status=status, pt_in=pin.copy(), ln_in=lin.copy(), checks=checks, n_feat=max(int(pin.sum() + lin.sum()), 1), events=events,
                    wide=dict(S=S_out, sj=sj) if S_out is not None else None)


# ---- the tolerance rule (track_ref.hold's, for this entry's outputs) ----------------------------------------------------------------------
QUANT = ("state_i", "state_j", "H", "next_prior", "chi2_initial", "chi2_final", "lambda_final")
EXACT = ("status", "iterations", "stop_reason", "trials", "solver_failures", "n_inliers_pt", "n_inliers_ln")


def tolerances(r64, rw):
    """per quantity max(8 noise, m u |value|): noise = |fp64 run - wide run| of this reference in the maximum norm of the quantity,
    m = the active features of the last pass (the terms of its sums), at least 64"""
    tol, noise = {}, {}
    m = max(64, rw["n_feat"])
    for k in QUANT:
        a, b = np.asarray(r64[k], np.float64), np.asarray(rw[k], np.float64)
        if not np.isfinite(b).all():
            continue
        noise[k] = float(np.abs(a - b).max())
        tol[k] = max(FACTOR * noise[k], m * U * float(np.abs(b).max()))
    return tol, noise


def decisions_have_margin(r64, rw, skip=()):
    """every decision of the wide run lies MARGIN x the noise of the compared quantity away from its threshold, and the fp64 run made the
    same decisions with the same outcome; returns the smallest margin / noise ratio.  `skip`: labels left out (see vitrack_cases.SKIP)."""
    c64 = [k for k in r64["checks"] if k[0] not in skip]
    cw = [k for k in rw["checks"] if k[0] not in skip]
    if len(c64) != len(cw):
        return 0.0
    worst = np.inf
    for (l6, v6, t6, k6, _), (lw, vw, tw, kw, m) in zip(c64, cw):
        if l6 != lw or k6 != kw:
            return 0.0
        v, v6 = float(vw), float(v6)
        if not np.isfinite(v):
            continue
        noise = max(abs(v - v6), m * U * abs(v))
        worst = min(worst, abs(v - tw) / noise if noise > 0 else np.inf)
    return worst


def hold(res, r64, rw, who, name, exact=True, skip=()):
    """the reference's own conditions, then every output of `res` against the wide run; prints each figure before it asserts"""
    tol, noise = tolerances(r64, rw)
    if exact:
        margin = decisions_have_margin(r64, rw, skip)
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
        print("%s %s %-12s error %.3e  noise %.3e  tolerance %.3e  error/noise %.2f" % (who, name, k, e, noise[k], tol[k], e / noise[k] if noise[k] > 0 else np.inf if e > 0 else 0.0))
        if not e <= tol[k]:
            bad.append((k, e, tol[k]))
    assert not bad, (who, name, bad)
