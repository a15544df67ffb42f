"""Extended-precision reference of the pre-init visual-only local BA, MapHandler::levMarquardtOptimizationLBA (numpy only).

Written from the reference's text, not from oracle/plba_oracle.c and not from csrc/plba_lba.hip:
    src/mapHandler.cpp:1490-1512     the point observation: pose row, landmark row
    src/mapHandler.cpp:1565-1622     the line observation (both end points' pieces from fx l_err(0), fy l_err(1), as written)
    src/mapHandler.cpp:1650-1680     the zero-counter division, max |H_ii| and lambda, the damped solve, the update
    src/mapHandler.cpp:1882-1911     the pass-to-pass control
    stvo-pl/src/auxiliar.cpp:113-173 inverse_se3 / expmap_se3 / logmap_se3,   :556-559 robustWeightCauchy
with the decisions DESIGN.md 9 lists for the defects of that text (line end points at stride 6, `use_iterate_poses`, the GBA variant's
`int Hmax` and per-pass zero division, a non-positive pivot ends the run).

Every function takes a working type `dt`: np.float64, np.longdouble, or "mp" (object arrays of mpmath numbers at 40 digits, for machines
whose long double is no wider than a double, as tests/solver_ref.py does): wide() names the one to use.  The arithmetic is written with
element-wise operations and axis sums only, so that all three run the same text.  The pose system of a pass is solved by
solver_ref.refine (fp64 Cholesky + refinement in extended precision) and, in a wide type, corrected against the wide system, so the
step is that of the wide matrix and not of its rounding to double.

The damped step comes in two forms: "dense" assembles the full 6 Nkf + 3 Np + 6 Nl normal equations as the reference does; "elim"
eliminates the landmark blocks in the working type, vectorised over observations (100 k observations take seconds), and solves 6 Nkf.
"""
import contextlib

import numpy as np

from . import solver_ref as SR

U = SR.U
DEFAULTS = dict(lambda_lm=1e-5, lambda_k=10.0, max_iters=15, homog_th=1e-7, min_error=1e-7, min_error_change=1e-7, use_iterate_poses=0, variant=0)


def wide():
    return np.longdouble if SR.LD_IS_EXTENDED else "mp"


@contextlib.contextmanager
def _prec(dt):
    if isinstance(dt, str):
        import mpmath
        with mpmath.workprec(136):      # 40 digits
            yield
    else:
        yield


def cast(a, dt):
    if isinstance(dt, str):
        import mpmath
        a = np.asarray(a)
        if a.dtype == object:
            return a
        out = np.empty(a.shape, object)
        out[...] = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)(a.astype(np.float64))
        return out
    return np.asarray(a, dtype=dt)


def f64(a):
    a = np.asarray(a)
    return np.frompyfunc(float, 1, 1)(a).astype(np.float64) if a.dtype == object else a.astype(np.float64)


def _zeros(shape, dt):
    return cast(np.zeros(shape), dt)


def _elementwise(mp_name, np_fn):
    def f(a):
        a = np.asarray(a)
        if a.dtype == object:
            import mpmath
            return np.frompyfunc(getattr(mpmath, mp_name), 1, 1)(a)
        return np_fn(a)
    return f


_sqrt, _sin, _cos, _acos = _elementwise("sqrt", np.sqrt), _elementwise("sin", np.sin), _elementwise("cos", np.cos), _elementwise("acos", np.arccos)


def _b(m):
    return np.asarray(m).astype(bool)


def _mm(A, B):
    return (A[..., :, :, None] * B[..., None, :, :]).sum(-2)


def _mv(A, v):
    return (A * v[..., None, :]).sum(-1)


def _tr(A):
    return np.swapaxes(A, -1, -2)


def _eye(dt):
    return cast(np.eye(3), dt)


def _skew(v):      # auxiliar.cpp:29-44
    z = v[..., 0] * 0
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1), np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


# ---- auxiliar.cpp:113-173 ----------------------------------------------------------------------------------------------------------------
def se3_inv(R, t):
    Ri = _tr(R)
    return Ri, -_mv(Ri, t)


def se3_exp(x, dt):
    t, w = x[..., :3], x[..., 3:]
    th = _sqrt((w * w).sum(-1))
    small = _b(th < 1e-6)
    ths = np.where(small, th * 0 + 1, th)[..., None, None]
    s = _skew(w) / ths
    ss = _mm(s, s)
    sn, cs = _sin(ths), _cos(ths)
    I = _eye(dt)
    R = I + s * sn + ss * (1 - cs)
    V = I + s * (1 - cs) / ths + ss * (ths - sn) / ths
    return np.where(small[..., None, None], I + R * 0, R), np.where(small[..., None], t, _mv(V, t))


def _inv3(A):      # Eigen's fixed-size inverse: cofactors over the determinant
    c = lambda i, j: A[..., (i + 1) % 3, (j + 1) % 3] * A[..., (i + 2) % 3, (j + 2) % 3] - A[..., (i + 1) % 3, (j + 2) % 3] * A[..., (i + 2) % 3, (j + 1) % 3]
    cof = np.stack([np.stack([c(i, j) for j in range(3)], -1) for i in range(3)], -2)
    det = (A[..., 0, :] * cof[..., 0, :]).sum(-1)
    return _tr(cof) / det[..., None, None]


def se3_log(R, t, dt):
    cosine = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) / 2
    cosine = np.where(_b(cosine > 1), cosine * 0 + 1, np.where(_b(cosine < -1), cosine * 0 - 1, cosine))
    sine = _sqrt(1 - cosine * cosine)
    sine = np.where(_b(sine > 1), sine * 0 + 1, sine)
    theta = _acos(cosine)
    big = _b(theta > 1e-6)
    th = np.where(big, theta, theta * 0 + 1); sn = np.where(big, sine, sine * 0 + 1)
    what = (th / (2 * sn))[..., None, None] * (R - _tr(R))
    w = np.stack([what[..., 2, 1], what[..., 0, 2], what[..., 1, 0]], -1)
    s = _skew(w) / th[..., None, None]
    I = _eye(dt)
    V = I + s * ((1 - cosine) / th)[..., None, None] + _mm(s, s) * ((th - sn) / th)[..., None, None]
    V = np.where(big[..., None, None], V, I + V * 0)
    w = np.where(big[..., None], w, w * 0)
    return np.concatenate([_mv(_inv3(V), t), w], -1)


# ---- the observations ---------------------------------------------------------------------------------------------------------------------
def _pieces(g, a, b, homog_th):      # :1491-1506 (= :1574-1589, :1597-1609): gz2 and the six terms for (a, b) = (fx e0, fy e1)
    gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
    gz2 = gz * gz
    gz2 = 1 / np.where(_b(gz2 < homog_th), gz2 * 0 + homog_th, gz2)
    return np.stack([gz2 * a * gz, gz2 * b * gz, -gz2 * (a * gx + b * gy), -gz2 * (a * gx * gy + b * gy * gy + b * gz * gz),
                     gz2 * (a * gx * gx + a * gz * gz + b * gx * gy), gz2 * (b * gx * gz - a * gy * gz)], -1)


def _clamp(n, homog_th):      # std::max(homogTh, norm)
    return np.where(_b(n < homog_th), n * 0 + homog_th, n)


def _project(cam, g):      # PinholeStereoCamera::projection
    return cam[2] + cam[0] * g[..., 0] / g[..., 2], cam[3] + cam[1] * g[..., 1] / g[..., 2]


def point_obs(cam, homog_th, Ri, ti, X, uv):
    """:1482-1516 for a batch: (n, w, Jp[.., 6], Jl[.., 3]); Ri, ti = the INVERSE pose"""
    g = _mv(Ri, X) + ti
    pu, pv = _project(cam, g)
    e0, e1 = uv[..., 0] - pu, uv[..., 1] - pv
    n = _sqrt(e0 * e0 + e1 * e1)
    J = _pieces(g, cam[0] * e0, cam[1] * e1, homog_th)
    dn = _clamp(n, homog_th)[..., None]
    Jl = (J[..., :3, None] * Ri).sum(-2) / dn      # Jij_Xwj^T R
    return n, 1 / (1 + n * n), J / dn, Jl


def line_obs(cam, homog_th, Ri, ti, PQ, l3):
    """:1561-1625 for a batch: (n, w, Jp[.., 6], Jl[.., 6])"""
    gp, gq = _mv(Ri, PQ[..., :3]) + ti, _mv(Ri, PQ[..., 3:]) + ti
    pu, pv = _project(cam, gp)
    qu, qv = _project(cam, gq)
    e0 = l3[..., 0] * pu + l3[..., 1] * pv + l3[..., 2]
    e1 = l3[..., 0] * qu + l3[..., 1] * qv + l3[..., 2]
    n = _sqrt(e0 * e0 + e1 * e1)
    a, b = cam[0] * e0, cam[1] * e1      # fxlx, fyly: used for BOTH end points (:1580-1581, :1604-1614)
    JP, JQ = _pieces(gp, a, b, homog_th), _pieces(gq, a, b, homog_th)
    dn = _clamp(n, homog_th)
    JlP = (JP[..., :3, None] * Ri).sum(-2) * (e0 / dn)[..., None]
    JlQ = (JQ[..., :3, None] * Ri).sum(-2) * (e1 / dn)[..., None]
    Jp = (JP * e0[..., None] + JQ * e1[..., None]) / dn[..., None]
    return n, 1 / (1 + n * n), Jp, np.concatenate([JlP, JlQ], -1)


# ---- one linearisation ------------------------------------------------------------------------------------------------------------------
class Window:
    """the inputs in the working type, and the state X = [x_kf_w per local keyframe | xyz | pq]"""
    def __init__(self, w, dt, o):
        self.dt, self.o = dt, o
        self.cam = [cast(v, dt)[()] for v in w["cam"]]
        self.th = cast(o["homog_th"], dt)[()]
        self.loc = np.asarray(w["kf_loc"], np.int64)
        self.K, self.Nkf = len(self.loc), int((self.loc >= 0).sum())
        self.kf_of = np.zeros(max(self.Nkf, 1), np.int64); self.kf_of[self.loc[self.loc >= 0]] = np.flatnonzero(self.loc >= 0)
        T = cast(np.asarray(w["T_kf_w"], np.float64).reshape(-1, 4, 4), dt)
        self.Rm, self.tm = T[:, :3, :3], T[:, :3, 3]
        self.xyz0, self.pq0 = cast(np.asarray(w["xyz"], np.float64).reshape(-1, 3), dt), cast(np.asarray(w["pq"], np.float64).reshape(-1, 6), dt)
        self.Np, self.Nl = len(self.xyz0), len(self.pq0)
        self.po_pt, self.po_kf = np.asarray(w["po_pt"], np.int64), np.asarray(w["po_kf"], np.int64)
        self.lo_ln, self.lo_kf = np.asarray(w["lo_ln"], np.int64), np.asarray(w["lo_kf"], np.int64)
        self.uv, self.l3 = cast(np.asarray(w["uv"], np.float64).reshape(-1, 2), dt), cast(np.asarray(w["l3"], np.float64).reshape(-1, 3), dt)
        self.Xp = se3_log(self.Rm[self.kf_of], self.tm[self.kf_of], dt) if self.Nkf else _zeros((0, 6), dt)      # X_aux: x_kf_w
        self.xyz, self.pq = self.xyz0.copy(), self.pq0.copy()

    def poses(self, iterate):
        R, t = self.Rm.copy(), self.tm.copy()
        if iterate and self.Nkf:
            R[self.kf_of], t[self.kf_of] = se3_exp(self.Xp, self.dt)
        return R, t

    def linearise(self, later):
        """the two observation loops of a pass: [(landmark, local keyframe or -1, n, w, Jp, Jl, count, width)] for points, lines"""
        parts = []
        Ri, ti = se3_inv(*self.poses(later))                                             # :1709-1714
        n, w, Jp, Jl = point_obs(self.cam, self.th, Ri[self.po_kf], ti[self.po_kf], self.xyz[self.po_pt], self.uv)
        parts.append((self.po_pt, self.loc[self.po_kf], n, w, Jp, Jl, self.Np, 3))
        Ri, ti = se3_inv(*self.poses(later and self.o["use_iterate_poses"]))            # :1790: the map pose
        n, w, Jp, Jl = line_obs(self.cam, self.th, Ri[self.lo_kf], ti[self.lo_kf], self.pq[self.lo_ln], self.l3)
        parts.append((self.lo_ln, self.loc[self.lo_kf], n, w, Jp, Jl, self.Nl, 6))
        return parts


def _scatter(shape, dt, idx, vals):
    out = _zeros(shape, dt)
    if len(vals):
        np.add.at(out, idx, vals)
    return out


def blocks(parts, Nkf, dt):
    """err sum, Hpp [Nkf, 6, 6], gp [Nkf, 6], and per part Hll [L, d, d], gl [L, d]"""
    err = cast(0.0, dt)[()]
    Hpp, gp, lm = _zeros((Nkf, 6, 6), dt), _zeros((Nkf, 6), dt), []
    for l, loc, n, w, Jp, Jl, L, d in parts:
        if len(n):
            err = err + (n * n * w).sum()
        s = loc >= 0
        if s.any():
            np.add.at(Hpp, loc[s], Jp[s][:, :, None] * Jp[s][:, None, :] * w[s][:, None, None])
            np.add.at(gp, loc[s], Jp[s] * (n * w)[s][:, None])
        lm.append((_scatter((L, d, d), dt, l, Jl[:, :, None] * Jl[:, None, :] * w[:, None, None]), _scatter((L, d), dt, l, Jl * (n * w)[:, None])))
    return err, Hpp, gp, lm


def hmax(Hpp, lm):      # :1653-1658
    m = 0
    for A in [Hpp] + [H for H, _ in lm]:
        if A.size:
            m = max(m, np.abs(A[:, np.arange(A.shape[1]), np.arange(A.shape[1])]).max())
    return m


def _damp(A, lam):      # H(i,i) += lambda * H(i,i)
    A = A.copy()
    i = np.arange(A.shape[-1])
    A[..., i, i] = A[..., i, i] + lam * A[..., i, i]
    return A


def _spd_inv(A, dt):
    """batched inverse of symmetric positive definite d x d blocks by Cholesky; (inverse, every pivot positive)"""
    L, d = A.shape[0], A.shape[1]
    Lm, Li = _zeros((L, d, d), dt), _zeros((L, d, d), dt)
    ok = np.ones(L, bool)
    for j in range(d):
        dj = A[:, j, j] - (Lm[:, j, :j] * Lm[:, j, :j]).sum(-1)
        ok &= _b(dj > 0)
        Lm[:, j, j] = _sqrt(np.where(_b(dj > 0), dj, dj * 0 + 1))
        for i in range(j + 1, d):
            Lm[:, i, j] = (A[:, i, j] - (Lm[:, i, :j] * Lm[:, j, :j]).sum(-1)) / Lm[:, j, j]
    for c in range(d):
        for r in range(c, d):
            Li[:, r, c] = ((1 if r == c else 0) - (Lm[:, r, c:r] * Li[:, c:r, c]).sum(-1)) / Lm[:, r, r]
    return _mm(_tr(Li), Li), bool(ok.all())


class SolverFailed(Exception):
    pass


def _solve(S, b, dt):
    """x of the wide S x = b: refine() on the double rounding, then corrections against the wide residual; (x, omega of refine)"""
    S64, b64 = f64(S), f64(b)
    if not (np.diag(S64) > 0).all():
        raise SolverFailed
    try:
        x, om = SR.refine(S64, b64)
        if dt is np.float64:
            return f64(x), om
        solve = SR._Factor(S64)
    except np.linalg.LinAlgError:
        raise SolverFailed
    x = cast(x, dt) if not isinstance(dt, str) else cast(f64(x), dt)
    for _ in range(3):
        x = x + cast(solve(f64(b - _mv(S, x))), dt)
    return x, om


def step_elim(parts, Hpp, gp, lm, lam, Nkf, dt):
    """(b) landmark blocks eliminated in the working type: (dx poses [Nkf, 6], [dx landmarks per part], omega, S, rhs)"""
    S = _zeros((Nkf, Nkf, 6, 6), dt)
    i = np.arange(Nkf)
    S[i, i] = _damp(Hpp, lam)
    rhs = gp.copy()
    keep = []
    for (l, loc, n, w, Jp, Jl, L, d), (Hll, gl) in zip(parts, lm):
        if L == 0:
            keep.append(None); continue
        D, ok = _spd_inv(_damp(Hll, lam), dt)
        if not ok:
            raise SolverFailed
        s = np.flatnonzero(loc >= 0)      # observations from local keyframes, landmark-major as the lists are
        ls, ks, Jps, Jls, ws = l[s], loc[s], Jp[s], Jl[s], w[s]
        keep.append((D, gl, ls, ks, Jps, Jls, ws))
        if not len(s):
            continue
        u = _mv(D[ls], Jls) * ws[:, None]
        sg = ws * (Jls * _mv(D, gl)[ls]).sum(-1)
        np.subtract.at(rhs, ks, Jps * sg[:, None])
        cnt = np.bincount(ls, minlength=L)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for a in range(int(cnt.max())):
            for b in range(int(cnt.max())):
                m = np.flatnonzero(cnt > max(a, b))
                ea, eb = start[m] + a, start[m] + b
                c = (u[ea] * Jls[eb]).sum(-1) * ws[eb]
                np.subtract.at(S, (ks[ea], ks[eb]), c[:, None, None] * Jps[ea][:, :, None] * Jps[eb][:, None, :])
    Sd = S.transpose(0, 2, 1, 3).reshape(6 * Nkf, 6 * Nkf)
    x, om = _solve(Sd, rhs.reshape(-1), dt)
    dxp = x.reshape(Nkf, 6)
    dxl = []
    for k in keep:
        if k is None:
            dxl.append(None); continue
        D, gl, ls, ks, Jps, Jls, ws = k
        v = gl.copy()
        if len(ls):
            np.subtract.at(v, ls, Jls * (ws * (Jps * dxp[ks]).sum(-1))[:, None])
        dxl.append(_mv(D, v))
    return dxp, dxl, om, Sd, rhs.reshape(-1)


def dense_system(parts, Nkf, dt):
    """(a) the full H and g of :1518-1538 / :1627-1647, observation by observation"""
    off, N = [], 6 * Nkf
    for p in parts:
        off.append(N); N += p[6] * p[7]
    H, g = _zeros((N, N), dt), _zeros(N, dt)
    for (l, loc, n, w, Jp, Jl, L, d), o in zip(parts, off):
        for e in range(len(n)):
            j = o + d * l[e]
            g[j:j + d] += Jl[e] * n[e] * w[e]
            H[j:j + d, j:j + d] += Jl[e][:, None] * Jl[e][None, :] * w[e]
            if loc[e] >= 0:
                i = 6 * loc[e]
                g[i:i + 6] += Jp[e] * n[e] * w[e]
                Haux = Jl[e][:, None] * Jp[e][None, :] * w[e]
                H[i:i + 6, i:i + 6] += Jp[e][:, None] * Jp[e][None, :] * w[e]
                H[j:j + d, i:i + 6] += Haux
                H[i:i + 6, j:j + d] += Haux.T
    return H, g, off


def step_dense(parts, lam, Nkf, dt):
    H, g, off = dense_system(parts, Nkf, dt)
    x, om = _solve(_damp(H, lam), g, dt)
    dxl = [x[o:o + p[6] * p[7]].reshape(p[6], p[7]) if p[6] else None for p, o in zip(parts, off)]
    return x[:6 * Nkf].reshape(Nkf, 6), dxl, om, _damp(H, lam), g


def apply_step(win, dxp, dxl):      # :1669-1680
    if win.Nkf:
        Rp, tp = se3_exp(win.Xp, win.dt)
        Rd, td = se3_inv(*se3_exp(dxp, win.dt))
        win.Xp = se3_log(_mm(Rp, Rd), _mv(Rp, td) + tp, win.dt)
    if dxl[0] is not None:
        win.xyz = win.xyz + dxl[0]
    if dxl[1] is not None:
        win.pq = win.pq + dxl[1]


def _norm_all(dxp, dxl):
    s = (dxp * dxp).sum()
    for d in dxl:
        if d is not None and d.size:
            s = s + (d * d).sum()
    return _sqrt(s)


def run(w, dt=np.float64, form="elim", **opts):
    """the whole function.  Returns the outputs of plba_lba_visual as doubles (T, xyz, pq, err_first, err_last, lam, iterations, updates,
    pt_moved, ln_moved, solver_failed) plus, for the tests, `omega` (largest refine residual), `passes` (per pass: err, err_prev, hmax, dxn,
    S, rhs, dxp in the working type), `moves` (each landmark's displacement) and `after[k]`: the same dictionary as a call with max_iters = k
    returns, for every pass k the run completed."""
    o = dict(DEFAULTS); o.update(opts)
    with _prec(dt), np.errstate(invalid="ignore"):
        c = lambda v: cast(v, dt)[()]
        win = Window(w, dt, o)
        inf = c(np.inf)
        err, err_prev, lam = c(0.0), c(999999999.9), c(o["lambda_lm"])
        lam_k, min_err, min_chg = c(o["lambda_k"]), c(o["min_error"]), c(o["min_error_change"])
        updates, failed, omega, passes, err_first = 0, 0, 0.0, [], c(0.0)
        after = {}

        def out(n_it):
            R, t = win.poses(True)
            T = np.tile(np.eye(4), (win.K, 1, 1)); T[:, :3, :3] = f64(R); T[:, :3, 3] = f64(t)
            fixed = win.loc < 0
            T[fixed] = np.asarray(w["T_kf_w"], np.float64).reshape(-1, 4, 4)[fixed]
            mp_, ml_ = _sqrt(((win.xyz - win.xyz0) ** 2).sum(-1)), _sqrt(((win.pq - win.pq0) ** 2).sum(-1))
            return dict(T=T, xyz=f64(win.xyz), pq=f64(win.pq), err_first=float(err_first), err_last=float(err), lam=float(lam), iterations=n_it,
                        updates=updates, solver_failed=failed, pt_moved=_b(mp_ > 0.01), ln_moved=_b(ml_ > 0.01), omega=omega, passes=list(passes),
                        moves=np.concatenate([f64(mp_), f64(ml_)]), n_obs=len(win.po_pt) + len(win.lo_ln), after=after,
                        obs_per_kf=np.bincount(np.concatenate([win.loc[win.po_kf], win.loc[win.lo_kf]]) + 1, minlength=win.Nkf + 1)[1:])
        it = 0
        while it < o["max_iters"]:
            parts = win.linearise(it > 0)
            err, Hpp, gp, lm = blocks(parts, win.Nkf, dt)
            rec = dict(err_prev=err_prev)
            if it == 0:
                err_first = err / (len(win.po_pt) + len(win.lo_ln))
                err = inf if err > 0 else c(np.nan)                       # :1650: x / 0
                hm = hmax(Hpp, lm)
                rec["hmax"] = hm
                lam = lam * (c(float(int(f64(hm)))) if o["variant"] == 1 else hm)      # :1659; GBA: `int Hmax`
            else:
                err = (inf if err > 0 else c(np.nan)) if o["variant"] == 1 else err / (win.Np + win.Nl)      # :1882 (GBA: / 0 again)
                rec["err"] = err
                if _b(abs(err - err_prev) < min_chg) or _b(err < min_err):      # :1884
                    passes.append(rec)
                    break
            rec["err"] = err
            try:
                if form == "dense":
                    dxp, dxl, om, S, rhs = step_dense(parts, lam, win.Nkf, dt)
                else:
                    dxp, dxl, om, S, rhs = step_elim(parts, Hpp, gp, lm, lam, win.Nkf, dt)
            except SolverFailed:
                failed = 1
                passes.append(rec)
                break
            omega = max(omega, om)
            rec.update(S=S, rhs=rhs, dxp=dxp, lam=lam, dxn=_norm_all(dxp, dxl))
            passes.append(rec)
            take = True
            if it > 0:
                if _b(err > err_prev):      # :1895
                    lam = lam / lam_k; take = False
                else:
                    lam = lam * lam_k
            if take:
                updates += 1
                apply_step(win, dxp, dxl)
            if it > 0 and _b(rec["dxn"] < min_chg):      # :1916
                err_prev = err; it += 1
                break
            err_prev = err
            it += 1
            after[it] = out(it)      # what a call with max_iters = it returns
        return out(it)


# ---- the tolerance rule of the exactness tests ------------------------------------------------------------------------------------------------
FACTOR = 8          # over the noise: covers another summation order (tree, atomics) and FMA contraction; not a measurement
MARGIN = 1000       # a decision is compared only where the reference's own margin is this many times the noise of the quantity


def tolerances(r64, rw):
    """per quantity max(8 noise, m u |value|), noise = |fp64 evaluation - wide evaluation| of this reference on the same window (the
    rounding of a plain fp64 evaluation of the same operation), taken in the maximum norm of the quantity: element by element the
    difference of two roundings is now and then zero, the largest element of an array is not.  m = terms of the sum (err_first: the
    observations; lam: the observations of the busiest keyframe, the longest diagonal sum), 64 for an entry of T / xyz / pq."""
    tol, noise = {}, {}
    for k, m in (("T", 64), ("xyz", 64), ("pq", 64), ("err_first", max(64, r64["n_obs"])), ("lam", max(64, int(r64["obs_per_kf"].max(initial=0))))):
        a, b = np.asarray(r64[k], np.float64), np.asarray(rw[k], np.float64)
        if a.size == 0:
            continue
        noise[k] = float(np.abs(a - b).max())
        tol[k] = max(FACTOR * noise[k], m * U * float(np.abs(b).max()))
    return tol, noise


def decisions_have_margin(r64, rw, o=None):
    """(iii): every comparison the control made, and every 1 cm test, has a margin of MARGIN x the noise of the compared quantity in the
    wide run; returns the smallest margin / noise ratio"""
    o = dict(DEFAULTS, **(o or {}))
    worst = np.inf
    if (r64["iterations"], r64["updates"], len(r64["passes"])) != (rw["iterations"], rw["updates"], len(rw["passes"])):
        return 0.0

    def hold(value, value64, against, m=64):
        nonlocal worst
        value, value64 = float(value), float(value64)
        if not np.isfinite(value):
            return
        noise = max(abs(value - value64), m * U * abs(value))
        worst = min(worst, abs(value - against) / noise if noise > 0 else np.inf)
    for p6, pw in zip(r64["passes"], rw["passes"]):
        if "err" in pw and np.isfinite(float(pw["err"])):
            e, e6, ep = float(pw["err"]), float(p6["err"]), float(pw["err_prev"])
            hold(e, e6, o["min_error"])
            if np.isfinite(ep):
                hold(abs(e - ep), abs(e6 - float(p6["err_prev"])), o["min_error_change"])
                hold(e - ep, e6 - float(p6["err_prev"]), 0.0)
        if "dxn" in pw:
            hold(pw["dxn"], p6["dxn"], o["min_error_change"])
        if "hmax" in pw and o["variant"] == 1:
            h = float(pw["hmax"])
            hold(h, p6["hmax"], np.floor(h)); hold(h, p6["hmax"], np.floor(h) + 1)
    mv, mv6 = rw["moves"], r64["moves"]
    if len(mv):
        noise = np.maximum(np.abs(mv - mv6), 64 * U * np.abs(mv))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = min(worst, float(np.where(noise > 0, np.abs(mv - 0.01) / noise, np.inf).min()))
    return worst


def at(r, k):
    """what the run returns for max_iters = k (k = None: the full run)"""
    return r if k is None or k not in r["after"] or k >= r["iterations"] else r["after"][k]


def pose_steps(T0, T1, kfs):
    """dx of T1 = T0 expmap(dx)^-1 for the keyframes kfs, in the wide type: logmap(T1^-1 T0)"""
    dt = wide()
    with _prec(dt):
        A, B = cast(np.asarray(T1, np.float64)[kfs], dt), cast(np.asarray(T0, np.float64)[kfs], dt)
        Ri, ti = se3_inv(A[:, :3, :3], A[:, :3, 3])
        return se3_log(_mm(Ri, B[:, :3, :3]), _mv(Ri, B[:, :3, 3]) + ti, dt)


# ---- holding a result (the oracle's, the device's) against the reference ------------------------------------------------------------------
LIMITS = dict(T=1e-9, xyz=1e-8, pq=1e-8, lam_rel=1e-12, err_first_rel=1e-12)      # what tests/test_lba_visual.py allows today: the new tolerances may only be tighter


def hold(res, r64, rw, who, name, opts=None, decisions=True):
    """asserts conditions (i)-(iii) on the reference's two runs, then every output of `res` against the wide run; prints each figure
    before it asserts.  The m u |value| floor of a tolerance is capped at today's limit (for lam at 65 536 terms and err_first at 82 000
    the floor alone is 7e-12 / 9e-12 relative, above the 1e-12 in use today for both): the tolerance is then the tighter of the two."""
    assert r64["omega"] <= SR.RESIDUAL_MAX and rw["omega"] <= SR.RESIDUAL_MAX, (r64["omega"], rw["omega"])      # (i)
    tol, noise = tolerances(r64, rw)
    lim = dict(T=LIMITS["T"], xyz=LIMITS["xyz"], pq=LIMITS["pq"], lam=LIMITS["lam_rel"] * abs(rw["lam"]),
               err_first=LIMITS["err_first_rel"] * abs(rw["err_first"]))
    for k in tol:      # (ii)
        assert FACTOR * noise[k] < lim[k], (name, k, noise[k], lim[k])
        tol[k] = min(tol[k], lim[k])
    if decisions:      # (iii)
        margin = decisions_have_margin(r64, rw, opts)
        print("%s %s: smallest decision margin / noise %.3g" % (who, name, margin))
        assert margin >= MARGIN, (name, margin)
        for k in ("iterations", "updates", "solver_failed"):
            assert res[k] == rw[k] == r64[k], (name, k, res[k], rw[k], r64[k])
        assert np.array_equal(res["pt_moved"], rw["pt_moved"]) and np.array_equal(res["ln_moved"], rw["ln_moved"]), name
    bad = []
    for k in tol:
        e = float(np.abs(np.asarray(res[k], np.float64) - np.asarray(rw[k], np.float64)).max())
        print("%s %s %-9s error %.3e  noise %.3e  tolerance %.3e  error/noise %.2f" % (who, name, k, e, noise[k], tol[k], e / noise[k] if noise[k] > 0 else np.inf if e > 0 else 0.0))
        if not e <= tol[k]:
            bad.append((k, e, tol[k]))
    assert not bad, (who, name, bad)


def hold_pose_step(T1, w, rw, who, name):
    """the pose step of the first pass, read back through T1 = T0 expmap(dx)^-1, in the E_D norm of solver_ref against n u kappa_s of the
    reference's damped reduced system.  The step is only visible through the doubles of T1, so an entry of T adds its own 64 u |T|
    (the floor every entry of T has above) in that norm; that share is 1e4 .. 1e5 times n u kappa_s on these heavily damped systems
    (kappa_s of 10), so the check is bounded by the read-back, not by the solve: it adds little over the comparison of T at 8 x noise,
    and the share is printed with every figure.  It scales with 1 / |step| (3.8e-9 on the 257-block window, whose 65 536 observations per
    keyframe make the multiplicative damping heaviest), so no fixed cap on it can be derived."""
    p = rw["passes"][0]
    S = f64(p["S"])
    loc = np.asarray(w["kf_loc"]); kfs = np.flatnonzero(loc >= 0)[np.argsort(loc[loc >= 0])]
    dx = f64(pose_steps(w["T_kf_w"], T1, kfs)).reshape(-1)
    ref = f64(p["dxp"]).reshape(-1)
    d = np.sqrt(np.diag(S))
    e = SR.scaled_error(dx, ref, S)
    readback = 64 * U * max(1.0, float(np.abs(np.asarray(w["T_kf_w"])[:, :3]).max())) * d.max() / (d * np.abs(ref)).max()
    b = SR.bound(S) + readback
    print("%s %s pose step: E_D %.3e  bound %.3e (n u kappa_s %.3e, read-back %.3e)" % (who, name, e, b, SR.bound(S), readback))
    assert e <= b, (who, name, e, b)
