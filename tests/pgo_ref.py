"""numpy restatement of the loop-closure pose graph that plba_optimize_pose_graph runs on the device.

g2o VertexSE3 / EdgeSE3 as include/plba_g2o/types_slam3d.h restates them (update X <- X fromVectorMQT(u), orthogonalizeAfter = 1000
counting every oplus; error toVectorMQT(Z^-1 Xi^-1 Xj); the analytic Jacobians derived there), under the Levenberg branch of
SparseOptimizer::optimizeHost and the facade's computeInitialGuess (include/plba_g2o/g2o_compat.h).  Poses are (R row-major 9, t 3).
Products of 3 x 3 matrices are written out term by term in the order of plba_math.h's mul, so that the initial guess agrees with the
oracle's bit for bit.  The linear system is solved densely (Cholesky: a failure counts as tempChi = DBL_MAX) up to DENSE_MAX dims and
by a sparse LU above (the graphs of the tests are positive definite at every lambda).

Also the graph shapes the tests and tools/time_pgo.py use: cov_graph() is the shape of loopClosureOptimizationCovGraphG2O
(src/mapHandler.cpp:4299-4528): odometry and covisibility edges within +-8 keyframes, loop closures, non-identity information."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
DENSE_MAX = 2400
ORTHO_AFTER = 1000


def mm(A, B):
    """3 x 3 products over leading axes, a0 b0 + a1 b1 + a2 b2 left to right (plba::mul)"""
    return A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :] + A[..., :, 2, None] * B[..., None, 2, :]


def mv(A, v):
    return A[..., :, 0] * v[..., 0, None] + A[..., :, 1] * v[..., 1, None] + A[..., :, 2] * v[..., 2, None]


def split(X):
    X = np.asarray(X, np.float64)
    return X[..., :9].reshape(X.shape[:-1] + (3, 3)), X[..., 9:12]


def join(R, t):
    return np.concatenate([R.reshape(R.shape[:-2] + (9,)), t], axis=-1)


def iso_mul(a, b):
    Ra, ta = split(a); Rb, tb = split(b)
    return join(mm(Ra, Rb), mv(Ra, tb) + ta)


def iso_inv(a):
    R, t = split(a)
    Rt = np.swapaxes(R, -1, -2)
    return join(Rt, -mv(Rt, t))


def q_to_R(x, y, z, w):
    """Eigen toRotationMatrix, as plba_math.h q_to_R"""
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(R.shape[:-1] + (3, 3))


def from_mqt(u):
    """internal::fromVectorMQT: translation + compact quaternion (identity rotation if |v| > 1)"""
    u = np.asarray(u, np.float64)
    w2 = 1.0 - (u[..., 3] * u[..., 3] + u[..., 4] * u[..., 4] + u[..., 5] * u[..., 5])
    R = q_to_R(u[..., 3], u[..., 4], u[..., 5], np.sqrt(np.maximum(w2, 0.0)))
    R = np.where((w2 < 0)[..., None, None], np.eye(3), R)
    return join(R, u[..., :3])


def R_to_q(m):
    """Eigen Quaterniond(Matrix3d) (plba_math.h R_to_q) over leading axes: (x, y, z, w)"""
    m = m.reshape(m.shape[:-2] + (9,))
    a = [m[..., i] for i in range(9)]
    tr = a[0] + a[4] + a[8]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(np.maximum(tr + 1.0, 0)); s = 0.5 / t
        q0 = np.stack([(a[7] - a[5]) * s, (a[2] - a[6]) * s, (a[3] - a[1]) * s, 0.5 * t], -1)
        t = np.sqrt(np.maximum(a[0] - a[4] - a[8] + 1.0, 0)); s = 0.5 / t
        q1 = np.stack([0.5 * t, (a[3] + a[1]) * s, (a[6] + a[2]) * s, (a[7] - a[5]) * s], -1)
        t = np.sqrt(np.maximum(a[4] - a[8] - a[0] + 1.0, 0)); s = 0.5 / t
        q2 = np.stack([(a[1] + a[3]) * s, 0.5 * t, (a[7] + a[5]) * s, (a[2] - a[6]) * s], -1)
        t = np.sqrt(np.maximum(a[8] - a[0] - a[4] + 1.0, 0)); s = 0.5 / t
        q3 = np.stack([(a[2] + a[6]) * s, (a[5] + a[7]) * s, 0.5 * t, (a[3] - a[1]) * s], -1)
    c0 = (tr > 0)[..., None]
    c1 = ((a[0] >= a[4]) & (a[0] >= a[8]))[..., None]
    c2 = ((a[4] > a[0]) & (a[4] >= a[8]))[..., None]
    return np.where(c0, q0, np.where(c1, q1, np.where(c2, q2, q3)))


def unit_q(R):
    """toVectorMQT's quaternion: normalised, w >= 0"""
    q = R_to_q(R)
    q = q / np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])[..., None]
    return np.where((q[..., 3] < 0)[..., None], -q, q)


def hat(v):
    z = np.zeros(v.shape[:-1])
    return np.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(v.shape[:-1] + (3, 3))


def edge_error(Xi, Xj, Zi):
    """EdgeSE3::computeError: toVectorMQT((Z^-1 Xi^-1) Xj)"""
    E = iso_mul(iso_mul(Zi, iso_inv(Xi)), Xj)
    R, t = split(E)
    return np.concatenate([t, unit_q(R)[..., :3]], -1)


def edge_jacobians(Xi, Xj, Zi):
    """EdgeSE3::linearizeOplus: J0 = de/du_i, J1 = de/du_j (6 x 6, rows = error)"""
    B = iso_mul(iso_inv(Xi), Xj)
    E = iso_mul(Zi, B)
    RE, _ = split(E)
    q = unit_q(RE)
    RZt, _ = split(Zi)
    _, tB = split(B)
    V = hat(q[..., :3])
    w = q[..., 3][..., None, None] * np.eye(3)
    Qm, Qp = w - V, w + V
    RZtTB, QmRZt = mm(RZt, hat(tB)), mm(Qm, RZt)
    sh = Xi.shape[:-1]
    J0 = np.zeros(sh + (6, 6)); J1 = np.zeros(sh + (6, 6))
    J0[..., :3, :3] = -RZt; J0[..., :3, 3:] = 2.0 * RZtTB; J0[..., 3:, 3:] = -QmRZt
    J1[..., :3, :3] = RE; J1[..., 3:, 3:] = Qp
    return J0, J1


def chi2_edges(e, om):
    """edgeChi2: sum_i e_i (sum_j O_ij e_j), per edge"""
    c = np.zeros(e.shape[:-1])
    for i in range(6):
        t = np.zeros(e.shape[:-1])
        for j in range(6):
            t = t + om[..., i, j] * e[..., j]
        c = c + e[..., i] * t
    return c


def initial_guess(X, fixed, ei, ej, Z):
    """the facade's computeInitialGuess: breadth first from the fixed vertices (in the order the edges name them); each `from` of a
    frontier takes its edges in insertion order: to = from Z (from is vertex 0) or from Z^-1"""
    X = np.array(X, np.float64)
    nv = len(X)
    inc = [[] for _ in range(nv)]
    for k in range(len(ei)):
        inc[ei[k]].append(k); inc[ej[k]].append(k)
    done = np.zeros(nv, bool)
    front = []
    for k in range(len(ei)):
        for v in (ei[k], ej[k]):
            if fixed[v] and not done[v]:
                done[v] = True; front.append(v)
    while front:
        nxt = []
        for f in front:
            for k in inc[f]:
                to = ej[k] if ei[k] == f else ei[k]
                if done[to] or fixed[to]:
                    continue
                X[to] = iso_mul(X[f], Z[k] if ei[k] == f else iso_inv(Z[k]))
                done[to] = True; nxt.append(to)
        front = nxt
    return X


def _solve(H, b, lam):
    N = len(b)
    A = H + lam * np.eye(N) if N <= DENSE_MAX else None
    if A is not None:
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return np.zeros(N), False
        return np.linalg.solve(L.T, np.linalg.solve(L, b)), True
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    A = sp.csc_matrix(H) + lam * sp.identity(N, format="csc")
    return spl.splu(A).solve(b), True


def optimize(pose12, ei, ej, meas12, info=None, fixed=None, iters=100, user_lambda=0.0, initial=False, tau=1e-5, max_trials=10,
             lower=1.0 / 3.0, upper=2.0 / 3.0):
    """optimizeHost, Levenberg branch.  Returns dict(poses, chi2_initial, chi2_final, lambda_final, iterations, trials, stop_reason,
    solver_failures, trace (list of dicts, one per trial), ortho (oplus calls that re-orthogonalised, per vertex))"""
    X = np.array(pose12, np.float64).reshape(-1, 12)
    nv = len(X)
    ei = np.asarray(ei, np.int64); ej = np.asarray(ej, np.int64)
    ne = len(ei)
    Z = np.asarray(meas12, np.float64).reshape(ne, 12)
    om = np.tile(np.eye(6), (ne, 1, 1)) if info is None else np.asarray(info, np.float64).reshape(ne, 6, 6)
    fx = np.zeros(nv, bool) if fixed is None else np.asarray(fixed).astype(bool)
    if initial and ne:
        X = initial_guess(X, fx, ei, ej, Z)
    Zi = iso_inv(Z)
    touched = np.zeros(nv, bool); touched[ei] = True; touched[ej] = True
    free = np.flatnonzero(touched & ~fx)
    hidx = -np.ones(nv, np.int64); hidx[free] = 6 * np.arange(len(free))
    N = 6 * len(free)
    cnt = np.zeros(nv, np.int64)
    ortho = np.zeros(nv, np.int64)

    def chi_of(X):
        return float(np.sum(chi2_edges(edge_error(X[ei], X[ej], Zi), om))) if ne else 0.0

    out = dict(trace=[], iterations=0, trials=0, stop_reason=0, solver_failures=0, ortho=ortho)
    chi = chi_of(X)
    out.update(chi2_initial=chi, chi2_final=chi, lambda_final=0.0)
    if iters <= 0 or N == 0:
        out["poses"] = X
        return out

    def build(X):
        e = edge_error(X[ei], X[ej], Zi)
        J0, J1 = edge_jacobians(X[ei], X[ej], Zi)
        we = np.einsum("kij,kj->ki", om, e)
        H = np.zeros((N, N)); b = np.zeros(N)
        n = N // 6
        H4 = H.reshape(n, 6, n, 6); b2 = b.reshape(n, 6)
        J = (J0, J1); rk = (hidx[ei] // 6, hidx[ej] // 6)
        for a in range(2):
            sa = rk[a] >= 0
            np.add.at(b2, rk[a][sa], -np.einsum("kri,kr->ki", J[a], we)[sa])
            OJ = om @ J[a]
            for bb in range(2):
                m = sa & (rk[bb] >= 0)
                np.add.at(H4, (rk[bb][m], slice(None), rk[a][m], slice(None)), np.swapaxes(J[bb][m], 1, 2) @ OJ[m])
        return H, b

    def oplus(X, x):
        X = X.copy()
        D = from_mqt(x.reshape(-1, 6))
        Xn = iso_mul(X[free], D)
        for r, v in enumerate(free):
            cnt[v] += 1
            if cnt[v] > ORTHO_AFTER:
                cnt[v] = 0; ortho[v] += 1
                R, t = split(Xn[r])
                E = mm(R.T[None], R[None])[0] - np.eye(3)
                Xn[r] = join(R - 0.5 * mm(R[None], E[None])[0], t)
        X[free] = Xn
        return X

    lam, ni = 0.0, 2.0
    for it in range(iters):
        cur = chi_of(X)
        H, b = build(X)
        if it == 0:
            lam = user_lambda if user_lambda > 0 else tau * np.max(np.abs(np.diag(H)))
            ni = 2.0
        qmax, rho = 0, 0.0
        while True:
            x, ok = _solve(H, b, lam)
            if not ok:
                out["solver_failures"] += 1
            Xt = oplus(X, x)
            tmp = chi_of(Xt) if ok else DBL_MAX
            scale = 1e-3 + float(x @ (lam * x + b))
            rho = (cur - tmp) / scale
            out["trials"] += 1
            acc = bool(rho > 0 and np.isfinite(tmp))
            out["trace"].append(dict(iteration=it, trial=qmax, accepted=int(acc), solver_ok=int(ok), lam=lam, chi2_current=cur,
                                     chi2_trial=tmp, scale=scale, rho=rho))
            if acc:
                alpha = min(1.0 - (2 * rho - 1) ** 3, upper)
                lam *= max(lower, alpha); ni = 2.0; cur = tmp; X = Xt
            else:
                lam *= ni; ni *= 2.0
                if not np.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < max_trials):
                break
        out["iterations"] += 1
        out["chi2_final"], out["lambda_final"] = cur, lam
        if qmax == max_trials or rho == 0 or not np.isfinite(lam):
            out["stop_reason"] = 1
            break
    out["poses"] = X
    return out


# ---- graph shapes ------------------------------------------------------------------------------------------------------------------
def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _T(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def _p12(T):
    return np.concatenate([T[:3, :3].ravel(), T[:3, 3]])


def cov_graph(nv, seed=1, window=8, n_loops=3, fixed=(0, 1)):
    """loopClosureOptimizationCovGraphG2O's shape: keyframes (world -> keyframe, as T_kf_w) on a looping trajectory, odometry
    edges between neighbours, covisibility edges within +-window keyframes (every other pair), n_loops loop closures between the
    last keyframes and early ones, each edge with its own non-identity information, drifted initial estimates, `fixed` held."""
    rng = np.random.default_rng(seed)
    T = []
    for k in range(nv):
        a = 2 * np.pi * k / max(nv // 3, 8)
        Rwb = _rot(np.array([0.05 * np.sin(0.3 * k), 0.04 * np.cos(0.2 * k), a]))
        p = np.array([10 * np.cos(a) + 0.01 * k, 10 * np.sin(a), 0.5 * np.sin(0.1 * k)])
        T.append(_T(Rwb.T, -Rwb.T @ p))
    edges = [(i, i + 1) for i in range(nv - 1)]
    edges += [(i, j) for i in range(nv) for j in range(i + 2, min(nv, i + window + 1)) if (i + j) % 2 == 0]
    L = max(nv // 10, 3)
    loops = [(int(rng.integers(0, L)), nv - 1 - int(rng.integers(0, L))) for _ in range(n_loops)]
    edges += loops
    meas, info = [], []
    for i, j in edges:
        Zm = np.linalg.inv(T[i]) @ T[j]
        Zm[:3, :3] = Zm[:3, :3] @ _rot(rng.normal(size=3) * 1e-3)
        Zm[:3, 3] += rng.normal(size=3) * 3e-3
        meas.append(_p12(Zm))
        A = rng.normal(size=(6, 6)) * 0.1
        info.append(np.diag(np.concatenate([np.full(3, 50.0), np.full(3, 200.0)]) * rng.uniform(0.5, 2.0, 6)) + A @ A.T)
    est = []
    drift = np.eye(4)
    for k in range(nv):
        d = _T(_rot(rng.normal(size=3) * 2e-3), rng.normal(size=3) * 5e-3)
        drift = drift @ d
        est.append(_p12(T[k] @ drift) if k not in fixed else _p12(T[k]))
    fx = np.zeros(nv, np.uint8); fx[list(fixed)] = 1
    e = np.array(edges, np.int32)
    return dict(nv=nv, pose=np.array(est), ei=e[:, 0].copy(), ej=e[:, 1].copy(), meas=np.array(meas), info=np.array(info), fixed=fx)
