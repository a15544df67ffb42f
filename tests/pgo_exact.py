"""Extended-precision reference of the loop-closure pose graph (plba_optimize_pose_graph, the H of plba_pose_graph_marginals); numpy only.

Written from include/plba_g2o/types_slam3d.h (VertexSE3::oplusImpl, EdgeSE3::computeError / linearizeOplus, from_mqt / unit_q), from
include/plba_g2o/g2o_compat.h (edgeChi2, buildHost, the Levenberg branch of optimizeHost, computeInitialGuess) and from Eigen's published
Quaternion(Matrix3) / toRotationMatrix, which g2o's toVectorMQT / fromVectorMQT call; not from tests/pgo_ref.py and not from
csrc/plba_pgo.hip.  Poses are 12-vectors (R row-major, t).

Every function takes the working type `dt` as tests/lba_ref.py does: np.float64, or lba_ref.wide() (long double where it is extended, else
40-digit mpmath); the arithmetic is element-wise operations and axis sums only, so that every type runs the same text.  The damped
system of a trial is solved, in the wide type, by lba_ref._solve: solver_ref.refine on the double rounding of the matrix, then corrections
against the wide matrix, so that the step is that of the wide system; in float64 by a plain fp64 Cholesky, the rounding of which belongs
to the noise of the rule.

run() records what the rule of the exactness tests needs: per evaluation of the edges the R_to_q branch of every edge, the value each
comparison of that branch tested, q.w before the flip and whether unit_q flipped; per oplus w2 = 1 - |u_r|^2 of every free vertex.

The rule: a quantity is held to max(FACTOR * noise, m u |value|), noise = |fp64 run - wide run| in the maximum norm of the
quantity, m = terms of the longest sum behind it.  m: 6 ne for a chi2 (and for rho, a difference of two chi2 over scale); 36 x the sources
of the block for an H block (the 6 x 6 x 6 products of J^T O J per source; lambda of the first iteration is tau x the largest diagonal
entry, so it takes the busiest diagonal block's m, and later lambdas are that times a few factors); 6 n + 1 for scale (one product pair
per dimension), against the sum of the MAGNITUDES of its terms, which have either sign, plus the backward error of an fp64 solve; rho = (chi2_current - chi2_trial) / scale takes the
floors of its three constituents through that formula, so that the cancellation of a small decrease is counted; 64 for a pose entry
(lba_ref.tolerances).  Each column of the trace (lambda, chi2_current, chi2_trial, scale, rho over the compared rows) is one quantity in its
maximum norm."""
import numpy as np

from . import lba_ref as LR
from . import solver_ref as SR
from .lba_ref import _b, _mm, _mv, _prec, _sqrt, _tr, _zeros, cast, f64

U = SR.U
FACTOR = LR.FACTOR
MARGIN = LR.MARGIN
DBL_MAX = float(np.finfo(np.float64).max)
ORTHO_AFTER = 1000      # VertexSE3::orthogonalizeAfter
# today's bars of tests/test_pgo.py: a tolerance of the rule may only be tighter
LIMITS = dict(poses=1e-8, chi2_initial_rel=1e-12, lam_rel=1e-9, chi2_current_rel=1e-9)
FIELDS_EXACT = ("iteration", "trial", "accepted", "solver_ok")
FIELDS_HELD = ("lam", "chi2_current", "chi2_trial", "scale", "rho")


def split(X):
    return X[..., :9].reshape(X.shape[:-1] + (3, 3)), X[..., 9:12]


def join(R, t):
    return np.concatenate([R.reshape(R.shape[:-2] + (9,)), t], -1)


def iso_mul(a, b):      # slam3d_detail::mul
    Ra, ta = split(a); Rb, tb = split(b)
    return join(_mm(Ra, Rb), _mv(Ra, tb) + ta)


def iso_inv(a):      # slam3d_detail::inv
    R, t = split(a)
    return join(_tr(R), -_mv(_tr(R), t))


def _stack(parts):
    return np.stack(parts, -1)


def q_to_R(q):
    """Eigen toRotationMatrix of (x, y, z, w)"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = _stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)])
    return R.reshape(R.shape[:-1] + (3, 3))


def R_to_q(R):
    """Eigen Quaternion(Matrix3): (q = (x, y, z, w), branch 0 .. 3, trace, gap).  Branch 0: trace > 0; else i = the largest diagonal entry
    (the first of equals) and branch 1 + i.  gap = the largest diagonal entry minus the second largest: what the comparisons among the
    diagonal entries decide by."""
    m = lambda i, j: R[..., i, j]
    d0, d1, d2 = m(0, 0), m(1, 1), m(2, 2)
    tr = d0 + d1 + d2

    def root(arg):
        t = _sqrt(np.where(_b(arg > 0), arg, arg * 0 + 1))
        return t, 0.5 / t
    t, s = root(tr + 1)
    q0 = _stack([(m(2, 1) - m(1, 2)) * s, (m(0, 2) - m(2, 0)) * s, (m(1, 0) - m(0, 1)) * s, 0.5 * t])
    t, s = root(d0 - d1 - d2 + 1)
    q1 = _stack([0.5 * t, (m(1, 0) + m(0, 1)) * s, (m(2, 0) + m(0, 2)) * s, (m(2, 1) - m(1, 2)) * s])
    t, s = root(d1 - d2 - d0 + 1)
    q2 = _stack([(m(0, 1) + m(1, 0)) * s, 0.5 * t, (m(2, 1) + m(1, 2)) * s, (m(0, 2) - m(2, 0)) * s])
    t, s = root(d2 - d0 - d1 + 1)
    q3 = _stack([(m(0, 2) + m(2, 0)) * s, (m(1, 2) + m(2, 1)) * s, 0.5 * t, (m(1, 0) - m(0, 1)) * s])
    c0 = _b(tr > 0)
    c1 = _b(d0 >= d1) & _b(d0 >= d2)
    c2 = _b(d1 > d0) & _b(d1 >= d2)
    branch = np.where(c0, 0, np.where(c1, 1, np.where(c2, 2, 3)))
    q = np.where(c0[..., None], q0, np.where(c1[..., None], q1, np.where(c2[..., None], q2, q3)))
    ds = np.sort(_stack([d0, d1, d2]), -1)
    return q, branch, tr, ds[..., 2] - ds[..., 1]


def unit_q(R):
    """toVectorMQT's quaternion: normalised, w >= 0.  (q, info): info = dict(branch, tr, gap, w (before the flip), flip)"""
    q, branch, tr, gap = R_to_q(R)
    q = q / _sqrt((q * q).sum(-1))[..., None]
    flip = _b(q[..., 3] < 0)
    return np.where(flip[..., None], -q, q), dict(branch=np.asarray(branch, np.int64), tr=tr, gap=gap, w=q[..., 3], flip=flip)


def hat(v):
    z = v[..., 0] * 0
    return np.stack([_stack([z, -v[..., 2], v[..., 1]]), _stack([v[..., 2], z, -v[..., 0]]), _stack([-v[..., 1], v[..., 0], z])], -2)


def edge_isometry(Xi, Xj, Zi):
    """the error isometry E = (Z^-1 Xi^-1) Xj of an edge, as a pose12"""
    return iso_mul(iso_mul(Zi, iso_inv(Xi)), Xj)


def edge_error(Xi, Xj, Zi):
    """EdgeSE3::computeError: toVectorMQT((Z^-1 Xi^-1) Xj); (e[.., 6], info of unit_q)"""
    R, t = split(edge_isometry(Xi, Xj, Zi))
    q, info = unit_q(R)
    return np.concatenate([t, q[..., :3]], -1), info


def edge_jacobians(Xi, Xj, Zi, dt):
    """EdgeSE3::linearizeOplus: (J0 = de/du_i, J1 = de/du_j), 6 x 6, rows = error"""
    B = iso_mul(iso_inv(Xi), Xj)
    RE, _ = split(iso_mul(Zi, B))
    q, _ = unit_q(RE)
    RZt, _ = split(Zi)
    _, tB = split(B)
    V = hat(q[..., :3])
    wI = q[..., 3][..., None, None] * cast(np.eye(3), dt)
    Qm, Qp = wI - V, wI + V
    J0, J1 = _zeros(Xi.shape[:-1] + (6, 6), dt), _zeros(Xi.shape[:-1] + (6, 6), dt)
    J0[..., :3, :3] = -RZt
    J0[..., :3, 3:] = 2 * _mm(RZt, hat(tB))
    J0[..., 3:, 3:] = -_mm(Qm, RZt)
    J1[..., :3, :3] = RE
    J1[..., 3:, 3:] = Qp
    return J0, J1


def chi2_edges(e, om):
    """edgeChi2 per edge: e^T O e"""
    return (e * _mv(om, e)).sum(-1)


def edge_blocks(e, J0, J1, om):
    """buildHost per edge: A00 = J0^T O J0, A11 = J1^T O J1, A10 = J1^T O J0, g0 = J0^T O e, g1 = J1^T O e"""
    we = _mv(om, e)
    OJ0, OJ1 = _mm(om, J0), _mm(om, J1)
    return _mm(_tr(J0), OJ0), _mm(_tr(J1), OJ1), _mm(_tr(J1), OJ0), _mv(_tr(J0), we), _mv(_tr(J1), we)


def from_mqt(u, dt):
    """internal::fromVectorMQT: (pose12, w2); the identity rotation where w2 = 1 - |u_r|^2 < 0"""
    w2 = 1 - (u[..., 3] * u[..., 3] + u[..., 4] * u[..., 4] + u[..., 5] * u[..., 5])
    neg = _b(w2 < 0)
    w = _sqrt(np.where(neg, w2 * 0, w2))
    R = q_to_R(_stack([u[..., 3], u[..., 4], u[..., 5], w]))
    R = np.where(neg[..., None, None], cast(np.eye(3), dt) + R * 0, R)
    return join(R, u[..., :3]), w2


def orthogonalized(X):
    """approximateNearestOrthogonalMatrix: R -= 0.5 R (R^T R - I)"""
    R, t = split(X)
    E = _mm(_tr(R), R)
    i = np.arange(3)
    E[..., i, i] = E[..., i, i] - 1
    return join(R - 0.5 * _mm(R, E), t)


def oplus(X, u, cnt, dt):
    """VertexSE3::oplusImpl over a batch: (X fromVectorMQT(u), the counters, w2, which re-orthogonalised)"""
    D, w2 = from_mqt(u, dt)
    Xn = iso_mul(X, D)
    cnt = cnt + 1
    fire = cnt > ORTHO_AFTER
    if fire.any():
        Xn = np.where(fire[..., None], orthogonalized(Xn), Xn)
        cnt = np.where(fire, 0, cnt)
    return Xn, cnt, w2, fire


class Graph:
    """the inputs in the working type; the free ranks (vertices an edge touches that are not fixed, ascending)"""
    def __init__(self, g, dt):
        self.dt = dt
        self.X0 = cast(np.asarray(g["pose"], np.float64).reshape(-1, 12), dt)
        self.nv = len(self.X0)
        self.ei, self.ej = np.asarray(g["ei"], np.int64), np.asarray(g["ej"], np.int64)
        self.ne = len(self.ei)
        self.Z = cast(np.asarray(g["meas"], np.float64).reshape(self.ne, 12), dt)
        self.Zi = iso_inv(self.Z)
        info = g.get("info")
        self.om = cast(np.tile(np.eye(6), (self.ne, 1, 1)) if info is None else np.asarray(info, np.float64).reshape(self.ne, 6, 6), dt)
        self.fixed = np.zeros(self.nv, bool) if g.get("fixed") is None else np.asarray(g["fixed"]).astype(bool)
        touched = np.zeros(self.nv, bool); touched[self.ei] = True; touched[self.ej] = True
        self.free = np.flatnonzero(touched & ~self.fixed)
        self.fr = -np.ones(self.nv, np.int64); self.fr[self.free] = np.arange(len(self.free))
        self.n = len(self.free)

    def errors(self, X):
        return edge_error(X[self.ei], X[self.ej], self.Zi)

    def chi2(self, X):
        """(sum of e^T O e, per edge, info)"""
        e, info = self.errors(X)
        c = chi2_edges(e, self.om)
        return c.sum(), c, info

    def linearize(self, X):
        """(H, b, per-edge blocks, e, info): buildHost over the free ranks, both triangles"""
        e, info = self.errors(X)
        J0, J1 = edge_jacobians(X[self.ei], X[self.ej], self.Zi, self.dt)
        blk = edge_blocks(e, J0, J1, self.om)
        A00, A11, A10, g0, g1 = blk
        n = self.n
        H = _zeros((n, n, 6, 6), self.dt); b = _zeros((n, 6), self.dt)
        for k in range(self.ne):
            a, c = self.fr[self.ei[k]], self.fr[self.ej[k]]
            if a >= 0:
                H[a, a] = H[a, a] + A00[k]; b[a] = b[a] - g0[k]
            if c >= 0:
                H[c, c] = H[c, c] + A11[k]; b[c] = b[c] - g1[k]
            if a >= 0 and c >= 0:
                H[c, a] = H[c, a] + A10[k]; H[a, c] = H[a, c] + _tr(A10[k])
        # the largest sum of magnitudes behind an entry of b and of H, and the busiest block row: for the floors of what is computed from them
        ba, Ha = np.zeros((n, 6)), np.zeros((n, n))
        for k in range(self.ne):
            a, c = self.fr[self.ei[k]], self.fr[self.ej[k]]
            if a >= 0:
                ba[a] += np.abs(f64(g0[k])); Ha[a, a] += float(np.abs(f64(A00[k])).max())
            if c >= 0:
                ba[c] += np.abs(f64(g1[k])); Ha[c, c] += float(np.abs(f64(A11[k])).max())
            if a >= 0 and c >= 0:
                Ha[a, c] += float(np.abs(f64(A10[k])).max()); Ha[c, a] += float(np.abs(f64(A10[k])).max())
        info = dict(info, b_abs=float(ba.max()) if n else 0.0, H_abs=float(Ha.max()) if n else 0.0, row_blocks=int((Ha > 0).sum(-1).max()) if n else 0)
        return np.swapaxes(H, 1, 2).reshape(6 * n, 6 * n), b.reshape(-1), blk, e, info


def initial_guess(g, dt, stats=None):
    """the facade's computeInitialGuess: breadth first from the fixed vertices in the order the edges name them; each `from` of a frontier
    takes the edges in insertion order: to = from Z (from is vertex 0 of the edge), to = from Z^-1 otherwise (counted in stats["inverse"])"""
    G = Graph(g, dt)
    stats = {} if stats is None else stats
    stats["inverse"] = 0
    X = G.X0.copy()
    inc = [[] for _ in range(G.nv)]
    for k in range(G.ne):
        inc[G.ei[k]].append(k); inc[G.ej[k]].append(k)
    done = np.zeros(G.nv, bool)
    front = []
    for k in range(G.ne):
        for v in (G.ei[k], G.ej[k]):
            if G.fixed[v] and not done[v]:
                done[v] = True; front.append(v)
    while front:
        nxt = []
        for f in front:
            for k in inc[f]:
                to = G.ej[k] if G.ei[k] == f else G.ei[k]
                if done[to] or G.fixed[to]:
                    continue
                X[to] = iso_mul(X[f], G.Z[k] if G.ei[k] == f else G.Zi[k])
                stats["inverse"] += int(G.ei[k] != f)
                done[to] = True; nxt.append(to)
        front = nxt
    return X


def _solve(H, b, lam, dt, variant=0):
    """(x, ok, omega, smallest Cholesky pivot over N u max diag, the infinity norm of S) of S x = b, S = H + lam I.  In the wide type the step of the wide system
    (lba_ref._solve); in float64 a plain fp64 Cholesky solve, so that the noise of the rule (fp64 run - wide run) carries the rounding of
    an fp64 factorisation of this system, its conditioning included, as every fp64 solver of it does."""
    N = len(b)
    S = H.copy()
    i = np.arange(N)
    S[i, i] = S[i, i] + lam
    S64 = f64(S)
    try:
        if dt is np.float64:      # variant: another fp64 factorisation of the same system (1: LU with pivoting, 2: Cholesky from the last unknown up)
            L = np.linalg.cholesky(S64)
            if variant == 1:
                x = np.linalg.solve(S64, f64(b))
            elif variant == 2:
                Lr = np.linalg.cholesky(S64[::-1, ::-1])
                x = np.linalg.solve(Lr.T, np.linalg.solve(Lr, f64(b)[::-1]))[::-1].copy()
            else:
                x = np.linalg.solve(L.T, np.linalg.solve(L, f64(b)))
            om = 0.0
        else:
            x, om = LR._solve(S, b, dt)
    except (LR.SolverFailed, np.linalg.LinAlgError):
        return _zeros(N, dt), False, 0.0, 0.0, 0.0
    piv = np.diag(np.linalg.cholesky(S64)) ** 2
    return x, True, om, float(piv.min() / (N * U * np.abs(np.diag(S64)).max())), float(np.abs(S64).sum(-1).max())


def run(g, dt=np.float64, iters=3, user_lambda=0.0, initial=False, tau=1e-5, max_trials=10, lower=1.0 / 3.0, upper=2.0 / 3.0, cnt0=0, solve_variant=0):
    """optimizeHost, Levenberg branch.  Returns what pgo_ref.optimize returns (poses, chi2_initial, chi2_final, lambda_final, iterations,
    trials, stop_reason, solver_failures, trace, ortho) with, besides,
        trace[i]["ev"]     info of the trial's evaluation of the edges (unit_q)         trace[i]["w2"]   w2 per free vertex of its oplus
        trace[i]["pivot"]  smallest pivot / (N u max diag) of its factorisation         trace[i]["x"]    its step
        lin[it]            info of the iteration's linearisation                         first            dict(H, b, blocks, e) of iteration 0
        after[k]           dict(poses, chi2_final, lambda_final, iterations, trials, stop_reason) after k iterations
        omega              the largest residual of refine() over the trials"""
    with _prec(dt):
        G = Graph(g, dt)
        ig = {}
        X = initial_guess(g, dt, ig) if (initial and G.ne) else G.X0.copy()
        cnt = np.full(G.n, int(cnt0), np.int64)
        ortho = np.zeros(G.nv, np.int64)
        out = dict(init_inverse=ig.get("inverse", 0),trace=[], lin=[], after={}, iterations=0, trials=0, stop_reason=0, solver_failures=0, ortho=ortho, omega=0.0, n=G.n, ne=G.ne, X_start=X.copy())
        chi, _, info = G.chi2(X)
        out.update(chi2_initial=chi, chi2_final=chi, lambda_final=0.0, ev0=info)
        if iters <= 0 or G.n == 0:
            out["poses"] = X
            return out
        lam, ni = cast(0.0, dt)[()], 2.0
        for it in range(iters):
            cur, _, _ = G.chi2(X)
            H, b, blk, e, info = G.linearize(X)
            out["lin"].append(info)
            if it == 0:
                out["first"] = dict(H=H, b=b, blocks=blk, e=e)
                md = np.abs(H[np.arange(len(b)), np.arange(len(b))]).max()
                lam = cast(user_lambda, dt)[()] if user_lambda > 0 else tau * md
                ni = 2.0
            qmax, rho = 0, 0.0
            while True:
                x, ok, om, piv, s_norm = _solve(H, b, lam, dt, solve_variant)
                out["omega"] = max(out["omega"], om)
                if not ok:
                    out["solver_failures"] += 1
                Xf, cnt, w2, fire = oplus(X[G.free], x.reshape(-1, 6), cnt, dt)
                ortho[G.free] += fire
                Xt = X.copy(); Xt[G.free] = Xf
                tmp, _, ev = G.chi2(Xt)
                if not ok:
                    tmp = DBL_MAX
                scale = 1e-3 + (x * (lam * x + b)).sum()
                scale_abs = 1e-3 + float(np.abs(f64(x * (lam * x + b))).sum())
                rho = (cur - tmp) / scale
                out["trials"] += 1
                acc = bool(rho > 0 and np.isfinite(float(tmp)))
                out["trace"].append(dict(iteration=it, trial=qmax, accepted=int(acc), solver_ok=int(ok), lam=lam, chi2_current=cur, chi2_trial=tmp,
                                         scale=scale, scale_abs=scale_abs, solve_floor=4 * len(b) * U * s_norm * float((f64(x) ** 2).sum()), x_norm=float(np.sqrt((f64(x) ** 2).sum())), rho=rho, ev=ev, w2=w2, pivot=piv, x=x))
                if acc:
                    alpha = 1 - (2 * rho - 1) ** 3
                    alpha = alpha if alpha < upper else upper
                    lam = lam * (alpha if alpha > lower else lower); ni = 2.0; cur = tmp; X = Xt
                else:
                    lam = lam * ni; ni *= 2.0
                    if not np.isfinite(float(lam)):
                        break
                qmax += 1
                if not (rho < 0 and qmax < max_trials):
                    break
            out["iterations"] += 1
            out["chi2_final"], out["lambda_final"] = cur, lam
            stop = qmax == max_trials or rho == 0 or not np.isfinite(float(lam))
            if stop:
                out["stop_reason"] = 1
            out["after"][it + 1] = dict(poses=X.copy(), chi2_final=cur, lambda_final=lam, iterations=it + 1, trials=out["trials"], stop_reason=out["stop_reason"])
            if stop:
                break
        out["poses"] = X
        return out


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def _f(v):
    """float64 of a scalar or an array of any working type, at least 1-d"""
    return np.asarray(f64(np.atleast_1d(np.asarray(v))), np.float64)


def _noise_tol(a, b, m):
    a, b = _f(a), _f(b)
    noise = float(np.abs(a - b).max()) if a.size else 0.0
    return noise, max(FACTOR * noise, m * U * (float(np.abs(b).max()) if b.size else 0.0))


def block_sources(g):
    """per block of pgo_cov_ref.block_list(g): the number of (edge, slot) sources summed into it"""
    from . import pgo_cov_ref as PC
    fr, _ = PC.free_ranks(g)
    rows, cols = PC.block_list(g)
    idx = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(rows, cols))}
    cnt = np.zeros(len(rows), np.int64)
    for a, b in zip(fr[np.asarray(g["ei"])], fr[np.asarray(g["ej"])]):
        if a >= 0:
            cnt[idx[(int(a), int(a))]] += 1
        if b >= 0:
            cnt[idx[(int(b), int(b))]] += 1
        if a >= 0 and b >= 0:
            cnt[idx[(int(max(a, b)), int(min(a, b)))]] += 1
    return rows, cols, cnt


def h_blocks(g, r):
    """the blocks of block_list(g) (row rank >= column rank) of the run's first H, in fp64: (nblk, 6, 6)"""
    rows, cols, _ = block_sources(g)
    H = f64(r["first"]["H"])
    return np.array([H[6 * a:6 * a + 6, 6 * c:6 * c + 6] for a, c in zip(rows, cols)])


def _decision(v, v64, against=0.0, m=64):
    """margin / noise of the comparison of v with `against` (smallest over an array)"""
    v, v64 = _f(v), _f(v64)
    noise = np.maximum(np.abs(v - v64), m * U * np.maximum(np.abs(v), abs(against)))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(noise > 0, np.abs(v - against) / noise, np.inf)
    return float(np.min(r)) if r.size else np.inf


def _ev_margin(e6, ew):
    """the R_to_q comparisons and q.w < 0 of one evaluation of the edges; 0 where a discrete outcome differs between the runs"""
    if not (np.array_equal(e6["branch"], ew["branch"]) and np.array_equal(e6["flip"], ew["flip"])):
        return 0.0
    worst = min(_decision(ew["tr"], e6["tr"]), _decision(ew["w"], e6["w"]))
    off = ew["branch"] > 0
    if off.any():
        worst = min(worst, _decision(ew["gap"][off], e6["gap"][off]))
    return worst


def horizon(r64, rw):
    """(T, margins): the number of leading trials every decision of which has MARGIN x the noise of the compared quantity between the two
    runs of the reference (condition (b)), and the margin / noise of each of those trials.  Decisions of a trial: the R_to_q comparisons
    and q.w < 0 of every edge in its iteration's linearisation and in its own evaluation, w2 < 0 of every vertex, the pivots of the
    factorisation, rho > 0 / rho < 0."""
    T, margins = 0, []
    if _ev_margin(r64["ev0"], rw["ev0"]) < MARGIN:
        return 0, margins
    for a, b in zip(r64["trace"], rw["trace"]):
        if any(a[k] != b[k] for k in FIELDS_EXACT):
            break
        mg = min(_ev_margin(r64["lin"][a["iteration"]], rw["lin"][b["iteration"]]), _ev_margin(a["ev"], b["ev"]), _decision(b["w2"], a["w2"]))
        mg = min(mg, b["pivot"], a["pivot"])      # a pivot of 1 unit = N u max diag, the backward error of the factorisation
        if b["solver_ok"]:
            mg = min(mg, _decision(b["rho"], a["rho"], m=6 * rw["ne"]))
        if mg < MARGIN:
            break
        margins.append(mg)
        T += 1
    return T, margins


def tolerances(g, r64, rw, T=None):
    """(tol, noise, lim) under the rule for chi2_initial, the blocks of H ("H": per block), every held field of the first T trace rows
    (key (field, row)) and the poses after k iterations (key ("poses", k)) for every k whose trials all lie within T.  lim: today's bar
    where there is one (condition (a): 8 noise must lie below it, and the tolerance is the tighter of the two)."""
    if T is None:
        T, _ = horizon(r64, rw)
    tol, noise, lim = {}, {}, {}
    ne, n = rw["ne"], rw["n"]
    noise["chi2_initial"], tol["chi2_initial"] = _noise_tol(r64["chi2_initial"], rw["chi2_initial"], 6 * ne)
    lim["chi2_initial"] = LIMITS["chi2_initial_rel"] * abs(float(rw["chi2_initial"]))
    if "first" in rw:
        _, _, cnt = block_sources(g)
        B6, Bw = h_blocks(g, r64), h_blocks(g, rw)
        nb = np.abs(B6 - Bw).reshape(len(cnt), -1).max(-1)
        noise["H"] = nb
        tol["H"] = np.maximum(FACTOR * nb, 36 * cnt * U * np.abs(Bw).reshape(len(cnt), -1).max(-1))
        mH = 36 * int(cnt.max())
        for i in range(min(T, len(rw["trace"]))):
            a, b = r64["trace"][i], rw["trace"][i]
            for f, m in (("lam", mH), ("chi2_current", 6 * ne), ("chi2_trial", 6 * ne)):
                noise[(f, i)], tol[(f, i)] = _noise_tol(a[f], b[f], m)
            # scale = 1e-3 + sum x_i (lam x_i + b_i): its terms have either sign, so the floor is (6 n + 1) u x the sum of their magnitudes,
            # plus what an fp64 factorisation leaves in x: a backward-stable solve gives (S + dS) x^ = b, |dS| <= N u |S|, and with b = S x
            # scale - 1e-3 = x^T (S + lam I) x moves by 2 x^T (I + lam S^-1) dS x, |.| <= 4 N u |S| |x|^2 as lam S^-1 <= I (solve_floor);
            # rho = (chi2_current - chi2_trial) / scale: the floors of its three constituents through that formula
            cur, tmp, sc, rho = (abs(float(b[f])) for f in ("chi2_current", "chi2_trial", "scale", "rho"))
            # and what the rounding of b and of H leaves in it: with x = S^-1 b, 2 x^T (I + lam S^-1) db and x^T (I + lam S^-1) dH x, so at most
            # 4 |x| sqrt(N) max|db| + 4 |x|^2 |dH|, max|db| <= (sources + 42) u x the largest sum of magnitudes behind an entry of b (42 products
            # in a g = J^T O e), |dH| <= 6 x (blocks in the busiest block row) x (sources + 42) u x the same for H
            li = rw["lin"][b["iteration"]]
            srcs = int(cnt.max())
            fl_sc = (6 * n + 1) * U * b["scale_abs"] + b["solve_floor"] + 4 * b["x_norm"] * (6 * n) ** 0.5 * (srcs + 42) * U * li["b_abs"] \
                + 4 * b["x_norm"] ** 2 * 6 * li["row_blocks"] * (srcs + 42) * U * li["H_abs"]
            fl_rho = (6 * ne * U * (cur + tmp) + rho * fl_sc) / sc if b["solver_ok"] else 0.0
            for f, fl in (("scale", fl_sc), ("rho", fl_rho)):
                noise[(f, i)] = float(abs(float(a[f]) - float(b[f])))
                tol[(f, i)] = max(FACTOR * noise[(f, i)], fl)
            lim[("lam", i)] = LIMITS["lam_rel"] * abs(float(b["lam"]))
            lim[("chi2_current", i)] = LIMITS["chi2_current_rel"] * abs(float(b["chi2_current"]))
        # a column of the trace is one quantity, held in its maximum norm over the compared rows (element by element the difference of two
        # roundings is now and then zero, the largest element of an array is not: lba_ref.tolerances); today's bars stay per row
        rows = range(min(T, len(rw["trace"])))
        for f in FIELDS_HELD:
            if len(rows):
                nz, tl = max(noise[(f, i)] for i in rows), max(tol[(f, i)] for i in rows)
                for i in rows:
                    noise[(f, i)], tol[(f, i)] = nz, tl
        for k, ak in rw["after"].items():
            if ak["trials"] <= T and k in r64["after"]:
                noise[("poses", k)], tol[("poses", k)] = _noise_tol(r64["after"][k]["poses"], ak["poses"], 64)
                lim[("poses", k)] = LIMITS["poses"]
    for k in lim:
        if k in tol:
            tol[k] = min(tol[k], lim[k])
    return tol, noise, lim


def tolerances_tighten(tol, noise, lim):
    """condition (a): the worst FACTOR * noise / today's bar over the quantities that have a bar (must be < 1)"""
    return max([FACTOR * noise[k] / lim[k] for k in lim if k in noise and lim[k] > 0] + [0.0])


def hold(label, key, value, ref, tol, noise, bad):
    """prints error, noise, tolerance and error / noise of one quantity and notes a miss in `bad`"""
    e = float(np.abs(_f(value) - _f(ref)).max())
    t, nz = float(np.max(tol)), float(np.max(noise))
    print("%s %-22s error %.3e  noise %.3e  tolerance %.3e  error/noise %.2f" % (label, key, e, nz, t, e / nz if nz > 0 else (np.inf if e > 0 else 0.0)))
    if not e <= t:
        bad.append((key, e, t))
    return e / nz if nz > 0 else (np.inf if e > 0 else 0.0)


def hold_run(label, g, res, r64, rw, T, iters):
    """a result in pgo_ref.optimize's layout (poses, chi2_initial, trace, iterations, trials), produced with max_iters = iters, against
    the wide run under the rule: discrete fields exactly and every held field of the rows within the horizon T, the poses where every
    trial of the run lies within it.  Returns the list of misses (empty = held)."""
    tol, noise, _ = tolerances(g, r64, rw, T)
    bad = []
    hold(label, "chi2_initial", res["chi2_initial"], rw["chi2_initial"], tol["chi2_initial"], noise["chi2_initial"], bad)
    want = [t for t in rw["trace"] if t["iteration"] < iters]
    rows = min(T, len(want))
    if len(res["trace"]) < rows:
        bad.append(("rows", len(res["trace"]), rows))
        return bad
    for i in range(rows):
        a, b = res["trace"][i], rw["trace"][i]
        for f in FIELDS_EXACT:
            if int(a[f]) != int(b[f]):
                bad.append((f, i, a[f], b[f]))
        for f in FIELDS_HELD:
            if float(b[f]) == DBL_MAX or float(a[f]) == DBL_MAX:
                if float(a[f]) != float(b[f]):
                    bad.append((f, i, a[f], b[f]))
                continue
            hold(label, "%s[%d]" % (f, i), a[f], b[f], tol[(f, i)], noise[(f, i)], bad)
    k = min(iters, rw["iterations"])
    if ("poses", k) in tol and len(want) <= T:
        if (res["iterations"], res["trials"]) != (rw["after"][k]["iterations"], rw["after"][k]["trials"]):
            bad.append(("iterations/trials", res["iterations"], res["trials"]))
        hold(label, "poses after %d" % k, res["poses"], rw["after"][k]["poses"], tol[("poses", k)], noise[("poses", k)], bad)
    return bad
