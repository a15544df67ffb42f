"""The Levenberg loop of pgo_ref.optimize with H assembled as a scipy.sparse matrix and solved by a sparse LU, for pose graphs too large
for pgo_ref's dense N x N assembly (tens of thousands of keyframes).  Edge errors, Jacobians, chi2 and the oplus are pgo_ref's own;
the trace, the stats and the lambda schedule are laid out as there.  The LU runs with a symmetric fill-reducing permutation and
diagonal pivots only, so U's diagonal holds the pivots of the Cholesky factorisation of H + lambda I in that order: a pivot <= 0 (or a
singular matrix) counts as a failed solve (tempChi = DBL_MAX), as the device's Cholesky does."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from .pgo_ref import DBL_MAX, ORTHO_AFTER, chi2_edges, edge_error, edge_jacobians, from_mqt, iso_inv, iso_mul, join, mm, split


def optimize(pose12, ei, ej, meas12, info=None, fixed=None, iters=100, user_lambda=0.0, tau=1e-5, max_trials=10, lower=1.0 / 3.0,
             upper=2.0 / 3.0):
    """pgo_ref.optimize without the initial guess, sparse.  Returns the same dict."""
    X = np.array(pose12, np.float64).reshape(-1, 12)
    nv = len(X)
    ei = np.asarray(ei, np.int64); ej = np.asarray(ej, np.int64)
    ne = len(ei)
    Z = np.asarray(meas12, np.float64).reshape(ne, 12)
    om = np.tile(np.eye(6), (ne, 1, 1)) if info is None else np.asarray(info, np.float64).reshape(ne, 6, 6)
    fx = np.zeros(nv, bool) if fixed is None else np.asarray(fixed).astype(bool)
    Zi = iso_inv(Z)
    touched = np.zeros(nv, bool); touched[ei] = True; touched[ej] = True
    free = np.flatnonzero(touched & ~fx)
    rank = -np.ones(nv, np.int64); rank[free] = np.arange(len(free))
    N = 6 * len(free)
    cnt = np.zeros(nv, np.int64)
    ortho = np.zeros(nv, np.int64)
    rk = (rank[ei], rank[ej])
    # COO pattern of the blocks (row block, column block) of every (edge, slot), entries in row-major 6 x 6 order
    ii, jj = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")

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
        J = edge_jacobians(X[ei], X[ej], Zi)
        we = np.einsum("kij,kj->ki", om, e)
        b = np.zeros(N)
        rows, cols, vals = [], [], []
        for a in range(2):
            sa = rk[a] >= 0
            np.add.at(b.reshape(-1, 6), rk[a][sa], -np.einsum("kri,kr->ki", J[a], we)[sa])
            OJ = om @ J[a]
            for bb in range(2):
                m = sa & (rk[bb] >= 0)
                blk = np.swapaxes(J[bb][m], 1, 2) @ OJ[m]          # block (rk[bb], rk[a])
                rows.append((6 * rk[bb][m])[:, None, None] + ii); cols.append((6 * rk[a][m])[:, None, None] + jj); vals.append(blk)
        H = sp.coo_matrix((np.concatenate([v.ravel() for v in vals]), (np.concatenate([r.ravel() for r in rows]),
                                                                        np.concatenate([c.ravel() for c in cols]))), shape=(N, N)).tocsc()
        return H, b

    def solve(H, b, lam):
        try:
            lu = spl.splu((H + lam * sp.identity(N, format="csc")).tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
                          options=dict(SymmetricMode=True))
        except RuntimeError:
            return np.zeros(N), False
        if not np.all(lu.U.diagonal() > 0):
            return np.zeros(N), False
        return lu.solve(b), True

    def oplus(X, x):      # pgo_ref.optimize's oplus (orthogonalizeAfter counts every call)
        X = X.copy()
        Xn = iso_mul(X[free], from_mqt(x.reshape(-1, 6)))
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
            lam = user_lambda if user_lambda > 0 else tau * np.max(np.abs(H.diagonal()))
            ni = 2.0
        qmax, rho = 0, 0.0
        while True:
            x, ok = solve(H, b, lam)
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
