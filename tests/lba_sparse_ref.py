"""The reference of the visual BA (tests/lba_ref.py) with the reduced camera system of a pass kept as its nonzero 6 x 6 blocks and solved
by a sparse factorisation (scipy.sparse), for windows whose 6 Nkf x 6 Nkf matrix lba_ref.step_elim cannot hold: a thousand local
keyframes and more.  Everything but the linear solve IS lba_ref: run() calls lba_ref.run with step_elim replaced by step_sparse below, so
there is one text of the observations, of the landmark elimination's arithmetic and of the pass-to-pass control.

step_sparse forms, in the working type, the same sums as step_elim (the same products, subtracted block by block in the same order of
the observation pairs), factors the fp64 rounding of S with a sparse LU and corrects the solution three times against the residual of
the wide S, as lba_ref._solve does with the dense Cholesky.  A pass's record holds S as a scipy.sparse matrix."""
from unittest import mock

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from . import lba_ref as LR


def _block_mv(Nkf, ka, kb, B, x, dt):
    """y = S x for S given by its blocks B[i] at (ka[i], kb[i]) (every ordered pair present), in the working type"""
    y = LR._zeros((Nkf, 6), dt)
    np.add.at(y, ka, LR._mv(B, x[kb]))
    return y


def step_sparse(parts, Hpp, gp, lm, lam, Nkf, dt):
    """lba_ref.step_elim with a block-sparse S: (dx poses [Nkf, 6], [dx landmarks per part], omega, S (csc, fp64), rhs)"""
    rhs = gp.copy()
    keep, pend = [], []
    keys = [np.arange(Nkf, dtype=np.int64) * (Nkf + 1)]      # the diagonal blocks
    for (l, loc, n, w, Jp, Jl, L, d), (Hll, gl) in zip(parts, lm):
        if L == 0:
            keep.append(None); continue
        D, ok = LR._spd_inv(LR._damp(Hll, lam), dt)
        if not ok:
            raise LR.SolverFailed
        s = np.flatnonzero(loc >= 0)
        ls, ks, Jps, Jls, ws = l[s], loc[s], Jp[s], Jl[s], w[s]
        keep.append((D, gl, ls, ks, Jps, Jls, ws))
        if not len(s):
            continue
        u = LR._mv(D[ls], Jls) * ws[:, None]
        sg = ws * (Jls * LR._mv(D, gl)[ls]).sum(-1)
        np.subtract.at(rhs, ks, Jps * sg[:, None])
        cnt = np.bincount(ls, minlength=L)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for a in range(int(cnt.max())):
            for b in range(int(cnt.max())):
                m = np.flatnonzero(cnt > max(a, b))
                ea, eb = start[m] + a, start[m] + b
                keys.append(ks[ea] * Nkf + ks[eb])
                pend.append((u, Jls, ws, Jps, ea, eb, keys[-1]))
    ukey = np.unique(np.concatenate(keys))
    ka, kb = ukey // Nkf, ukey % Nkf
    B = LR._zeros((len(ukey), 6, 6), dt)
    B[np.searchsorted(ukey, keys[0])] = LR._damp(Hpp, lam)
    for u, Jls, ws, Jps, ea, eb, key in pend:
        c = (u[ea] * Jls[eb]).sum(-1) * ws[eb]
        np.subtract.at(B, np.searchsorted(ukey, key), c[:, None, None] * Jps[ea][:, :, None] * Jps[eb][:, None, :])
    B64 = LR.f64(B)
    i6 = np.arange(6)
    rows = (6 * ka[:, None, None] + i6[None, :, None] + 0 * i6[None, None, :]).reshape(-1)
    cols = (6 * kb[:, None, None] + 0 * i6[None, :, None] + i6[None, None, :]).reshape(-1)
    S = sp.coo_matrix((B64.reshape(-1), (rows, cols)), shape=(6 * Nkf, 6 * Nkf)).tocsc()
    if not (S.diagonal() > 0).all():
        raise LR.SolverFailed
    try:
        lu = spl.splu(S, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    except RuntimeError:
        raise LR.SolverFailed
    # the corrections run in the wide type also for an fp64 evaluation (long double there), as solver_ref.refine's do: x is the solution
    # of the system as it stands in the working type, rounded once at the end
    wt = np.longdouble if dt is np.float64 else dt
    Bw, bw = LR.cast(B, wt), LR.cast(rhs, wt)
    x = LR.cast(lu.solve(LR.f64(rhs).reshape(-1)).reshape(Nkf, 6), wt)
    for _ in range(3):
        x = x + LR.cast(lu.solve(LR.f64(bw - _block_mv(Nkf, ka, kb, Bw, x, wt)).reshape(-1)).reshape(Nkf, 6), wt)
    r = np.abs(LR.f64(bw - _block_mv(Nkf, ka, kb, Bw, x, wt)))
    scale = LR.f64(_block_mv(Nkf, ka, kb, abs(Bw), abs(x), wt) + abs(bw))
    om = float((r / np.where(scale > 0, scale, 1.0)).max())
    if dt is np.float64:
        x = LR.f64(x)
    dxl = []
    for k in keep:
        if k is None:
            dxl.append(None); continue
        D, gl, ls, ks, Jps, Jls, ws = k
        v = gl.copy()
        if len(ls):
            np.subtract.at(v, ls, Jls * (ws * (Jps * x[ks]).sum(-1))[:, None])
        dxl.append(LR._mv(D, v))
    return x, dxl, om, S, rhs.reshape(-1)


def run(w, dt=np.float64, **opts):
    """lba_ref.run(form="elim") with the sparse solve of a pass; the same dictionary comes back"""
    with mock.patch.object(LR, "step_elim", step_sparse):
        return LR.run(w, dt, form="elim", **opts)
