"""The marginalization step (IMU/marginalization.cpp:330-372) in mpmath, shared by make_marg_exact.py (40 digits, the device's J and r)
and make_marg_quad.py (50 digits, the quad oracle's J and r): A = J^T J, the eigen-decomposition of the dropped block Amm, the
thresholded pseudo-inverse, the Schur complement A', b', and what the prior is defined by — A' restricted to its eigenvalues above eps,
the projection of b' on that eigenspace, r0^T r0 = b'^T A'^+ b'.  The working precision is the caller's mp.mp.dps."""
import mpmath as mp
import numpy as np


def exact_mp(J, r, m, n, eps):
    """J (R x pos) and r (R) as arrays of floats or of mpmath numbers -> dict of mpmath results"""
    R, pos = J.shape
    Jm = mp.matrix(J.tolist()); rm = mp.matrix(r.tolist())
    A = Jm.T * Jm; b = Jm.T * rm
    W = mp.matrix(m, m)
    if m:
        E, Q = mp.eigsy(A[0:m, 0:m])
        for i in range(m):
            if E[i] > eps:
                W[i, i] = 1 / E[i]
        Ainv = Q * W * Q.T
        Ar = A[m:pos, m:pos] - A[m:pos, 0:m] * Ainv * A[0:m, m:pos]
        br = b[m:pos, 0] - A[m:pos, 0:m] * Ainv * b[0:m, 0]
    else:
        E = []
        Ar = A[m:pos, m:pos]; br = b[m:pos, 0]
    E2, Q2 = mp.eigsy(Ar)
    r0r0 = mp.mpf(0)
    drop = [i for i in range(n) if not E2[i] > eps]
    Ath = Ar.copy(); bp = br.copy()
    for i in range(n):
        if E2[i] > eps:
            vb = sum(Q2[k, i] * br[k] for k in range(n))
            r0r0 += vb * vb / E2[i]
    for i in drop:      # (the discarded directions are taken out: far fewer than the kept ones)
        vb = sum(Q2[k, i] * br[k] for k in range(n))
        for a in range(n):
            bp[a] -= Q2[a, i] * vb
            for c in range(n):
                Ath[a, c] -= E2[i] * Q2[a, i] * Q2[c, i]
    return dict(Ar=Ar, br=br, r0r0=r0r0, lam_mm=[E[i] for i in range(m)], lam_r=[E2[i] for i in range(n)], Ath=Ath, bproj=bp)


def to_f64(M):
    return np.array(M.tolist(), dtype=float)


def exact(J, r, m, n, eps):
    """(A', b', r0^T r0, eigenvalues of Amm, eigenvalues of A') rounded to fp64"""
    x = exact_mp(J, r, m, n, eps)
    return (to_f64(x["Ar"]), to_f64(x["br"]).ravel(), float(x["r0r0"]), np.array([float(v) for v in x["lam_mm"]]), np.array([float(v) for v in x["lam_r"]]))
