"""Extended-precision reference for the reduced-camera solve (numpy only), and the norm the solver tests measure in.

The pose systems of a window have condition numbers of 1e8 .. 1e9 and solutions whose entries span eight decades (gyro bias against
position), so `max |x - xref| / max |x|` says nothing about the small variables.  The tests measure instead

    E_D(x) = max_i d_i |x_i - xref_i| / max_i d_i |xref_i|,        d_i = sqrt(H_ii)

— the diagonal of the energy norm: it weighs a bias entry of 1e-7 under a diagonal of 1e10 like a position entry of 0.1 under a diagonal
of 1e2, and needs no knowledge of the variable layout.  In this norm Cholesky's a-priori forward bound is n u kappa_s, with kappa_s the
condition number of D^-1 H D^-1 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.6 with van der Sluis's scaling),
up to a modest constant: bound(H) below.

refine(): fp64 Cholesky, then iterative refinement with residuals and accumulation in 80-bit long double (mpmath at 40 digits where long
double is no wider than a double) until the component-wise relative residual stops falling.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
LD_IS_EXTENDED = bool(np.finfo(LD).eps < 1e-18)
RESIDUAL_MAX = 1e-17      # precondition of every comparison against refine(): asserted by the tests, never skipped


def _chol_solve(L, r):
    return np.linalg.solve(L.T, np.linalg.solve(L, r))


class _Factor:
    """the Cholesky factor as the correction solver of the refinement: numpy has no triangular solve, so L^-1 is formed once (one O(n^3)
    step) and every correction is two matrix-vector products.  The refinement only needs its solver to contract."""
    def __init__(self, H):
        self.Li = np.linalg.inv(np.linalg.cholesky(H))

    def __call__(self, r):
        return self.Li.T @ (self.Li @ r)


def _residual_ld(H, b, x):
    """r = b - H x and the component-wise scale |H||x| + |b|, both in long double (x is long double)"""
    Hl = H.astype(LD)
    return b.astype(LD) - Hl @ x, np.abs(Hl) @ np.abs(x) + np.abs(b.astype(LD))


def _residual_mp(H, b, x):
    """the same with mpmath; x is a list of mpf.  Returns (r, scale) as lists of mpf"""
    import mpmath
    r, s = [], []
    for i in range(len(b)):
        row = H[i]
        acc = mpmath.mpf(float(b[i])); sc = abs(acc)
        for j in np.flatnonzero(row):
            t = mpmath.mpf(float(row[j])) * x[j]
            acc -= t; sc += abs(t)
        r.append(acc); s.append(sc)
    return r, s


def refine(H, b, max_iter=40, solve=None):
    """(x, omega): x solves H x = b to extended precision, as long double (a double-double pair folded into it where mpmath did the work);
    omega = max_i |b - Hx|_i / (|H||x| + |b|)_i of the returned x, which the caller holds against RESIDUAL_MAX.
    H given as long double is taken at that width in the residual (its fp64 rounding is factored for the corrections); solve: the
    _Factor of H, for a caller that refines many right-hand sides of one matrix."""
    Hw = H if (LD_IS_EXTENDED and getattr(H, "dtype", None) == LD) else None
    H = np.ascontiguousarray(H, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if solve is None:
        solve = _Factor(H)
    if LD_IS_EXTENDED:
        if Hw is None:
            Hw = H
        x = solve(b).astype(LD)
        best, best_x = np.inf, x
        for _ in range(max_iter):
            r, s = _residual_ld(Hw, b, x)
            om = float(np.max(np.abs(r) / np.where(s > 0, s, LD(1))))
            if om >= best:
                break
            best, best_x = om, x.copy()
            x = x + solve(r.astype(np.float64)).astype(LD)
        return best_x, best
    import mpmath
    with mpmath.workprec(136):      # 40 digits
        x = [mpmath.mpf(float(v)) for v in solve(b)]
        best, best_x = np.inf, x
        for _ in range(max_iter):
            r, s = _residual_mp(H, b, x)
            om = float(max(abs(ri) / (si if si > 0 else mpmath.mpf(1)) for ri, si in zip(r, s)))
            if om >= best:
                break
            best, best_x = om, list(x)
            dx = solve(np.array([float(ri) for ri in r]))
            x = [xi + mpmath.mpf(float(d)) for xi, d in zip(x, dx)]
        hi = np.array([float(v) for v in best_x])
        lo = np.array([float(v - mpmath.mpf(float(h))) for v, h in zip(best_x, hi)])
        return hi.astype(LD) + lo.astype(LD), best


def scaled_error(x, xref, H):
    """E_D: max_i d_i |x_i - xref_i| / max_i d_i |xref_i| with d = sqrt(diag H); the difference is taken in long double"""
    d = np.sqrt(np.diag(np.asarray(H, dtype=np.float64))).astype(LD)
    xr = np.asarray(xref, dtype=LD)
    num = np.max(d * np.abs(np.asarray(x).astype(LD) - xr))
    den = np.max(d * np.abs(xr))
    return float(num / den) if den > 0 else float(num)


def kappa_s(H):
    """condition number of D^-1 H D^-1"""
    H = np.asarray(H, dtype=np.float64)
    d = np.sqrt(np.diag(H))
    ev = np.linalg.eigvalsh(H / np.outer(d, d))
    return float(ev[-1] / ev[0])


def bound(H):
    """n u kappa_s(H): what a Cholesky solve in fp64 may lose in the E_D norm"""
    return H.shape[0] * U * kappa_s(H)


def cpu_solvers(H, b, xref=None):
    """the spread among correct fp64 solvers on (H, b): Cholesky + two triangular solves, the same on the reversed ordering, and
    inv(L)^T (inv(L) b).  Returns the largest E_D of the three against refine(H, b) (or the xref given)."""
    H = np.asarray(H, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if xref is None:
        xref, om = refine(H, b)
        assert om <= RESIDUAL_MAX, om
    L = np.linalg.cholesky(H)
    x1 = _chol_solve(L, b)
    x2 = _chol_solve(np.linalg.cholesky(H[::-1, ::-1]), b[::-1])[::-1]
    Li = np.linalg.inv(L)
    x3 = Li.T @ (Li @ b)
    return max(scaled_error(x, xref, H) for x in (x1, x2, x3))


# ---- synthetic matrices of the direct-entry tests ------------------------------------------------------------------------------------------
def graded_spd(n, g, seed):
    """A = D (M M^T / n + I) D with D = diag(10^(g i / n)): condition number beyond 10^(2 g), kappa_s of a few units"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n))
    D = 10.0 ** (g * np.arange(n) / n)
    A = (M @ M.T / n + np.eye(n)) * np.outer(D, D)
    return 0.5 * (A + A.T), rng.normal(size=n) * D


def block_tridiagonal_spd(n, seed, blk=15, coupling=0.4999):
    """15 x 15 diagonal blocks with weak coupling between neighbours, the shape of the IMU chain: block row k is
    [-c Q_{k-1}, I, -c Q_k^T] with orthogonal Q, positive definite for c < 1/2 with smallest eigenvalue >= 1 - 2c, so kappa_s <~ 2 / (1 - 2c)
    = 1e4 at the default; then scaled by a random diagonal over four decades (which kappa_s does not see)."""
    rng = np.random.default_rng(seed)
    A = np.eye(n)
    for a in range(0, n - blk, blk):
        e, f = a + blk, min(n, a + 2 * blk)
        Q = np.linalg.qr(rng.normal(size=(blk, blk)))[0]
        A[e:f, a:e] = -coupling * Q[:f - e]
        A[a:e, e:f] = A[e:f, a:e].T
    D = 10.0 ** rng.uniform(-2, 2, size=n)
    A = A * np.outer(D, D)
    return 0.5 * (A + A.T), rng.normal(size=n) * D
