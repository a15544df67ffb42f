"""Extended-precision reference of plba_compute_marginals (include/plba.h), beside the plain fp64 one of tests/marginals_ref.py.

Numpy only.  The arithmetic is 80-bit long double where numpy has it and mpmath at 40 digits (object arrays) otherwise, by the switch of
tests/solver_ref.py.  The inputs are the oracle's fp64 per-edge values (Jacobians, errors, information matrices): what is exact here is
every product, sum, factorisation and inverse made from them.

    Hpp      built directly: IMU PVR edges (orc.eval_pvr_edge), bias edges (J = -I, +I), the prior J0^T J0, the pose blocks of the landmark
             observations — no detour through the damped Schur complement (marginals_ref.Reference.hpp, which this pins);
    S_ref    = Hpp - sum_l W_l (B^T Hll B)^-1 W_l^T by the status rules of the header, with the absolutely accumulated |S| (every product
             taken by its absolute value) and the number of non-zero products per entry beside it;
    inverse  columns of S^-1 by solver_ref.refine(S, e_j), the residual precondition asserted on every column;
    Sigma_ll = B (Hr^-1 + Hr^-1 (sum_ab W_a^T Sigma(a, b) W_b) Hr^-1) B^T from that inverse.

The three rules the tests hold the device and the fp64 reference to are rule_S, rule_inverse and rule_landmarks below."""
import numpy as np

from oracle import oracle as orc
from tests import marginals_ref as mr
from tests import solver_ref as R

U = R.U
LD = R.LD
FACTOR = 8            # over the reference's own fp64 noise: another summation order and FMA contraction (tests/lba_ref.py); not a measurement
MARGIN = 32.0         # over the spread of correct fp64 inverses (tests/test_solver_accuracy.py)
PIV_REL = 1e-12       # the header's rule for a degenerate reduced block
PIV_CLEAR = 100.0     # no landmark of a case lies within this factor of PIV_REL


# ---- the wide number format ------------------------------------------------------------------------------------------------------------------
def wide(a):
    a = np.asarray(a)
    if R.LD_IS_EXTENDED:
        return a.astype(LD)
    import mpmath
    if a.dtype == object:
        return a
    out = np.empty(a.shape, dtype=object)
    with mpmath.workprec(136):
        for i, v in np.ndenumerate(np.asarray(a, np.float64)):
            out[i] = mpmath.mpf(float(v))
    return out


def wzeros(*shape):
    return wide(np.zeros(shape))


def narrow(a):
    return np.array(a, dtype=np.float64)


def _prec(fn):
    """run under mpmath's 40 digits where mpmath does the work"""
    def run(*a, **k):
        if R.LD_IS_EXTENDED:
            return fn(*a, **k)
        import mpmath
        with mpmath.workprec(136):
            return fn(*a, **k)
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


def _sqrt(x):
    return np.sqrt(x) if R.LD_IS_EXTENDED else x ** 0.5


def _chol(A):
    """(L, pivots) of a small symmetric matrix, in its own number format; stops at the first non-positive pivot (L is then None)"""
    n = A.shape[0]
    L = wzeros(n, n)
    piv = []
    for j in range(n):
        p = A[j, j] - sum(L[j, t] * L[j, t] for t in range(j))
        piv.append(p)
        if not p > 0:
            return None, piv
        L[j, j] = _sqrt(p)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, t] * L[j, t] for t in range(j))) / L[j, j]
    return L, piv


def _inv_from_chol(L):
    n = L.shape[0]
    Li = wzeros(n, n)
    for c in range(n):
        Li[c, c] = 1 / L[c, c]
        for i in range(c + 1, n):
            Li[i, c] = -sum(L[i, t] * Li[t, c] for t in range(c, i)) / L[i, i]
    return Li.T @ Li


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def line_axis(x):
    """the unit axis the device's basis starts from: the one of the direction's smallest component, x before y before z at a tie
    (k_cov_lm).  Evaluated in fp64 as the device does; the result does not depend on it, the cases assert which branch they reach."""
    d = x[3:] - x[:3]
    d = d / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    ax, ay, az = np.abs(d)
    return 0 if (ax <= ay and ax <= az) else (1 if ay <= az else 2)


def line_basis_wide(x):
    """B = blockdiag(N, N), N orthonormal and orthogonal to the line direction, in the wide format"""
    xw = wide(x)
    d = xw[3:] - xw[:3]
    d = d / _sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    a = wide(np.eye(3)[line_axis(np.asarray(x, np.float64))])
    n1 = _cross(d, a)
    n1 = n1 / _sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2])
    n2 = _cross(d, n1)
    B = wzeros(6, 4)
    for c in range(3):
        B[c, 0] = n1[c]; B[c, 1] = n2[c]; B[3 + c, 2] = n1[c]; B[3 + c, 3] = n2[c]
    return B


def _nz(a):
    return (np.asarray(a, np.float64) != 0).astype(np.int64)


class _Acc:
    """a P x P sum with its absolute accumulation and the count of non-zero products per entry"""
    def __init__(self, P):
        self.H, self.A, self.M = wzeros(P, P), wzeros(P, P), np.zeros((P, P), np.int64)
        self.sum_only = False

    def copy(self, sum_only=False):
        c = _Acc(0)
        c.H, c.A, c.M, c.sum_only = self.H.copy(), self.A.copy(), self.M.copy(), sum_only
        return c

    def add(self, oa, ob, Ja, Om, Jb, sign=1):
        """block (oa, ob) += sign Ja^T Om Jb; Ja, Om, Jb wide"""
        na, nb = Ja.shape[1], Jb.shape[1]
        t = Ja.T @ Om @ Jb
        self.H[oa:oa + na, ob:ob + nb] += t if sign > 0 else -t
        if self.sum_only:
            return
        self.A[oa:oa + na, ob:ob + nb] += np.abs(Ja).T @ np.abs(Om) @ np.abs(Jb)
        self.M[oa:oa + na, ob:ob + nb] += _nz(Ja).T @ _nz(Om) @ _nz(Jb)


class Exact:
    """One window at the oracle problem's current estimate.  robust: {kind: delta or None} for the four edge kinds."""

    @_prec
    def __init__(self, op, w, robust):
        self.w, self.robust = w, robust
        self.ref = mr.Reference(op, w, {0: robust.get(0), 1: robust.get(1)})
        self.P = self.ref.P
        self.imu_rho1 = []
        self.pose = self._pose_side()
        self._landmarks()

    # ---- IMU and prior edges ---------------------------------------------------------------------------------------------------------------
    def _pose_side(self):
        w, ref = self.w, self.ref
        acc = _Acc(self.P)
        nav, op_off, ob_off = ref.nav, ref.op_off, ref.ob_off

        def add(blocks, Om, rho1):
            Omw = wide(Om) * wide(rho1)
            for oa, Ja in blocks:
                for ob, Jb in blocks:
                    acc.add(oa, ob, wide(Ja), Omw, wide(Jb))
        im = w.get("imu")
        for m in range(len(im["kf_i"]) if im is not None else 0):
            i, j = int(im["kf_i"][m]), int(im["kf_j"][m])
            e, J0, J1, J2 = orc.eval_pvr_edge(w["gw"], nav[i], nav[j], nav[i], im["preint"][m])
            Om = im["info_pvr"][m].reshape(9, 9)
            r_pvr = 1.0 if self.robust.get(2) is None else float(orc.huber(float(e @ Om @ e), self.robust[2])[1])
            add([(o, J) for o, J in ((op_off[i], J0), (op_off[j], J1), (ob_off[i], J2)) if o >= 0], Om, r_pvr)
            eb = np.concatenate([(nav[j][10:13] + nav[j][16:19]) - (nav[i][10:13] + nav[i][16:19]),
                                 (nav[j][13:16] + nav[j][19:22]) - (nav[i][13:16] + nav[i][19:22])])
            Ob = im["info_bias"][m].reshape(6, 6)
            r_b = 1.0 if self.robust.get(3) is None else float(orc.huber(float(eb @ Ob @ eb), self.robust[3])[1])
            add([(o, J) for o, J in ((ob_off[i], -np.eye(6)), (ob_off[j], np.eye(6))) if o >= 0], Ob, r_b)
            self.imu_rho1.append((r_pvr, r_b))
        pr = w.get("prior")
        if pr is not None:
            k = w["kf"]
            J0 = np.asarray(pr["J0"], np.float64)
            blocks = []
            for vid, size, idx in zip(pr["vid"], pr["size"], pr["idx"]):
                hit = [(ref.op_off[q], 9) for q in range(ref.K) if k["vid_pvr"][q] == vid] + \
                      [(ref.ob_off[q], 6) for q in range(ref.K) if k["vid_bias"][q] == vid]
                assert len(hit) == 1 and hit[0][1] == size, (vid, size, hit)
                if hit[0][0] >= 0:
                    blocks.append((hit[0][0], J0[:, idx:idx + size]))
            add(blocks, np.eye(J0.shape[0]), 1.0)
        return acc

    # ---- the landmarks: their pose blocks, statuses, reduced blocks and Schur terms ---------------------------------------------------------
    def _landmarks(self):
        ref = self.ref
        full = self.pose.copy(sum_only=True)      # Hpp with every active observation's pose block (what the recovered Hpp of marginals_ref holds)
        S = self.pose.copy()         # the pose blocks of status 0 / 1 landmarks only, then the Schur terms
        self.status, self.red, self.ratio = [], [], []
        one = wide(np.eye(2))
        for lm in ref.lm:
            nd = 3 if lm["kind"] == 0 else 6
            Hll = wzeros(nd, nd)
            obs = []
            for k, we, Jl, Jp in lm["edges"]:
                Jlw, Jpw, wew = wide(Jl), wide(Jp), wide(we)
                Hll += (Jlw.T @ Jlw) * wew
                o = ref.op_off[k]
                if o >= 0:
                    obs.append((o, Jpw, Jlw, wew))
                    full.add(o, o, Jpw, one * wew, Jpw)
            st, red, ratio = 0, None, None
            if lm["fixed"]:
                st = 1
            elif len(lm["edges"]) < 2:
                st = 2
            else:
                B = wide(np.eye(3)) if lm["kind"] == 0 else line_basis_wide(lm["x"])
                Hr = B.T @ Hll @ B
                L, piv = _chol(Hr)
                dmax = max(Hr[q, q] for q in range(Hr.shape[0]))
                ratio = float(min(piv) / dmax)      # (a factorisation stopped early: its last pivot, not positive)
                if L is None or not ratio > PIV_REL:
                    st = 3
                else:
                    Hi = _inv_from_chol(L)
                    red = (B, Hi, [(o, (Jpw.T @ Jlw @ B) * wew) for o, Jpw, Jlw, wew in obs])
            if st in (0, 1):
                for o, Jpw, Jlw, wew in obs:
                    S.add(o, o, Jpw, one * wew, Jpw)
            if st == 0:
                for oa, Wa in red[2]:
                    for ob, Wb in red[2]:
                        S.add(oa, ob, Wa.T, red[1], Wb.T, sign=-1)
            self.status.append(st); self.red.append(red); self.ratio.append(ratio)
        self.status = np.array(self.status, np.uint8)
        self.Hpp, self.S, self.Sabs, self.Sterms = full.H, S.H, S.A, S.M
        self.d = np.array([_sqrt(self.Sabs[i, i]) for i in range(self.P)], dtype=self.S.dtype)

    def pivot_margin(self):
        """how far the nearest landmark's pivot ratio lies from PIV_REL, as a factor (> 1 on either side)"""
        r = [x for x in self.ratio if x is not None]
        return min((x / PIV_REL if x > PIV_REL else (np.inf if x <= 0 else PIV_REL / x)) for x in r) if r else np.inf

    # ---- the inverse and the landmark covariances -------------------------------------------------------------------------------------------
    @_prec
    def landmark_cov(self, cols_of):
        """Sigma_ll of every status-0 landmark whose observing keyframes' PVR columns are all in cols_of (dict column -> wide column of
        S^-1); {landmark index: wide nd x nd}"""
        out = {}
        for i, red in enumerate(self.red):
            if red is None:
                continue
            B, Hi, W = red
            if any(o + c not in cols_of for o, _ in W for c in range(9)):
                continue
            M = wzeros(*Hi.shape)
            for oa, Wa in W:
                for ob, Wb in W:
                    blk = np.stack([cols_of[ob + c][oa:oa + 9] for c in range(9)], axis=1)
                    M += Wa.T @ blk @ Wb
            out[i] = B @ (Hi + Hi @ M @ Hi) @ B.T
        return out

    def landmark_cols(self):
        """the columns of S^-1 that landmark_cov needs for every status-0 landmark"""
        return sorted({o + c for red in self.red if red is not None for o, _ in red[2] for c in range(9)})


def inverse_ext(S, cols):
    """{j: column j of S^-1 as long double} by solver_ref.refine(S, e_j).  The residual precondition is asserted on every column."""
    S64 = narrow(S)
    solve = R._Factor(S64)
    Sw = S if (R.LD_IS_EXTENDED and getattr(S, "dtype", None) == LD) else S64
    out, worst = {}, 0.0
    for j in cols:
        e = np.zeros(S64.shape[0]); e[j] = 1.0
        x, om = R.refine(Sw, e, solve=solve)
        assert om <= R.RESIDUAL_MAX, (j, om)
        worst = max(worst, om)
        out[int(j)] = x
    return out, worst


def compared_columns(P):
    """every column up to P = 256; beyond, every column of the first and the last 32-column tile and the two columns either side of every
    tile boundary"""
    if P <= 256:
        return list(range(P))
    c = set(range(32)) | set(range((P - 1) // 32 * 32, P))
    for b in range(32, P, 32):
        c |= {b - 2, b - 1, b, b + 1}
    return sorted(x for x in c if 0 <= x < P)


# ---- the three rules ---------------------------------------------------------------------------------------------------------------------------
def rule_S(S, S64, ex):
    """(a) entrywise |S - S_ref| / (d_i d_j), d = sqrt(diag |S|_abs): tolerance max(8 noise, m_ij u), noise = the same measure of the fp64
    reference's S.  Returns (worst error / tolerance, noise, worst error)."""
    dd = narrow(np.outer(ex.d, ex.d))
    noise = float(np.max(np.abs(narrow(wide(S64) - ex.S)) / dd))
    err = np.abs(narrow(wide(S) - ex.S)) / dd
    tol = np.maximum(FACTOR * noise, ex.Sterms * U)
    return float(np.max(err / tol)), noise, float(err.max())


def scaled_matrix_error(Sig_cols, ext_cols, S):
    """E = max d_i d_j |Sig_ij - Sigma_ij| / max d_i d_j |Sigma_ij| over the columns of ext_cols, d = sqrt(diag S)"""
    d = np.sqrt(np.diag(np.asarray(S, np.float64))).astype(LD)
    num = den = LD(0)
    for j, x in ext_cols.items():
        num = max(num, np.max(d * d[j] * np.abs(np.asarray(Sig_cols[:, j]).astype(LD) - x)))
        den = max(den, np.max(d * d[j] * np.abs(x)))
    return float(num / den)


def _tri_inv(L):
    """inverse of a lower triangular matrix by forward substitution, row by row.  (Not np.linalg.inv: its row pivoting takes a factor whose
    rows differ by decades — a bias row against a position row — out of the order in which substitution is stable whatever the scaling; the
    result was up to 1 200 x n u kappa_s off in the scaled norm at kappa_s = 2, which is no property of a Cholesky inverse.)"""
    n = L.shape[0]
    Li = np.zeros((n, n))
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1.0 / L[i, i]
    return Li


def gather_mismatches(blocks, Sig, ref, pairs):
    """the indices of the 15 x 15 blocks that are not, bit for bit, the entries of Sig at their keyframes' pose indices, with zeros in the
    rows and columns of a fixed vertex (what k_cov_gather and kf_dim have to deliver)"""
    bad = []
    for q, (i, j) in enumerate(pairs):
        a, b = ref.kf_index(int(i)), ref.kf_index(int(j))
        want = np.where((a[:, None] >= 0) & (b[None, :] >= 0), Sig[np.maximum(a, 0)][:, np.maximum(b, 0)], 0.0)
        if not np.array_equal(np.asarray(blocks[q]), want):
            bad.append(q)
    return bad


def cpu_inverses(S):
    """three correct fp64 inverses: numpy's, L^-T L^-1 of the Cholesky factor, and the same on the reversed ordering"""
    S = np.asarray(S, np.float64)
    Li = _tri_inv(np.linalg.cholesky(S))
    Lr = _tri_inv(np.linalg.cholesky(S[::-1, ::-1]))
    return [np.linalg.inv(S), Li.T @ Li, (Lr.T @ Lr)[::-1, ::-1]]


def rule_inverse(Sig, S, ext_cols, c):
    """(b) Sig against the extended inverse of S on the columns given.  Returns dict(E, bound = c n u kappa_s, cpu = the largest E of the
    three fp64 inverses, each = their three E)."""
    S = np.asarray(S, np.float64)
    each = [scaled_matrix_error(X, ext_cols, S) for X in cpu_inverses(S)]
    ks = R.kappa_s(S)
    return dict(E=scaled_matrix_error(Sig, ext_cols, S), kappa_s=ks, bound=c * S.shape[0] * U * ks, cpu=max(each), each=each)


def rule_landmarks(cov, cov_ref, formulas, terms):
    """(c) per landmark max |cov - ref| / max |ref| over the landmarks of cov_ref: tolerance max(8 noise, terms u), noise = the larger of the
    fp64 formulas' same measure.  cov: sequence indexed by landmark; formulas: list of dicts / sequences indexed by landmark.
    Returns (worst error / tolerance, noise, worst error)."""
    def measure(c):
        worst = 0.0
        for i, ref in cov_ref.items():
            worst = max(worst, float(np.max(np.abs(wide(c[i]) - ref)) / np.max(np.abs(ref))))
        return worst
    noise = max(measure(f) for f in formulas)
    err = measure(cov)
    return err / max(FACTOR * noise, terms * U), noise, err


def landmark_terms(ex):
    """products summed into an entry of the busiest landmark's coupling term: 81 per pair of observing keyframes"""
    return max([81 * len(red[2]) ** 2 for red in ex.red if red is not None] + [64])


def hybrid_dense_cov(ex, res64, which):
    """fp64, for windows too large for marginals_ref's dense_check: the landmarks `which` kept beside the poses, every other one eliminated
    by its Schur term, and that matrix inverted densely.  res64: Reference.solve's result on the same Hpp; returns {index: cov}."""
    ref = ex.ref
    S = res64["S"].copy()
    red = {}
    for i in which:
        lm = ref.lm[i]
        Hll, obs = ref.landmark_blocks(lm)
        B = np.eye(3) if lm["kind"] == 0 else mr.line_basis(lm["x"])
        Hr = B.T @ Hll @ B
        W = [(o, Hpl @ B) for o, Hpl, _ in obs]
        red[i] = (B, Hr, W)
        ref._schur(S, [(o, w, None) for o, w in W], np.linalg.inv(Hr), +1.0)      # back out of S
    dims = [red[i][1].shape[0] for i in which]
    P = ref.P
    n = P + sum(dims)
    A = np.zeros((n, n))
    A[:P, :P] = S
    o = P
    for i, dm in zip(which, dims):
        B, Hr, W = red[i]
        A[o:o + dm, o:o + dm] = Hr
        for oa, wa in W:
            A[oa:oa + 9, o:o + dm] += wa
            A[o:o + dm, oa:oa + 9] += wa.T
        o += dm
    Ai = np.linalg.inv(A)
    out, o = {}, P
    for i, dm in zip(which, dims):
        out[i] = red[i][0] @ Ai[o:o + dm, o:o + dm] @ red[i][0].T
        o += dm
    return out
