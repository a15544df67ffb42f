"""Reference of plba_pose_graph_marginals (include/plba.h): the marginal covariances of a whole pose graph.

    H        = sum J^T Omega J over the free vertices, in fp64 from pgo_ref.edge_jacobians — or from the blocks the device summed
               (plba_debug_get "pgo_cov_H"), so that the assembly's rounding is not charged to the inversion;
    inverse  extended-precision columns of H^-1 by marginals_exact.inverse_ext (dense), or by a sparse LU refined once with a long
               double residual where the dense form does not fit;
    status   the header's rules in numpy;
    E_sel    = max d_i d_j |Sig^_ij - Sig_ij| / max d_i d_j |Sig_ij| over the REPORTED entries, d = sqrt(diag H):
               marginals_exact.scaled_matrix_error restricted to the selection;
    kappa_s  of D^-1 H D^-1, by eigsh for the graphs too large for solver_ref.kappa_s.

Also the graphs and the requests the tests use (tests/test_pgo_cov.py on the device, tests/test_pgo_cov_cpu.py for the reference's own
rule and the bound of every graph)."""
import numpy as np

from . import marginals_exact as MX
from . import pgo_ref
from . import solver_ref as R

U = R.U
LD = R.LD
C_BOUND = 32          # E_sel <= 32 n u kappa_s: the constant rule (b) of marginals_exact holds the dense Cholesky inverse to
FACTOR = MX.FACTOR    # over the fp64 CPU inverses' own error: another summation order of the same sums


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def free_ranks(g):
    """(fr, free): free rank of every vertex (-1: fixed or untouched), vertex of every free rank"""
    nv = len(g["pose"])
    touched = np.zeros(nv, bool); touched[g["ei"]] = True; touched[g["ej"]] = True
    fx = np.zeros(nv, bool) if g.get("fixed") is None else np.asarray(g["fixed"]).astype(bool)
    free = np.flatnonzero(touched & ~fx)
    fr = -np.ones(nv, np.int64); fr[free] = np.arange(len(free))
    return fr, free


def vertex_status(g):
    nv = len(g["pose"])
    fr, _ = free_ranks(g)
    fx = np.zeros(nv, bool) if g.get("fixed") is None else np.asarray(g["fixed"]).astype(bool)
    return np.where(fr >= 0, 0, np.where(fx, 1, 2)).astype(np.uint8)


def statuses(g, pairs, fill=()):
    """(v_status, pair_status, n_status).  A pair of free vertices is inside the pattern (0) when i == j or an edge joins it — the
    header's guarantee — or when the caller lists it in `fill` (unordered pairs the elimination is known to fill); otherwise 3."""
    vs = vertex_status(g)
    joined = {(min(a, b), max(a, b)) for a, b in zip(np.asarray(g["ei"]).tolist(), np.asarray(g["ej"]).tolist())}
    joined |= {(min(a, b), max(a, b)) for a, b in fill}
    ps = np.zeros(len(pairs), np.uint8)
    for k, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if vs[i] == 2 or vs[j] == 2:
            ps[k] = 2
        elif vs[i] == 1 or vs[j] == 1:
            ps[k] = 1
        elif i == j or (min(i, j), max(i, j)) in joined:
            ps[k] = 0
        else:
            ps[k] = 3
    return vs, ps, np.array([(vs == 0).sum(), (vs == 1).sum(), (vs == 2).sum(), (ps == 3).sum()], np.int32)


def block_list(g):
    """(rows, cols) of the blocks of H in the order the host code builds: ascending (row rank, column rank), row >= column"""
    fr, free = free_ranks(g)
    a, b = fr[np.asarray(g["ei"])], fr[np.asarray(g["ej"])]
    both = (a >= 0) & (b >= 0)
    keys = {(int(max(x, y)), int(min(x, y))) for x, y in zip(a[both], b[both])} | {(int(r), int(r)) for r in range(len(free))}
    keys = sorted(keys)
    return np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)


def edge_blocks(g):
    """per edge the fp64 blocks A00, A11, A10 = J1^T O J0 (pgo_ref.edge_jacobians at g's poses)"""
    X = np.asarray(g["pose"], np.float64)
    ei, ej = np.asarray(g["ei"]), np.asarray(g["ej"])
    ne = len(ei)
    om = np.tile(np.eye(6), (ne, 1, 1)) if g.get("info") is None else np.asarray(g["info"], np.float64).reshape(ne, 6, 6)
    J0, J1 = pgo_ref.edge_jacobians(X[ei], X[ej], pgo_ref.iso_inv(np.asarray(g["meas"], np.float64).reshape(ne, 12)))
    OJ0, OJ1 = om @ J0, om @ J1
    return np.swapaxes(J0, 1, 2) @ OJ0, np.swapaxes(J1, 1, 2) @ OJ1, np.swapaxes(J1, 1, 2) @ OJ0


def blocks_from_graph(g):
    """the blocks of block_list(g) summed in fp64 from the edges"""
    fr, _ = free_ranks(g)
    rows, cols = block_list(g)
    idx = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(rows, cols))}
    B = np.zeros((len(rows), 6, 6))
    A00, A11, A10 = edge_blocks(g)
    for k, (i, j) in enumerate(zip(np.asarray(g["ei"]).tolist(), np.asarray(g["ej"]).tolist())):
        a, b = fr[i], fr[j]
        if a >= 0:
            B[idx[(a, a)]] += A00[k]
        if b >= 0:
            B[idx[(b, b)]] += A11[k]
        if a >= 0 and b >= 0:
            B[idx[(max(a, b), min(a, b))]] += A10[k] if b > a else A10[k].T
    return B


def dense_H(g, blocks=None):
    """H (6 n x 6 n) from the blocks given (the device's dump, n_blocks x 36) or from the edges; the lower triangle is what the
    factorisation reads, so a diagonal block's lower triangle is mirrored"""
    rows, cols = block_list(g)
    B = blocks_from_graph(g) if blocks is None else np.asarray(blocks, np.float64).reshape(-1, 6, 6)
    assert len(B) == len(rows), (len(B), len(rows))
    n = int(rows.max()) + 1 if len(rows) else 0
    H = np.zeros((6 * n, 6 * n))
    for k, (r, c) in enumerate(zip(rows, cols)):
        blk = np.tril(B[k]) + np.tril(B[k], -1).T if r == c else B[k]
        H[6 * r:6 * r + 6, 6 * c:6 * c + 6] = blk
        H[6 * c:6 * c + 6, 6 * r:6 * r + 6] = blk.T
    return H


def sparse_H(g, blocks=None):
    import scipy.sparse as sp
    rows, cols = block_list(g)
    B = blocks_from_graph(g) if blocks is None else np.asarray(blocks, np.float64).reshape(-1, 6, 6)
    assert len(B) == len(rows)
    n = int(rows.max()) + 1
    dg = rows == cols
    Bd = np.tril(B[dg]) + np.swapaxes(np.tril(B[dg], -1), 1, 2)
    i6, j6 = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")

    def coo(r, c, blk):
        return (6 * r[:, None, None] + i6).ravel(), (6 * c[:, None, None] + j6).ravel(), blk.ravel()
    parts = [coo(rows[dg], cols[dg], Bd), coo(rows[~dg], cols[~dg], B[~dg]), coo(cols[~dg], rows[~dg], np.swapaxes(B[~dg], 1, 2))]
    return sp.csc_matrix((np.concatenate([p[2] for p in parts]), (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))),
                         shape=(6 * n, 6 * n))


# ---- condition ---------------------------------------------------------------------------------------------------------------------------
def kappa_s_sparse(Hs):
    """condition number of D^-1 H D^-1 of a sparse H by eigsh: the largest eigenvalue, and the smallest by shift-invert at 0"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    d = 1.0 / np.sqrt(Hs.diagonal())
    A = (sp.diags(d) @ Hs @ sp.diags(d)).tocsc()
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-6)[0]
    return float(hi / lo)


def bound(n6, ks):
    return C_BOUND * n6 * U * ks


# ---- the inverse on a selection ------------------------------------------------------------------------------------------------------------
def exact_columns(H, col_vertices):
    """{column index: long double column of H^-1} for the six columns of every free rank given"""
    cols = [6 * int(v) + b for v in sorted(set(int(v) for v in col_vertices)) for b in range(6)]
    ext, worst = MX.inverse_ext(H, cols)
    return ext


def refined_sparse_columns(Hs, col_vertices):
    """the same from a sparse LU, refined once with a long double residual; returns (columns, worst relative residual after)"""
    import scipy.sparse.linalg as spl
    lu = spl.splu(Hs.tocsc())
    coo = Hs.tocoo()
    data, ri, ci = coo.data.astype(LD), coo.row, coo.col
    out, worst = {}, 0.0
    for v in sorted(set(int(v) for v in col_vertices)):
        for b in range(6):
            j = 6 * v + b
            e = np.zeros(Hs.shape[0]); e[j] = 1.0
            x = lu.solve(e).astype(LD)
            for _ in range(2):
                r = e.astype(LD); np.subtract.at(r, ri, data * x[ci])
                x = x + lu.solve(r.astype(np.float64)).astype(LD)
            r = e.astype(LD); np.subtract.at(r, ri, data * x[ci])
            s = np.zeros(Hs.shape[0], LD); np.add.at(s, ri, np.abs(data * x[ci])); s[j] += 1
            worst = max(worst, float(np.max(np.abs(r) / s)))
            out[j] = x
    return out, worst


def e_sel(entries, ext, d):
    """entries: list of (i_rank, j_rank, 6 x 6 block = Cov(x_i, x_j)); ext: the columns of H^-1 of every j; d = sqrt(diag H)"""
    d = np.asarray(d).astype(LD)
    num = den = LD(0)
    for i, j, blk in entries:
        ref = np.stack([ext[6 * j + b][6 * i:6 * i + 6] for b in range(6)], axis=1)
        w = np.outer(d[6 * i:6 * i + 6], d[6 * j:6 * j + 6])
        num = max(num, np.max(w * np.abs(np.asarray(blk).astype(LD) - ref)))
        den = max(den, np.max(w * np.abs(ref)))
    return float(num / den)


def entries_of_dense(Sig, sel):
    return [(i, j, Sig[6 * i:6 * i + 6, 6 * j:6 * j + 6]) for i, j in sel]


def e_cpu(H, sel, ext):
    """the three fp64 CPU inverses of marginals_exact.cpu_inverses on the same entries: their E_sel"""
    d = np.sqrt(np.diag(H))
    return [e_sel(entries_of_dense(S, sel), ext, d) for S in MX.cpu_inverses(H)]


# ---- the graphs and the requests of the tests --------------------------------------------------------------------------------------------
def chain_graph(n_free, seed=4):
    """a chain of n_free free vertices behind one fixed vertex"""
    from .test_pgo_sparse import _base_poses, _make
    nv = n_free + 1
    edges = [(i, i + 1) for i in range(nv - 1)]
    return _make(_base_poses(nv), edges, fixed=[0], seed=seed)


def clique_graph(n_free, seed=5):
    from .test_pgo_sparse import _base_poses, _make
    nv = n_free + 1
    return _make(_base_poses(nv), [(i, j) for i in range(nv) for j in range(i + 1, nv)], fixed=[0], seed=seed)


SMALL = ["one_free", "chain16", "chain17", "clique3", "clique4", "clique6", "clique9", "cov20", "cov40", "star", "fixed_hub", "two_components",
         "complete80"]
_G = {}


def graph(name):
    if name not in _G:
        from .test_pgo_sparse import _structures
        if name.startswith("chain"):
            g = chain_graph(int(name[5:]))
        elif name.startswith("clique"):
            g = clique_graph(int(name[6:]))
        elif name.startswith("cov"):
            g = pgo_ref.cov_graph(int(name[3:]), seed=7 if int(name[3:]) >= 300 else 3)
        else:
            g = _structures()[name]
        _G[name] = g
    return _G[name]


def request(name, g):
    """(pairs, fill): every edge in both orientations, one repeated pair, (i, i), a pair with a fixed end, a pair with an untouched end
    where there is one, and the two ends of the chain (inside the pattern of a one-front chain, outside where the chain is dissected)"""
    vs = vertex_status(g)
    e = np.stack([g["ei"], g["ej"]], 1).astype(np.int64)
    pairs = [tuple(x) for x in e.tolist()] + [tuple(x) for x in e[:, ::-1].tolist()]
    free, fixed, unt = np.flatnonzero(vs == 0), np.flatnonzero(vs == 1), np.flatnonzero(vs == 2)
    pairs += [pairs[0], (int(free[0]), int(free[0])), (int(free[-1]), int(free[-1]))]
    if len(fixed):
        pairs += [(int(fixed[0]), int(free[0])), (int(free[-1]), int(fixed[0]))]
    if len(unt):
        pairs += [(int(unt[0]), int(free[0])), (int(fixed[0]) if len(fixed) else int(free[0]), int(unt[-1]))]
    fill = []
    if name.startswith("chain"):
        ends = (int(free[0]), int(free[-1]))
        pairs += [ends, ends[::-1]]
        if len(free) <= 16:      # SP_LEAF: one front holds the whole chain, and a front is dense
            fill.append(ends)
    return np.array(pairs, np.int32), fill
