"""The graphs of the pose-graph exactness tests (tests/test_pgo_exact_cpu.py, tests/test_pgo_exact.py), in the scheme of tests/track_cases.py:
BUILD[name](seed) builds a case, EXPECT[name](reference run) says whether the run serves the case's purpose, SEED[name] is the first seed
from 0 that qualifies BY THE REFERENCE ALONE (pick_seed, which can be rerun).  A case is a graph in pgo_ref's layout (nv, pose, ei, ej,
meas, info, fixed) with "opts" = the arguments of pgo_exact.run (iters, user_lambda, initial).

What each family is for (what the existing pose-graph tests never ask of the device):
    branch_x / _y / _z    the three off-trace branches of R_to_q inside k_pgo_edges, the q.w < 0 flip of unit_q, Qm / Qp away from the
                          identity quaternion: every second vertex's estimate turned by 2.2 .. 3.1 rad about one axis
    near_pi_*             error rotations at pi - 1e-3 / 1e-6 / 1e-9 on a single edge (one fixed, one free vertex) and on a six-vertex ring
    big_step(_rejected)   an oplus with |u_r| > 1 (the identity-rotation branch of iso_from_mqt) in an accepted / in a rejected trial
    reversed / mixed / dup_both_ways / relabelled      edges whose vertex 1 has the lower free rank: slot 3 of k_pgo_sum (the transpose)
    edges_N               N around the 64-thread block of k_pgo_edges and the 256 stride and tree of chi_total
    free_N                N free vertices around the block of k_pgo_update, nblk % 4 = 1, 2, 3 between them (k_pgo_sum: 4 blocks a workgroup)
    hub_300               one free vertex with 300 incident edges to fixed vertices, half of them reversed: a long source list for one wave
                          of k_pgo_sum
    info_none / info_scaled     info36 = NULL; information entries over 1e-3 .. 1e6
    init_guess            initial_guess = 1 through the Z^-1 direction of a reversed edge, two fixed vertices

Reversing an edge.  E = Z^-1 Xi^-1 Xj.  The edge given as (j, i, Z^-1) has E' = Z Xj^-1 Xi = Z E^-1 Z^-1: the inverse of E conjugated by
the measurement.  Its error vector is no function of e alone (the rotation of E acts on t_Z and enters the translation rows at the order
of e itself: on `reversed`, max|e' + e| = 5.8e-2 at max|e| = 2.9e-2), so chi2 and H of a reversed graph do NOT equal those of the
unreversed one, to rounding or to any order in the error; no such equality is asserted.  What is exact is the relation between the
isometries, which tests/test_pgo_exact_cpu.py asserts in the wide type, and every reversed graph is held to the wide reference OF THAT
GRAPH under the rule.  The equality that does hold to rounding is the one under a relabelling of the vertices: `relabelled` is the graph of
`reversed`'s base with vertex v named nv - 1 - v, so that every edge has the lower free rank at its vertex 1 with the measurements untouched;
its chi2 is that of the base graph and its H blocks are the base's, transposed and renumbered, and both are asserted under the rule, for
the reference and for the device.

near_pi: which could be compared.  See NOT_COMPARED below: it is filled by the rule (pgo_exact.horizon), never by what the library gives.
"""
import functools
import os
import shutil
import subprocess

import numpy as np

from . import lba_ref as LR
from . import pgo_cov_ref as PC
from . import pgo_exact as PX
from . import pgo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e-10      # userLambdaInit of the reference's loop closure (src/mapHandler.cpp), as tests/test_pgo.py uses
AXES = dict(x=0, y=1, z=2)


def _g(nv, pose, edges, meas, info, fixed, **opts):
    e = np.asarray(edges, np.int32).reshape(-1, 2)
    fx = np.zeros(nv, np.uint8); fx[list(fixed)] = 1
    o = dict(iters=3, user_lambda=LAM, initial=False); o.update(opts)
    return dict(nv=nv, pose=np.asarray(pose, np.float64).reshape(nv, 12), ei=e[:, 0].copy(), ej=e[:, 1].copy(), meas=np.asarray(meas, np.float64).reshape(len(e), 12),
                info=None if info is None else np.asarray(info, np.float64).reshape(len(e), 6, 6), fixed=fx, opts=o)


def _from(g, **opts):
    return _g(g["nv"], g["pose"], np.stack([g["ei"], g["ej"]], -1), g["meas"], g["info"], np.flatnonzero(g["fixed"]), **opts)


def _turn(pose12, w):
    """the pose with its estimate turned by the rotation vector w (X <- X D)"""
    D = pgo_ref.join(pgo_ref._rot(np.asarray(w, np.float64))[None], np.zeros((1, 3)))[0]
    return pgo_ref.iso_mul(pose12, D)


def reverse(g, mask):
    """the graph with the edges of `mask` given as (j, i) and their measurements inverted"""
    g = dict(g)
    mask = np.asarray(mask, bool)
    g["ei"], g["ej"] = np.where(mask, g["ej"], g["ei"]).astype(np.int32), np.where(mask, g["ei"], g["ej"]).astype(np.int32)
    g["meas"] = np.where(mask[:, None], pgo_ref.iso_inv(g["meas"]), g["meas"])
    return g


def keep_edges(g, idx):
    g = dict(g)
    for k in ("ei", "ej", "meas"):
        g[k] = g[k][idx]
    if g["info"] is not None:
        g["info"] = g["info"][idx]
    return g


def rotated(nv, seed, axis, lo=2.2, hi=3.1, **opts):
    """a cov_graph of nv vertices with every second free vertex's estimate turned by lo .. hi rad about the axis"""
    g = _from(pgo_ref.cov_graph(nv, seed=seed, window=3, n_loops=1), **opts)
    rng = np.random.default_rng(1000 + seed)
    for v in range(3, nv, 2):
        w = np.zeros(3); w[AXES[axis]] = rng.uniform(lo, hi) * rng.choice([-1.0, 1.0])
        g["pose"][v] = _turn(g["pose"][v], w)
    return g


def near_pi(kind, delta, seed):
    """error rotations at pi - delta about a seeded axis: "edge" = one fixed and one free vertex joined by one edge, "ring" = six vertices
    in a ring, vertex 0 fixed, vertex 3 turned (its two edges carry the error); non-identity information"""
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    pose = lambda: pgo_ref.join(pgo_ref._rot(rng.normal(size=3) * 0.5)[None], rng.normal(size=(1, 3)))[0]

    def info():
        A = rng.normal(size=(6, 6)) * 0.1
        return np.diag(np.concatenate([np.full(3, 50.0), np.full(3, 200.0)]) * rng.uniform(0.5, 2.0, 6)) + A @ A.T
    if kind == "edge":
        X0, Z = pose(), pose()
        X1 = _turn(pgo_ref.iso_mul(X0, Z), ax * (np.pi - delta))
        X1[9:] += rng.normal(size=3) * 5e-3
        return _g(2, [X0, X1], [(0, 1)], [Z], [info()], [0])
    X = [pose()]
    Z = [pose() for _ in range(6)]
    for k in range(5):
        X.append(pgo_ref.iso_mul(X[k], Z[k]))
    Z[5] = pgo_ref.iso_mul(pgo_ref.iso_inv(X[5]), X[0])
    for k in range(1, 6):
        X[k] = X[k].copy(); X[k][9:] += rng.normal(size=3) * 5e-3
    X[3] = _turn(X[3], ax * (np.pi - delta))
    return _g(6, X, [(k, (k + 1) % 6) for k in range(6)], Z, [info() for _ in range(6)], [0])


def with_edge_count(ne, seed):
    """a chain with covisibility edges (cov_graph without its loops), 2 fixed vertices, small drift, cut to exactly ne edges (the odometry
    edges come first, so every vertex stays touched)"""
    nv = max(8, int(ne / 3.6))
    g = pgo_ref.cov_graph(nv, seed=seed, n_loops=0)
    assert nv - 1 < ne <= len(g["ei"]), (nv, ne, len(g["ei"]))
    return _from(keep_edges(g, np.arange(ne)))


def nblk_of(g):
    return len(PC.block_list(g)[0])


def with_free_count(nfree, mod4, seed):
    """nfree free vertices (2 fixed) on a chain with covisibility edges within +-3, cut to the largest edge count at which the number of
    nonzero blocks of H is mod4 modulo 4"""
    g = pgo_ref.cov_graph(nfree + 2, seed=seed, window=3, n_loops=0)
    for ne in range(len(g["ei"]), nfree + 1, -1):
        c = keep_edges(g, np.arange(ne))
        if nblk_of(c) % 4 == mod4:
            return _from(c)
    raise RuntimeError("no edge count gives nblk % 4 == %d" % mod4)


def hub(n_spokes, seed):
    """the one free vertex, n_spokes // 2, joined to every other vertex, all of them fixed; every second edge given from the spoke to the hub,
    so that the hub's block sums A00 and A11 sources (and b both g0 and g1) in turn; each edge with its own information"""
    rng = np.random.default_rng(seed)
    nv, h = n_spokes + 1, n_spokes // 2
    T = [pgo_ref.join(pgo_ref._rot(rng.normal(size=3) * 0.4)[None], rng.normal(size=(1, 3)) * 3)[0] for _ in range(nv)]
    edges, meas, info = [], [], []
    for k, v in enumerate([v for v in range(nv) if v != h]):
        Z = pgo_ref.iso_mul(pgo_ref.iso_inv(T[h]), T[v])
        Z = _turn(Z, rng.normal(size=3) * 1e-3); Z[9:] += rng.normal(size=3) * 3e-3
        edges.append((v, h) if k % 2 else (h, v)); meas.append(pgo_ref.iso_inv(Z) if k % 2 else Z)
        A = rng.normal(size=(6, 6)) * 0.1
        info.append(np.diag(np.concatenate([np.full(3, 50.0), np.full(3, 200.0)]) * rng.uniform(0.5, 2.0, 6)) + A @ A.T)
    est = [T[v] if v != h else _turn(T[v], rng.normal(size=3) * 2e-2) + np.concatenate([np.zeros(9), rng.normal(size=3) * 5e-2]) for v in range(nv)]
    return _g(nv, est, edges, meas, info, [v for v in range(nv) if v != h])


def relabel(g):
    """the graph with vertex v named nv - 1 - v (measurements untouched)"""
    g = dict(g)
    nv = g["nv"]
    g["pose"] = g["pose"][::-1].copy(); g["fixed"] = g["fixed"][::-1].copy()
    g["ei"], g["ej"] = (nv - 1 - g["ei"]).astype(np.int32), (nv - 1 - g["ej"]).astype(np.int32)
    return g


def _base12(seed):
    return _from(pgo_ref.cov_graph(12, seed=seed, window=4, n_loops=2))


def _dup(seed):
    g = _base12(seed)
    k = np.flatnonzero((g["fixed"][g["ei"]] == 0) & (g["fixed"][g["ej"]] == 0))[:3]
    d = reverse(keep_edges(g, k), np.ones(len(k), bool))
    for q in ("ei", "ej", "meas", "info"):
        g[q] = np.concatenate([g[q], d[q]])
    return g


def _info_scaled(seed):
    g = _base12(seed)
    rng = np.random.default_rng(2000 + seed)
    s = 10.0 ** rng.uniform(-1.5, 3.0, (len(g["ei"]), 6))      # O = S O S: entries over 1e-3 .. 1e6
    g["info"] = g["info"] * s[:, :, None] * s[:, None, :]
    return g


def _init_guess(seed):
    g = pgo_ref.cov_graph(12, seed=seed, window=4, n_loops=1, fixed=(0, 6))
    ne = len(g["ei"])
    mask = np.zeros(ne, bool); mask[-1] = True; mask[np.arange(0, 11, 3)] = True      # the loop edge and every third odometry edge
    return _from(reverse(g, mask), initial=True)


BUILD = {}
for _a in AXES:
    BUILD["branch_" + _a] = (lambda seed, a=_a: rotated(8, seed, a))
for _k in ("edge", "ring"):
    for _d in (3, 6, 9):
        BUILD["near_pi_%s_%d" % (_k, _d)] = (lambda seed, k=_k, d=_d: near_pi(k, 10.0 ** -d, seed))
BUILD["big_step"] = lambda seed: rotated(8, seed, "y", 1.8, 3.1)
BUILD["big_step_rejected"] = lambda seed: rotated(8, seed, "z", 1.8, 3.1)
BUILD["base12"] = _base12
BUILD["reversed"] = lambda seed: (lambda g: reverse(g, np.ones(len(g["ei"]), bool)))(_base12(seed))
BUILD["mixed"] = lambda seed: (lambda g: reverse(g, np.arange(len(g["ei"])) % 2 == 1))(_base12(seed))
BUILD["dup_both_ways"] = _dup
BUILD["relabelled"] = lambda seed: relabel(_base12(seed))
for _n in (63, 64, 65, 255, 256, 257, 513):
    BUILD["edges_%d" % _n] = (lambda seed, n=_n: with_edge_count(n, seed))
for _n, _m in ((63, 1), (64, 2), (65, 3)):
    BUILD["free_%d" % _n] = (lambda seed, n=_n, m=_m: with_free_count(n, m, seed))
BUILD["hub_300"] = lambda seed: hub(300, seed)
BUILD["info_none"] = lambda seed: (lambda g: dict(g, info=None))(_base12(seed))
BUILD["info_scaled"] = _info_scaled
BUILD["init_guess"] = _init_guess
NBLK_MOD4 = dict(free_63=1, free_64=2, free_65=3)


def _census(r, branch):
    """(edges of the first linearisation in the branch, those of them unit_q flipped)"""
    ev = r["lin"][0]
    hit = ev["branch"] == branch
    return int(hit.sum()), int((hit & ev["flip"]).sum())


def _w2neg(r, accepted):
    return [i for i, t in enumerate(r["trace"]) if t["accepted"] == accepted and t["solver_ok"] and bool((PX.f64(t["w2"]) < 0).any())]


_converges = lambda r: r["trials"] >= 1 and float(r["chi2_final"]) < float(r["chi2_initial"])
EXPECT = {n: _converges for n in BUILD}
for _a, _b in (("x", 1), ("y", 2), ("z", 3)):
    EXPECT["branch_" + _a] = (lambda r, b=_b: _census(r, b)[0] >= 2 and _census(r, b)[1] >= 1)
for _n in BUILD:
    if _n.startswith("near_pi"):
        EXPECT[_n] = (lambda r, k=_n: int((r["ev0"]["branch"] > 0).sum()) == (1 if "edge" in k else 2))
EXPECT["big_step"] = lambda r: len(_w2neg(r, 1)) >= 1
EXPECT["big_step_rejected"] = lambda r: len(_w2neg(r, 0)) >= 1
EXPECT["init_guess"] = lambda r: _converges(r) and r["init_inverse"] >= 1
EXPECT["hub_300"] = lambda r: _converges(r) and r["n"] == 1


def compared_trials(r64, rw):
    """the number of leading trials compared: those within the horizon of condition (b)"""
    return PX.horizon(r64, rw)[0]


REORDER = 12


def reordered(case, k):
    """the case with its edges in the k-th other order; with initial = 1 the propagated start is taken first (the propagation follows the
    insertion order of the edges, so another order is another start)"""
    c = dict(case)
    if case["opts"]["initial"]:
        c["pose"] = PX.f64(PX.initial_guess(case, np.float64)); c["opts"] = dict(case["opts"], initial=False)
    p = np.random.default_rng(7000 + k).permutation(len(case["ei"]))
    return keep_edges(c, p)


def reference_is_stable(case, r64, rw, T):
    """condition (c): the largest error / tolerance of the fp64 reference with the edges in REORDER other orders (and the damped system
    solved by Cholesky, by LU with pivoting and by Cholesky from the last unknown up in turn: the noise of one fp64 factorisation of an
    ill-conditioned system says little about another's) against the wide run, over
    the quantities compared (chi2_initial, the blocks of H, the held fields of the first T rows, the poses within T); stable = at most 1/2"""
    tol, _, _ = PX.tolerances(case, r64, rw, T)
    worst = 0.0
    for k in range(REORDER):
        c = reordered(case, k)
        r = PX.run(c, np.float64, solve_variant=k % 3, **c["opts"])      # each order with one of three fp64 factorisations in turn
        err = {"chi2_initial": abs(float(r["chi2_initial"]) - float(rw["chi2_initial"]))}
        if "first" in rw:
            err["H"] = np.abs(PX.h_blocks(c, r) - PX.h_blocks(case, rw)).reshape(len(tol["H"]), -1).max(-1)
        for key in tol:
            if isinstance(key, tuple) and key[0] == "poses":
                if key[1] not in r["after"] or r["after"][key[1]]["trials"] != rw["after"][key[1]]["trials"]:
                    return np.inf
                err[key] = np.abs(PX.f64(r["after"][key[1]]["poses"]) - PX.f64(rw["after"][key[1]]["poses"])).max()
            elif isinstance(key, tuple):
                if key[1] >= len(r["trace"]) or any(r["trace"][key[1]][f] != rw["trace"][key[1]][f] for f in PX.FIELDS_EXACT):
                    return np.inf
                a, b = float(r["trace"][key[1]][key[0]]), float(rw["trace"][key[1]][key[0]])
                err[key] = 0.0 if a == b else abs(a - b)
        for key, e in err.items():
            t = np.asarray(tol[key], np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.max(np.where(t > 0, np.asarray(e) / t, np.where(np.asarray(e) > 0, np.inf, 0.0)))))
    return worst


def qualifies(name, case, r64, rw):
    """(a) - (c) and EXPECT on both runs, by the reference alone"""
    if not (EXPECT[name](r64) and EXPECT[name](rw)):
        return False
    T = compared_trials(r64, rw)
    if T < 1:
        return False
    if name == "big_step" and not [i for i in _w2neg(rw, 1) if i < T]:
        return False
    if name == "big_step_rejected" and not [i for i in _w2neg(rw, 0) if i < T]:
        return False
    tol, noise, lim = PX.tolerances(case, r64, rw, T)
    return PX.tolerances_tighten(tol, noise, lim) < 1.0 and reference_is_stable(case, r64, rw, T) <= 0.5


def pick_seed(name, start=0, tries=400):
    for seed in range(start, start + tries):
        case = BUILD[name](seed)
        r64 = PX.run(case, np.float64, **case["opts"])
        if not EXPECT[name](r64):
            continue
        rw = PX.run(case, LR.wide(), **case["opts"])
        if qualifies(name, case, r64, rw):
            return seed
    raise RuntimeError("no seed for %s" % name)


# SEED[name] = pick_seed(name): no seed was chosen by what the library gives.  reversed, mixed, dup_both_ways, relabelled, info_none and
# info_scaled are variants of base12 and must share ITS graph to be comparable with it, so they take the first seed at which all of them
# qualify (pick_shared_seed).
SHARED = ("base12", "reversed", "mixed", "dup_both_ways", "relabelled", "info_none", "info_scaled")


def pick_shared_seed(start=0, tries=400):
    for seed in range(start, start + tries):
        ok = True
        for name in SHARED:
            case = BUILD[name](seed)
            r64, rw = PX.run(case, np.float64, **case["opts"]), PX.run(case, LR.wide(), **case["opts"])
            if not qualifies(name, case, r64, rw):
                ok = False
                break
        if ok:
            return seed
    raise RuntimeError("no shared seed")


SEED = {"branch_x": 0, "branch_y": 0, "branch_z": 0, "near_pi_edge_3": 0, "near_pi_edge_6": 178, "near_pi_edge_9": 1, "near_pi_ring_3": 0,
        "near_pi_ring_6": 0, "near_pi_ring_9": 0, "big_step": 1, "big_step_rejected": 0, "edges_63": 0, "edges_64": 0, "edges_65": 0, "edges_255": 0,
        "edges_256": 0, "edges_257": 0, "edges_513": 0, "free_63": 0, "free_64": 0, "free_65": 0, "hub_300": 0, "init_guess": 0}      # {n: pick_seed(n)}
SEED.update({n: 0 for n in SHARED})      # pick_shared_seed()
# TRIALS[name]: the number of leading trials the case is compared over = pgo_exact.horizon of its two reference runs (condition (b)); every
# case but three is compared over its whole run of three iterations.  near_pi_edge_9: beyond the first trial q.w = sin(delta / 2) of the
# trial's evaluation has less than 1000 x its noise.  init_guess and hub_300: the third trial's rho has less.
TRIALS = {"branch_x": 12, "branch_z": 15, "near_pi_edge_3": 5, "near_pi_edge_6": 5, "near_pi_edge_9": 1, "near_pi_ring_3": 11, "near_pi_ring_6": 11,
          "near_pi_ring_9": 11, "big_step_rejected": 15, "hub_300": 2, "init_guess": 2}
NAMES = [n for n in BUILD]
TRIALS.update({n: 3 for n in NAMES if n not in TRIALS})
CASES = {n: (lambda n=n: BUILD[n](SEED[n])) for n in BUILD}
# near_pi: which could not be compared.  Every one of the six qualifies at some seed, so none is left out; what the rule refused are
# seeds.  near_pi_edge_6 qualifies at seed 178 only and near_pi_edge_9 at seed 1: on a single edge the damped 6 x 6 system has the singular
# rotation block w I + [v]x, w = sin(delta / 2), and lambda = 1e-10, so its condition number is 1 / w^2 and one fp64 factorisation differs
# from another by more than half the tolerance (condition (c)) unless the axis is kind, or the q.w < 0 comparison of an evaluation (a
# difference of two entries of R that agree to delta) falls short of 1000 x its noise (condition (b)).  The rings qualify at seed 0
# at every delta: five more edges keep the system regular.  NOT_COMPARED would name a case no seed in 400 serves.
NOT_COMPARED = {}


def undamped_pivot_margin(rw):
    """smallest Cholesky pivot of the first H at lambda = 0 over N u max diag: the margin of `Cholesky success` for plba_pose_graph_marginals,
    whose dump is the only way the ABI shows the summed H blocks"""
    H = PX.f64(rw["first"]["H"])
    try:
        piv = np.diag(np.linalg.cholesky(H)) ** 2
    except np.linalg.LinAlgError:
        return 0.0
    return float(piv.min() / (len(H) * PX.U * np.abs(np.diag(H)).max()))


# the cases whose H the marginals can factor with margin (undamped_pivot_margin >= MARGIN): all but the single edge at pi - 1e-9, whose
# rotation block w I + [v]x is singular to 5e-10.  plba_pose_graph_marginals copies the "pgo_cov_H" dump only behind a factorisation that
# succeeded (a failed one returns PLBA_ERR_NUMERIC before the copy), so without that margin the ABI shows no H to compare; that case's H
# is held on the host (tests/test_pgo_exact_cpu.py) and through the damped steps
H_READABLE = [n for n in NAMES if n != "near_pi_edge_9"]


@functools.lru_cache(maxsize=None)
def runs(name):
    """(case, float64 run, wide run, compared trials) of the named case, computed once and shared"""
    case = CASES[name]()
    r64, rw = PX.run(case, np.float64, **case["opts"]), PX.run(case, LR.wide(), **case["opts"])
    return case, r64, rw, compared_trials(r64, rw)


# ---- the device formula on the host (csrc/plba_pgo_hostcheck.cpp) -----------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_pgo_hostcheck.cpp")


def build_hostcheck(out_dir, sanitize=True, src_dir=CSRC):
    """the stand-alone host program, with the host sanitizers unless told otherwise; returns its path"""
    exe = os.path.join(out_dir, "plba_pgo_hostcheck" + ("_san" if sanitize else ""))
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    deps = [os.path.join(src_dir, f) for f in ("plba_pgo_hostcheck.cpp", "plba_pgo_dev.h", "plba_pgo_edge_body.inc", "plba_math.h")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    os.makedirs(out_dir, exist_ok=True)
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Wall"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", src_dir, deps[0], "-o", exe])
    return exe


def host_blocks(g):
    """the block list as pgo_graph_setup builds it: (blk_start, blk_src, blk_diag, blk_row, blk_col, free_v); sources edge * 4 + slot in edge
    order, slot 0 A00, 1 A11, 2 A10 (vertex 1 has the higher free rank), 3 its transpose"""
    fr, free = PC.free_ranks(g)
    s = []
    for k, (i, j) in enumerate(zip(np.asarray(g["ei"]).tolist(), np.asarray(g["ej"]).tolist())):
        a, b = int(fr[i]), int(fr[j])
        if a >= 0:
            s.append((a, a, 4 * k))
        if b >= 0:
            s.append((b, b, 4 * k + 1))
        if a >= 0 and b >= 0:
            s.append((b, a, 4 * k + 2) if b > a else (a, b, 4 * k + 3))
    s.sort(key=lambda t: (t[0], t[1]))      # stable: edge order within a block
    start, row, col = [], [], []
    for q, t in enumerate(s):
        if q == 0 or t[:2] != s[q - 1][:2]:
            start.append(q); row.append(t[0]); col.append(t[1])
    start.append(len(s))
    i32 = lambda a: np.asarray(a, np.int32)
    return i32(start), i32([t[2] for t in s]), i32([int(r == c) for r, c in zip(row, col)]), i32(row), i32(col), i32(free)


def host_run(exe, tmp, g, X, x, cnt0=0):
    """one linearisation at the poses X, one update by the step x and the errors behind it, through the host program: dict(erec, echi,
    Hblk, b, X, echi_trial, cnt)"""
    start, src, diag, row, col, free = host_blocks(g)
    nv, ne, n, nblk = g["nv"], len(g["ei"]), len(free), len(row)
    info = np.tile(np.eye(6), (ne, 1, 1)) if g["info"] is None else g["info"]
    fin, fout = os.path.join(tmp, "pgo_in.bin"), os.path.join(tmp, "pgo_out.bin")
    with open(fin, "wb") as f:
        np.array([nv, ne, n, nblk, len(src), cnt0], np.int32).tofile(f)
        np.ascontiguousarray(X, np.float64).tofile(f)
        np.asarray(g["ei"], np.int32).tofile(f); np.asarray(g["ej"], np.int32).tofile(f)
        np.ascontiguousarray(g["meas"], np.float64).tofile(f); np.ascontiguousarray(info, np.float64).tofile(f)
        free.tofile(f); start.tofile(f); src.tofile(f); diag.tofile(f); row.tofile(f)
        np.ascontiguousarray(x, np.float64).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        rd = lambda cnt, shape: np.fromfile(f, np.float64, cnt).reshape(shape)
        out = dict(erec=rd(120 * ne, (ne, 120)), echi=rd(ne, (ne,)), Hblk=rd(36 * nblk, (nblk, 6, 6)), b=rd(6 * n, (6 * n,)), X=rd(12 * nv, (nv, 12)), echi_trial=rd(ne, (ne,)))
        out["cnt"] = np.fromfile(f, np.int32, nv)
    return out
