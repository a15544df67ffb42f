"""The covisibility graph in numpy, written from the reference's text and the definition of include/plba.h (not from the kernels' header):
the recount C[i][j] = sum_l m_l(i) m_l(j), the replay of the reference's increments (src/mapHandler.cpp:371-372, :395-400 and their line
twins, :652-680), the edge loop of loopClosureOptimizationCovGraphG2O (:4373-4408) as two literal `for`s, formLocalMap (:955-1017), and
Z = T_i^-1 T_j in float64 and in lba_ref's wide type.  Also the generated maps the CPU and GPU tests share, and the driver of the host
program csrc/plba_covis_hostcheck.cpp."""
import functools
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(min_lm_ess_graph=150, min_lm_cov_graph=75, min_kf_local_map=3)      # src/slamConfig.cpp:60-62
W = 8192      # the row kernel's tile width (csrc/plba_covis.hip: COVIS_W); the tile-boundary maps are built around it


# ---- maps ---------------------------------------------------------------------------------------------------------------------------
def csr(lists):
    """(start, kf) of a list of keyframe lists"""
    start = np.zeros(len(lists) + 1, np.int32)
    if lists:
        start[1:] = np.cumsum([len(l) for l in lists])
    kf = np.array([k for l in lists for k in l], np.int32)
    return start, kf


def make_map(K, pts, lns=(), live=None):
    ps, pk = csr(list(pts))
    ls, lk = csr(list(lns))
    return dict(K=int(K), pts=[list(l) for l in pts], lns=[list(l) for l in lns], pt_start=ps, pt_kf=pk, ln_start=ls, ln_kf=lk,
                live=None if live is None else np.asarray(live, np.uint8))


def live_of(m):
    return np.ones(m["K"], np.uint8) if m["live"] is None else m["live"]


# ---- the recount --------------------------------------------------------------------------------------------------------------------
def recount_dense(m):
    """C as a K x K int64 array (small K): per landmark the outer product of the multiplicities, the diagonal and the dead cleared"""
    K = m["K"]
    Cm = np.zeros((K, K), np.int64)
    for l in m["pts"] + m["lns"]:
        if len(l):
            mult = np.bincount(np.asarray(l, np.int64), minlength=K)
            nz = np.flatnonzero(mult)
            Cm[np.ix_(nz, nz)] += np.outer(mult[nz], mult[nz])
    np.fill_diagonal(Cm, 0)
    dead = live_of(m) == 0
    Cm[dead, :] = 0; Cm[:, dead] = 0
    return Cm


def recount_keys(m):
    """the same as sorted 64-bit pair keys (large K): (i, j, count) arrays over the nonzero entries, i-major, j ascending"""
    if "_keys" in m:
        return m["_keys"]
    K = m["K"]
    lv = live_of(m)
    keys, wts = [], []
    all_l = m["pts"] + m["lns"]
    two = np.array([l for l in all_l if len(l) == 2 and l[0] != l[1]], np.int64).reshape(-1, 2)      # (the bulk of a map, taken at once)
    if len(two):
        keys += [two[:, 0] * K + two[:, 1], two[:, 1] * K + two[:, 0]]; wts += [np.ones(len(two), np.int64)] * 2
    for l in all_l:
        if len(l) < 3:
            continue      # (two equal entries: only the diagonal)
        u, mult = np.unique(np.asarray(l, np.int64), return_counts=True)
        if len(u) < 2:
            continue
        a, b = np.meshgrid(np.arange(len(u)), np.arange(len(u)), indexing="ij")
        off = a != b
        keys.append(u[a[off]] * K + u[b[off]]); wts.append(mult[a[off]] * mult[b[off]])
    if not keys:
        z = np.zeros(0, np.int64)
        m["_keys"] = (z, z, z)
        return m["_keys"]
    keys, wts = np.concatenate(keys), np.concatenate(wts)
    uk, inv = np.unique(keys, return_inverse=True)
    cnt = np.bincount(inv, weights=wts).astype(np.int64)
    i, j = uk // K, uk % K
    keep = (lv[i] != 0) & (lv[j] != 0)
    m["_keys"] = (i[keep], j[keep], cnt[keep])
    return m["_keys"]


def rows_ref(m, kf, min_count):
    """plba_covis_rows: (row_start, col, cnt)"""
    i, j, c = recount_keys(m)
    thr = max(1, int(min_count))
    rs, col, cnt = [0], [], []
    for r in kf:
        a, b = np.searchsorted(i, r), np.searchsorted(i, r, side="right")      # (the keys are sorted: i-major, j ascending)
        sel = c[a:b] >= thr
        col.append(j[a:b][sel]); cnt.append(c[a:b][sel])
        rs.append(rs[-1] + int(sel.sum()))
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)
    return np.array(rs, np.int32), cat(col), cat(cnt)


def column_ref(m, idx):
    i, j, c = recount_keys(m)
    out = np.zeros(idx, np.int32)
    sel = (j == idx) & (i < idx)
    out[i[sel]] = c[sel]
    return out


# ---- the reference's increments -----------------------------------------------------------------------------------------------------
def replay_increments(K, events):
    """full_graph as the reference's increments leave it (no removals).  events, in insertion order:
    ("new", kind, kf1, kf2): a landmark created from a KF-to-KF match: kf_obs_list = [kf1, kf2], full_graph[kf2][kf1]++ and its mirror
    (:358-372 and the line twin); ("obs", kind, lm, kf2): addMap*Observation(kf2), then for every obs of the list, obs != kf2:
    full_graph[kf2][obs]++ and its mirror (:390-400, :670-677 and the line twins).  Returns (full_graph, point lists, line lists)."""
    G = np.zeros((K, K), np.int64)
    lists = {0: [], 1: []}
    for ev in events:
        if ev[0] == "new":
            _, kind, kf1, kf2 = ev
            lists[kind].append([kf1, kf2])
            G[kf2][kf1] += 1
            G[kf1][kf2] += 1
        else:
            _, kind, lm, kf2 = ev
            lists[kind][lm].append(kf2)
            for obs in lists[kind][lm]:
                if obs != kf2:
                    G[kf2][obs] += 1
                    G[obs][kf2] += 1
    return G, lists[0], lists[1]


def remove_keyframe(G, kf):
    """:3033-3038: the removed keyframe's row and column are cleared"""
    G[kf, :] = 0
    G[:, kf] = 0


def insertion_sequence(K, seed, n_new=6, p_obs=0.7, p_twice=0.1):
    """a generated insertion sequence: every keyframe creates landmarks with its predecessor and re-observes some of the landmarks of the
    last few keyframes, now and then the same landmark twice"""
    rng = np.random.default_rng(seed)
    events, n = [], {0: 0, 1: 0}
    recent = []      # (kind, landmark, keyframe it was last seen from)
    for kf in range(1, K):
        for kind in (0, 1):
            for (kd, lm, last) in list(recent):
                if kd == kind and kf - last <= 4 and rng.random() < p_obs:
                    events.append(("obs", kind, lm, kf))
                    if rng.random() < p_twice:
                        events.append(("obs", kind, lm, kf))
                    recent.remove((kd, lm, last)); recent.append((kd, lm, kf))
            for _ in range(n_new if kind == 0 else max(n_new // 3, 1)):
                events.append(("new", kind, kf - 1, kf))
                recent.append((kind, n[kind], kf)); n[kind] += 1
        recent = [r for r in recent if kf - r[2] <= 4]
    return events


# ---- the readers of the graph -------------------------------------------------------------------------------------------------------
def edge_loop(Cm, live, nv, opts=None, loops=()):
    """:4373-4408 as two literal fors over a dense C (small K); the loop edges follow in the order given"""
    o = dict(DEFAULTS); o.update(opts or {})
    ei, ej = [], []
    for i in range(nv):
        for j in range(i + 1, nv):
            if live[i] and live[j] and (Cm[i][j] >= o["min_lm_ess_graph"] or Cm[i][j] >= o["min_lm_cov_graph"] or abs(i - j) == 1):
                ei.append(i); ej.append(j)
    for a, b in loops:
        ei.append(a); ej.append(b)
    return np.array(ei, np.int32), np.array(ej, np.int32)


def edge_loop_keys(m, nv, opts=None, loops=()):
    """the same from the pair keys (large K): the entries over a threshold and the live neighbours, sorted i-major"""
    o = dict(DEFAULTS); o.update(opts or {})
    lv = live_of(m)
    i, j, c = recount_keys(m)
    sel = (j > i) & (j < nv) & ((c >= o["min_lm_ess_graph"]) | (c >= o["min_lm_cov_graph"]))
    a = np.arange(nv - 1)
    a = a[(lv[a] != 0) & (lv[a + 1] != 0)]
    K = m["K"]
    keys = np.unique(np.concatenate([i[sel] * K + j[sel], a.astype(np.int64) * K + a + 1]))
    ei, ej = (keys // K).astype(np.int32), (keys % K).astype(np.int32)
    if len(loops):
        lp = np.asarray(loops, np.int32).reshape(-1, 2)
        ei, ej = np.concatenate([ei, lp[:, 0]]), np.concatenate([ej, lp[:, 1]])
    return ei, ej


def local_map_ref(m, kf, opts=None):
    """formLocalMap with the row of kf and a dead keyframe never local (the two stated deviations): flags and the three counts"""
    o = dict(DEFAULTS); o.update(opts or {})
    K, lv = m["K"], live_of(m)
    row = np.zeros(K, np.int64)
    i, j, c = recount_keys(m)
    row[j[i == kf]] = c[i == kf]
    kl = np.zeros(K, np.uint8)
    for i_ in range(K):
        if lv[i_] and (i_ == kf or row[i_] >= o["min_lm_cov_graph"] or abs(kf - i_) <= o["min_kf_local_map"]):
            kl[i_] = 1
    pl = np.array([1 if any(kl[k] for k in l) else 0 for l in m["pts"]], np.uint8)
    ll = np.array([1 if any(kl[k] for k in l) else 0 for l in m["lns"]], np.uint8)
    return dict(kf_local=kl, pt_local=pl, ln_local=ll, counts=np.array([kl.sum(), pl.sum(), ll.sum()], np.int32))


def relative_pose(pose12, ei, ej, dt=np.float64):
    """Z = T_i^-1 T_j, T^-1 = [R^T, -R^T t], in the working type dt (np.float64, np.longdouble or "mp"); (ne, 12) of that type"""
    if dt == "mp":
        import mpmath
        mpmath.mp.dps = 40
        conv = np.vectorize(lambda v: mpmath.mpf(float(v)), otypes=[object])
        P = conv(np.asarray(pose12, np.float64))
    else:
        P = np.asarray(pose12, np.float64).astype(dt)
    out = np.empty((len(ei), 12), dtype=P.dtype)
    for e, (i, j) in enumerate(zip(ei, ej)):
        Ri, ti, Rj, tj = P[i, :9].reshape(3, 3), P[i, 9:], P[j, :9].reshape(3, 3), P[j, 9:]
        R = np.array([[sum(Ri[k, r] * Rj[k, c] for k in range(3)) for c in range(3)] for r in range(3)], dtype=P.dtype)
        t = np.array([sum(Ri[k, r] * (tj[k] - ti[k]) for k in range(3)) for r in range(3)], dtype=P.dtype)
        out[e, :9] = R.ravel(); out[e, 9:] = t
    return out


def meas_bound(pose12, ei, ej):
    """8 u sum_k |a_k| |b_k| per entry (u = 2^-53): rotation entries with the products of R_i^T R_j, translation entries with a_k =
    R_i[k][r], b_k = |t_j[k]| + |t_i[k]|.  First order 4 u for either association of R_i^T (t_j - t_i), contracted or not; the factor 2
    covers the second-order terms."""
    P = np.abs(np.asarray(pose12, np.float64))
    u = 2.0 ** -53
    out = np.empty((len(ei), 12))
    for e, (i, j) in enumerate(zip(ei, ej)):
        Ri, ti, Rj, tj = P[i, :9].reshape(3, 3), P[i, 9:], P[j, :9].reshape(3, 3), P[j, 9:]
        out[e, :9] = (Ri.T @ Rj).ravel()
        out[e, 9:] = Ri.T @ (tj + ti)
    return 8 * u * out


# ---- generated maps -----------------------------------------------------------------------------------------------------------------
def trajectory(K, seed, per_kf=40, live=None):
    """a trajectory in the manner of bow_ref.cov_columns: many landmarks shared with the recent keyframes (tracks of 2 - 12 observers), a
    few with keyframes further back, points and lines"""
    rng = np.random.default_rng(seed)
    pts, lns = [], []
    for k in range(K):
        for n, dst in ((per_kf, pts), (per_kf // 4, lns)):
            for _ in range(n):
                ln = int(rng.integers(2, 13))
                l = [k + d for d in range(ln) if k + d < K]
                if rng.random() < 0.05 and k > 20:
                    l.append(int(rng.integers(0, k - 10)))
                rng.shuffle(l)
                dst.append(l)
    return make_map(K, pts, lns, live)


def planted(counts, K=None, extra=()):
    """pairs (i, j) sharing exactly the given numbers of two-observer landmarks: counts is {(i, j): n}"""
    pts = []
    for (i, j), n in counts.items():
        pts += [[i, j]] * n
    pts += [list(e) for e in extra]
    K = K or 1 + max(max(p) for p in pts)
    return make_map(K, pts)


@functools.lru_cache(maxsize=None)
def case(name):
    """the maps of the tests; every one small enough for a few seconds on the CPU"""
    if name == "k1":
        return make_map(1, [[0], [0, 0]])
    if name == "k2":
        return make_map(2, [[0, 1], [1, 0], [1]], [[0, 1]])
    if name == "empty":
        return make_map(5, [], [])
    if name == "points_only":
        return make_map(6, [[0, 1, 2], [2, 3], [5, 0], []], [])
    if name == "lines_only":
        return make_map(6, [], [[0, 1, 2], [2, 3], [5, 0], []])
    if name == "one_observer":
        return make_map(4, [[2], [0, 1]], [[3]])
    if name == "multiplicity":      # unsorted lists with the same keyframe 2 and 3 times, adjacent and apart
        return make_map(5, [[3, 0, 3], [1, 1, 2], [4, 0, 4, 4], [2, 2, 2, 0, 0]], [[1, 3, 1, 3], [0, 0]])
    if name.startswith("kf_lms_"):      # a keyframe with n landmarks
        n = int(name[7:])
        return make_map(7, [[0, 1 + (l % 6)] for l in range(n)], [[3, 0, 5]])
    if name.startswith("observers_"):      # a landmark with n observers
        n = int(name[10:])
        return make_map(n + 3, [list(range(n))[::-1], [0, n + 1], [n + 2, 1, 0]])
    if name.startswith("tiles_"):      # K around the tile width, keyframe 0 sharing landmarks with W - 1, W and 2 W where they exist
        K = {"tiles_wm1": W - 1, "tiles_w": W, "tiles_wp1": W + 1, "tiles_2wp1": 2 * W + 1}[name]
        pts = [[0, 1], [1, 2, 0]] * 3 + [[K - 1, K - 2]] * 4
        for far in (W - 1, W, 2 * W):
            if far < K:
                pts += [[0, far]] * (2 + far % 3) + [[far, 5, 0]]
        return make_map(K, pts, [[0, K - 1], [W - 2, 0]])
    if name == "wide_row":      # one row with 1 100 nonzero columns: more than a workgroup's threads in the compaction
        return make_map(1101, [list(range(1101))])
    if name == "counter":      # two keyframes sharing 70 000 landmarks: a 16-bit or a saturating counter fails
        return make_map(3, [[0, 1]] * 70000 + [[1, 2]])
    if name == "thresholds":
        return planted({(0, 2): 74, (0, 3): 75, (0, 4): 76, (1, 5): 149, (1, 6): 150, (1, 7): 151, (2, 9): 80, (7, 9): 160}, K=10)
    if name == "traj200":
        return trajectory(200, 11)
    if name == "dead":
        lv = np.ones(60, np.uint8); lv[[7, 20, 21, 59]] = 0
        return trajectory(60, 5, per_kf=60, live=lv)
    if name == "traj60":
        return trajectory(60, 17, per_kf=60)
    raise KeyError(name)


CASES = ["k1", "k2", "empty", "points_only", "lines_only", "one_observer", "multiplicity", "kf_lms_63", "kf_lms_64", "kf_lms_65", "kf_lms_257",
         "observers_65", "observers_257", "tiles_wm1", "tiles_w", "tiles_wp1", "tiles_2wp1", "wide_row", "counter", "thresholds", "traj200", "dead", "traj60"]
OPTION_SETS = [dict(DEFAULTS), dict(min_lm_ess_graph=40, min_lm_cov_graph=90, min_kf_local_map=1), dict(min_lm_ess_graph=150, min_lm_cov_graph=1, min_kf_local_map=0),
               dict(min_lm_ess_graph=149, min_lm_cov_graph=151, min_kf_local_map=2)]


def poses(K, seed=3):
    """K poses (world -> keyframe) on a looping trajectory, pose12 layout"""
    from . import pgo_ref
    out = []
    for k in range(K):
        a = 2 * np.pi * k / max(K // 3, 8)
        Rwb = pgo_ref._rot(np.array([0.05 * np.sin(0.3 * k), 0.04 * np.cos(0.2 * k), a]))
        p = np.array([10 * np.cos(a) + 0.01 * k, 10 * np.sin(a), 0.5 * np.sin(0.1 * k)])
        out.append(np.concatenate([Rwb.T.ravel(), -Rwb.T @ p]))
    return np.array(out)


def queries(m, name):
    """the queries the host program and the device answer on a case: rows (descending with a repeat), min_count, column index, nv, loop
    edges, keyframe of the local map"""
    K = m["K"]
    rows = list(range(K))[::-1][:300] + [K // 2]
    if name.startswith("tiles_"):
        rows = [0, K - 1, W - 1 if W - 1 < K else 1, 0, 5]
    nv = K if K < 4 else K - 2
    loops = [(0, nv - 1), (nv - 2, 1), (2, nv - 1)] if nv >= 6 else []
    return dict(rows=np.array(rows, np.int32), min_count=(75 if name in ("thresholds", "traj200") else 0), idx=K - 1, nv=nv, loops=loops, kf=max(K - 5, 0))


def expected(m, q, opts):
    """every output of the four queries by this module alone"""
    nv = q["nv"]
    if m["K"] <= 400:
        ei, ej = edge_loop(recount_dense(m), live_of(m), nv, opts, q["loops"])
        ei2, ej2 = edge_loop_keys(m, nv, opts, q["loops"])
        assert np.array_equal(ei, ei2) and np.array_equal(ej, ej2)      # the two forms of the edge loop agree where both run
    else:
        ei, ej = edge_loop_keys(m, nv, opts, q["loops"])
    return dict(rows=rows_ref(m, q["rows"], q["min_count"]), cov=column_ref(m, q["idx"]), ei=ei, ej=ej, local=local_map_ref(m, q["kf"], opts))


# ---- the host check -----------------------------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
HOSTCHECK_SRC = os.path.join(CSRC, "plba_covis_hostcheck.cpp")
DEV_HEADER = os.path.join(CSRC, "plba_covis_dev.h")


def build_hostcheck(out_dir, sanitize=True, header_dir=None):
    """csrc/plba_covis_hostcheck.cpp, a stand-alone program, with the host sanitizers unless told otherwise; header_dir: a directory
    whose plba_covis_dev.h is taken instead of csrc's (the mutation tests).  Returns its path."""
    exe = os.path.join(out_dir, "plba_covis_hostcheck" + ("_san" if sanitize else ""))
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    deps = [HOSTCHECK_SRC, DEV_HEADER, os.path.join(CSRC, "plba_match_dev.h"), os.path.join(ROOT, "include", "plba_g2o", "covis.h")]
    if header_dir is None and os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    os.makedirs(out_dir, exist_ok=True)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if sanitize else ["-O2"]
    inc = (["-I", header_dir] if header_dir else []) + ["-I", os.path.join(ROOT, "include"), "-I", CSRC]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-ffp-contract=off"] + flags + inc + [HOSTCHECK_SRC, "-o", exe])
    return exe


def write_host_input(path, m, q, opts, pose12):
    o = dict(DEFAULTS); o.update(opts or {})
    loops = np.asarray(q["loops"], np.int32).reshape(-1, 2)
    hd = [m["K"], len(m["pts"]), len(m["lns"]), 0 if m["live"] is None else 1, len(q["rows"]), q["min_count"], q["idx"], q["nv"], len(loops),
          o["min_lm_ess_graph"], o["min_lm_cov_graph"], o["min_kf_local_map"], q["kf"]]
    with open(path, "wb") as f:
        f.write(np.array(hd, np.int32).tobytes())
        if m["live"] is not None:
            f.write(m["live"].tobytes())
        for a in (m["pt_start"], m["pt_kf"], m["ln_start"], m["ln_kf"], np.asarray(q["rows"], np.int32)):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        f.write(np.ascontiguousarray(pose12[:q["nv"]], np.float64).tobytes())
        f.write(loops.tobytes())
        f.write(np.ascontiguousarray(loop_meas(pose12, loops), np.float64).tobytes())


def loop_meas(pose12, loops):
    """measurements of the loop edges: the relative pose of the poses given (a consistent graph)"""
    loops = np.asarray(loops, np.int32).reshape(-1, 2)
    return relative_pose(pose12, loops[:, 0], loops[:, 1]).astype(np.float64).reshape(-1, 12)


def host_run(exe, tmp, m, q, opts, pose12):
    """the host program's answers: dict like expected()'s plus meas; None when it refuses (exit code 3)"""
    pin, pout = os.path.join(tmp, "covis_in.bin"), os.path.join(tmp, "covis_out.bin")
    write_host_input(pin, m, q, opts, pose12)
    rc = subprocess.call([exe, pin, pout], stderr=subprocess.DEVNULL)
    if rc == 3:
        return None
    assert rc == 0, rc
    raw = open(pout, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(raw, dt, cnt, at[0]); at[0] += a.nbytes; return a
    n = len(q["rows"])
    rs = take(np.int32, n + 1)
    col, cnt = take(np.int32, rs[n]), take(np.int32, rs[n])
    cov = take(np.int32, q["idx"])
    ne = int(take(np.int32, 1)[0])
    ei, ej, meas = take(np.int32, ne), take(np.int32, ne), take(np.float64, 12 * ne).reshape(ne, 12)
    kl, pl, ll = take(np.uint8, m["K"]), take(np.uint8, len(m["pts"])), take(np.uint8, len(m["lns"]))
    c3 = take(np.int32, 3)
    assert at[0] == len(raw)
    return dict(rows=(rs, col, cnt), cov=cov, ei=ei, ej=ej, meas=meas, local=dict(kf_local=kl, pt_local=pl, ln_local=ll, counts=c3))


def same(got, want):
    """None when every integer output is equal, else the first that differs"""
    for k in range(3):
        if not np.array_equal(got["rows"][k], want["rows"][k]):
            return "rows[%d]" % k
    for k in ("cov", "ei", "ej"):
        if not np.array_equal(got[k], want[k]):
            return k
    for k in ("kf_local", "pt_local", "ln_local", "counts"):
        if not np.array_equal(got["local"][k], want["local"][k]):
            return "local." + k
    return None
