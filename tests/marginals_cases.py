"""The windows of the exact marginal-covariance tests (tests/test_marginals_exact_cpu.py holds the fp64 reference to the rules on them,
tests/test_marginals_exact.py the device).  Every case is a window.make_window window edited by hand — fixed flags, vertex ids, dropped
or re-made observations, moved landmarks — and asserts the property it is there for on the reference built from it (check), so that a
change of the generator cannot hollow it out.

The layout string has one letter per keyframe: x both vertices fixed, F both free (15 dims), P the PVR free and the bias fixed (9),
B the bias free and the PVR fixed (6).

prepare() builds, once per session, everything of a case that does not depend on the device: the oracle problem's fp64 reference
(tests/marginals_ref.py), the extended one (tests/marginals_exact.py), the extended inverse's columns and the landmark covariances."""
import numpy as np

from tests import marginals_exact as X
from tests import marginals_ref as mr
from tests.test_marginals_cpu import small_window

DIMS = {"x": 0, "F": 15, "P": 9, "B": 6}


def set_layout(w, layout):
    k = w["kf"]
    assert len(layout) == len(k["vid_pvr"])
    k["fixed_pvr"] = np.array([c in "xB" for c in layout], np.uint8)
    k["fixed_bias"] = np.array([c in "xP" for c in layout], np.uint8)
    return w


def _win(pkg, layout, npts, nlines, seed, track=(2, 6)):
    return set_layout(pkg.window.make_window(len(layout), npts, nlines, imu=True, seed=seed, track=track), layout)


def _drop_obs(w, kind, mask):
    keys = ("po_pt", "po_kf", "po_uv", "po_w") if kind == 0 else ("lo_ln", "lo_kf", "lo_l", "lo_w")
    for key in keys:
        w[key] = w[key][~mask]


def _cam_point(pkg, w, k, Xw):
    """(u, v, z) of a world point in keyframe k at the window's estimate (window._project's convention)"""
    c, kf = w["cam"], w["kf"]
    Rwb = pkg.window.R_from_quat(kf["q"][k])
    Rcb = np.asarray(c["Rbc"]).T
    Pc = Rcb @ (Rwb.T @ (Xw - kf["P"][k])) - Rcb @ np.asarray(c["Pbc"])
    return np.array([c["fx"] * Pc[0] / Pc[2] + c["cx"], c["fy"] * Pc[1] / Pc[2] + c["cy"]]), Pc[2]


def _remake_point_obs(pkg, w, l):
    """the observations of point l become its exact projections at the estimate (zero residual)"""
    for e in np.flatnonzero(w["po_pt"] == l):
        uv, z = _cam_point(pkg, w, int(w["po_kf"][e]), w["points"][l])
        assert z > 0.1
        w["po_uv"][e] = uv


def _remake_line_obs(pkg, w, l):
    for e in np.flatnonzero(w["lo_ln"] == l):
        k = int(w["lo_kf"][e])
        (s, zs), (t, zt) = _cam_point(pkg, w, k, w["lines"][l][:3]), _cam_point(pkg, w, k, w["lines"][l][3:])
        assert zs > 0.1 and zt > 0.1
        lv = np.cross(np.append(s, 1.0), np.append(t, 1.0))
        w["lo_l"][e] = lv / np.sqrt(lv[0] ** 2 + lv[1] ** 2)


def _pairs(w):
    """(i, j), (j, i), a repeat, i == j, and pairs with a fixed vertex (keyframe 0 is fixed in every case)"""
    k = w["kf"]
    free = [q for q in range(len(k["vid_pvr"])) if not k["fixed_pvr"][q] or not k["fixed_bias"][q]]
    i, j = free[0], free[-1]
    return np.array([[i, j], [j, i], [i, j], [i, i], [0, i], [i, 0], [0, 0]], np.int32)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def _layout_case(layout, P, seed, npts=None, nlines=None):
    def build(pkg, orc):
        K = len(layout)
        return dict(w=_win(pkg, layout, npts or 10 * K, nlines or 3 * K, seed))

    def check(c):
        assert c["ex"].P == P == sum(DIMS[ch] for ch in layout)
    return build, check


def _cfg2(pkg, orc):
    return dict(w=pkg.window.make_config(3, scale=0.1))


def _cfg2_check(c):
    assert c["ex"].P == 735 and (735 + 63) // 64 * 64 // 32 - 1 == 23      # 23 block steps; the column subset is in use
    assert len(c["cols"]) < 735


def _biasfirst(pkg, orc):
    w = small_window(pkg)
    k = w["kf"]
    old = (k["vid_pvr"].copy(), k["vid_bias"].copy())
    k["vid_pvr"] = (old[0] + 1).astype(np.int32)
    k["vid_bias"] = (k["vid_pvr"] - 1).astype(np.int32)
    pr = w["prior"]      # the prior follows its vertices
    pr["vid"] = np.array([k["vid_pvr"][1], k["vid_bias"][1]], np.int32)
    return dict(w=w)


def _biasfirst_check(c):
    k, ref = c["w"]["kf"], c["ex"].ref
    assert (np.diff(k["vid_pvr"]) > 0).all() and (np.diff(k["vid_bias"]) > 0).all() and (k["vid_bias"] < k["vid_pvr"]).all()
    free = [q for q in range(ref.K) if ref.op_off[q] >= 0 and ref.ob_off[q] >= 0]
    assert len(free) == 3 and all(ref.op_off[q] == ref.ob_off[q] + 6 for q in free)      # bias first
    assert c["ex"].P == 45 and c["w"]["prior"] is not None


def _mixed(pkg, orc):
    return dict(w=set_layout(small_window(pkg), "xFPB"))


def _mixed_check(c):
    ref = c["ex"].ref
    assert c["ex"].P == 30 and c["w"]["prior"] is not None
    assert ref.op_off[2] >= 0 and ref.ob_off[2] < 0 and ref.op_off[3] < 0 and ref.ob_off[3] >= 0


AXIS_DIRS = {0: (0.125, 0.75, 0.625), 1: (0.75, 0.125, -0.625), 2: (-0.625, 0.75, 0.125), "tie": (0.5, 0.5, 0.5)}


def _landmarks(pkg, orc):
    """keyframes 0 and 1 fixed; a point and a line seen from them only; a fixed point and a fixed line seen from free keyframes; a point with
    one active edge after set_levels; four lines turned to the three axis branches of the line basis and to its tie"""
    w = _win(pkg, "xxFFF", 60, 24, 0x3A11C7, track=(2, 5))
    tag = {}
    used = {0: set(), 1: set()}

    def pick(kind, want):
        lm_of, kf_of = (w["po_pt"], w["po_kf"]) if kind == 0 else (w["lo_ln"], w["lo_kf"])
        for l in range(len(w["points"] if kind == 0 else w["lines"])):
            kfs = set(int(q) for q in kf_of[lm_of == l])
            if l not in used[kind] and want(kfs):
                used[kind].add(l)
                return l
        raise AssertionError("no landmark of kind %d fits" % kind)
    for kind in (0, 1):
        l = pick(kind, lambda kfs: {0, 1} <= kfs)
        lm_of, kf_of = (w["po_pt"], w["po_kf"]) if kind == 0 else (w["lo_ln"], w["lo_kf"])
        _drop_obs(w, kind, (lm_of == l) & (kf_of >= 2))
        tag["fixed_kf_only_%d" % kind] = l
    w["point_fixed"] = np.zeros(len(w["points"]), np.uint8)
    w["line_fixed"] = np.zeros(len(w["lines"]), np.uint8)
    for kind, key in ((0, "point_fixed"), (1, "line_fixed")):
        l = pick(kind, lambda kfs: len(kfs & {2, 3, 4}) >= 2)
        w[key][l] = 1
        tag["fixed_lm_%d" % kind] = l
    l = pick(0, lambda kfs: len(kfs) >= 2 and max(kfs) >= 2)
    lev = np.zeros(len(w["po_pt"]), np.uint8)
    lev[np.flatnonzero(w["po_pt"] == l)[1:]] = 1
    tag["one_active"] = l
    for name, dv in AXIS_DIRS.items():
        l = pick(1, lambda kfs: len(kfs) >= 2 and max(kfs) >= 2)
        s = np.round(w["lines"][l][:3] * 8) / 8      # (a start and a step that are exact in fp64: the tie is an exact tie)
        w["lines"][l] = np.concatenate([s, s + np.array(dv)])
        _remake_line_obs(pkg, w, l)
        tag["axis_%s" % name] = l
    return dict(w=w, levels={0: lev}, tag=tag)


def _landmarks_check(c):
    ex, w, tag = c["ex"], c["w"], c["tag"]
    ref = ex.ref
    Np = ref.Np
    for kind in (0, 1):
        i = tag["fixed_kf_only_%d" % kind] + kind * Np
        assert ex.status[i] == 0 and len(ref.lm[i]["edges"]) >= 2 and ex.red[i][2] == []      # no coupling term: Sigma_ll = B Hr^-1 B^T
        i = tag["fixed_lm_%d" % kind] + kind * Np
        assert ex.status[i] == 1 and sum(ref.op_off[k] >= 0 for k, _, _, _ in ref.lm[i]["edges"]) >= 2
    i = tag["one_active"]
    assert ex.status[i] == 2 and len(ref.lm[i]["edges"]) == 1
    for name in AXIS_DIRS:
        i = tag["axis_%s" % name] + Np
        x = ref.lm[i]["x"]
        d = np.abs(x[3:] - x[:3])
        assert ex.status[i] == 0 and len(ex.red[i][2]) >= 1
        if name == "tie":
            assert d[0] == d[1] == d[2] and X.line_axis(x) == 0
        else:
            assert X.line_axis(x) == name and d[name] < np.delete(d, name).min()
    # Huber is on and acts: at least one point edge and one line edge beyond delta
    for kind, sl in ((0, slice(0, Np)), (1, slice(Np, None))):
        assert w["huber"].get(kind) is not None and any(r < 1.0 for lm in ref.lm[sl] for r in lm["rho1"])
    assert (ex.status == 0).sum() > 40


def _degenerate(pkg, orc):
    """two points moved out along their first observation's ray until the reduced block's pivot ratio is 3e-15 (degenerate, status 3) and
    3e-10 (sound, status 0): a factor 300 either side of the 1e-12 rule, so that no rounding of the Jacobians brings either within 100"""
    w = _win(pkg, "xFFF", 30, 8, 0x3A11C9, track=(3, 4))
    cam = orc.cam_vec(w["cam"])
    kf = w["kf"]
    nav = [orc.nav_vec(kf["P"][k], kf["V"][k], kf["q"][k], kf["bg"][k], kf["ba"][k], kf["dbg"][k], kf["dba"][k]) for k in range(4)]
    tag = {}

    def ratio_at(l, Xw):
        H = X.wzeros(3, 3)
        for e in np.flatnonzero(w["po_pt"] == l):
            k = int(w["po_kf"][e])
            uv, z = _cam_point(pkg, w, k, Xw)
            Jl = X.wide(orc.eval_point_edge(cam, nav[k], Xw, uv)[1])
            H += Jl.T @ Jl
        piv = X._chol(H)[1]
        return float(min(piv) / max(H[q, q] for q in range(3)))
    long_tracks = [l for l in range(len(w["points"])) if (w["po_pt"] == l).sum() >= 3]
    for l, (name, target) in zip(long_tracks, (("degenerate", 3e-15), ("sound", 3e-10))):
        es = np.flatnonzero(w["po_pt"] == l)
        c0 = kf["P"][int(w["po_kf"][es[0]])]
        ray = (w["points"][l] - c0) / np.linalg.norm(w["points"][l] - c0)
        lo, hi = 1.0, 1e9
        for _ in range(60):      # the ratio falls like 1 / distance^2
            mid = np.sqrt(lo * hi)
            lo, hi = (mid, hi) if ratio_at(l, c0 + mid * ray) > target else (lo, mid)
        w["points"][l] = c0 + lo * ray
        _remake_point_obs(pkg, w, l)
        tag[name] = l
    assert len(tag) == 2
    return dict(w=w, tag=tag)


def _degenerate_check(c):
    ex, tag = c["ex"], c["tag"]
    a, b = tag["degenerate"], tag["sound"]
    assert ex.status[a] == 3 and 1e-15 < ex.ratio[a] < 1e-14, ex.ratio[a]
    assert ex.status[b] == 0 and 1e-10 < ex.ratio[b] < 1e-9, ex.ratio[b]
    assert (ex.status == 3).sum() == 1


CASES = {}
for _name, _layout, _P, _seed in (("P15", "xFx", 15, 0x3A1115), ("P9", "xPx", 9, 0x3A1109), ("P63", "xFFFPP", 63, 0x3A1163),
                                  ("P66", "xFFFFB", 66, 0x3A1166), ("P192", "x" + "F" * 12 + "BB", 192, 0x3A1192),
                                  ("P195", "x" + "F" * 13, 195, 0x3A1195)):
    CASES[_name] = _layout_case(_layout, _P, _seed)
CASES["P735"] = (_cfg2, _cfg2_check)
CASES["biasfirst"] = (_biasfirst, _biasfirst_check)
CASES["mixed"] = (_mixed, _mixed_check)
CASES["landmarks"] = (_landmarks, _landmarks_check)
CASES["degenerate"] = (_degenerate, _degenerate_check)
NAMES = sorted(CASES)

_READY = {}


def robust_of(w):
    return {k: w["huber"].get(k) for k in range(4)}


def oracle_problem(orc, c):
    op = orc.new_problem()
    op.upload_window(c["w"])
    for kind, lev in c.get("levels", {}).items():
        op.set_levels(kind, lev)
    return op


def prepare(pkg, orc, name):
    if name in _READY:
        return _READY[name]
    build, check = CASES[name]
    c = build(pkg, orc)
    c["name"], c["pairs"] = name, _pairs(c["w"])
    op = oracle_problem(orc, c)
    rob = robust_of(c["w"])
    ex = c["ex"] = X.Exact(op, c["w"], rob)
    P = ex.P
    out64, ref, res64, Hs = mr.reference(op, c["w"], {0: rob[0], 1: rob[1]}, dense_check=P <= 256)
    op.close()
    c["out64"], c["res64"], c["Hs"] = out64, res64, Hs
    c["cols"] = X.compared_columns(P)
    # the extended inverse of S_ref: the compared columns, and up to P = 256 every column a landmark needs (beyond, the landmarks whose
    # observing keyframes lie inside the compared columns are the ones compared)
    need = sorted(set(c["cols"]) | (set(ex.landmark_cols()) if P <= 256 else set()))
    c["ext"], c["omega"] = X.inverse_ext(ex.S, need)
    c["cov_ref"] = ex.landmark_cov(c["ext"])
    live = sorted(c["cov_ref"])
    c["formulas"] = [res64["cov"], res64["dense"]["cov"] if P <= 256 else X.hybrid_dense_cov(ex, res64, live)]
    assert np.array_equal(res64["status"], ex.status)
    assert ex.pivot_margin() >= X.PIV_CLEAR, ex.pivot_margin()
    if P <= 256:
        assert set(live) == set(np.flatnonzero(ex.status == 0))
    else:
        assert len(live) >= 20
    check(c)
    _READY[name] = c
    return c
