"""Multi-step landmark groups, forced chain segment lengths and windows past 256 keyframes against the oracle.

The stage-by-stage comparisons of tests/test_lm_fused.py run on windows small enough that the host sizes every landmark group to one
workgroup step (csrc/plba_api.hip, build_lm_groups).  The step loop of lm_schur_group / lm_schur_group_wide / the trial pass
(csrc/plba_lm_dev.h) — the prefetch of step s + 1's data and step s + 2's indices, the wide form's shared panel handed from step to step —
then never runs more than once under a 1e-9 comparison, while the measured configurations run it 4 .. 9 times.  Here:
  * options.lm_group_steps forced on windows whose groups are known exactly (every group's keyframe window fits, so the host cuts them
    purely by count): the built system, the solution and the two-stage protocol against the oracle;
  * the default sizing at BASELINE configs[2] and configs[4], where groups take several steps on their own;
  * options.chain_seg forced to 1 .. 8 on IMU windows with fixed keyframes, a dropped IMU edge and a marginalization prior, on the record-based
    and the fused passes (where the segments ride in the trial launch);
  * windows of 257 and 300 keyframes: the group cut by stamp array and the table fill by search instead of bit masks and lookup tables.
Every case first asserts that the path it is about is the one that ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUILT = ("chi2", "maxdiag", "err_pt", "err_ln", "hll_pt", "bl_pt", "hll_ln", "bl_ln", "bp", "bschur", "Hschur")
LMF_W = 8             # window slots of a standard group; a landmark with more observations goes to a wide group (16 slots)
LMF_UNITS = 32        # units per workgroup step: a point takes one, a line two, a wide landmark twice as many


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def _pose_delta(a, b, pkg):
    dphi = max(np.linalg.norm(pkg.window.log_so3(pkg.window.R_from_quat(qb).T @ pkg.window.R_from_quat(qa))) for qa, qb in zip(a["q"], b["q"]))
    return max(np.abs(a["P"] - b["P"]).max(), np.abs(a["V"] - b["V"]).max(), dphi, np.abs(a["dbg"] - b["dbg"]).max(), np.abs(a["dba"] - b["dba"]).max())


def _keep(w, npt, nln, nobs):
    """w cut to its first `npt` points and `nln` lines with lo <= observations <= hi (nobs = (lo, hi)), renumbered"""
    out = dict(w)
    for pts, ob_lm, ob_kf, rest, n in (("points", "po_pt", "po_kf", ("po_uv", "po_w"), npt), ("lines", "lo_ln", "lo_kf", ("lo_l", "lo_w"), nln)):
        cnt = np.bincount(w[ob_lm], minlength=len(w[pts]))
        keep = np.flatnonzero((cnt >= nobs[0]) & (cnt <= nobs[1]))[:n]
        assert len(keep) == n, (pts, len(keep), n)
        new = np.full(len(w[pts]), -1, np.int64); new[keep] = np.arange(n)
        sel = new[w[ob_lm]] >= 0
        out[pts] = w[pts][keep]
        out[ob_lm] = new[w[ob_lm][sel]].astype(np.int32); out[ob_kf] = w[ob_kf][sel]
        for k in rest: out[k] = w[k][sel]
    out["meta"] = dict(w["meta"], Np=npt, Nl=nln, Ep=len(out["po_pt"]), El=len(out["lo_ln"]))
    return out


def _tracks(pkg, K, npt, nln, nobs, seed, over=1):
    """a K-keyframe IMU window of `npt` points and `nln` lines, each seen from nobs[0] .. nobs[1] keyframes (drawn `over` times as many and cut)"""
    w = pkg.window.make_window(K, over * npt, over * nln, imu=True, seed=seed, kf_dt=0.1, track=(nobs[0], K))
    return _keep(w, npt, nln, nobs)


def _groups(w, steps):
    """the groups the host cuts where every group's keyframe window fits (all landmarks standard in <= 8 keyframes, or all wide in <= 16):
    per kind, landmarks in (first keyframe, last keyframe, index) order, cut every 32 * steps points / 16 * steps lines, half as many in a wide
    group.  Returns [(kind, wide, landmark indices in group order, window keyframes)]"""
    out = []
    for kind, (lm, kf, n) in enumerate(((w["po_pt"], w["po_kf"], len(w["points"])), (w["lo_ln"], w["lo_kf"], len(w["lines"])))):
        cnt = np.bincount(lm, minlength=n)
        kmin = np.full(n, 1 << 30); np.minimum.at(kmin, lm, kf)
        kmax = np.full(n, -1); np.maximum.at(kmax, lm, kf)
        for wide in (0, 1):
            idx = np.flatnonzero((cnt > 0) & ((cnt > LMF_W) == bool(wide)))
            idx = idx[np.lexsort((idx, kmax[idx], kmin[idx]))]
            cap = (16 if kind else 32) * steps // (2 if wide else 1)
            for a in range(0, len(idx), cap):
                ch = idx[a:a + cap]
                out.append((kind, wide, ch, np.unique(kf[np.isin(lm, ch)])))
    assert all(len(win) <= (16 if wd else LMF_W) for _, wd, _, win in out), "the case's groups would not be cut by count alone"
    return out


def _units(kind, wide):
    return (2 if kind else 1) * (2 if wide else 1)


def _hist(groups):
    """debug_get("lm_groups") of those groups: [0..7] point groups of 1 .. 8+ steps, [8..15] line groups, [16] window slots, [17] steps,
    [18] wide groups"""
    h = [0.0] * 20
    for kind, wide, ch, win in groups:
        st = (_units(kind, wide) * len(ch) + LMF_UNITS - 1) // LMF_UNITS
        h[8 * kind + min(st, 8) - 1] += 1; h[16] += len(win); h[17] += st; h[18] += wide
    return h


def _fixed_past_step0(groups, w):
    """(points, lines): some fixed landmark sits in the second or a later step of its group"""
    res = [False, False]
    for kind, wide, ch, _ in groups:
        fx = w.get("line_fixed" if kind else "point_fixed")
        if fx is not None:
            res[kind] |= any(fx[s] and (k * _units(kind, wide)) // LMF_UNITS >= 1 for k, s in enumerate(ch))
    return tuple(res)


_ORACLE = {}


def _oracle_system(orc, key, w, solve=True):
    if key not in _ORACLE:
        o = orc.new_problem(); o.upload_window(w); o.debug_build(5.0, solve)
        _ORACLE[key] = {k: o.debug_get(k).copy() for k in BUILT + (("x",) if solve else ())}
        o.close()
    return _ORACLE[key]


def _check_system(g, ref, solve=True):
    g.debug_build(5.0, solve)
    for what in BUILT:
        assert _rel(g.debug_get(what), ref[what]) < 1e-9, what
    if solve:
        assert g.debug_get("solver_ok")[0] == 1
        assert _rel(g.debug_get("x"), ref["x"]) < 1e-7


def _oracle_protocol(pkg, orc, key, w, **opts):
    if key not in _ORACLE:
        o = orc.new_problem(**opts); o.upload_window(w)
        r = pkg.protocol.local_ba(o)
        _ORACLE[key] = (r, o.get_keyframes(), [(t["iteration"], t["trial"], t["accepted"]) for t in o.trace()])
        o.close()
    return _ORACLE[key]


def _check_protocol(pkg, g, ref):
    ro, ko, tro = ref
    r = pkg.protocol.local_ba(g)
    assert r["gated"] == ro["gated"]
    assert [(t["iteration"], t["trial"], t["accepted"]) for t in g.trace()] == tro
    assert r["stage2"].chi2_final == pytest.approx(ro["stage2"].chi2_final, rel=1e-9)
    assert _pose_delta(g.get_keyframes(), ko, pkg) < 1e-9


# ---- 1. group steps forced ----------------------------------------------------------------------------------------------------------------
# (K, points, lines, observations per landmark, seed, over-draw): K = 8 — every landmark standard and any 8 keyframes fit one window; K = 16 / 13
# with tracks over 9+ keyframes — every landmark wide (two units), windows of 16 slots (tile variant 1) / at most 13 (tile variant 0)
TILED = {
    # steps 2: points 64 | 64 | 40 (2 full, 2 full, 2 partial), lines 32 | 32 | 20 (64 | 64 | 40 units)
    "std_s2": (2, (8, 168, 84, (2, 8), 0x6A01, 1)),
    # steps 3: points 96 | 96 | 40 (3, 3 full, 2 partial), lines 48 | 40 (3 full, 3 partial)
    "std_s3": (3, (8, 232, 88, (2, 8), 0x6A02, 1)),
    # steps 5: points 160 | 160 | 100 (5, 5 full, 4 partial), lines 80 | 33 (5 full, 3 partial)
    "std_s5": (5, (8, 420, 113, (2, 8), 0x6A03, 1)),
    # steps 16 (the largest): points 512 | 300 (16 full, 10 partial), lines 256 | 17 (16 full, 2 partial)
    "std_s16": (16, (8, 812, 273, (2, 8), 0x6A04, 1)),
    # wide, 16 slots: points 32 | 32 | 20 (2, 2 full, 2 partial), lines 16 | 16 | 8 (2, 2, 1 full)
    "wide16_s2": (2, (16, 84, 40, (9, 16), 0x6A05, 4)),
    # wide, 16 slots: points 48 | 40 (3 full, 3 partial), lines 24 | 10 (3 full, 2 partial)
    "wide16_s3": (3, (16, 88, 34, (9, 16), 0x6A06, 4)),
    # wide, 16 slots: points 256 | 50 (16 full, 4 partial), lines 128 | 9 (16 full, 2 partial)
    "wide16_s16": (16, (16, 306, 137, (9, 16), 0x6A07, 4)),
    # wide, <= 13 slots: points 32 | 32 | 20, lines 16 | 16 | 8
    "wide13_s2": (2, (13, 84, 40, (9, 13), 0x6A08, 5)),
    # wide, <= 13 slots: points 80 | 70 (5 full, 5 partial), lines 40 | 25 (5 full, 4 partial)
    "wide13_s5": (5, (13, 150, 65, (9, 13), 0x6A09, 5)),
}
_WIN = {}


def _tiled_window(pkg, name):
    if name not in _WIN:
        _WIN[name] = _tracks(pkg, *TILED[name][1][:5], over=TILED[name][1][5])
    return _WIN[name]


@pytest.mark.parametrize("name", list(TILED))
def test_forced_group_steps_built_system(pkg, orc, hip, name):
    steps = TILED[name][0]
    w = _tiled_window(pkg, name)
    grp = _groups(w, steps)
    st = [(_units(k, wd) * len(ch) + LMF_UNITS - 1) // LMF_UNITS for k, wd, ch, _ in grp]
    full = [(_units(k, wd) * len(ch)) % LMF_UNITS == 0 for k, wd, ch, _ in grp]
    # the case covers what it is there for: the largest group takes exactly `steps` steps (with steps >= 3 the s + 2 index prefetch runs
    # too), some multi-step group ends on a full step and some on a partial one
    assert max(st) == steps and any(f and s > 1 for f, s in zip(full, st)) and any(not f and s > 1 for f, s in zip(full, st))
    wide = {wd for _, wd, _, _ in grp}
    assert wide == ({1} if name.startswith("wide") else {0})
    if name.startswith("wide16"):
        assert any(len(win) > 13 for _, _, _, win in grp)      # the 16-slot tile variant (next to the 13-slot one where a group spans fewer keyframes)
    if name.startswith("wide13"):
        assert all(len(win) <= 13 for _, _, _, win in grp)
    g = pkg.new_problem(lm_fused=2, lm_group_steps=steps); g.upload_window(w)
    _check_system(g, _oracle_system(orc, name, w))
    lf = g.debug_get("lm_fused")
    assert lf[0] == 1 and lf[1] == len(grp) and lf[3] == (len(grp) if wide == {1} else 0)
    assert list(g.debug_get("lm_groups")) == _hist(grp)      # exactly these groups, step for step
    g.close()


@pytest.mark.parametrize("name", ["mixed30", "k12_long"])
@pytest.mark.parametrize("steps", [2, 3, 5])
def test_forced_group_steps_standard_and_wide_side_by_side(pkg, orc, hip, name, steps):
    from tests.test_lm_fused import WINDOWS
    if name not in _WIN:
        _WIN[name] = WINDOWS[name](pkg)
    w = _WIN[name]
    g = pkg.new_problem(lm_fused=2, lm_group_steps=steps); g.upload_window(w)
    _check_system(g, _oracle_system(orc, name, w))
    lf, h = g.debug_get("lm_fused"), g.debug_get("lm_groups")
    assert lf[0] == 1 and 0 < lf[3] < lf[1]                                   # standard and wide groups
    assert h[17] > lf[1] and h[1:8].sum() + h[9:16].sum() > 0                 # more steps than groups: multi-step groups ran
    g.close()


# the two-stage protocol on a subset: fixed keyframes, fixed points and lines in the second or a later step of their group, a marginalization
# prior, trials that overshoot (user_lambda_init = 1e-2 on wide13_s5: the second stage rejects its first six).  (With the prior of their own
# first BA the 8- and 16-keyframe windows leave the chain path, and with it the fused passes: the prior rides on the 13-keyframe window.)
PROTOCOL = [("std_s3", "fixed", 0.0, False), ("std_s16", "", 0.0, False), ("wide16_s2", "fixed", 1e4, False), ("wide13_s5", "prior+fixed", 1e-2, True)]


@pytest.mark.parametrize("name,extras,lam,rejects", PROTOCOL)
def test_forced_group_steps_protocol(pkg, orc, hip, name, extras, lam, rejects):
    steps, (K, npt, nln, nobs, seed, over) = TILED[name]
    w = _tracks(pkg, K, npt, nln, nobs, seed, over)
    if "prior" in extras:
        o = orc.new_problem(); o.upload_window(w); pkg.protocol.local_ba(o); pr = o.marginalize(0, 50); o.close()
        w = _tracks(pkg, K, npt, nln, nobs, seed, over)
        w["prior"] = pr
    if "fixed" in extras:
        w["kf"]["fixed_pvr"][K // 2] = 1
        w["point_fixed"] = np.zeros(npt, np.uint8); w["point_fixed"][5::7] = 1
        w["line_fixed"] = np.zeros(nln, np.uint8); w["line_fixed"][3::5] = 1
        assert _fixed_past_step0(_groups(w, steps), w) == (True, True)
    ref = _oracle_protocol(pkg, orc, ("protocol", name, extras, lam), w, user_lambda_init=lam)
    assert (not all(a for _, _, a in ref[2])) == rejects      # rejected trials on the oracle's own run
    g = pkg.new_problem(lm_fused=2, lm_group_steps=steps, user_lambda_init=lam); g.upload_window(w)
    _check_protocol(pkg, g, ref)
    assert g.debug_get("lm_fused")[0] == 1 and g.debug_get("lm_groups")[17] > g.debug_get("lm_fused")[1]
    g.close()


# ---- 2. the default sizing at full size -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_windows(pkg):
    return {}


@pytest.mark.parametrize("cfg", [3, 5])
def test_default_group_sizing_at_full_size(pkg, orc, hip, full_windows, cfg):
    """BASELINE configs[2] (make_config(3)) and configs[4] (make_config(5)) with default options: the host sizes the groups to several steps
    itself (how many depends on the CU count: read, not assumed)"""
    w = full_windows.setdefault(cfg, pkg.window.make_config(cfg))
    g = pkg.new_problem(); g.upload_window(w)
    _check_system(g, _oracle_system(orc, ("config", cfg), w))
    lf, h = g.debug_get("lm_fused"), g.debug_get("lm_groups")
    assert lf[0] == 1 and h[17] > lf[1], (lf, h)
    print("configs[%d]: %d groups, %d steps, histogram %s" % (cfg - 1, lf[1], h[17], h[:16]))
    g.close()


# ---- 3. chain segments forced ---------------------------------------------------------------------------------------------------------------
def _chain_window(pkg, orc, name):
    if name == "k12":
        return pkg.window.make_window(12, 300, 60, imu=True, seed=0xC5E0)
    if name == "k23":      # K - 1 = 22: no multiple of 3 .. 8
        return pkg.window.make_window(23, 460, 92, imu=True, seed=0xC5E1)
    if name == "k19_fixed_dropped":      # a fixed middle keyframe (two chains) and no IMU edge between keyframes 6 and 7
        w = pkg.window.make_window(19, 760, 152, imu=True, seed=0xC5E2)
        K = 19; kf = w["kf"]
        kf["fixed_pvr"] = kf["fixed_pvr"].copy(); kf["fixed_bias"] = kf["fixed_bias"].copy()
        kf["fixed_pvr"][K // 2] = 1; kf["fixed_bias"][K // 2] = 1
        im = dict(w["imu"]); keep = np.ones(K - 1, bool); keep[K // 3] = False
        for k in ("kf_i", "kf_j", "preint", "info_pvr", "info_bias"): im[k] = im[k][keep]
        w["imu"] = im
        return w
    if name == "k30_prior":      # a marginalization prior: its kept keyframes are separators (dense)
        w = pkg.window.make_window(30, 600, 120, imu=True, seed=0xC5E3)
        o = orc.new_problem(); o.upload_window(w); pkg.protocol.local_ba(o); pr = o.marginalize(0, 50); o.close()
        w = pkg.window.make_window(30, 600, 120, imu=True, seed=0xC5E3); w["prior"] = pr
        return w
    raise KeyError(name)


CHAIN = ["k12", "k23", "k19_fixed_dropped", "k30_prior"]
# (window, segment length) pairs whose plan falls back to the dense path (a segment's column window over 192): none at these sizes
DENSE_FALLBACK = set()


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("seg", range(1, 9))
@pytest.mark.parametrize("name", CHAIN)
def test_forced_chain_segments(pkg, orc, hip, name, seg, fused):
    key = ("chain", name)
    if key not in _WIN:
        _WIN[key] = _chain_window(pkg, orc, name)
    w = _WIN[key]
    g = pkg.new_problem(lm_fused=fused, chain_seg=seg); g.upload_window(w)
    _check_system(g, _oracle_system(orc, key, w))
    chained = g.debug_get("dense_dim")[0] < g.debug_get("pose_dim")[0]
    assert chained == ((name, seg) not in DENSE_FALLBACK), (name, seg, g.debug_get("dense_dim")[0], g.debug_get("pose_dim")[0])
    assert g.debug_get("lm_fused")[0] == (1 if fused else 0)
    g.close()
    g = pkg.new_problem(lm_fused=fused, chain_seg=seg); g.upload_window(w)
    _check_protocol(pkg, g, _oracle_protocol(pkg, orc, ("chain protocol", name), w))
    g.close()


# ---- 4. over 256 keyframes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,revisit", [(257, 0.0), (300, 0.2)])
def test_windows_past_256_keyframes(pkg, orc, hip, K, revisit):
    """past 256 keyframes the group cut keeps a stamp array instead of keyframe bit masks, and the table fill searches each group's window
    instead of a keyframe -> slot table.  The built system against the oracle (no solve: a dense solve of 3800+ dimensions takes the oracle
    seconds), and at K = 257 two LM iterations on the fused and the record-based passes against the oracle."""
    w = pkg.window.make_window(K, 12 * K, 2 * K, imu=True, seed=0x257 + K, revisit=revisit)
    assert w["meta"]["K"] == K > 256
    g = pkg.new_problem(lm_fused=2); g.upload_window(w)
    _check_system(g, _oracle_system(orc, ("past256", K), w, solve=False), solve=False)
    assert g.debug_get("lm_fused")[0] == 1
    g.close()
    if K != 257:
        return
    res = {}
    for key, mk in (("fused", lambda: pkg.new_problem(lm_fused=2)), ("record", lambda: pkg.new_problem(lm_fused=0)), ("oracle", orc.new_problem)):
        q = mk(); q.upload_window(w)
        st = q.optimize(2)
        res[key] = (st, [t["accepted"] for t in q.trace()], q.get_keyframes(), q.get_points())
        if key != "oracle":
            assert q.debug_get("lm_fused")[0] == (1 if key == "fused" else 0)
        q.close()
    so, ao, ko, po = res["oracle"]
    for key in ("fused", "record"):
        s, a, k, p = res[key]
        assert (s.iterations, s.trials, s.solver_failures) == (so.iterations, so.trials, so.solver_failures) and a == ao
        assert s.chi2_final == pytest.approx(so.chi2_final, rel=1e-9)
        assert _pose_delta(k, ko, pkg) < 1e-9 and np.abs(p - po).max() < 1e-8
