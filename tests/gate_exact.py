"""The rule that holds the gate, the cull and the per-edge chi2 — k_gate, k_cull, plba_get_edge_chi2 and the level handling behind them —
to the quad-precision oracle (numpy only).

Why.  plba_gate_outliers and plba_cull_observations decide per observation: chi2 > thresh || !isDepthPositive.  The suite compared those
decisions with the fp64 oracle bit for bit on windows where no depth is ever non-positive and no chi2 is near the threshold: deleting
`|| !dpos`, testing one end point of a line only, or gating at 5.99 passed everything.  Here the windows have landmarks behind a camera
and observations planted 1e-6 either side of the threshold, the reference is the oracle in __float128, and a decision is compared
exactly where the reference itself is sure of it.

The windows (tests/build_exact_cases.py makes them; `threshold` is made here):
  behind         three points, the first end of a line, the second of another and both of a third 0.3 m behind a camera, their
                 observations at the moved estimate
  stage2_mixed   state and levels of the quad oracle's own optimize(5) + gate_outliers(5.991): gated edges that the cull re-evaluates
  noimu7         no IMU edge, no prior: pose dimension 9 per keyframe, the IMU kinds empty
  threshold      `mixed` at the quad stage-1 state, every edge at level 0; six point and four line observations moved along their
                 residual until the quad chi2 is 5.991 x (1 +- 1e-6), half on each side

The sequence run() takes on one problem, and what it keeps of it:
  upload, apply, recompute_errors        chi2 and depth flag of every edge, all five kinds
  gate_outliers(5.991)                   both counts, the levels, chi2 of the point and line edges again (unchanged bit for bit: a gated
                                         observation keeps the value it was gated on), a second gate's counts (0, 0)
  debug_build(5, no solve)               chi2: the sum over the level-0 edges with the point and line kernels off
  cull_observations(5.991)               (a) flags, counts, chi2 of the point and line edges afterwards
and on a second problem, the refresh made visible:
  upload, apply, recompute_errors at the window's state A;  set_levels(the levels above);  set_keyframes / set_points / set_lines to a
  state B (the setters leave the levels alone);  cull_observations: (b) flags, counts, chi2 afterwards.  A level-1 edge is evaluated at B;
  a level-0 edge keeps what the last evaluation pass left, at A — the reference's edge->chi2() reads the cached error.
and on a third, the levels the gate itself left, with no set_levels in between:
  upload, apply, recompute_errors;  gate_outliers(5.991);  the setters to B;  get_levels;  cull_observations: (c) levels, flags, counts,
  chi2 afterwards.  (In the reference (c) gives what (b) gives; a device that rebuilds its image from levels older than the gate does not.)
The depth flags are kept at every reading — after the gate and cull (a) at state A, after culls (b) and (c) at state B.

Tolerance of a per-edge chi2, from what the err_* rows of tests/build_exact.py already pass: with delta = tol(err_kind) x max|e_kind|
(tol = max(FACTOR x noise, m u), the noise of the window kept in the fixture: measured at state A for the readings at A, and at state
B with every edge at level 0 for the readings after culls (b) and (c), the larger of the two, since those hold values of both states),
    |chi_e - chi_e^q| <= w_e (2 |e_e| delta + delta^2) + 4 u chi_e^q
|e_e| the 2-norm of the edge's residual, sqrt(chi_e^q / w_e) for a point or a line; for an IMU edge w_e is the largest eigenvalue of its
information matrix and |e_e| the 2-norm of its nine or six residuals; the prior's chi2 is a plain sum of squares, w_e = 1.

Decisions.  An edge's flag (level, bad) is compared only where |chi_e^q - thresh| >= MARGIN x that bound and every depth involved has
|z| >= 1e-6 |X - C| (z in numpy.longdouble from the window; its fp64 evaluation error is about 1e-15 |X - C|).  tests/test_gate_exact_cpu.py
asserts on the references alone that this excludes no edge of any case, that the fp64 oracle agrees with the quad oracle on every flag
and passes every bound, that `behind` has its edges bad by depth alone and that the planted edges fall on their sides."""
import numpy as np

from . import build_exact as BX
from . import build_exact_cases as BC

U, FACTOR, MARGIN = BX.U, BX.FACTOR, BX.MARGIN
THRESH = 5.991
REL = 1e-6             # the planted distance from the threshold, relative
DEPTH_MARGIN = 1e-6    # |z| / |X - C| below which a depth flag is not compared
CASES = ("behind", "stage2_mixed", "noimu7", "threshold")
KINDS = ("pt", "ln", "pvr", "bias", "prior")
ERR = ("err_pt", "err_ln", "err_pvr", "err_bias", "err_prior")
N_PLANT = (6, 4)


# ---- the decision ---------------------------------------------------------------------------------------------------------------------------
def decide(chi, dpos, thresh=THRESH):
    """chi2() > thresh || !isDepthPositive()"""
    return (np.asarray(chi) > thresh) | ~np.asarray(dpos).astype(bool)


# ---- the windows ----------------------------------------------------------------------------------------------------------------------------
def plant(orc, w):
    """what `threshold` carries: N_PLANT point and line observations of `w` (inliers of distinct landmarks, quad chi2 in 0.5 .. 4) moved
    along their residual so that the quad chi2 becomes THRESH x (1 +- REL), alternately above and below.  A point observation moves to
    projection + s e; a line observation is shifted in its offset c, which adds one t to the distances of both end points."""
    q = orc.new_quad_problem(); q.upload_window(w); q.recompute_errors()
    chi = [q.edge_chi2(0)[0], q.edge_chi2(1)[0]]
    err = [q.debug_get("err_pt").reshape(-1, 2), q.debug_get("err_ln").reshape(-1, 3)]
    q.close()
    out = {}
    for kind, (lm, key, n) in enumerate((("po_pt", "po_uv", N_PLANT[0]), ("lo_ln", "lo_l", N_PLANT[1]))):
        ok = (chi[kind] > 0.5) & (chi[kind] < 4.0) & ~w["truth"]["line_outlier" if kind else "point_outlier"]
        idx = []
        for e in np.flatnonzero(ok):
            if w[lm][e] not in [w[lm][f] for f in idx]:
                idx.append(int(e))
        idx = np.array(idx[:n]); assert len(idx) == n
        side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        meas = w[key][idx].copy()
        for j, e in enumerate(idx):
            target = np.longdouble(THRESH) * (1 + np.longdouble(side[j]) * np.longdouble(REL))
            if kind == 0:
                s = np.sqrt(target / np.longdouble(chi[0][e]))
                meas[j] = (meas[j].astype(np.longdouble) + err[0][e].astype(np.longdouble) * (s - 1)).astype(np.float64)
            else:
                e0, e1 = err[1][e, :2].astype(np.longdouble)
                t = (-(e0 + e1) + np.sqrt((e0 + e1) ** 2 - 2 * (e0 * e0 + e1 * e1 - target))) / 2
                meas[j, 2] = np.float64(np.longdouble(meas[j, 2]) + t)
        out.update({"plant/%s_idx" % KINDS[kind]: idx, "plant/%s_meas" % KINDS[kind]: meas, "plant/%s_side" % KINDS[kind]: side})
    return out


def window(name, W, carried):
    """the window of a case; carried: {"state/..": .., "plant/..": ..} of the fixture (stage2_mixed, threshold)"""
    if name != "threshold":
        return BC.CASES[name]["make"](W, {k[6:]: v for k, v in carried.items() if k.startswith("state/")} or None)
    w = BC.with_state(BC.CASES["mixed"]["make"](W, None), {k[6:]: v for k, v in carried.items() if k.startswith("state/")}, levels=False)
    if "plant/pt_idx" in carried:
        w["po_uv"], w["lo_l"] = w["po_uv"].copy(), w["lo_l"].copy()
        w["po_uv"][carried["plant/pt_idx"]] = carried["plant/pt_meas"]
        w["lo_l"][carried["plant/ln_idx"]] = carried["plant/ln_meas"]
    return w


def state_b(W, w):
    """the state B of sequence (b): the window's estimates moved by a few millimetres (a few pixels of every residual)"""
    rng = W.Rng(0xB57A7E)
    kf = {k: np.array(v, copy=True) for k, v in w["kf"].items()}
    K = len(kf["vid_pvr"])
    kf["P"][1:] += rng.normal((K - 1, 3), 2e-3)
    return kf, w["points"] + rng.normal(w["points"].shape, 5e-3), w["lines"] + rng.normal(w["lines"].shape, 5e-3)


def at_b(W, w):
    kf, pts, lns = state_b(W, w)
    w2 = dict(w); w2["kf"], w2["points"], w2["lines"] = kf, pts, lns
    return w2


def depth_ratio(w):
    """(points (Ep,), lines (El, 2)): z / |X - C| of every observed landmark point in its keyframe's camera, in numpy.longdouble"""
    ld = np.longdouble
    K = len(w["kf"]["vid_pvr"])
    Rbc, Pbc = np.asarray(w["cam"]["Rbc"]).astype(ld), np.asarray(w["cam"]["Pbc"]).astype(ld)
    cams = []
    for k in range(K):
        x, y, z, s = (w["kf"]["q"][k].astype(ld) / np.sqrt((w["kf"]["q"][k].astype(ld) ** 2).sum()))
        Rwb = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                        [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                        [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]], ld)
        cams.append(((Rbc.T @ Rwb.T)[2], w["kf"]["P"][k].astype(ld) + Rwb @ Pbc))      # the optical axis in the world, the camera centre

    def ratio(X, k):
        d = X.astype(ld) - cams[k][1]
        return (cams[k][0] @ d) / np.sqrt(d @ d)
    rp = np.array([ratio(w["points"][i], k) for i, k in zip(w["po_pt"], w["po_kf"])], ld).reshape(-1)
    rl = np.array([[ratio(w["lines"][i, o:o + 3], k) for o in (0, 3)] for i, k in zip(w["lo_ln"], w["lo_kf"])], ld).reshape(-1, 2)
    return rp, rl


def depth_sure(w):
    """(points, lines): the depth flag of the observation is compared"""
    rp, rl = depth_ratio(w)
    return np.abs(rp) >= DEPTH_MARGIN, (np.abs(rl) >= DEPTH_MARGIN).all(axis=1)


# ---- the sequence ---------------------------------------------------------------------------------------------------------------------------
def _emax(p):
    return np.array([np.abs(p.debug_get(k)).max(initial=0.0) for k in ERR[:2]])


def run(p, p2, p3, w, wb, levels=None, read_err=True):
    """the sequence of the module docstring on the problems p (gate, cull (a)), p2 (cull (b)) and p3 (cull (c)); levels: what p2 is given (None: p's own
    after the gate — the references; a device is given the fixture's).  read_err: also keep max|e| of the point and line residuals at each
    reading (the oracles' debug_get reads the cached residuals at any time; a device is not asked)."""
    o = {}
    p.upload_window(w); BX.apply(p, w); p.recompute_errors()
    for k, name in enumerate(KINDS):
        o["chi0_" + name], o["dpos0_" + name] = p.edge_chi2(k)
    if read_err:
        o["emax0"] = _emax(p)
        o["err_pvr"], o["err_bias"], o["err_prior"] = (p.debug_get(k).copy() for k in ERR[2:])
    o["gate"] = np.array(p.gate_outliers(THRESH))
    o["lev_pt"], o["lev_ln"] = p.get_levels(0), p.get_levels(1)
    (o["chi1_pt"], o["dpos1_pt"]), (o["chi1_ln"], o["dpos1_ln"]) = p.edge_chi2(0), p.edge_chi2(1)
    o["gate_again"] = np.array(p.gate_outliers(THRESH))
    p.debug_build(5.0, False)
    o["chi2_gated"] = p.debug_get("chi2").copy()
    c = p.cull_observations(THRESH)
    o["badA_pt"], o["badA_ln"], o["cullA"] = c["bad_points"], c["bad_lines"], np.array([c["n_points"], c["n_lines"]])
    (o["chiA_pt"], o["dposA_pt"]), (o["chiA_ln"], o["dposA_ln"]) = p.edge_chi2(0), p.edge_chi2(1)
    if read_err:
        o["emaxA"] = _emax(p)
    lv = (o["lev_pt"], o["lev_ln"]) if levels is None else levels
    p2.upload_window(w); BX.apply(p2, w); p2.recompute_errors()
    p2.set_levels(0, lv[0]); p2.set_levels(1, lv[1])
    k = wb["kf"]
    p2.set_keyframes(k["vid_pvr"], k["vid_bias"], k["P"], k["V"], k["q"], k["bg"], k["ba"], k["dbg"], k["dba"], k["fixed_pvr"], k["fixed_bias"])
    p2.set_points(wb["points"], w.get("point_fixed")); p2.set_lines(wb["lines"], w.get("line_fixed"))
    o["levB_pt"], o["levB_ln"] = p2.get_levels(0), p2.get_levels(1)      # (the setters leave the levels alone: include/plba.h)
    c = p2.cull_observations(THRESH)
    o["badB_pt"], o["badB_ln"], o["cullB"] = c["bad_points"], c["bad_lines"], np.array([c["n_points"], c["n_lines"]])
    (o["chiB_pt"], o["dposB_pt"]), (o["chiB_ln"], o["dposB_ln"]) = p2.edge_chi2(0), p2.edge_chi2(1)
    if read_err:
        o["emaxB"] = _emax(p2)
    p3.upload_window(w); BX.apply(p3, w); p3.recompute_errors()
    o["gateC"] = np.array(p3.gate_outliers(THRESH))
    p3.set_keyframes(k["vid_pvr"], k["vid_bias"], k["P"], k["V"], k["q"], k["bg"], k["ba"], k["dbg"], k["dba"], k["fixed_pvr"], k["fixed_bias"])
    p3.set_points(wb["points"], w.get("point_fixed")); p3.set_lines(wb["lines"], w.get("line_fixed"))
    o["levC_pt"], o["levC_ln"] = p3.get_levels(0), p3.get_levels(1)      # (the gate's own levels, through a rebuild of the device image)
    c = p3.cull_observations(THRESH)
    o["badC_pt"], o["badC_ln"], o["cullC"] = c["bad_points"], c["bad_lines"], np.array([c["n_points"], c["n_lines"]])
    (o["chiC_pt"], o["dposC_pt"]), (o["chiC_ln"], o["dposC_ln"]) = p3.edge_chi2(0), p3.edge_chi2(1)
    o["levC2_pt"], o["levC2_ln"] = p3.get_levels(0), p3.get_levels(1)    # (and as the device holds them after the rebuild)
    if read_err:
        o["emaxC"] = _emax(p3)
    return o


def run_on(mk, w, wb, **kw):
    p, p2, p3 = mk(), mk(), mk()
    try:
        return run(p, p2, p3, w, wb, **kw)
    finally:
        p.close(); p2.close(); p3.close()


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------
READINGS = (("chi0", "emax0", ""), ("chi1", "emax0", ""), ("chiA", "emaxA", ""), ("chiB", "emaxB", "B/"), ("chiC", "emaxC", "B/"))      # (reading, the residuals' size at it, its noise)


def err_tol(noise, lay):
    return BX.tolerances({k: noise[k] for k in ERR if k in noise}, lay)


def bounds(ref, w, noise):
    """{reading_kind: per-edge bound on |chi - chi^q|} of every per-edge chi2 the sequence reads, from the quad run `ref`"""
    lay = BX.layout(w)
    tol = {"": err_tol(noise, lay)}
    tol["B/"] = {k: max(v, err_tol({q[2:]: n for q, n in noise.items() if q.startswith("B/")}, lay).get(k, 0.0)) for k, v in tol[""].items()}
    wgt = (np.asarray(w["po_w"], np.float64), np.asarray(w["lo_w"], np.float64))
    out = {}
    for rd, em, nz in READINGS:
        for kind, name in enumerate(KINDS[:2]):
            cq = ref["%s_%s" % (rd, name)]
            if not len(cq):
                out["%s_%s" % (rd, name)] = np.zeros(0); continue
            delta = tol[nz][ERR[kind]] * ref[em][kind]
            out["%s_%s" % (rd, name)] = wgt[kind] * (2 * np.sqrt(cq / wgt[kind]) * delta + delta * delta) + 4 * U * cq
    if w.get("imu") is not None:
        for name, key, n in (("pvr", "info_pvr", 9), ("bias", "info_bias", 6)):
            e = ref["err_" + name].reshape(-1, n)
            lmax = np.array([np.linalg.eigvalsh(A.reshape(n, n)).max() for A in w["imu"][key]])
            delta = tol[""]["err_" + name] * np.abs(e).max()
            out["chi0_" + name] = lmax * (2 * np.sqrt((e * e).sum(axis=1)) * delta + delta * delta) + 4 * U * ref["chi0_" + name]
    else:
        out["chi0_pvr"], out["chi0_bias"] = np.zeros(0), np.zeros(0)
    out["chi0_prior"] = np.zeros(1)      # (no case has a prior: both sides return 0)
    return out


def sure(ref, w, wb, bnd):
    """{flags: bool per edge — the flag is compared}: the levels after the gate, the bad flags of culls (a), (b) and (c)"""
    da, db = depth_sure(w), depth_sure(wb)
    out = {}
    for kind, name in enumerate(KINDS[:2]):
        for flags, rd, dp in (("lev", "chi0", da), ("badA", "chiA", da), ("badB", "chiB", db), ("badC", "chiC", db)):
            k = "%s_%s" % (rd, name)
            out["%s_%s" % (flags, name)] = (np.abs(ref[k] - THRESH) >= MARGIN * bnd[k]) & dp[kind]
    return out


def hold(res, ref, w, wb, noise, who, name):
    """every reading and decision of `res` (run()) against the quad run `ref` under the rule.  Prints each figure before it asserts;
    returns {quantity: error / tolerance}."""
    bnd = bounds(ref, w, noise)
    ok = sure(ref, w, wb, bnd)
    bad, fig = [], {}

    def note(q, ratio, detail=""):
        fig[q] = ratio
        print("%s %s %-12s error / tolerance %.3e %s" % (who, name, q, ratio, detail))
        if not ratio <= 1.0:
            bad.append((q, ratio, detail))
    for k, b in bnd.items():
        a, r = np.asarray(res[k], np.float64), ref[k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        d = np.abs(a - r)
        ratio = float(np.where(d > 0, d / np.where(b > 0, b, 1e-300), 0.0).max(initial=0.0))
        note(k, ratio)
    for k in ["dpos%s_%s" % (r, nm) for r in "01ABC" for nm in ("pt", "ln")]:
        dp = depth_sure(wb if k[4] in "BC" else w)[0 if k.endswith("pt") else 1]
        n = int((np.asarray(res[k]).astype(bool) != ref[k].astype(bool))[dp].sum())
        note(k, float(n), "(%d flags differ, %d compared of %d)" % (n, dp.sum(), len(dp)))
    for k in ("dpos0_pvr", "dpos0_bias", "dpos0_prior"):
        note(k, float((np.asarray(res[k]) != 1).sum()))
    for k, m in ok.items():
        n = int((np.asarray(res[k]).astype(bool) != ref[k].astype(bool))[m].sum())
        note(k, float(n), "(%d decisions differ, %d compared of %d)" % (n, m.sum(), len(m)))
    # counts: what the compared decisions fix of them; where every edge is compared (the references assert it) they are the counts themselves
    for cnt, fl in (("gate", "lev"), ("gateC", "lev"), ("cullA", "badA"), ("cullB", "badB"), ("cullC", "badC")):
        every = ok[fl + "_pt"].all() and ok[fl + "_ln"].all()
        want = np.asarray(ref[cnt]) if every else None
        if cnt in ("gate", "gateC") and every:      # newly gated: level 1 now, level 0 in the window
            gp, gl = BX.levels(w)
            want = np.array([(ref["lev_pt"].astype(bool) & ~gp).sum(), (ref["lev_ln"].astype(bool) & ~gl).sum()])
            assert np.array_equal(want, ref[cnt]), "the reference's own counts"
        if want is not None:
            note(cnt, float(np.abs(np.asarray(res[cnt]) - want).sum()), "(%s against %s)" % (list(res[cnt]), list(want)))
    note("gate_again", float(np.abs(np.asarray(res["gate_again"])).sum()), "(%s)" % list(res["gate_again"]))
    for kname in ("pt", "ln"):      # a gated observation keeps the value it was gated on: the second reading is the first, bit for bit
        same = np.array_equal(np.asarray(res["chi1_" + kname]), np.asarray(res["chi0_" + kname]))
        note("kept_" + kname, 0.0 if same else np.inf)
        note("levB_" + kname, float((np.asarray(res["levB_" + kname]) != ref["lev_" + kname]).sum()), "(levels after set_levels and the setters)")
        m = ok["lev_" + kname]      # the gate's own levels after the setters: where the gate's decision is compared, what the host reads and what the device holds
        for k in ("levC_", "levC2_"):
            note(k + kname, float((np.asarray(res[k + kname]) != ref["lev_" + kname])[m].sum()), "(levels after the gate and the setters, %d compared)" % m.sum())
    c, cq = float(res["chi2_gated"][0]), float(ref["chi2_gated"][0])
    lay = BX.layout(dict(w, po_level=ref["lev_pt"], lo_level=ref["lev_ln"]))
    tol = max(FACTOR * noise["chi2_gated"], BX.floor("chi2", lay))
    note("chi2_gated", abs(c - cq) / abs(cq) / tol, "(relative error %.3e, noise %.3e, tolerance %.3e)" % (abs(c - cq) / abs(cq), noise["chi2_gated"], tol))
    assert not bad, (who, name, bad)
    return fig


# ---- the references (generator and CPU test only) ---------------------------------------------------------------------------------------------
def generate(name, W, orc, carried=None):
    """everything the fixture of case `name` holds, as a flat {key: array}"""
    if carried is None:
        carried = {}
        if name in ("stage2_mixed", "threshold"):
            st = BC.stage1_state(orc, BC.CASES["mixed"]["make"](W, None))
            carried.update({"state/" + k: np.asarray(st[k]) for k in BC.STATE_KEYS})
        if name == "threshold":
            carried.update(plant(orc, window(name, W, carried)))
    w = window(name, W, carried)
    wb = at_b(W, w)
    out = dict(carried)
    out["sha"] = np.array(BC.window_sha(w)); out["sha_b"] = np.array(BC.window_sha(wb))
    ref = run_on(orc.new_quad_problem, w, wb)
    out.update({"q/" + k: v for k, v in ref.items()})
    # the noise of the residuals: the rule of tests/build_exact.py at this window (the fp64 oracle and three reorderings against quad)
    _, _, _, nz, _, _ = BX.references(orc, w, 5.0)
    noise = {k: nz[k] for k in ERR if k in nz}
    wb0 = {k: v for k, v in wb.items() if k not in ("po_level", "lo_level")}      # at B a cull evaluates the gated edges: every row counts
    _, _, _, nzb, _, _ = BX.references(orc, wb0, 5.0)
    noise.update({"B/" + k: nzb[k] for k in ERR[:2] if k in nzb})
    # and of the gated chi2: the fp64 oracle's sequence on the window and on the same three reorderings
    r64 = run_on(orc.new_problem, w, wb)
    cq = float(ref["chi2_gated"][0])
    noise["chi2_gated"] = abs(float(r64["chi2_gated"][0]) - cq) / abs(cq)
    for s in BX.REORDER_SEEDS:
        w2, _, _ = BX.reorder(w, s)
        p = orc.new_problem(); p.upload_window(w2); BX.apply(p, w2); p.recompute_errors(); p.gate_outliers(THRESH); p.debug_build(5.0, False)
        noise["chi2_gated"] = max(noise["chi2_gated"], abs(float(p.debug_get("chi2")[0]) - cq) / abs(cq))
        p.close()
    out["noise_names"] = np.array(sorted(noise)); out["noise"] = np.array([noise[k] for k in sorted(noise)])
    return out


def load(fx):
    """(carried, quad run, noise) of a loaded fixture"""
    carried = {k: fx[k] for k in fx if k.startswith(("state/", "plant/"))}
    ref = {k[2:]: fx[k] for k in fx if k.startswith("q/")}
    noise = dict(zip([str(s) for s in fx["noise_names"]], [float(v) for v in fx["noise"]]))
    return carried, ref, noise
