"""The rule that holds the built reduced-camera system of plba_optimize to the quad-precision build of the oracle (numpy only).

Why.  The 1e-9 comparisons of the built system (test_gpu_parity, test_lm_fused, test_lm_balanced, test_group_tiling, test_call_setup)
take max|a - b| / max|b| over a whole array.  On an IMU window the largest entry of Hschur is a bias-information term of 2e10 .. 5e10
while everything the landmark kernels produce is 1e3 .. 1e6: that bar accepts a pose-pose block that is wrong in its fourth to second
digit (DESIGN.md 9 has the table).  Here every quantity is compared in a diagonal-scaled norm, like solver_ref's E_D, against the
oracle built in __float128 (oracle/make_quad.py), with a tolerance taken from the fp64 oracle's own distance to that build.

Norms (d = sqrt(diag Hschur) and dl = sqrt(diag Hll) per landmark, both of the quad run; every figure is dimensionless):
  Hschur        max |dH_ij| / (d_i d_j) over the structural nonzeros of the quad run's lower triangle (the matrix is symmetric; the rule
                compares both triangles of a result entry by entry); an entry outside that pattern must be exactly 0
  bschur, bp    max(|db_i| / d_i) / max(|b_i| / d_i)
  hll_pt/ln     max |dHll_ab| / (dl_a dl_b) over the free landmarks (a fixed landmark has no block)
  bl_pt/ln      as bp, with dl
  x_pose        max(d_i |dx_i|) / max(d_i |x_i|)
  x_lm          the same with each landmark's dl
  err_*         per edge kind, max |de| / max |e|
  chi2, maxdiag, chi2_trial   relative

Noise.  noise(q) = the largest of those distances over four fp64 CPU evaluations: the oracle as it is, and the oracle on three
reorderings of the window (landmarks relabelled at random, each landmark's observations shuffled; the lists stay landmark-major, as
set_point_obs demands; outputs permuted back): other summation orders of the same sums.

Tolerance.  tol(q) = max(FACTOR x noise(q), m u):  FACTOR = lba_ref.FACTOR = 8, the project's figure for another summation order of
the same sums; 32 for x and chi2_trial, the figure test_solver_accuracy.py takes from the largest ratio seen between two correct fp64
solvers (the device factors a chain-eliminated system, the oracle a dense one);  m = max(64, observations of the busiest keyframe),
lba_ref.tolerances' count of the longest diagonal sum, and the observation count for chi2 and chi2_trial.  No other constants.

Levels.  A window may carry po_level / lo_level (uint8 per observation) and robust ({kind: (enabled, delta)}); apply() sets them after
every upload_window, on the build problem and on the trial problem.  Only level-0 observations are rows of the system: they alone count
towards m, make a landmark free and have their residuals compared (the reference never evaluates a gated edge); a product of gated
observations only must come out as an exact 0 (it is outside the quad pattern).  Where the levels leave a keyframe without any edge the
reference drops it from the pose layout and the device does not: pose_map() relates the two, and on the dimensions the reference lacks
the device must hold exact zeros beside a finite diagonal.

Conditions on a case, asserted by tests/test_build_exact_cpu.py on the references alone:
  (i)   the fixture equals what the quad build computes now;
  (ii)  FACTOR x noise(q) <= 1e-10 for every quantity of the built system and <= 1e-9 for x and for chi2_trial, which is a function of
        x (today's bars: 1e-9 max-norm on the system, 1e-7 on x, 1e-9 on a chi2) — every new bar is at least ten times tighter than
        the one in use, on every window;
  (iii) the fp64 oracle itself passes hold();
  (iv)  `accepted` of the first trial agrees between the quad and the fp64 run and rho is lba_ref.MARGIN x its noise away from the
        acceptance threshold rho > 0; where not, only chi2_trial is compared."""
import numpy as np

from . import build_exact_cases as BC
from . import lba_ref as LR

U = LR.U
FACTOR, FACTOR_SOLVE, MARGIN = LR.FACTOR, 32, LR.MARGIN
CAP, CAP_SOLVE = 1e-10, 1e-9
RAW = ("chi2", "maxdiag", "err_pt", "err_ln", "err_pvr", "err_bias", "err_prior", "hll_pt", "bl_pt", "hll_ln", "bl_ln", "bp", "bschur", "Hschur", "x")
QUANT = ("chi2", "maxdiag", "err_pt", "err_ln", "err_pvr", "err_bias", "err_prior", "hll_pt", "bl_pt", "hll_ln", "bl_ln", "bp", "bschur", "Hschur",
         "x_pose", "x_lm")
SOLVED = ("x_pose", "x_lm", "chi2_trial")
TRIAL = ("chi2_trial", "accepted", "lam", "rho")


def factor(q):
    return FACTOR_SOLVE if q in SOLVED else FACTOR


def cap(q):
    return CAP_SOLVE if q in SOLVED else CAP


# ---- the window's layout --------------------------------------------------------------------------------------------------------------------
def levels(w):
    """(point, line) observation levels of a window as bool arrays (True: level 1, gated); a window without the keys has every edge at 0"""
    out = []
    for key, n in (("po_level", len(w["po_pt"])), ("lo_level", len(w["lo_ln"]))):
        out.append(np.zeros(n, bool) if w.get(key) is None else np.asarray(w[key]).astype(bool))
        assert len(out[-1]) == n, key
    return out


def apply(p, w):
    """what a case carries besides the arrays upload_window reads — the observation levels and the robust switches — set on a problem
    right after upload_window(w); a replaced state is in the window's own arrays already"""
    if w.get("po_level") is not None:
        p.set_levels(0, np.asarray(w["po_level"], np.uint8))
    if w.get("lo_level") is not None:
        p.set_levels(1, np.asarray(w["lo_level"], np.uint8))
    for kind, (enabled, delta) in sorted((w.get("robust") or {}).items()):
        p.set_robust(int(kind), bool(enabled), float(delta))


def layout(w):
    """what the norms need of a window: the free landmarks (not fixed, at least one level-0 observation) — x carries 3 / 6 entries for
    each, in order —, the level-0 observations (act_pt, act_ln: a gated observation is no row of the system and its residual is not
    compared) and the two observation counts m of the floors, which count level-0 observations only"""
    Np, Nl = len(w["points"]), len(w["lines"])
    fp = np.zeros(Np, bool) if w.get("point_fixed") is None else np.asarray(w["point_fixed"]).astype(bool)
    fl = np.zeros(Nl, bool) if w.get("line_fixed") is None else np.asarray(w["line_fixed"]).astype(bool)
    gp, gl = levels(w)
    free_pt = ~fp & (np.bincount(w["po_pt"][~gp], minlength=Np) > 0)
    free_ln = ~fl & (np.bincount(w["lo_ln"][~gl], minlength=Nl) > 0)
    K = len(w["kf"]["vid_pvr"])
    per_kf = np.bincount(np.concatenate([w["po_kf"][~gp], w["lo_kf"][~gl]]).astype(np.int64), minlength=K)
    n_obs = int((~gp).sum() + (~gl).sum())
    return dict(Np=Np, Nl=Nl, free_pt=free_pt, free_ln=free_ln, act_pt=~gp, act_ln=~gl, n_obs=n_obs, m=max(64, int(per_kf.max(initial=0))), m_chi=max(64, n_obs))


def pose_map(w):
    """the pose layout of the device against the reference's, for a window whose levels leave a keyframe without any edge: the device
    indexes every non-fixed keyframe whatever the levels (include/plba.h), the reference drops a keyframe that has no level-0
    observation, no IMU edge and no prior entry (initializeOptimization(0)).  Returns None where the two layouts are the same, else an
    int array over the device's pose dimensions: the reference's dimension, or -1 for a dimension the reference does not have."""
    kf = w["kf"]
    K = len(kf["vid_pvr"])
    gp, gl = levels(w)
    act_pvr, act_bias = np.zeros(K, bool), np.zeros(K, bool)
    act_pvr[w["po_kf"][~gp]] = True; act_pvr[w["lo_kf"][~gl]] = True
    if w.get("imu") is not None:
        for k in ("kf_i", "kf_j"):
            act_pvr[w["imu"][k]] = True; act_bias[w["imu"][k]] = True
    if w.get("prior") is not None:
        vid = set(int(v) for v in w["prior"]["vid"])
        act_pvr |= np.array([int(v) in vid for v in kf["vid_pvr"]]); act_bias |= np.array([int(v) in vid for v in kf["vid_bias"]])
    out, ref = [], 0
    for k in range(K):
        pv, bv = not kf["fixed_pvr"][k], kf["vid_bias"][k] >= 0 and not kf["fixed_bias"][k]
        parts = [(pv, act_pvr[k], 9), (bv, act_bias[k], 6)]
        if pv and bv and kf["vid_bias"][k] < kf["vid_pvr"][k]:
            parts.reverse()
        for on, act, n in parts:
            if on and act:
                out += list(range(ref, ref + n)); ref += n
            elif on:
                out += [-1] * n
    out = np.array(out, np.int64)
    return None if (out >= 0).all() else out


def floor(q, lay):
    return (lay["m_chi"] if q in ("chi2", "chi2_trial") else lay["m"]) * U


# ---- reading a problem ----------------------------------------------------------------------------------------------------------------------
def read(p):
    """the built system of a problem after debug_build(lambda, True): the raw arrays of RAW and P"""
    r = {k: p.debug_get(k).copy() for k in RAW}
    r["P"] = int(p.debug_get("pose_dim")[0])
    return r


AT_THE_STATE = ("err_pvr", "err_bias", "err_prior")


def read_device(p, lam):
    """the same of a device problem.  The residuals of the IMU and prior edges are read after debug_build(lam, False): with a solve, the
    fused passes' trial launch has re-evaluated those edges at the trial state (the launch forms the two trial states of an IMU edge
    itself) and debug_get returns the trial's residuals, where the oracle and the record-based passes return the current state's."""
    p.debug_build(lam, False)
    at = {k: p.debug_get(k).copy() for k in AT_THE_STATE}
    p.debug_build(lam, True)
    r = read(p)
    r.update(at)
    return r


def first_trial(p):
    """the first trace row after optimize(1)"""
    t = p.trace()[0]
    return np.array([t["chi2_trial"], float(t["accepted"]), t["lam"], t["rho"]])


# ---- the reference of one (case, lambda) ----------------------------------------------------------------------------------------------------
class Ref:
    """the quad run: raw arrays, Hschur as the structural nonzeros (rows, cols, vals) of its lower triangle, and the scales d, dl"""
    def __init__(self, raw, lay):
        self.lay, self.P = lay, int(raw["P"])
        self.a = {k: np.asarray(raw[k], np.float64) for k in RAW if k != "Hschur"}
        if "Hschur" in raw:
            H = np.asarray(raw["Hschur"], np.float64).reshape(self.P, self.P)
            assert np.array_equal(H, H.T), "the reference's Hschur is not symmetric entry by entry"
            self.rows, self.cols = np.nonzero(np.tril(H))
            self.vals = H[self.rows, self.cols]
        else:
            self.rows, self.cols, self.vals = (np.asarray(raw[k]) for k in ("H_rows", "H_cols", "H_vals"))
        self.rows, self.cols = self.rows.astype(np.int64), self.cols.astype(np.int64)
        diag = np.zeros(self.P); on = self.rows == self.cols
        diag[self.rows[on]] = self.vals[on]
        assert (diag > 0).all(), "a pose dimension without a diagonal entry"
        self.d = np.sqrt(diag)
        self.dl = {}
        for nm, n in (("pt", 3), ("ln", 6)):
            Hl = self.a["hll_" + nm].reshape(-1, n, n)
            free = lay["free_" + nm]
            dg = np.einsum("kii->ki", Hl)
            assert (dg[free] > 0).all() and len(Hl) == len(free), nm
            self.dl[nm] = np.sqrt(np.where(free[:, None], dg, 1.0))
        self.dl_x = np.concatenate([self.dl["pt"][lay["free_pt"]].ravel(), self.dl["ln"][lay["free_ln"]].ravel()])
        assert len(self.a["x"]) == self.P + len(self.dl_x), (len(self.a["x"]), self.P, len(self.dl_x))

    def dense(self):
        H = np.zeros((self.P, self.P))
        H[self.rows, self.cols] = self.vals; H[self.cols, self.rows] = self.vals
        return H

    def stored(self):
        """what a fixture keeps"""
        out = dict(self.a)
        it = np.int16 if self.P < 2 ** 15 else np.int32
        out.update(H_rows=self.rows.astype(it), H_cols=self.cols.astype(it), H_vals=self.vals, P=np.int64(self.P))
        return out


def _relmax(da, a):
    return float(np.abs(da).max() / np.abs(a).max()) if a.size and np.abs(a).max() > 0 else (0.0 if not da.size or not np.abs(da).max() else np.inf)


def _without_dropped(res, pmap, n_free):
    """`res` in the reference's pose layout (pmap: pose_map()).  On the dimensions the reference does not have the result must hold
    nothing but a finite diagonal: every off-diagonal entry of Hschur, and bp, bschur and x there, exactly 0."""
    Pd = int(res["P"])
    assert len(pmap) == Pd, ("pose_dim", Pd, len(pmap))
    keep, drop = np.flatnonzero(pmap >= 0), np.flatnonzero(pmap < 0)
    assert np.array_equal(pmap[keep], np.arange(len(keep)))
    H = np.asarray(res["Hschur"], np.float64).reshape(Pd, Pd)
    off = H.copy(); off[drop, drop] = 0.0
    assert not off[drop].any() and not off[:, drop].any(), "Hschur: an off-diagonal entry in a dimension without any edge"
    assert np.isfinite(H[drop, drop]).all(), "Hschur: the diagonal of a dimension without any edge is not finite"
    x = np.asarray(res["x"])
    assert len(x) == Pd + n_free, ("x", len(x), Pd, n_free)
    for k, v in (("bp", res["bp"]), ("bschur", res["bschur"]), ("x", x[:Pd])):
        assert not np.asarray(v)[drop].any(), "%s: not exactly 0 in a dimension without any edge" % k
    out = dict(res)
    out["P"] = len(keep)
    out["Hschur"] = H[np.ix_(keep, keep)].ravel()
    out["bp"], out["bschur"] = np.asarray(res["bp"])[keep], np.asarray(res["bschur"])[keep]
    out["x"] = np.concatenate([x[:Pd][keep], x[Pd:]])
    return out


def errors(res, ref, pmap=None):
    """{quantity: distance of `res` (raw arrays of read()) from the reference in the norms above}; quantities the window does not have
    (no lines, no IMU, no prior, no level-0 edge of a kind) are left out.  Raises AssertionError where a shape differs or Hschur has an
    entry outside the pattern.  pmap: the device's pose layout where it differs from the reference's (pose_map())."""
    a, lay, P = ref.a, ref.lay, ref.P
    if pmap is not None:
        res = _without_dropped(res, pmap, len(ref.dl_x))
    assert int(res["P"]) == P, ("pose_dim", res["P"], P)
    out = {}
    for k in RAW:
        if k != "Hschur":
            assert np.asarray(res[k]).shape == a[k].shape, (k, np.asarray(res[k]).shape, a[k].shape)
    for k in ("chi2", "maxdiag"):
        out[k] = abs(float(res[k][0]) - float(a[k][0])) / abs(float(a[k][0]))
    for k, n, act in (("err_pt", 2, lay["act_pt"]), ("err_ln", 3, lay["act_ln"])):      # the rows of the level-0 observations
        if act.any():
            out[k] = _relmax((res[k] - a[k]).reshape(-1, n)[act], a[k].reshape(-1, n)[act])
    for k in ("err_pvr", "err_bias", "err_prior"):
        if a[k].size:
            out[k] = _relmax(res[k] - a[k], a[k])
    for nm, n in (("pt", 3), ("ln", 6)):
        free, dl = lay["free_" + nm], ref.dl[nm]
        if not free.any():
            continue
        dH = np.abs(res["hll_" + nm].reshape(-1, n, n) - a["hll_" + nm].reshape(-1, n, n)) / (dl[:, :, None] * dl[:, None, :])
        out["hll_" + nm] = float(dH[free].max())
        b = a["bl_" + nm].reshape(-1, n)
        out["bl_" + nm] = float((np.abs(res["bl_" + nm].reshape(-1, n) - b) / dl)[free].max() / (np.abs(b) / dl)[free].max())
    d = ref.d
    for k in ("bp", "bschur"):
        out[k] = float((np.abs(res[k] - a[k]) / d).max() / (np.abs(a[k]) / d).max())
    H = np.asarray(res["Hschur"], np.float64).reshape(P, P)
    inside = np.zeros((P, P), bool); inside[ref.rows, ref.cols] = True; inside[ref.cols, ref.rows] = True
    stray = np.flatnonzero((H != 0) & ~inside)
    assert not len(stray), ("Hschur: %d entries outside the reference's pattern, the first at (%d, %d) = %r" % (len(stray), stray[0] // P, stray[0] % P, H.flat[stray[0]]))
    sc = d[ref.rows] * d[ref.cols]
    out["Hschur"] = float(max((np.abs(H[ref.rows, ref.cols] - ref.vals) / sc).max(), (np.abs(H[ref.cols, ref.rows] - ref.vals) / sc).max()))
    x, xr = np.asarray(res["x"]), a["x"]
    out["x_pose"] = float((d * np.abs(x[:P] - xr[:P])).max() / (d * np.abs(xr[:P])).max())
    if len(ref.dl_x):
        out["x_lm"] = float((ref.dl_x * np.abs(x[P:] - xr[P:])).max() / (ref.dl_x * np.abs(xr[P:])).max())
    return out


def trial_error(row, row_q):
    return abs(float(row[0]) - float(row_q[0])) / abs(float(row_q[0]))


def tolerances(noise, lay):
    """{quantity: max(FACTOR x noise, m u)} for the quantities of `noise`"""
    return {q: max(factor(q) * n, floor(q, lay)) for q, n in noise.items()}


def hold(res, ref, noise, who, name, trial=None, pmap=None):
    """every quantity of `res` against the reference under the rule; `trial` = (row, quad row, compare `accepted` too); pmap: pose_map()
    for a device result.  Prints quantity, error, noise, tolerance and error / noise before it asserts; returns
    {quantity: (error, noise, tolerance)}."""
    err = errors(res, ref, pmap)
    assert set(err) == set(noise) - {"chi2_trial"}, (sorted(err), sorted(noise))
    if trial is not None and "chi2_trial" in noise:      # (no figure: the trial of this case and lambda is not compared, build_exact_cases.TRIAL_DROPPED)
        row, row_q, decided = trial
        err["chi2_trial"] = trial_error(row, row_q)
        assert float(row[2]) == float(row_q[2]), ("the first trial's lambda", row[2], row_q[2])
        if decided:
            assert bool(row[1]) == bool(row_q[1]), ("accepted", row[1], row_q[1], "rho", row[3], row_q[3])
    tol = tolerances(noise, ref.lay)
    bad, fig = [], {}
    for q in [q for q in QUANT + ("chi2_trial",) if q in err]:
        e, n, t = err[q], noise[q], tol[q]
        print("%s %s %-10s error %.3e  noise %.3e  tolerance %.3e  error/noise %s" % (who, name, q, e, n, t, "%.2f" % (e / n) if n > 0 else ("inf" if e > 0 else "0")))
        fig[q] = (e, n, t)
        if not e <= t:
            bad.append((q, e, t))
    assert not bad, (who, name, bad)
    return fig


# ---- the references on the CPU: evaluation, reorderings, noise (generator and CPU test only) -----------------------------------------------
def evaluate(mk, w, lam):
    """(raw arrays after debug_build(lam, True), first trace row of optimize(1) with user_lambda_init = lam) of the implementation `mk`"""
    p = mk(); p.upload_window(w); apply(p, w); p.debug_build(lam, True)
    raw = read(p); p.close()
    p = mk(user_lambda_init=lam); p.upload_window(w); apply(p, w); p.optimize(1)
    row = first_trial(p); p.close()
    return raw, row


def reorder(w, seed):
    """the window with its landmarks relabelled at random and each landmark's observations shuffled (lists landmark-major), and what
    undoes it: (window, landmark permutations (points, lines), observation orders (points, lines))"""
    rng = np.random.default_rng(seed)
    w2, inv, orders = dict(w), [], []
    for lm, idx, keys, fx in (("points", "po_pt", ("po_pt", "po_kf", "po_uv", "po_w", "po_level"), "point_fixed"),
                              ("lines", "lo_ln", ("lo_ln", "lo_kf", "lo_l", "lo_w", "lo_level"), "line_fixed")):
        n = len(w[lm]); perm = rng.permutation(n); iv = np.empty(n, np.int64); iv[perm] = np.arange(n)      # new landmark j is old perm[j]
        w2[lm] = w[lm][perm]
        if w.get(fx) is not None:
            w2[fx] = np.asarray(w[fx])[perm]
        new_idx = iv[w[idx]] if len(w[idx]) else np.zeros(0, np.int64)
        order = np.lexsort((rng.random(len(new_idx)), new_idx))                                            # new observation e is old order[e]
        for k in keys:
            if w.get(k) is not None:      # (the levels are there only where a case sets them)
                w2[k] = (new_idx.astype(w[idx].dtype) if k == idx else np.asarray(w[k]))[order]
        inv.append(iv); orders.append(order)
    return w2, inv, orders


def undo(raw, lay, inv, orders):
    """the raw arrays of a run on reorder()'s window, in the original numbering"""
    r = dict(raw)
    (ip, il), (op, ol) = inv, orders
    Np, Nl, P = lay["Np"], lay["Nl"], raw["P"]
    for k, n, iv in (("hll_pt", 9, ip), ("bl_pt", 3, ip), ("hll_ln", 36, il), ("bl_ln", 6, il)):
        r[k] = raw[k].reshape(-1, n)[iv].ravel()
    for k, n, od in (("err_pt", 2, op), ("err_ln", 3, ol)):
        e = np.empty_like(raw[k].reshape(-1, n)); e[od] = raw[k].reshape(-1, n)
        r[k] = e.ravel()
    x = raw["x"]
    parts, o = [x[:P]], P
    for free, iv, n in ((lay["free_pt"], ip, 3), (lay["free_ln"], il, 6)):
        new_free = np.empty(len(free), bool); new_free[iv] = free          # free flags in the new numbering
        slot = np.cumsum(new_free) - 1                                     # new landmark -> its position among the new free ones
        blocks = x[o:o + n * int(free.sum())].reshape(-1, n); o += blocks.size
        parts.append(blocks[slot[iv[free]]].ravel())
    assert o == len(x)
    r["x"] = np.concatenate(parts)
    return r


REORDER_SEEDS = (1, 2, 3)


def references(orc, w, lam):
    """(Ref of the quad run, quad trial row, fp64 trial row, noise {quantity: figure}, `accepted` may be compared, raw fp64 arrays)"""
    lay = layout(w)
    rq, tq = evaluate(orc.new_quad_problem, w, lam)
    ref = Ref(rq, lay)
    r64, t64 = evaluate(orc.new_problem, w, lam)
    noise = errors(r64, ref)
    noise["chi2_trial"] = trial_error(t64, tq)
    rho_noise = abs(t64[3] - tq[3])
    for s in REORDER_SEEDS:
        w2, inv, orders = reorder(w, s)
        r2, t2 = evaluate(orc.new_problem, w2, lam)
        e2 = errors(undo(r2, lay, inv, orders), ref)
        e2["chi2_trial"] = trial_error(t2, tq)
        rho_noise = max(rho_noise, abs(t2[3] - tq[3]))
        for q in noise:
            noise[q] = max(noise[q], e2[q])
    rho_noise = max(rho_noise, lay["m_chi"] * U * abs(tq[3]))
    decided = bool(t64[1] == tq[1]) and abs(tq[3]) >= MARGIN * rho_noise       # (iv): rho > 0 is the acceptance test
    return ref, tq, t64, noise, decided, r64


def generate(name, W, orc, prior=None):
    """everything the fixture of case `name` holds, as a flat {key: array} (W: the package's window module)"""
    case = BC.CASES[name]
    if name in BC.NEEDS_PRIOR and prior is None:      # the reference's marginalization of the window's own first BA (tests/test_group_tiling.py)
        from importlib import import_module
        protocol = import_module(W.__name__.rsplit(".", 1)[0] + ".protocol")
        o = orc.new_problem(); o.upload_window(case["make"](W, None)); protocol.local_ba(o); prior = _prior(o.marginalize(0, 50)); o.close()
    if name in BC.NEEDS_STATE and prior is None:
        prior = BC.stage1_state(orc, BC.CASES[BC.NEEDS_STATE[name]]["make"](W, None))
    w = case["make"](W, prior)
    out = {"sha": np.array(BC.window_sha(w))}
    if name in BC.NEEDS_PRIOR:
        for k in ("n", "vid", "size", "idx", "x0", "J0", "r0"):
            out["prior/" + k] = np.asarray(prior[k])
    if name in BC.NEEDS_STATE:
        for k in BC.STATE_KEYS:
            out["state/" + k] = np.asarray(prior[k])
    o = orc.new_quad_problem(); o.upload_window(w); apply(o, w); o.debug_build(5.0, False); maxdiag = float(o.debug_get("maxdiag")[0]); o.close()
    lams = BC.lambdas_of(name, maxdiag)
    out["lams"] = np.array([v for _, v in lams])
    for i, (label, lam) in enumerate(lams):
        ref, tq, t64, noise, decided, _ = references(orc, w, lam)
        if (name, label) in BC.TRIAL_DROPPED:
            del noise["chi2_trial"]
        for k, v in ref.stored().items():      # (what does not depend on lambda is kept once, with the first)
            if not (i and np.array_equal(out.get("0/" + k), v)):
                out["%d/%s" % (i, k)] = v
        out["%d/trial_q" % i], out["%d/trial_64" % i], out["%d/decided" % i] = tq, t64, np.array(decided)
        out["%d/noise_names" % i] = np.array(sorted(noise))
        out["%d/noise" % i] = np.array([noise[q] for q in sorted(noise)])
    return out


def load(fx, w, i):
    """(Ref, quad trial row, fp64 trial row, noise, decided) of lambda number i from a loaded fixture"""
    raw = {k.split("/", 1)[1]: fx[k] for k in fx if k.startswith("0/")}      # (a key lambda number i lacks equals the first lambda's)
    raw.update({k.split("/", 1)[1]: fx[k] for k in fx if k.startswith("%d/" % i)})
    ref = Ref(raw, layout(w))
    noise = dict(zip([str(s) for s in raw["noise_names"]], [float(v) for v in raw["noise"]]))
    return ref, raw["trial_q"], raw["trial_64"], noise, bool(raw["decided"])


def _prior(pr):
    """what set_prior reads of a prior, in the types a fixture keeps"""
    out = {k: np.asarray(pr[k], np.int32) for k in ("vid", "size", "idx")}
    out.update({k: np.asarray(pr[k], np.float64) for k in ("x0", "J0", "r0")})
    out["n"] = int(pr["n"])
    return out


def prior_of(fx):
    """what a fixture carries for its case's make(): the prior of prior13, the state and levels of a stage2 case, None elsewhere"""
    if "state/P" in fx:
        return {k: fx["state/" + k] for k in BC.STATE_KEYS}
    return _prior({k: fx["prior/" + k] for k in ("n", "vid", "size", "idx", "x0", "J0", "r0")}) if "prior/n" in fx else None
