"""The rule that holds the state plba_optimize leaves behind — after the retraction, the publish, the accept and the restore of every LM
trial — to the quad-precision run of the oracle (numpy only; tests/build_exact.py holds the system and the step x the same way).

Why.  The comparisons of the state in use (test_gpu_parity, test_lm_fused, test_large_configs, test_facade) are absolute: 1e-8 on P, V,
phi and on max(|d dbg|, |d dba|), 1e-8 x max|array| on landmarks.  The whole gyro-bias step of an iteration is about 1e-7: a gyro-bias
update that is wrong by 10 % passes them, and the trial's chi2 does not see it either.  Here the error of a state is the error of the
step that was applied, in the norm build_exact uses for x.

State distance (the subscript q marks the quad run; d = sqrt(diag Hschur), dl = sqrt(diag Hll) of the quad build at the uploaded state
and the sequence's lambda, which the build_exact fixture of the window holds):
  a keyframe with a free PVR vertex    delta = (Rq^T (P - Pq), V - Vq, Log(qq^-1 q)), the order of the step (kf_oplus_pvr: P += R u,
                                       V += u, q = q Exp(u)); q and -q are the same rotation
  a free bias vertex                   (dbg - dbgq, dba - dbaq)
  a free landmark                      the difference of its 3 / 6 stored parameters (the oracle's update of a line is additive in them)
  state_pose = max_i d_i |delta_i| / max_i d_i |D_i|,  D the quad run's displacement from the uploaded state in the same coordinates;
  state_pt, state_ln the same with dl over the free landmarks;  chi2_final relative;  over the trials of the trace the largest relative
  error of lam, chi2_current and chi2_trial.
The scales are indexed by the reference's pose layout (offsets(): ascending vertex ids, the bias block first where vid_bias < vid_pvr, a
keyframe that the levels leave without an edge absent); the state is read per keyframe, so the device's own layout does not enter.

Noise and tolerance are build_exact's: noise(q) = the largest distance from the quad run over the fp64 oracle as it is and on the three
reorderings of the window (build_exact.reorder, REORDER_SEEDS; landmark arrays permuted back); tol(q) = max(32 x noise(q), m u) with
FACTOR_SOLVE = 32 and the floors of build_exact.floor — the state is a function of x, the trace's chi2 a function of the state.

Exact conditions (bytes, no tolerance): every entry of a keyframe's P, V, q without a free PVR vertex (fixed, or left without an edge
by the levels) and of dbg, dba without a free bias vertex, of a fixed landmark and of a landmark without a level-0 observation equals the
upload;  | |q| - 1 | <= 4 u for every keyframe;  where every trial of the call is rejected the whole state equals the upload.
(get_keyframes returns nothing that the step does not write: bg and ba are not read back.)

Decisions: (iteration, trial, accepted, solver_ok) of every trial are compared.  A sequence is kept only where it is decided: the four
fp64 runs take the quad run's decisions and every rho of the quad run is MARGIN x its noise (floored at m u |rho|) away from 0
(build_exact's condition (iv), per trial).  A sequence that is not is shortened to the iterations that are, or dropped
(tests/step_exact_cases.py); nothing undecided is compared.

What misses a condition.  A sequence of three iterations that misses (ii) or (iv) is shortened to two; if it still misses it is dropped
(step_exact_cases.SHORTENED, DROPPED).  A sequence of one iteration keeps what it can, as build_exact_cases.TRIAL_DROPPED does: where only
the landmarks' tolerance in absolute units, or only chi2_trial, is over its cap, that quantity alone is not compared
(step_exact_cases.QUANT_DROPPED) and the keyframes, the decisions, the other trace values and the exact conditions are; where state_pose or
a keyframe kind misses, the sequence is dropped.  No cap is widened for any of this.

Conditions on a sequence, asserted by tests/test_step_exact_cpu.py on the references alone:
  (i)   the fixture equals what the generator computes now;
  (ii)  32 x noise(q) <= CAP_SOLVE = 1e-9 for every quantity, and the tolerance of the state turned back into absolute units — the
        budget tol x max d |D| over the smallest scale of the kind — is at most CAP_ABS = 1e-9 for each of P, V, phi, dbg, dba, points
        and lines that moves: ten times below every bar in use;
  (iii) the fp64 oracle passes hold();
  (iv)  the sequence is decided;
  (v)   what is dropped hides nothing: every case keeps n = 1 at lambda = 5, at least half of the cases keep two or more iterations,
        one kept sequence has IMU edges and lines, one contains a rejected trial."""
import numpy as np

from . import build_exact as BX
from . import step_exact_cases as SC

U, FACTOR_SOLVE, MARGIN, CAP_SOLVE = BX.U, BX.FACTOR_SOLVE, BX.MARGIN, BX.CAP_SOLVE
CAP_ABS = 1e-9
Q_NORM = 4 * U
KF = ("P", "V", "q", "dbg", "dba")
STATE = KF + ("points", "lines")
COLS = ("iteration", "trial", "accepted", "solver_ok", "lam", "chi2_current", "chi2_trial", "rho")
TRACE = {"lam": 4, "chi2_current": 5, "chi2_trial": 6}
QUANT = ("state_pose", "state_pt", "state_ln", "chi2_final", "lam", "chi2_current", "chi2_trial")
KINDS = ("P", "V", "phi", "dbg", "dba", "points", "lines")


# ---- rotations (quaternions x, y, z, w) ------------------------------------------------------------------------------------------------
def _qmul(a, b):
    av, bv = a[:3], b[:3]
    return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - av @ bv]])


def _qinv(a):
    return np.array([-a[0], -a[1], -a[2], a[3]])


def _rot(q):
    x, y, z, s = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                     [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                     [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]])


def _log(q):
    v, s = (-q[:3], -q[3]) if q[3] < 0 else (q[:3], q[3])
    n = float(np.linalg.norm(v))
    return v * (2.0 * np.arctan2(n, s) / n) if n > 0 else np.zeros(3)


# ---- the window's layout and state -------------------------------------------------------------------------------------------------------
def offsets(w):
    """(offset of the PVR block, offset of the bias block) per keyframe in the reference's pose layout, -1 for a vertex that is fixed,
    absent or left without an edge, and the pose dimension (oracle/plba_oracle.c build_index; build_exact.pose_map follows the same walk)"""
    kf = w["kf"]
    K = len(kf["vid_pvr"])
    gp, gl = BX.levels(w)
    act_pvr, act_bias = np.zeros(K, bool), np.zeros(K, bool)
    act_pvr[w["po_kf"][~gp]] = True; act_pvr[w["lo_kf"][~gl]] = True
    if w.get("imu") is not None:
        for k in ("kf_i", "kf_j"):
            act_pvr[w["imu"][k]] = True; act_bias[w["imu"][k]] = True
    if w.get("prior") is not None:
        vid = set(int(v) for v in w["prior"]["vid"])
        act_pvr |= np.array([int(v) in vid for v in kf["vid_pvr"]]); act_bias |= np.array([int(v) in vid for v in kf["vid_bias"]])
    op, ob, off = np.full(K, -1, np.int64), np.full(K, -1, np.int64), 0
    for k in range(K):
        pv = bool(act_pvr[k] and not kf["fixed_pvr"][k])
        bv = bool(kf["vid_bias"][k] >= 0 and act_bias[k] and not kf["fixed_bias"][k])
        if pv and bv and kf["vid_bias"][k] < kf["vid_pvr"][k]:
            ob[k] = off; off += 6; op[k] = off; off += 9
        else:
            if pv:
                op[k] = off; off += 9
            if bv:
                ob[k] = off; off += 6
    return op, ob, off


def upload(w):
    """the state as uploaded"""
    out = {k: np.array(w["kf"][k], np.float64) for k in KF}
    out["points"], out["lines"] = np.array(w["points"], np.float64).reshape(-1, 3), np.array(w["lines"], np.float64).reshape(-1, 6)
    return out


def read(p, st):
    """state, trace and final chi2 of a problem after optimize() returned `st`"""
    r = dict(p.get_keyframes())
    r["points"], r["lines"] = p.get_points(), p.get_lines()
    r["trace"] = np.array([[float(t[c]) for c in COLS] for t in p.trace()], np.float64).reshape(-1, len(COLS))
    r["chi2_final"] = float(st.chi2_final)
    return r


def run(mk, w, lam, n, opts):
    p = mk(user_lambda_init=lam, **opts); p.upload_window(w); BX.apply(p, w)
    r = read(p, p.optimize(n)); p.close()
    return r


def decisions(trace):
    return np.asarray(trace)[:, :4].astype(np.int64)


def displacement(a, b, offs):
    """state a seen from state b in the coordinates of the step: (vector over the reference's pose dimensions, points, lines)"""
    op, ob, P = offs
    v = np.zeros(P)
    for k in range(len(op)):
        if op[k] >= 0:
            o = op[k]
            v[o:o + 3] = _rot(b["q"][k]).T @ (a["P"][k] - b["P"][k])
            v[o + 3:o + 6] = a["V"][k] - b["V"][k]
            v[o + 6:o + 9] = _log(_qmul(_qinv(b["q"][k]), a["q"][k]))
        if ob[k] >= 0:
            o = ob[k]
            v[o:o + 3] = a["dbg"][k] - b["dbg"][k]; v[o + 3:o + 6] = a["dba"][k] - b["dba"][k]
    return v, a["points"] - b["points"], a["lines"] - b["lines"]


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def scales(q, up, ref, offs):
    """{quantity: max d |D|} of the quad run's displacement from the upload; a quantity that does not move at all is left out"""
    Dv, Dp, Dl = displacement(up, q, offs)
    lay = ref.lay
    out = {"state_pose": float((ref.d * np.abs(Dv)).max(initial=0.0))}
    for nm, key, D in (("pt", "state_pt", Dp), ("ln", "state_ln", Dl)):
        out[key] = float((ref.dl[nm] * np.abs(D))[lay["free_" + nm]].max(initial=0.0))
    return {k: v for k, v in out.items() if v > 0}


def errors(res, q, up, ref, w):
    """{quantity: distance of the run `res` from the quad run `q` in the norms above}.  The traces must have the same length."""
    offs = offsets(w)
    assert offs[2] == ref.P, ("pose dimension", offs[2], ref.P)
    for k in STATE:
        assert np.asarray(res[k]).shape == q[k].shape, (k, np.asarray(res[k]).shape, q[k].shape)
    assert res["trace"].shape == q["trace"].shape, ("trials", len(res["trace"]), len(q["trace"]))
    sc = scales(q, up, ref, offs)
    dv, dp, dl = displacement(res, q, offs)
    lay, out = ref.lay, {}
    if "state_pose" in sc:
        out["state_pose"] = float((ref.d * np.abs(dv)).max()) / sc["state_pose"]
    for nm, key, dd in (("pt", "state_pt", dp), ("ln", "state_ln", dl)):
        if key in sc:
            out[key] = float((ref.dl[nm] * np.abs(dd))[lay["free_" + nm]].max()) / sc[key]
    out["chi2_final"] = _rel(res["chi2_final"], q["chi2_final"])
    for key, c in TRACE.items():
        out[key] = max(_rel(a, b) for a, b in zip(res["trace"][:, c], q["trace"][:, c]))
    return out


def floor(qn, lay):
    return (lay["m"] if qn.startswith("state_") else lay["m_chi"]) * U


def tolerances(noise, lay):
    return {qn: max(FACTOR_SOLVE * n, floor(qn, lay)) for qn, n in noise.items()}


def absolute(tol, q, up, ref, w):
    """{kind: the state's tolerance in the kind's own units}: tol x max d |D| over the smallest scale among the kind's free dimensions.
    A kind of which nothing moves in the quad run (V of a window without IMU edges) has no figure."""
    offs = offsets(w)
    op, ob, _ = offs
    sc = scales(q, up, ref, offs)
    Dv, Dp, Dl = displacement(up, q, offs)
    out = {}
    if "state_pose" in sc and "state_pose" in tol:
        budget = tol["state_pose"] * sc["state_pose"]
        for kind, base, o in (("P", op, 0), ("V", op, 3), ("phi", op, 6), ("dbg", ob, 0), ("dba", ob, 3)):
            idx = np.concatenate([np.arange(b + o, b + o + 3) for b in base if b >= 0] or [np.zeros(0, np.int64)]).astype(np.int64)
            if len(idx) and np.abs(Dv[idx]).max() > 0:
                out[kind] = budget / float(ref.d[idx].min())
    for nm, key, kind in (("pt", "state_pt", "points"), ("ln", "state_ln", "lines")):
        if key in sc and key in tol:
            out[kind] = tol[key] * sc[key] / float(ref.dl[nm][ref.lay["free_" + nm]].min())
    return out


KIND_OF = {"P": "state_pose", "V": "state_pose", "phi": "state_pose", "dbg": "state_pose", "dba": "state_pose", "points": "state_pt", "lines": "state_ln"}


def misses(noise, q, up, ref, w):
    """condition (ii) on one sequence: ({what is over its cap: figure}, the quantities those belong to, the absolute figures per kind)"""
    over = {qn: n for qn, n in noise.items() if FACTOR_SOLVE * n > CAP_SOLVE}
    ab = absolute(tolerances(noise, ref.lay), q, up, ref, w)
    quantities = set(over) | {KIND_OF[k] for k, v in ab.items() if v > CAP_ABS}
    over.update({k: v for k, v in ab.items() if v > CAP_ABS})
    return over, quantities, ab


# ---- the exact conditions ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def exact(res, up, w, lay):
    """the conditions that hold to the bit; returns the list of those that do not"""
    op, ob, _ = offsets(w)
    bad = []
    for k in range(len(op)):
        for keys, off in ((("P", "V", "q"), op[k]), (("dbg", "dba"), ob[k])):
            if off < 0:
                bad += ["keyframe %d %s: moved without a free vertex" % (k, key) for key in keys if not _same(res[key][k], up[key][k])]
        n = float(np.sqrt((np.asarray(res["q"][k], np.longdouble) ** 2).sum()))
        if not abs(n - 1.0) <= Q_NORM:
            bad.append("keyframe %d: |q| - 1 = %.3e" % (k, n - 1.0))
    for key, free in (("points", lay["free_pt"]), ("lines", lay["free_ln"])):
        bad += ["%s %d: moved though it is fixed or has no level-0 observation" % (key, i) for i in np.flatnonzero(~free) if not _same(res[key][i], up[key][i])]
    if not res["trace"][:, 2].any():
        bad += ["%s: not the upload after a call all of whose trials were rejected" % key for key in STATE if not _same(res[key], up[key])]
    return bad


def hold(res, seq, ref, w, who, name, dropped=()):
    """a run (read()) against a sequence of the fixture (load()) under the rule; `dropped`: the quantities the sequence does not compare
    (step_exact_cases.QUANT_DROPPED).  Prints quantity, error, noise, tolerance and error / noise before it asserts; returns
    {quantity: (error, noise, tolerance)}."""
    up, q, noise = upload(w), seq["q"], seq["noise"]
    bad = exact(res, up, w, ref.lay)
    same = res["trace"].shape == q["trace"].shape and np.array_equal(decisions(res["trace"]), decisions(q["trace"]))
    if not same:
        bad.append(("decisions", decisions(res["trace"]).tolist(), decisions(q["trace"]).tolist(), "rho", res["trace"][:, 7].tolist(), q["trace"][:, 7].tolist()))
        assert not bad, (who, name, bad)
    err = errors(res, q, up, ref, w)
    assert set(err) - set(dropped) == set(noise), (sorted(err), sorted(noise), sorted(dropped))
    tol, fig = tolerances(noise, ref.lay), {}
    for qn in [qn for qn in QUANT if qn in noise]:
        e, n, t = err[qn], noise[qn], tol[qn]
        print("%s %s %-12s error %.3e  noise %.3e  tolerance %.3e  error/noise %s" % (who, name, qn, e, n, t, "%.2f" % (e / n) if n > 0 else ("inf" if e > 0 else "0")))
        fig[qn] = (e, n, t)
        if not e <= t:
            bad.append((qn, e, t))
    assert not bad, (who, name, bad)
    return fig


# ---- the references on the CPU (generator and CPU test only) --------------------------------------------------------------------------------
def references(orc, w, lam, n, opts, ref):
    """(quad run, fp64 run, noise {quantity: figure} — empty where a fp64 run takes other decisions —, decided, smallest |rho| / its noise)"""
    lay, up = ref.lay, upload(w)
    q = run(orc.new_quad_problem, w, lam, n, opts)
    runs = [run(orc.new_problem, w, lam, n, opts)]
    for s in BX.REORDER_SEEDS:
        w2, inv, _ = BX.reorder(w, s)
        r = run(orc.new_problem, w2, lam, n, opts)
        r["points"], r["lines"] = r["points"][inv[0]], r["lines"][inv[1]]
        runs.append(r)
    dq = decisions(q["trace"])
    agree = all(r["trace"].shape == q["trace"].shape and np.array_equal(decisions(r["trace"]), dq) for r in runs)
    noise, margin = {}, 0.0
    if agree:
        for r in runs:
            for qn, e in errors(r, q, up, ref, w).items():
                noise[qn] = max(noise.get(qn, 0.0), e)
        rho_q = q["trace"][:, 7]
        rho_noise = np.maximum(np.max([np.abs(r["trace"][:, 7] - rho_q) for r in runs], axis=0), lay["m_chi"] * U * np.abs(rho_q))
        margin = float((np.abs(rho_q) / rho_noise).min())
    decided = bool(agree and margin >= MARGIN and q["trace"][:, 3].all())
    return q, runs[0], noise, decided, margin


def generate(name, W, orc, fxb):
    """everything the fixture of case `name` holds, as a flat {key: array} (W: the package's window module; fxb: the loaded build_exact
    fixture of the case, which carries the window's prior or state and the scales)"""
    from . import build_exact_cases as BC
    w = BC.CASES[name]["make"](W, BX.prior_of(fxb))
    assert BC.window_sha(w) == str(fxb["sha"]), name
    out = {"sha": np.array(BC.window_sha(w))}
    seqs = SC.sequences(name)
    out["keys"] = np.array([k for k, _, _, _ in seqs])
    for j, (key, label, n, opts) in enumerate(seqs):
        i = SC.lambda_index(name, label)
        lam = float(fxb["lams"][i])
        q, r64, noise, decided, margin = references(orc, w, lam, n, opts, BX.load(fxb, w, i)[0])
        noise = {qn: v for qn, v in noise.items() if qn not in SC.QUANT_DROPPED.get((name, key), ())}
        for k in STATE:
            out["%d/%s" % (j, k)] = q[k]
        out["%d/trace_q" % j], out["%d/trace_64" % j] = q["trace"], r64["trace"]
        out["%d/chi2_final" % j] = np.array(q["chi2_final"])
        out["%d/lam" % j], out["%d/n" % j] = np.array(lam), np.array(n)
        out["%d/decided" % j], out["%d/margin" % j] = np.array(decided), np.array(margin)
        out["%d/noise_names" % j] = np.array(sorted(noise), dtype="U12")
        out["%d/noise" % j] = np.array([noise[qn] for qn in sorted(noise)], np.float64)
    return out


def load(fx, j):
    """sequence number j of a loaded fixture: dict(q: the quad run, trace_64, noise, decided, lam, n)"""
    g = lambda k: fx["%d/%s" % (j, k)]
    q = {k: g(k) for k in STATE}
    q["trace"], q["chi2_final"] = g("trace_q"), float(g("chi2_final"))
    noise = dict(zip([str(s) for s in g("noise_names")], [float(v) for v in g("noise")]))
    return dict(q=q, trace_64=g("trace_64"), noise=noise, decided=bool(g("decided")), margin=float(g("margin")), lam=float(g("lam")), n=int(g("n")))
