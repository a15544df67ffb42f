"""The windows of the marginalization exactness tests (tests/marg_quad.py is the rule, tests/golden/make_marg_quad.py writes the
fixtures, tests/test_marg_quad_cpu.py holds the references to their conditions, tests/test_marg_quad.py holds the device).

Every window is marginalized at the uploaded state — no optimisation in between — so the device and the reference see identical inputs;
the generator's initial estimates are already off the optimum.  Each is the smallest shape that reaches its code:
  far1 .. far1e6, k12full   the five windows of tests/golden/marg_cases.py (eigenvalues of Amm through the 1e-8 threshold; n = 105)
  full11, full15, full16    tracks over the whole window: n = 96, 132, 141 — with k12full's 105 one on each side of JLDS_MAX_N = 100, of
                            128 and of JLDS_MAX_N2 = 140 (csrc/plba_marg.hip: marg_kept_block); kf_dt as tests/test_gpu_parity.py
  full6                     the same at K = 6 (n = 51): the window whose prior chain_n105 carries
  chain_drop                the next window of far1's trajectory (keyframe ids 1 .. 6) with far1's prior: the prior holds the dropped
                            keyframe's two vertices
  chain_lone                the same with tracks of two keyframes: the prior holds vertices no other selected factor touches
  chain_n105                k12full with full6's prior: n > 100 with an old prior among the factors
                            (the chained windows come from other draws of the generator's noise than the window their prior was made
                            from, so the prior's error at the state is not 0)
  points_only, lines_only   one landmark kind alone
  m15                       no landmark first seen in keyframe 0: the dropped block is the keyframe's 15 dims
  noimu                     no IMU edges (the oracle accepts it: no bias vertices, the dropped keyframe block has 9 dims)
  cap3                      max_edges = 3: the cut of `num > NUM` falls inside a landmark's run of observations, points and lines
  once                      a point and a line seen once only: rank-deficient landmark blocks
  eps1e3                    far1 with marg_eps = 1e3

A case is dict(make(window_module, prior) -> window, prior_of: the case whose reference prior the window carries or None, max_edges,
marg_eps)."""
import numpy as np

from .build_exact_cases import window_sha      # noqa: F401  (SHA-256 of everything upload_window reads)


def _far(W, far):      # tests/golden/marg_cases.py::case_window, on the window module
    w = W.make_window(6, 120, 20, imu=True, seed=31, outlier_frac=0.0)
    P0 = w["kf"]["P"][0]
    sp = sorted(set(w["po_pt"][w["po_kf"] == 0].tolist())); sl = sorted(set(w["lo_ln"][w["lo_kf"] == 0].tolist()))
    w["points"][sp] = P0 + far * (w["points"][sp] - P0)
    w["lines"][sl] = np.tile(P0, 2) + far * (w["lines"][sl] - np.tile(P0, 2))
    return w


def _full(W, K, dt):
    return W.make_window(K, 300, 60, imu=True, seed=77, kf_dt=dt, track=(K, K))


def select_obs(w, sel_pt, sel_ln):
    """w with the point / line observations of the boolean masks only; landmarks left without one go, the rest are renumbered in order"""
    out = dict(w)
    for pts, ob_lm, ob_kf, rest, sel in (("points", "po_pt", "po_kf", ("po_uv", "po_w"), sel_pt), ("lines", "lo_ln", "lo_kf", ("lo_l", "lo_w"), sel_ln)):
        sel = np.asarray(sel, bool)
        keep = np.flatnonzero(np.bincount(w[ob_lm][sel], minlength=len(w[pts])) > 0)
        new = np.full(len(w[pts]), -1, np.int64); new[keep] = np.arange(len(keep))
        out[pts] = w[pts][keep]
        out[ob_lm] = new[w[ob_lm][sel]].astype(np.int32); out[ob_kf] = w[ob_kf][sel]
        for k in rest: out[k] = w[k][sel]
    out["meta"] = dict(w["meta"], Np=len(out["points"]), Nl=len(out["lines"]), Ep=len(out["po_pt"]), El=len(out["lo_ln"]))
    return out


def first_kf_of(ob_lm, ob_kf, n):
    """keyframe of each landmark's first listed observation (-1: none)"""
    first = np.full(n, -1, np.int64)
    for e in range(len(ob_lm) - 1, -1, -1):
        first[ob_lm[e]] = ob_kf[e]
    return first


def _m15(W, prior):
    w = W.make_window(6, 120, 20, imu=True, seed=43, outlier_frac=0.0)
    fp = first_kf_of(w["po_pt"], w["po_kf"], len(w["points"])); fl = first_kf_of(w["lo_ln"], w["lo_kf"], len(w["lines"]))
    return select_obs(w, fp[w["po_pt"]] != 0, fl[w["lo_ln"]] != 0)


def _once(W, prior):
    w = W.make_window(6, 120, 20, imu=True, seed=46, outlier_frac=0.0)
    sel = []
    for ob_lm, ob_kf, n in ((w["po_pt"], w["po_kf"], len(w["points"])), (w["lo_ln"], w["lo_kf"], len(w["lines"]))):
        first = first_kf_of(ob_lm, ob_kf, n)
        l = int(np.flatnonzero(first == 0)[0])      # the first landmark the marginalization selects: only its first observation stays
        s = np.ones(len(ob_lm), bool); e = np.flatnonzero(ob_lm == l); s[e[1:]] = False
        sel.append(s)
    return select_obs(w, sel[0], sel[1])


def _chain(make):
    def f(W, prior):
        w = make(W); w["prior"] = prior
        return w
    return f


def _case(make, prior_of=None, max_edges=50, marg_eps=None):
    return dict(make=make, prior_of=prior_of, max_edges=max_edges, marg_eps=marg_eps)


CASES = {
    "far1": _case(lambda W, pr: _far(W, 1.0)),
    "far1e2": _case(lambda W, pr: _far(W, 1e2)),
    "far1e3": _case(lambda W, pr: _far(W, 1e3)),
    "far1e6": _case(lambda W, pr: _far(W, 1e6)),
    "k12full": _case(lambda W, pr: _full(W, 12, 0.1)),
    "full6": _case(lambda W, pr: _full(W, 6, 0.1)),
    "full11": _case(lambda W, pr: _full(W, 11, 0.1)),
    "full15": _case(lambda W, pr: _full(W, 15, 0.08)),
    "full16": _case(lambda W, pr: _full(W, 16, 0.075)),
    "chain_drop": _case(_chain(lambda W: W.make_window(6, 120, 20, imu=True, seed=31, outlier_frac=0.0, t0=W.KF_DT, kf_id0=1)), prior_of="far1"),
    "chain_lone": _case(_chain(lambda W: W.make_window(6, 120, 20, imu=True, seed=33, outlier_frac=0.0, t0=W.KF_DT, kf_id0=1, track=(2, 2))), prior_of="far1"),
    "chain_n105": _case(_chain(lambda W: _full(W, 12, 0.1)), prior_of="full6"),
    "points_only": _case(lambda W, pr: W.make_window(6, 120, 0, imu=True, seed=41, outlier_frac=0.0)),
    "lines_only": _case(lambda W, pr: W.make_window(6, 0, 40, imu=True, seed=42, outlier_frac=0.0)),
    "m15": _case(_m15),
    "noimu": _case(lambda W, pr: W.make_window(6, 120, 20, imu=False, seed=44, outlier_frac=0.0)),
    "cap3": _case(lambda W, pr: W.make_window(6, 120, 20, imu=True, seed=46, outlier_frac=0.0), max_edges=3),
    "once": _case(_once),
    "eps1e3": _case(lambda W, pr: _far(W, 1.0), marg_eps=1e3),
}
N_EXPECT = {"full6": 51, "full11": 96, "k12full": 105, "full15": 132, "full16": 141, "chain_n105": 105}
FAR = ("far1e2", "far1e3", "far1e6")      # eigenvalues of Amm around the threshold: the device's certificate sends these down the dense path
# ... and eps1e3: a threshold of 1e3 discards directions that are no block-local null spaces, so the block-wise form is wrong there
# (tests/test_marg_quad_cpu.py: it misses the rule by 8.9e10) and the dense path is the right one
DENSE = FAR + ("eps1e3",)
