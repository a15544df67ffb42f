"""Reference of the structure-only landmark refinement, plba_refine_landmarks (numpy only).

A restatement of the semantics DESIGN.md 9b specifies, with its own text of the two edge formulas (IMU/g2otypes.h:243-260 and
g2otypes.cpp:286-341 for the point edge, g2otypes.h:783-825 and g2otypes.cpp:1306-1359 for the line edge: Pc = Rcb Rwb^T (Pw - Pwb) -
Rcb Pbc, e = obs - proj(Pc) for a point, e_k = l . (proj(Pc_k), 1) for the two end points of a line), not taken from csrc/plba_math.h
nor from oracle/plba_oracle.c.  g2o's StructureOnlySolver::calc is the model of the loop; its text is not available, so the loop below
IS the specification.

Every function takes a working type `dt`: np.float64, np.longdouble, or "mp" (object arrays of mpmath numbers, for machines whose long
double is a double, as tests/lba_ref.py does).  Per landmark the run records every decision — the gain ratio rho of a solved trial, the
smallest pivot of its LDL^T — so that compare() can tell which landmarks' counts are decided far enough from rounding noise.
"""
import numpy as np

from . import lba_ref as LR

cast, f64, wide, _prec, _sqrt, _mv, _mm, _tr = LR.cast, LR.f64, LR.wide, LR._prec, LR._sqrt, LR._mv, LR._mm, LR._tr
DONE, EXHAUSTED, NONFINITE, FIXED, UNSELECTED, NO_OBS = range(6)
U = 2.0 ** -53


def _finite(v):
    return bool(np.isfinite(float(v)))


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=x.dtype if hasattr(x, "dtype") and x.dtype != object else object)


class Rig:
    """Camera and fixed keyframes of a window in the working type: M_k = Rcb Rwb_k^T, Pwb_k, c0 = Rcb Pbc."""

    def __init__(self, w, dt, kf=None):
        c = w["cam"]
        self.dt = dt
        self.fx, self.fy, self.cx, self.cy = (cast(np.array([c[k]]), dt)[0] for k in ("fx", "fy", "cx", "cy"))
        Rcb = _tr(cast(np.asarray(c["Rbc"], np.float64).reshape(3, 3), dt))
        self.c0 = _mv(Rcb, cast(np.asarray(c["Pbc"], np.float64), dt))
        kf = w["kf"] if kf is None else kf
        P, q = cast(np.asarray(kf["P"], np.float64), dt), cast(np.asarray(kf["q"], np.float64), dt)
        self.Pwb = P
        self.M = [_mm(Rcb, _tr(_rot(q[k]).astype(P.dtype))) for k in range(len(P))]

    def project(self, k, Pw):
        """(u, v), d(u, v)/dPw (2 x 3)"""
        Pc = _mv(self.M[k], Pw - self.Pwb[k]) - self.c0
        iz = 1 / Pc[2]
        uv = np.array([self.fx * Pc[0] * iz + self.cx, self.fy * Pc[1] * iz + self.cy], dtype=Pc.dtype)
        z = Pc[0] * 0
        Jpi = np.array([[self.fx * iz, z, -self.fx * Pc[0] * iz * iz], [z, self.fy * iz, -self.fy * Pc[1] * iz * iz]], dtype=Pc.dtype)
        return uv, _mm(Jpi, self.M[k])

    def point_edge(self, k, Pw, obs):
        """e (2), de/dPw (2 x 3): e = obs - proj"""
        uv, J = self.project(k, Pw)
        return obs - uv, -J

    def line_edge(self, k, L6, l3):
        """e (2), de0/dsP (3), de1/deP (3): e_k = l . (proj(P_k), 1)"""
        us, Js = self.project(k, L6[0:3])
        ue, Je = self.project(k, L6[3:6])
        e = np.array([l3[0] * us[0] + l3[1] * us[1] + l3[2], l3[0] * ue[0] + l3[1] * ue[1] + l3[2]], dtype=us.dtype)
        return e, l3[0] * Js[0] + l3[1] * Js[1], l3[0] * Je[0] + l3[1] * Je[1]


def huber(s, delta):
    """rho(s), rho'(s) of g2o's RobustKernelHuber on the squared error s"""
    if s <= delta * delta:
        return s, s * 0 + 1
    r = _sqrt(np.array([s], dtype=object if not hasattr(s, "dtype") else s.dtype))[0]
    return 2 * r * delta - delta * delta, delta / r


def _ldl_solve(H, b, mu):
    """(H + mu I) x = b by LDL^T without pivoting: x, smallest pivot (x = None when a pivot is not positive)"""
    a = H[0, 0] + mu
    if not a > 0:
        return None, a
    l10, l20 = H[1, 0] / a, H[2, 0] / a
    d1 = H[1, 1] + mu - l10 * H[1, 0]
    if not d1 > 0:
        return None, min(a, d1)
    l21 = (H[2, 1] - l20 * H[1, 0]) / d1
    d2 = H[2, 2] + mu - l20 * H[2, 0] - l21 * l21 * d1
    piv = min(a, d1, d2)
    if not d2 > 0:
        return None, piv
    y0 = b[0]; y1 = b[1] - l10 * y0; y2 = b[2] - l20 * y0 - l21 * y1
    x2 = y2 / d2; x1 = y1 / d1 - l21 * x2; x0 = y0 / a - l10 * x1 - l20 * x2
    return np.array([x0, x1, x2], dtype=b.dtype), piv


def _linearize(rig, is_pt, x, obs, delta, jac=True):
    """chi2, H (blocks of 3 x 3), b (blocks of 3) over the landmark's active observations: obs = [(k, measurement, inv_sigma2)]"""
    nb = 1 if is_pt else 2
    zero = x[0] * 0
    chi = zero
    H = [np.full((3, 3), zero, dtype=x.dtype) for _ in range(nb)]
    b = [np.full(3, zero, dtype=x.dtype) for _ in range(nb)]
    for k, m, w0 in obs:
        if is_pt:
            e, J = rig.point_edge(k, x[0:3], m)
            rows = [(0, J[0], e[0]), (0, J[1], e[1])]
        else:
            e, Js, Je = rig.line_edge(k, x, m)
            rows = [(0, Js, e[0]), (1, Je, e[1])]
        s = w0 * (e[0] * e[0] + e[1] * e[1])
        r0, r1 = (s, zero + 1) if delta is None else huber(s, delta)
        chi = chi + r0
        if jac:
            wgt = r1 * w0
            for blk, j, ee in rows:
                H[blk] = H[blk] + wgt * j[:, None] * j[None, :]
                b[blk] = b[blk] - wgt * j * ee
    return chi, H, b


def refine_one(rig, is_pt, x0, obs, delta, max_iters, max_trials, lambda_init, perturb=None):
    """The LM of one landmark.  Returns dict(x, status, iters, trials, chi2_before, chi2_after, rho=[...], piv=[...], path="ar..."),
    path: a = accepted trial, r = rejected by rho / chi2', p = rejected for a pivot."""
    dt = rig.dt
    x = x0.copy()
    chi, H, b = _linearize(rig, is_pt, x, obs, delta)
    out = dict(x=x, status=DONE, iters=0, trials=0, chi2_before=chi, chi2_after=chi, rho=[], piv=[], path="", chis=[chi])
    if not _finite(chi):
        out["status"] = NONFINITE
        return out
    mu = cast(np.array([lambda_init]), dt)[0]
    nu = mu * 0 + 2
    third = (mu * 0 + 1) / 3
    for _ in range(max_iters):
        accepted = False
        for _ in range(max_trials):
            out["trials"] += 1
            sol = [_ldl_solve(H[i], b[i], mu) for i in range(len(H))]
            out["piv"].append(min(s[1] for s in sol))
            if all(s[0] is not None for s in sol):
                d = np.concatenate([s[0] for s in sol])
                bb = np.concatenate(b)
                xt = x.copy()
                xt[:len(d)] = x[:len(d)] + d
                chit, Ht, bt = _linearize(rig, is_pt, xt, obs, delta)
                den = (d * (mu * d + bb)).sum()
                rho = (chi - chit) / den if den != 0 else (chi - chit) * float("inf") if chi != chit else den * float("nan")
                out["rho"].append(rho)
                if _finite(rho) and rho > 0 and _finite(chit):
                    accepted = True
                    x, chi, H, b = xt, chit, Ht, bt
                    g = 2 * rho - 1
                    mu = mu * max(third, 1 - g * g * g)
                    nu = mu * 0 + 2
                    out["path"] += "a"
                    out["chis"].append(chi)
                    break
                out["path"] += "r"
            else:
                out["path"] += "p"
            mu = mu * nu
            nu = nu * 2
        if accepted:
            out["iters"] += 1
        else:
            out["status"] = EXHAUSTED
            break
    out["x"], out["chi2_after"] = x, chi
    return out


def landmark_obs(w, dt, levels_pt=None, levels_ln=None):
    """Per landmark (points, then lines) the list of its level-0 observations in upload order, in the working type; weights rounded to
    float as the upload rounds them."""
    Np, Nl = len(w["points"]), len(w["lines"])
    obs = [[] for _ in range(Np + Nl)]
    nobs = np.zeros(Np + Nl, int)
    uv, l3 = cast(np.asarray(w["po_uv"], np.float64).reshape(-1, 2), dt), cast(np.asarray(w["lo_l"], np.float64).reshape(-1, 3), dt)
    wp = cast(np.asarray(w["po_w"], np.float64).astype(np.float32).astype(np.float64), dt)
    wl = cast(np.asarray(w["lo_w"], np.float64).astype(np.float32).astype(np.float64), dt)
    for e in range(len(w["po_pt"])):
        if levels_pt is None or not levels_pt[e]:
            obs[int(w["po_pt"][e])].append((int(w["po_kf"][e]), uv[e], wp[e]))
    for e in range(len(w["lo_ln"])):
        if levels_ln is None or not levels_ln[e]:
            obs[Np + int(w["lo_ln"][e])].append((int(w["lo_kf"][e]), l3[e], wl[e]))
    return obs


def refine(w, dt, max_iters=5, max_trials=10, lambda_init=1e-2, select_point=None, select_line=None, levels_pt=None, levels_ln=None,
           huber_on=True, kf=None):
    """plba_refine_landmarks on the window dict `w` (window.make_window's layout; optional point_fixed / line_fixed).  huber_on: True =
    w["huber"]'s deltas for both kinds, False = off, or a dict kind -> delta / None.  Returns a list of refine_one() results, one per
    landmark (skipped ones: x = the input, status only)."""
    with _prec(dt):
        rig = Rig(w, dt, kf)
        Np, Nl = len(w["points"]), len(w["lines"])
        obs = landmark_obs(w, dt, levels_pt, levels_ln)
        if huber_on is True:
            deltas = {0: w["huber"].get(0), 1: w["huber"].get(1)}
        elif huber_on is False:
            deltas = {0: None, 1: None}
        else:
            deltas = dict(huber_on)
        deltas = {k: (None if v is None else cast(np.array([v]), dt)[0]) for k, v in deltas.items()}
        pts, lns = cast(np.asarray(w["points"], np.float64).reshape(-1, 3), dt), cast(np.asarray(w["lines"], np.float64).reshape(-1, 6), dt)
        fixed = np.concatenate([np.zeros(Np, bool) if w.get("point_fixed") is None else np.asarray(w["point_fixed"]).astype(bool),
                                np.zeros(Nl, bool) if w.get("line_fixed") is None else np.asarray(w["line_fixed"]).astype(bool)])
        sel = np.concatenate([np.ones(Np, bool) if select_point is None else np.asarray(select_point).astype(bool),
                              np.ones(Nl, bool) if select_line is None else np.asarray(select_line).astype(bool)])
        res = []
        for i in range(Np + Nl):
            is_pt = i < Np
            x0 = pts[i] if is_pt else lns[i - Np]
            skip = FIXED if fixed[i] else UNSELECTED if not sel[i] else NO_OBS if not obs[i] else None
            if skip is not None:
                res.append(dict(x=x0, status=skip, iters=0, trials=0, chi2_before=x0[0] * 0, chi2_after=x0[0] * 0, rho=[], piv=[], path="", chis=[]))
                continue
            res.append(refine_one(rig, is_pt, x0, obs[i], deltas[0 if is_pt else 1], max_iters, max_trials, lambda_init))
        return res


def arrays(res, Np):
    """points (Np, 3), lines (Nl, 6), status, iters, trials, chi2_before, chi2_after as float64 / int arrays"""
    pts = np.array([f64(r["x"]) for r in res[:Np]]).reshape(-1, 3)
    lns = np.array([f64(r["x"]) for r in res[Np:]]).reshape(-1, 6)
    return dict(points=pts, lines=lns, status=np.array([r["status"] for r in res], np.uint8), iters=np.array([r["iters"] for r in res], np.int32),
                trials=np.array([r["trials"] for r in res], np.int32), chi2_before=np.array([float(r["chi2_before"]) for r in res]),
                chi2_after=np.array([float(r["chi2_after"]) for r in res]))


def compare(r64, rw, Np, factor=1000.0):
    """The tolerance rule of DESIGN.md 9 applied to the two reference runs (float64 / wide) of one window.
    same[i]:  both runs took the same decisions for landmark i (path and status): only those enter the position comparison.
    exact[i]: additionally every decision of the wide run — each solved trial's rho against 0, each trial's smallest pivot against 0 — is
              at least `factor` x its own rounding noise |float64 value - wide value| away from the threshold: counts compared exactly.
    noise_pt / noise_ln: max |x64 - xwide| over the `same` refined points / line end points (the window's noise in the maximum norm)."""
    n = len(rw)
    same, exact = np.zeros(n, bool), np.zeros(n, bool)
    noise = [0.0, 0.0]
    for i in range(n):
        a, b = r64[i], rw[i]
        same[i] = a["path"] == b["path"] and a["status"] == b["status"]
        if not same[i]:
            continue
        ok = True
        for key in ("rho", "piv"):
            for va, vb in zip(a[key], b[key]):
                va, vb = float(va), float(vb)
                if not (np.isfinite(va) and np.isfinite(vb)) or abs(vb) < factor * abs(va - vb):
                    ok = False
        exact[i] = ok
        d = np.abs(f64(a["x"]) - f64(b["x"])).max()
        k = 0 if i < Np else 1
        noise[k] = max(noise[k], float(d))
    return dict(same=same, exact=exact, noise_pt=noise[0], noise_ln=noise[1])


# ---- hand-built windows: landmarks with EXACT track lengths (tests/test_refine*.py) ----------------------------------------------------
def hand_window(K, pt_tracks, ln_tracks, seed=1, noise_px=1.0, lm_noise=0.05, kf_dt=0.02, free_kf=2):
    """K keyframes on window.py's trajectory, `kf_dt` apart (slow enough that a landmark in front of the middle of its track stays in
    every image of it); point i is seen from exactly pt_tracks[i] consecutive keyframes, line j from ln_tracks[j].  All keyframes but the
    last `free_kf` are fixed, no IMU, no prior.  The layout is window.make_window's."""
    import __graft_entry__ as g
    W = g.load_package().window
    rng = W.Rng(0xF1E0000 + seed)
    Rbc, Pbc = W.T_BS[:3, :3].copy(), W.T_BS[:3, 3].copy()
    tk = kf_dt * np.arange(K)
    Rwb, Pwb, Vwb = W.traj_R(tk), W.traj_p(tk), W.traj_v(tk)

    def tracks(lens, is_line):
        lms, ob_lm, ob_kf, ob_uv = [], [], [], []
        for i, n in enumerate(lens):
            assert 1 <= n <= K
            a = int(rng.integers(1, 0, K - n)[0])
            ks = np.arange(a, a + n)
            mid = a + n // 2
            for _ in range(200):
                u, v, depth = rng.uniform(1, 280, 470)[0], rng.uniform(1, 170, 310)[0], rng.uniform(1, 3.0, 6.0)[0]
                Pc = np.array([(u - W.CX) / W.FX * depth, (v - W.CY) / W.FY * depth, depth])
                Pw = Rwb[mid] @ (Rbc @ Pc + Pbc) + Pwb[mid]
                uv_s, z_s = W._project(Rwb[ks], Pwb[ks], Rbc, Pbc, Pw)
                ok = (z_s > 0.5) & (uv_s[:, 0] >= 0) & (uv_s[:, 0] < W.IMG_W) & (uv_s[:, 1] >= 0) & (uv_s[:, 1] < W.IMG_H)
                lm, uv = Pw, uv_s
                if is_line:
                    dirv = rng.normal((1, 3))[0]
                    Pe = Pw + dirv / np.linalg.norm(dirv) * rng.uniform(1, 0.3, 1.0)[0]
                    uv_e, z_e = W._project(Rwb[ks], Pwb[ks], Rbc, Pbc, Pe)
                    ok &= (z_e > 0.5) & (uv_e[:, 0] >= 0) & (uv_e[:, 0] < W.IMG_W) & (uv_e[:, 1] >= 0) & (uv_e[:, 1] < W.IMG_H)
                    lm, uv = np.concatenate([Pw, Pe]), np.concatenate([uv_s, uv_e], 1)
                if ok.all():
                    break
            else:
                raise AssertionError("no landmark visible over a track of %d keyframes" % n)
            lms.append(lm); ob_lm.append(np.full(n, i)); ob_kf.append(ks); ob_uv.append(uv)
        if not lens:
            return np.zeros((0, 6 if is_line else 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4 if is_line else 2))
        return np.array(lms), np.concatenate(ob_lm).astype(np.int32), np.concatenate(ob_kf).astype(np.int32), np.concatenate(ob_uv)
    pts, po_pt, po_kf, po_uv = tracks(list(pt_tracks), False)
    lns, lo_ln, lo_kf, lo_uv4 = tracks(list(ln_tracks), True)
    Ep, El = len(po_pt), len(lo_ln)
    po_uv = po_uv + rng.normal((Ep, 2), noise_px)
    lo_uv4 = lo_uv4 + rng.normal((El, 4), noise_px)
    sp = np.concatenate([lo_uv4[:, 0:2], np.ones((El, 1))], 1)
    ep = np.concatenate([lo_uv4[:, 2:4], np.ones((El, 1))], 1)
    lvec = np.cross(sp, ep).reshape(-1, 3)
    lo_l = lvec / np.sqrt(lvec[:, 0:1] ** 2 + lvec[:, 1:2] ** 2) if El else np.zeros((0, 3))
    q = np.stack([W.quat_from_R(Rwb[k]) for k in range(K)])
    fixed = np.ones(K, np.uint8); fixed[K - free_kf:] = 0
    vid = (2 * np.arange(K)).astype(np.int32)
    z3 = np.zeros((K, 3))
    kf = dict(vid_pvr=vid, vid_bias=np.full(K, -1, np.int32), P=Pwb.copy(), V=Vwb.copy(), q=q, bg=z3.copy(), ba=z3.copy(), dbg=z3.copy(), dba=z3.copy(),
              fixed_pvr=fixed, fixed_bias=fixed.copy())
    return dict(cam=dict(fx=W.FX, fy=W.FY, cx=W.CX, cy=W.CY, Rbc=Rbc, Pbc=Pbc), gw=W.GW.copy(), kf=kf,
                points=pts + rng.normal((len(pts), 3), lm_noise), lines=lns + rng.normal((len(lns), 6), lm_noise),
                po_pt=po_pt, po_kf=po_kf, po_uv=po_uv, po_w=np.ones(Ep), lo_ln=lo_ln, lo_kf=lo_kf, lo_l=lo_l, lo_w=np.ones(El),
                imu=None, prior=None, huber={0: W.HUBER[0], 1: W.HUBER[1]}, truth=dict(points=pts, lines=lns),
                meta=dict(K=K, Np=len(pts), Nl=len(lns), Ep=Ep, El=El, imu=False, seed=int(seed)))
