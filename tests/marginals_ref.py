"""Numpy reference of plba_compute_marginals (include/plba.h), built on the CPU oracle.

Landmark blocks come from the oracle's per-edge evaluators (eval_point_edge, eval_line_edge with fix_q1 = 0, huber).  The oracle
does not expose Hpp, so the pose side is reconstructed from its damped Schur complement:
    Hpp = Hschur(lam) - lam I + sum_l Hpl (Hll + lam I)^-1 Hlp
at two values of lam (they must agree).  Then the elimination rules of the header: status 1 fixed, 2 fewer than two active
edges (no contribution), 3 degenerate reduced block, lines reduced to the 4-dimensional subspace orthogonal to the line.
"""
import numpy as np

from oracle import oracle as orc


def pose_offsets(w):
    """The pose-side index map of the library and the oracle: non-fixed vertices in keyframe order, bias first when its id is
    the smaller one (plba_api.hip prepare())."""
    k = w["kf"]
    K = len(k["vid_pvr"])
    op, ob = -np.ones(K, int), -np.ones(K, int)
    off = 0
    for i in range(K):
        pv = not k["fixed_pvr"][i]
        bv = k["vid_bias"][i] >= 0 and not k["fixed_bias"][i]
        if pv and bv and k["vid_bias"][i] < k["vid_pvr"][i]:
            ob[i] = off; off += 6; op[i] = off; off += 9
        else:
            if pv:
                op[i] = off; off += 9
            if bv:
                ob[i] = off; off += 6
    return op, ob, off


def line_basis(L):
    d = L[3:] - L[:3]
    d = d / np.linalg.norm(d)
    N = np.linalg.svd(d.reshape(1, 3))[2][1:].T      # 3 x 2, orthonormal, orthogonal to d
    B = np.zeros((6, 4))
    B[:3, :2] = N
    B[3:, 2:] = N
    return B


class Reference:
    """Everything of one window at the oracle problem's current estimate.  robust: {0: delta or None, 1: delta or None}."""

    def __init__(self, op, w, robust):
        self.w = w
        cam = orc.cam_vec(w["cam"])
        kfs = op.get_keyframes()
        pts, lns = op.get_points(), op.get_lines()
        kw = w["kf"]
        K = len(kw["vid_pvr"])
        nav = [orc.nav_vec(kfs["P"][i], kfs["V"][i], kfs["q"][i], kw["bg"][i], kw["ba"][i], kfs["dbg"][i], kfs["dba"][i]) for i in range(K)]
        self.nav = nav
        self.op_off, self.ob_off, self.P = pose_offsets(w)
        lvp = op.get_levels(0) if len(w["po_pt"]) else np.zeros(0, np.uint8)
        lvl = op.get_levels(1) if len(w["lo_ln"]) else np.zeros(0, np.uint8)
        Np, Nl = len(pts), len(lns)
        self.Np, self.Nl, self.K = Np, Nl, K
        pfix = np.zeros(Np, bool) if w.get("point_fixed") is None else np.asarray(w["point_fixed"], bool)
        lfix = np.zeros(Nl, bool) if w.get("line_fixed") is None else np.asarray(w["line_fixed"], bool)
        # per landmark: list of (kf, w_e, Jl (2 x nd), Jp (2 x 9))
        self.lm = []
        for kind, N, arr, lm_of, kf_of, meas, wts, lv, fix in (
                (0, Np, pts, w["po_pt"], w["po_kf"], w["po_uv"], w["po_w"], lvp, pfix),
                (1, Nl, lns, w["lo_ln"], w["lo_kf"], w["lo_l"], w["lo_w"], lvl, lfix)):
            edges = [[] for _ in range(N)]
            rho = [[] for _ in range(N)]      # Huber's rho' per kept edge (1 without a kernel)
            for e in range(len(lm_of)):
                if lv[e]:
                    continue
                k, l = int(kf_of[e]), int(lm_of[e])
                if kind == 0:
                    err, Ji, Jj, _ = orc.eval_point_edge(cam, nav[k], arr[l], meas[e])
                else:
                    err, Ji, Jj, _ = orc.eval_line_edge(cam, nav[k], arr[l], meas[e], fix_q1=0)
                    err, Ji, Jj = err[:2], Ji[:2], Jj[:2]
                isg = float(wts[e])
                chi = isg * float(err @ err)
                rho1 = 1.0
                if robust.get(kind) is not None:
                    rho1 = orc.huber(chi, robust[kind])[1]
                edges[l].append((k, isg * rho1, Ji, Jj))
                rho[l].append(float(rho1))
            for l in range(N):
                self.lm.append(dict(kind=kind, idx=l, x=arr[l], fixed=bool(fix[l]), edges=edges[l], rho1=rho[l]))

    def landmark_blocks(self, lm):
        """Hll, and per observation from a free keyframe (pose offset, Hpl block 9 x nd, Hpp block 9 x 9)."""
        nd = 3 if lm["kind"] == 0 else 6
        Hll = np.zeros((nd, nd))
        obs = []
        for k, we, Jl, Jp in lm["edges"]:
            Hll += we * Jl.T @ Jl
            o = self.op_off[k]
            if o >= 0:
                obs.append((o, we * Jp.T @ Jl, we * Jp.T @ Jp))
        return Hll, obs

    @staticmethod
    def _schur(H, obs, Dinv, sign):
        for oa, Ba, _ in obs:
            BD = Ba @ Dinv
            for ob, Bb, _ in obs:
                H[oa:oa + 9, ob:ob + 9] += sign * BD @ Bb.T

    def hpp(self, op, lam):
        """Hpp at the oracle's linearisation point from its damped Schur complement."""
        op.debug_build(lam)
        Hs = op.debug_get("Hschur").reshape(self.P, self.P)
        H = Hs - lam * np.eye(self.P)
        for lm in self.lm:
            if lm["fixed"] or not lm["edges"]:
                continue
            Hll, obs = self.landmark_blocks(lm)
            self._schur(H, obs, np.linalg.inv(Hll + lam * np.eye(len(Hll))), +1.0)
        return H

    def solve(self, Hpp, dense_check=False):
        P = self.P
        S0 = Hpp.copy()
        st, red = [], []
        for lm in self.lm:
            Hll, obs = self.landmark_blocks(lm)
            if lm["fixed"]:
                st.append(1); red.append(None); continue
            if len(lm["edges"]) >= 2:
                B = np.eye(3) if lm["kind"] == 0 else line_basis(lm["x"])
                Hr = B.T @ Hll @ B
                try:
                    Lr = np.linalg.cholesky(Hr)
                    ok = np.min(np.diag(Lr) ** 2) > 1e-12 * np.max(np.diag(Hr))
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    st.append(0); red.append((B, Hr, [(o, Hpl @ B) for o, Hpl, _ in obs])); continue
            st.append(2 if len(lm["edges"]) < 2 else 3); red.append(None)
            for o, _, Hp in obs:
                S0[o:o + 9, o:o + 9] -= Hp
        S = S0.copy()
        for r in red:
            if r is not None:
                B, Hr, W = r
                self._schur(S, [(o, w, None) for o, w in W], np.linalg.inv(Hr), -1.0)
        Spp = np.linalg.inv(S)
        cov = []
        for i, (r, s) in enumerate(zip(red, st)):
            if r is None:
                nd = 3 if i < self.Np else 6
                cov.append(np.zeros((nd, nd)) if s == 1 else np.full((nd, nd), np.nan))
                continue
            B, Hr, W = r
            Hi = np.linalg.inv(Hr)
            M = np.zeros_like(Hr)
            for oa, wa in W:
                for ob, wb in W:
                    M += wa.T @ Spp[oa:oa + 9, ob:ob + 9] @ wb
            cov.append(B @ (Hi + Hi @ M @ Hi) @ B.T)
        out = dict(Spp=Spp, S=S, status=np.array(st, np.uint8), cov=cov)
        if dense_check:      # the full undamped Hessian in the reduced landmark coordinates, inverted densely
            live = [i for i, r in enumerate(red) if r is not None]
            dims = [red[i][1].shape[0] for i in live]
            n = P + sum(dims)
            A = np.zeros((n, n))
            A[:P, :P] = S0
            o = P
            for i, dm in zip(live, dims):
                B, Hr, W = red[i]
                A[o:o + dm, o:o + dm] = Hr
                for oa, wa in W:
                    A[oa:oa + 9, o:o + dm] += wa
                    A[o:o + dm, oa:oa + 9] += wa.T
                o += dm
            Ai = np.linalg.inv(A)
            dcov, o = {}, P
            for i, dm in zip(live, dims):
                B = red[i][0]
                dcov[i] = B @ Ai[o:o + dm, o:o + dm] @ B.T
                o += dm
            out["dense"] = dict(Spp=Ai[:P, :P], cov=dcov)
        return out

    def kf_index(self, k):
        idx = []
        for r in range(15):
            o = self.op_off[k] if r < 9 else self.ob_off[k]
            idx.append(-1 if o < 0 else o + (r if r < 9 else r - 9))
        return np.array(idx)

    def block(self, Spp, i, j):
        a, b = self.kf_index(i), self.kf_index(j)
        out = np.zeros((15, 15))
        for r in range(15):
            for c in range(15):
                if a[r] >= 0 and b[c] >= 0:
                    out[r, c] = Spp[a[r], b[c]]
        return out


def _huber1(chi, delta):
    return 1.0 if chi <= delta * delta else delta / np.sqrt(chi)


def reference(op, w, robust, lams=(1e-3, 1.0), dense_check=False):
    """Marginals of the oracle problem `op` (window `w` uploaded, levels / robust kernels as given) in the layout of
    Problem.marginals.  Returns (dict, Reference, [Hpp at each lam])."""
    ref = Reference(op, w, robust)
    Hs = [ref.hpp(op, lam) for lam in lams]
    H = Hs[0]
    res = ref.solve(H, dense_check)
    out = dict(kf=np.array([ref.block(res["Spp"], k, k) for k in range(ref.K)]),
               pt=np.array(res["cov"][:ref.Np]).reshape(-1, 3, 3), ln=np.array(res["cov"][ref.Np:]).reshape(-1, 6, 6),
               pt_status=res["status"][:ref.Np], ln_status=res["status"][ref.Np:])
    return out, ref, res, Hs
