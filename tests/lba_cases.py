"""Hand-built windows of the visual-only local BA for the exactness tests (numpy only): every landmark's track is given, so that the
sizes the kernels loop and chunk over (entries per keyframe pair, observations per keyframe, landmarks per block) are exact numbers."""
import numpy as np

CAM = (458.654, 457.296, 367.215, 248.375)


def _rot(v):
    v = np.asarray(v, float)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def _proj(T, X):
    g = T[:3, :3].T @ (X - T[:3, 3])
    return np.array([CAM[2] + CAM[0] * g[0] / g[2], CAM[3] + CAM[1] * g[1] / g[2]])


def from_tracks(K, n_fixed, pt_tracks, ln_tracks, seed, identity_kf=None, noise_px=0.5, pose_noise=(0.02, 0.01), lm_noise=0.03):
    """K keyframes moving sideways in front of the landmarks (every rotation, true and estimated, 1e-2 rad or more away from the
    identity), the first n_fixed fixed; landmark i is seen from the keyframes pt_tracks[i] / ln_tracks[i] (a keyframe may repeat).
    identity_kf: that keyframe's ESTIMATED rotation is exactly the identity (its true one is not)."""
    rng = np.random.default_rng(seed)
    Tt = np.tile(np.eye(4), (K, 1, 1))
    for k in range(K):
        Tt[k, :3, :3] = _rot([0.03 + 0.02 * np.sin(0.7 * k), 0.05 * np.cos(0.4 * k + 0.3), 0.02 + 0.01 * k])
        Tt[k, :3, 3] = [0.25 * k, 0.03 * np.sin(k), 0.05 * k]

    def cloud():
        return np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.5, 1.5), rng.uniform(4.0, 10.0)])
    xyz = np.zeros((len(pt_tracks), 3)); po_pt, po_kf, uv = [], [], []
    for i, ks in enumerate(pt_tracks):
        xyz[i] = Tt[0, :3, 3] + Tt[0, :3, :3] @ cloud()
        for k in ks:
            po_pt.append(i); po_kf.append(k); uv.append(_proj(Tt[k], xyz[i]) + rng.normal(0, noise_px, 2))
    pq = np.zeros((len(ln_tracks), 6)); lo_ln, lo_kf, l3 = [], [], []
    for i, ks in enumerate(ln_tracks):
        P = Tt[0, :3, 3] + Tt[0, :3, :3] @ cloud()
        Q = P + Tt[0, :3, :3] @ np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 0.5)])
        pq[i] = np.concatenate([P, Q])
        for k in ks:
            a, b = _proj(Tt[k], P) + rng.normal(0, noise_px, 2), _proj(Tt[k], Q) + rng.normal(0, noise_px, 2)
            l = np.cross(np.append(a, 1.0), np.append(b, 1.0))
            lo_ln.append(i); lo_kf.append(k); l3.append(l / np.hypot(l[0], l[1]))
    T = Tt.copy()
    for k in range(n_fixed, K):
        d = rng.normal(0, 1, 3)
        d *= max(pose_noise[1], 0.01) * (1 + abs(rng.normal())) / np.linalg.norm(d)      # 1e-2 rad or more
        T[k, :3, :3] = T[k, :3, :3] @ _rot(d)
        T[k, :3, 3] += rng.normal(0, pose_noise[0], 3)
    if identity_kf is not None:
        T[identity_kf, :3, :3] = np.eye(3)
    kf_loc = np.array([-1 if k < n_fixed else k - n_fixed for k in range(K)], np.int32)
    return dict(cam=CAM, T_kf_w=T, kf_loc=kf_loc, xyz=xyz + rng.normal(0, lm_noise, xyz.shape), pq=pq + rng.normal(0, lm_noise, pq.shape),
                po_pt=np.array(po_pt, np.int32), po_kf=np.array(po_kf, np.int32), uv=np.array(uv).reshape(-1, 2),
                lo_ln=np.array(lo_ln, np.int32), lo_kf=np.array(lo_kf, np.int32), l3=np.array(l3).reshape(-1, 3))


def three_keyframes(n, lines, seed=1):
    """one fixed and two local keyframes, n landmarks each seen from all three: every keyframe pair has exactly n Schur entries and every
    local keyframe exactly n observations.  lines: about a fifth of the landmarks are lines."""
    nl = n // 5 if lines else 0
    return from_tracks(3, 1, [[0, 1, 2]] * (n - nl), [[0, 1, 2]] * nl, seed)


def blocks_257(seed=4):
    """32 768 points and one line = 257 landmark blocks of 128: every point from both local keyframes, every other one from the fixed one too"""
    return from_tracks(3, 1, [[0, 1, 2] if i % 2 else [1, 2] for i in range(32768)], [[0, 1, 2]], seed)


def block_boundary(Np, Nl, seed=6):
    return from_tracks(4, 1, [[k % 3, k % 3 + 1] if k % 4 else [0, 1, 2, 3] for k in range(Np)], [[1, 2, 3] if k % 2 else [0, 2] for k in range(Nl)], seed)


def _small():
    pts = [[k % 2 + 1, k % 2 + 2] if k % 3 else [0, 1, 2, 3] for k in range(40)]
    lns = [[1, 2, 3] if k % 2 else [0, 1, 3] for k in range(8)]
    return pts, lns


def edge_duplicate(seed=7):
    """point 0 is observed twice from keyframe 2 (local index 1)"""
    pts, lns = _small()
    pts[0] = [1, 2, 2, 3]
    return from_tracks(4, 1, pts, lns, seed)


def edge_fixed_only(seed=8):
    """two fixed keyframes; point 0 and line 0 are seen from fixed keyframes only"""
    pts, lns = _small()
    pts[0] = [0, 1]; lns[0] = [0, 1]
    return from_tracks(4, 2, pts, lns, seed)


def edge_identity(seed=9):
    """local keyframe 2's map rotation is exactly the identity: the theta < 1e-6 branches of logmap_se3 (X_aux) and expmap_se3"""
    pts, lns = _small()
    return from_tracks(4, 1, pts, lns, seed, identity_kf=2)


def edge_exact_uv(seed=10):
    """observation 1's (point 0 from keyframe 1, a local one) uv is the fp64 projection of the ESTIMATE: a residual norm below homog_th"""
    pts, lns = _small()
    w = from_tracks(4, 1, pts, lns, seed)
    k, i = w["po_kf"][1], w["po_pt"][1]      # (observation 1: keyframe 1, local)
    T = w["T_kf_w"][k]
    w["uv"][1] = _proj(T, w["xyz"][i])
    return w


def fail_unobserved_point(seed=11):
    pts, lns = _small()
    w = from_tracks(4, 1, pts, lns, seed)
    w["xyz"] = np.vstack([w["xyz"], [[0.3, 0.2, 7.0]]])      # index 40: no observation
    return w


def fail_unobserved_keyframe(seed=12):
    pts = [[0, 1, 2]] * 30
    lns = [[0, 1], [1, 2], [0, 2], [0, 1, 2]]
    return from_tracks(4, 1, pts, lns, seed)      # keyframe 3 (local index 2) has no observation


EDGES = dict(duplicate=edge_duplicate, fixed_only=edge_fixed_only, identity=edge_identity, exact_uv=edge_exact_uv)
CHUNK_N = (64, 65, 255, 256, 257, 513)
