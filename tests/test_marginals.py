"""plba_compute_marginals on the GPU: parity with the numpy reference of tests/marginals_ref.py on both landmark paths, the exact
properties of the result, a state left alone, and the refusals."""
import numpy as np
import pytest

from tests import marginals_ref as mr
from tests.test_marginals_cpu import small_window

pytestmark = pytest.mark.gpu


def _problems(pkg, orc, w, fused, gate=False):
    """The product problem and an oracle problem at the SAME estimate.  gate: optimize(5) + gate_outliers on the product, whose
    estimates and levels are then given to the oracle (Huber off on point / line edges, as the gating leaves it)."""
    hp = pkg.new_problem(lm_fused_min_obs=1) if fused else pkg.new_problem(lm_fused=0)
    hp.upload_window(w)
    op = orc.new_problem()
    if gate:
        hp.optimize(5)
        hp.gate_outliers(5.991)
        w = dict(w)
        k = dict(w["kf"])
        k.update({key: v for key, v in hp.get_keyframes().items()})
        w["kf"], w["points"], w["lines"] = k, hp.get_points(), hp.get_lines()
        op.upload_window(w)
        for kind in (0, 1):
            op.set_robust(kind, False, 0.0)
            op.set_levels(kind, hp.get_levels(kind))
    else:
        op.upload_window(w)
    hp.debug_build(1.0)
    assert int(hp.debug_get("lm_fused")[0]) == (1 if fused else 0)
    return hp, op, w


def _close(a, b, tol, floor=0.0):
    """|a - b| <= tol x max(the largest entry of b, floor), NaN where b has NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    if not a.size:
        return
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    scale = max(np.abs(b[m]).max() if m.any() else 0.0, floor, 1e-300)
    err = np.abs(a[m] - b[m]).max() if m.any() else 0.0
    assert err <= tol * scale, (err, scale, tol)


def _blockwise(a, b, tol):
    for x, y in zip(a, b):
        _close(x, y, tol)


def _kf_blockwise(a, b, tol, gmax):
    """15 x 15 keyframe / pair blocks, each PVR / bias sub-block against its own largest entry (the bias variances are orders of
    magnitude below the position ones).  An inverse's error is bounded relative to the whole matrix (~ kappa u |Sigma|), so a
    sub-block's scale is floored at 1e-3 of its 15 x 15 block's largest entry and at 1e-3 of the largest keyframe variance (gmax)."""
    for x, y in zip(a, b):
        whole = max(np.abs(y).max(), gmax)
        for r in (slice(0, 9), slice(9, 15)):
            for c in (slice(0, 9), slice(9, 15)):
                _close(x[r, c], y[r, c], tol, 1e-3 * whole)


def _parity(pkg, orc, w, fused, gate):
    hp, op, w = _problems(pkg, orc, w, fused, gate)
    robust = {k: (None if gate else w["huber"].get(k)) for k in (0, 1)}
    for kind in (0, 1):
        if (len(w["po_pt"]) if kind == 0 else len(w["lo_ln"])):
            assert np.array_equal(hp.get_levels(kind), op.get_levels(kind))
    K = len(w["kf"]["vid_pvr"])
    pairs = np.array([[i, j] for i in range(K) for j in range(K) if abs(i - j) <= 2], np.int32)
    got = hp.marginals(pairs=pairs)
    ref, R, res, _ = mr.reference(op, w, robust)
    # The windows' pose systems have kappa(S) from 6e7 to 3e10 (150 keyframes): two double-precision inverses of S (each within about
    # kappa u of the exact one, u = 1.1e-16, relative to the whole matrix) then agree to tens of kappa u relative to a 9 x 9 or 6 x 6
    # sub-block, not 1e-9 — measured up to 6e-15 kappa (the gated 12-keyframe window, kappa 7e7).  The tolerance is kappa x 1e-14,
    # stated here and printed with kappa (pytest -s).
    kappa = np.linalg.cond(res["S"])
    tol = max(1e-9, kappa * 1e-14)
    print("marginals parity: P %d kappa(S) %.2e tol %.2e" % (R.P, kappa, tol))
    assert kappa < 1e11
    assert np.array_equal(got["pt_status"], ref["pt_status"]) and np.array_equal(got["ln_status"], ref["ln_status"])
    gmax = np.abs(ref["kf"]).max()
    _kf_blockwise(got["kf"], ref["kf"], tol, gmax)
    _kf_blockwise(got["pairs"], [R.block(res["Spp"], i, j) for i, j in pairs], tol, gmax)
    _blockwise(got["pt"], ref["pt"], tol)
    _blockwise(got["ln"], ref["ln"], tol)
    assert got["n_excluded"] == (int((ref["pt_status"] >= 2).sum()), int((ref["ln_status"] >= 2).sum()))
    hp.close(); op.close()
    return got, ref


def _fixed_variant(pkg):
    w = small_window(pkg)
    w["point_fixed"] = np.zeros(len(w["points"]), np.uint8); w["point_fixed"][0] = 1
    w["line_fixed"] = np.zeros(len(w["lines"]), np.uint8); w["line_fixed"][0] = 1
    w["kf"]["fixed_pvr"][2] = 1      # PVR fixed, bias free
    return w


WINDOWS = {
    "small": lambda pkg: small_window(pkg),
    "fixed": _fixed_variant,
    # the reference's 12-keyframe window with tracks over 6 to 12 keyframes (wide groups)
    "k12": lambda pkg: pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AA, track=(6, 12)),
    # 50 keyframes, landmarks revisited 10 to 29 keyframes later (no band in the pose system)
    "rev50": lambda pkg: pkg.window.make_window(50, 600, 120, imu=True, seed=0x5EED0050, kf_dt=0.25, revisit=0.3, revisit_gap=(10, 30)),
    # configs[2]'s shape (50 keyframes, IMU, its track statistics; P = 735, 23 block steps) with a tenth of its landmarks, so that the
    # numpy reference stays quick
    "cfg2": lambda pkg: pkg.window.make_config(3, scale=0.1),
    # 150 free keyframes (P = 2235 > 2048: 70 block steps of the factorisation), few landmarks
    "k150": lambda pkg: pkg.window.make_window(150, 300, 60, imu=True, seed=0x5EED0150, kf_dt=0.25),
}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_parity(pkg, orc, hip, name, fused):
    w = WINDOWS[name](pkg)
    if name == "rev50":
        span = [np.ptp(w["po_kf"][w["po_pt"] == l]) for l in range(len(w["points"]))]
        assert max(span) >= 25
    got, ref = _parity(pkg, orc, w, fused, gate=False)
    if name == "fixed":
        assert got["pt_status"][0] == 1 and got["ln_status"][0] == 1
        assert not got["pt"][0].any() and not got["ln"][0].any()
        assert not got["kf"][2][:9].any() and not got["kf"][2][:, :9].any() and got["kf"][2][9:, 9:].any()


@pytest.mark.parametrize("fused", [False, True])
def test_parity_after_gating(pkg, orc, hip, fused):
    w = pkg.window.make_window(12, 300, 60, imu=True, seed=0x5EED00AB)
    got, ref = _parity(pkg, orc, w, fused, gate=True)
    assert (got["pt_status"] == 2).any() or (got["ln_status"] == 2).any()
    assert np.isnan(got["pt"][got["pt_status"] == 2]).all()


def test_exact_properties(pkg, hip):
    w = WINDOWS["k12"](pkg)
    hp = pkg.new_problem()
    hp.upload_window(w)
    hp.optimize(5)
    K = len(w["kf"]["vid_pvr"])
    pairs = np.array([[i, j] for i in range(K) for j in range(K)], np.int32)
    a = hp.marginals(pairs=pairs)
    b = hp.marginals(pairs=pairs)
    for key in ("kf", "pairs", "pt", "ln", "pt_status", "ln_status"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for k in range(K):
        assert np.array_equal(a["kf"][k], a["kf"][k].T)
        assert np.array_equal(a["pairs"][k * K + k], a["kf"][k])
    for i in range(K):
        for j in range(K):
            assert np.array_equal(a["pairs"][i * K + j], a["pairs"][j * K + i].T)
    lns = hp.get_lines()
    for c, s, L in zip(a["ln"], a["ln_status"], lns):
        if s:
            continue
        dv = L[3:] - L[:3]
        dv /= np.linalg.norm(dv)
        assert np.abs(c[:3, :3] @ dv).max() <= 1e-12 * np.abs(c).max() and np.abs(c[3:, 3:] @ dv).max() <= 1e-12 * np.abs(c).max()
        ev = np.linalg.eigvalsh(c)
        assert (np.abs(ev) <= 1e-10 * ev.max()).sum() == 2
    for c, s in zip(a["pt"], a["pt_status"]):
        if s == 0:
            assert np.array_equal(c, c.T) and np.linalg.eigvalsh(c).min() > 0
    hp.close()


def test_single_observation_landmark_changes_nothing(pkg, hip):
    w = WINDOWS["small"](pkg)
    w2 = {k: v for k, v in w.items()}
    Np = len(w["points"])
    w2["points"] = np.vstack([w["points"], w["points"][:1] + 0.3])
    w2["po_pt"] = np.concatenate([w["po_pt"], [Np]]).astype(np.int32)
    w2["po_kf"] = np.concatenate([w["po_kf"], [1]]).astype(np.int32)
    w2["po_uv"] = np.vstack([w["po_uv"], w["po_uv"][:1]])
    w2["po_w"] = np.concatenate([w["po_w"], w["po_w"][:1]])
    out = []
    for win in (w, w2):
        hp = pkg.new_problem()
        hp.upload_window(win)
        out.append(hp.marginals())
        hp.close()
    assert out[1]["pt_status"][-1] == 2 and np.isnan(out[1]["pt"][-1]).all()
    _close(out[1]["kf"], out[0]["kf"], 1e-12)


def _run(pkg, w, between=None, slide=False, marg=False):
    hp = pkg.new_problem()
    hp.upload_window(w)
    hp.optimize(5)
    if marg:
        hp.marginalize_to_prior(0, 50)
    if between:
        between(hp)
    hp.optimize(10)
    r = (hp.get_keyframes(), hp.get_points(), hp.get_lines(), hp.trace())
    hp.close()
    return r


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        if isinstance(x, dict):
            for k in x:
                assert np.array_equal(x[k], y[k]), k
        else:
            assert np.array_equal(x, y)
    assert len(a[3]) == len(b[3])
    for r, s in zip(a[3], b[3]):
        assert r == s


def test_call_changes_no_state(pkg, hip):
    w = WINDOWS["k12"](pkg)
    _same(_run(pkg, w, lambda p: p.marginals()), _run(pkg, w))
    _same(_run(pkg, w, lambda p: p.marginals(), marg=True), _run(pkg, w, marg=True))


def test_refusals(pkg, hip):
    fresh = pkg.new_problem()
    with pytest.raises(pkg.abi.PlbaError, match="STATE"):
        fresh.marginals()
    fresh.close()
    # a keyframe without any edge: S is singular
    w5 = pkg.window.make_window(5, 40, 10, imu=True, seed=0x3A11C1, track=(2, 4))
    keep_p = w5["po_kf"] != 4
    keep_l = w5["lo_kf"] != 4
    for k, m in (("po_pt", keep_p), ("po_kf", keep_p), ("po_uv", keep_p), ("po_w", keep_p),
                 ("lo_ln", keep_l), ("lo_kf", keep_l), ("lo_l", keep_l), ("lo_w", keep_l)):
        w5[k] = w5[k][m]
    im = w5["imu"]
    keep_i = (im["kf_i"] != 4) & (im["kf_j"] != 4)
    for k in ("kf_i", "kf_j", "preint", "info_pvr", "info_bias"):
        im[k] = im[k][keep_i]
    ref = _run(pkg, w5)
    hp = pkg.new_problem()
    hp.upload_window(w5)
    hp.optimize(5)
    import ctypes as C
    K = 5
    kf = np.full((K, 15, 15), 7.25)
    m = pkg.abi.Marginals()
    m.want = 1
    m.kf_cov = kf.ctypes.data_as(C.POINTER(C.c_double))
    rc = hp.lib.fn["compute_marginals"](hp._h, C.byref(m))
    assert rc == -4      # PLBA_ERR_NUMERIC
    assert "keyframe slot 4" in hp.lib.fn["last_error"](hp._h).decode()
    assert (kf == 7.25).all()
    with pytest.raises(pkg.abi.PlbaError, match="INVALID"):
        hp.marginals(pairs=[[0, 5]])
    hp.optimize(10)
    _same((hp.get_keyframes(), hp.get_points(), hp.get_lines(), hp.trace()), ref)
    hp.close()


def test_local_ba_marginals(pkg, hip):
    w = WINDOWS["k12"](pkg)
    a = pkg.new_problem(); a.upload_window(w)
    out = pkg.protocol.local_ba(a, marginals=True)
    b = pkg.new_problem(); b.upload_window(w)
    b.optimize(5); b.gate_outliers(5.991); b.optimize(10)
    direct = b.marginals()
    for key in ("kf", "pt", "ln", "pt_status", "ln_status"):
        assert np.array_equal(out["marginals"][key], direct[key], equal_nan=True), key
    a.close(); b.close()


def test_slid_window(pkg, hip):
    """After plba_slide_window (carried observations, a device-made prior): the marginals equal those of a fresh upload of the same
    window bit for bit, and a following BA is the one without the call."""
    W = pkg.window
    seq = W.make_sequence(12, 2, 300, 60, seed=0x511DE + 12, kf_dt=0.1)
    w0 = W.window_at(seq, 0, 12)
    w1 = W.window_at(seq, 1, 12, prev=w0)
    runs = []
    for call in (False, True):
        slid = pkg.new_problem()
        slid.upload_window(w0)
        pkg.protocol.local_ba(slid)
        res0 = pkg.protocol.results(slid)
        prior = slid.marginalize(0, pkg.protocol.MARG_NUM)
        slid.slide_window(W.slide_delta(w0, w1))
        for kind, d in w1["huber"].items():
            slid.set_robust(kind, True, d)
        slid.set_prior(prior)
        m = slid.marginals() if call else None
        pkg.protocol.local_ba(slid)
        runs.append((m, pkg.protocol.results(slid), slid.trace()))
        slid.close()
    for k in runs[0][1]:
        assert np.array_equal(np.asarray(runs[0][1][k]), np.asarray(runs[1][1][k])), k
    assert runs[0][2] == runs[1][2]
    wf = dict(W.window_from_results(w1, w0, res0))
    wf["prior"] = prior
    fresh = pkg.new_problem()
    fresh.upload_window(wf)
    mf = fresh.marginals()
    fresh.close()
    for key in ("kf", "pt", "ln", "pt_status", "ln_status"):
        assert np.array_equal(runs[1][0][key], mf[key], equal_nan=True), key
