"""plba_marginalize_to_prior / plba_get_prior (include/plba.h): the marginalization whose result stays on the device as the problem's next
prior — the reference's MapHandler::marg_info, built at the end of one BA call and read at the start of the next (src/mapHandler.cpp:
6190-6197 -> 6007-6034) — must compute exactly what plba_marginalize computes, and a sequence that carries it on the device must be the
sequence that carries it through the host (plba_marginalize -> plba_slide_window -> plba_set_prior), bit for bit."""
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIOR_KEYS = ("vid", "size", "idx", "x0", "J0", "r0", "Ar", "br")


def _marg_cases():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if here not in sys.path:
        sys.path.insert(0, here)
    import marg_cases
    return marg_cases


def _same_prior(a, b, what):
    for k in ("n", "m"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in PRIOR_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def _window(pkg, case):
    W = pkg.window
    if case in ("default", "exact0", "exact2"):
        return W.make_window(12, 260, 50, imu=True, seed=21), 0
    if case == "far":
        return _marg_cases().case_window(pkg, dict(far=1e3)), None      # (as uploaded, like tests/test_gpu_parity.py's far-landmark cases)
    if case == "n105":
        return W.make_window(12, 300, 60, imu=True, seed=77, kf_dt=0.1, track=(12, 12)), 2
    if case == "n186":
        return W.make_window(21, 300, 60, imu=True, seed=77, kf_dt=0.05, track=(21, 21)), 2
    raise ValueError(case)


def _opts(case):
    return dict(marg_exact=0) if case == "exact0" else dict(marg_exact=2) if case == "exact2" else {}


@pytest.mark.parametrize("case", ["default", "exact0", "exact2", "far", "n105", "n186"])
def test_same_output_as_marginalize(pkg, hip, case):
    w, iters = _window(pkg, case)
    out = []
    for dev in (False, True):
        p = pkg.new_problem(**_opts(case)); p.upload_window(w)
        if iters:
            p.optimize(iters)
        elif iters == 0:
            pkg.protocol.local_ba(p)
        if dev:
            d = p.marginalize_to_prior(0, 50)
            pr = p.get_prior()
            assert (d["n"], d["m"], d["nv"]) == (pr["n"], pr["m"], len(pr["vid"]))
        else:
            pr = p.marginalize(0, 50)
        out.append((pr, p.debug_get("marg_path")))
        p.close()
    _same_prior(out[0][0], out[1][0], case)
    assert np.array_equal(out[0][1], out[1][1]), (case, out[0][1], out[1][1])
    if case == "far":
        assert int(out[1][1][0]) == 1      # the certificate failed: the dense path ran when get_prior resolved the marginalization
    if case == "n105":
        assert out[1][0]["n"] == 105
    if case == "n186":
        assert out[1][0]["n"] == 186


def _restore_robust(p, w):
    for kind, d in w["huber"].items():      # (gating switched the point / line kernels off: a new graph has them again, mapHandler.cpp:5937)
        p.set_robust(kind, True, d)


def _stats(r):
    return (r["stage1"].iterations, r["stage1"].trials, r["stage1"].chi2_initial, r["stage1"].chi2_final, r["gated"],
            r["stage2"].iterations, r["stage2"].trials, r["stage2"].chi2_final, r["stage2"].lambda_final)


def _same_results(a, b, what):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k, np.abs(np.asarray(a[k]) - np.asarray(b[k])).max())


def _carried(pkg, seq, K, nwin, opts, device, deltas=None, read_prior="end"):
    """nwin windows of one handle, slid in place.  device: the prior stays on the device (plba_marginalize_to_prior, never plba_set_prior);
    else plba_marginalize -> slide -> plba_set_prior.  Per window: (stats, results, the prior made at its end or None, trial sequence,
    marg_path).  read_prior (device form): "end" = plba_get_prior after the LAST window only, so that every other marginalization is still
    pending when the slide runs and is resolved by the next window's plba_optimize (the reference's life-cycle); "each" = after every window
    (which resolves it before the slide).  The host form returns every prior and its marg_path."""
    W = pkg.window
    p = pkg.new_problem(**opts)
    rows, w_prev, prior = [], None, None
    for i in range(nwin):
        w = W.window_at(seq, i, K, prev=w_prev)
        if i == 0:
            p.upload_window(w)
        else:
            d = W.slide_delta(w_prev, w)
            if deltas is not None:
                d = deltas(i, p, w_prev, w, d)
            p.slide_window(d)
            _restore_robust(p, w)
            if not device:
                p.set_prior(prior)
        path = None
        if device:
            r = pkg.protocol.local_ba(p, marginalize="device")
            res = pkg.protocol.results(p)
            prior = p.get_prior() if read_prior == "each" or i == nwin - 1 else None
        else:
            r = pkg.protocol.local_ba(p)
            prior = p.marginalize(0, pkg.protocol.MARG_NUM)
            path = p.debug_get("marg_path")
            res = pkg.protocol.results(p)
        rows.append((_stats(r), res, prior, [(t["iteration"], t["trial"], t["accepted"]) for t in p.trace()], path))
        w_prev = w
    p.close()
    return rows


@pytest.mark.parametrize("K,Np,Nl,opts", [(12, 300, 60, dict(lm_fused=0)), (12, 900, 200, dict(lm_fused=2)), (20, 2500, 500, dict(lm_fused=2))])
def test_carried_sequence_equals_the_host_round_trip(pkg, hip, K, Np, Nl, opts):
    nwin = 4
    seq = pkg.window.make_sequence(K, nwin, Np, Nl, seed=0x9A1D + K, kf_dt=0.1 if K <= 12 else 0.25)
    A = _carried(pkg, seq, K, nwin, opts, True)      # pending across every slide
    B = _carried(pkg, seq, K, nwin, opts, False)
    _same_sequence(A, B)
    A_each = _carried(pkg, seq, K, nwin, opts, True, read_prior="each")      # every intermediate prior, read back
    _same_sequence(A_each, B)


def _same_sequence(A, B):
    for i, (a, b) in enumerate(zip(A, B)):
        assert a[0] == b[0], ("window %d" % i, a[0], b[0])
        _same_results(a[1], b[1], "window %d" % i)
        if a[2] is not None:
            _same_prior(a[2], b[2], "window %d" % i)
        assert a[3] == b[3], "window %d: trial sequence" % i
    assert A[-1][2] is not None


def test_carried_sequence_with_the_dense_path_at_resolution(pkg, hip):
    """Far landmarks seen first from each window's oldest keyframe (tests/golden/marg_cases.py's far case, along a sequence): the
    certificate fails, so the dense path runs when the next window's plba_optimize resolves the pending marginalization — after the slide"""
    W = pkg.window
    K, nwin, far = 6, 4, 1e3
    seq = W.make_sequence(K, nwin, 120, 20, seed=31, outlier_frac=0.0)
    P = seq["kf"]["P"]
    for lm, ob_lm, ob_kf, w in (("points", "po_pt", "po_kf", 3), ("lines", "lo_ln", "lo_kf", 6)):
        first = np.full(len(seq[lm]), 1 << 30, np.int64)
        np.minimum.at(first, seq[ob_lm].astype(np.int64), seq[ob_kf].astype(np.int64))
        for l in np.flatnonzero(first < nwin):
            o = np.tile(P[first[l]], w // 3)
            seq[lm][l] = o + far * (seq[lm][l] - o)
    A = _carried(pkg, seq, K, nwin, {}, True)
    B = _carried(pkg, seq, K, nwin, {}, False)
    _same_sequence(A, B)
    assert sum(int(b[4][0]) for b in B[:-1]) >= 1, [b[4] for b in B]      # a dense path that ran at a resolution after a slide


def test_carried_sequence_at_half_the_headline_shape_with_drop_masks(pkg, hip):
    """half of BASELINE configs[2] (fused landmark passes, multi-chain factorisation), 4 windows; the second slide also drops culled
    observations by mask (w_prev's observation list is the problem's only up to that slide, so the third is a plain one again)"""
    K, nwin = 50, 4
    seq = pkg.window.make_sequence(K, nwin, 10000, 2000, seed=0x9A1D50)

    def masks(i, p, w_prev, w, d):
        if i != 2:
            return d
        cull = p.cull_observations(pkg.window.CHI2_GATE)

        def thin(bad, ob_lm):      # an observation leaves only when its landmark keeps at least two
            left = np.bincount(ob_lm[bad == 0], minlength=ob_lm.max() + 1)
            bad = bad.copy(); bad[left[ob_lm] < 2] = 0
            return bad
        d["drop_point_obs"] = thin(cull["bad_points"].astype(np.uint8), w_prev["po_pt"])
        d["drop_line_obs"] = thin(cull["bad_lines"].astype(np.uint8), w_prev["lo_ln"])
        assert d["drop_point_obs"].sum() > 10
        return d
    A = _carried(pkg, seq, K, nwin, {}, True, masks)
    B = _carried(pkg, seq, K, nwin, {}, False, masks)
    _same_sequence(A, B)


def _pose_delta(a, b, pkg):
    dP = np.abs(a["P"] - b["P"]).max()
    dphi = 0.0
    for qa, qb in zip(a["q"], b["q"]):
        Ra, Rb = pkg.window.R_from_quat(qa), pkg.window.R_from_quat(qb)
        dphi = max(dphi, np.linalg.norm(pkg.window.log_so3(Rb.T @ Ra)))
    return dP, dphi


def test_device_carried_sequence_pinned_to_the_oracle(pkg, orc, hip):
    """The device-carried sequence against the oracle, which runs the same windows through fresh uploads and carries its own priors"""
    W = pkg.window
    K, nwin = 12, 3
    seq = W.make_sequence(K, nwin, 300, 60, seed=0x9A1D0C)
    A = _carried(pkg, seq, K, nwin, dict(lm_fused=0), True)
    w_prev, res_prev, prior = None, None, None
    for i in range(nwin):
        w = W.window_at(seq, i, K, prev=w_prev)
        wf = dict(w if i == 0 else W.window_from_results(w, w_prev, res_prev)); wf["prior"] = prior
        o = orc.new_problem(); o.upload_window(wf)
        r = pkg.protocol.local_ba(o)
        prior = o.marginalize(0, pkg.protocol.MARG_NUM)
        res_prev = pkg.protocol.results(o)
        tr = [(t["iteration"], t["trial"], t["accepted"]) for t in o.trace()]
        o.close()
        a = A[i]
        assert a[0][4] == r["gated"], ("window %d: gating" % i, a[0][4], r["gated"])
        assert a[3] == tr, "window %d: accept / reject sequence" % i
        dP, dphi = _pose_delta(a[1], res_prev, pkg)
        assert dP <= 1e-5 and dphi <= 1e-5, ("window %d" % i, dP, dphi)
        w_prev = w


def test_enqueue_only_on_the_certified_path(pkg, hip):
    w, _ = _window(pkg, "n105")
    p = pkg.new_problem(); p.upload_window(w); p.optimize(2)
    h0 = p.debug_get("host_waits")[0]
    p.marginalize_to_prior(0, 50)
    assert p.debug_get("host_waits")[0] == h0      # neither the certificate nor any result came back
    p.get_prior()
    assert p.debug_get("marg_path")[0] == 0.0
    p.close()
    w, _ = _window(pkg, "n186")
    p = pkg.new_problem(); p.upload_window(w); p.optimize(2)
    h0 = p.debug_get("host_waits")[0]
    p.marginalize_to_prior(0, 50)
    assert p.debug_get("host_waits")[0] > h0       # n > 140: the documented blocking path
    p.close()


def test_optimize_straight_after_marginalize_to_prior(pkg, hip):
    w = pkg.window.make_window(12, 260, 50, imu=True, seed=23)
    out = []
    for dev in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        pkg.protocol.local_ba(p)
        if dev:
            p.marginalize_to_prior(0, 50)
        else:
            p.set_prior(p.marginalize(0, 50))
        st = p.optimize(5)
        out.append(((st.iterations, st.trials, st.chi2_initial, st.chi2_final), p.get_keyframes()))
        p.close()
    assert out[0][0] == out[1][0]
    _same_results(out[0][1], out[1][1], "optimize after the prior")


def test_set_prior_after_marginalize_to_prior(pkg, hip):
    w = pkg.window.make_window(12, 260, 50, imu=True, seed=23)
    g = pkg.new_problem(); g.upload_window(w); pkg.protocol.local_ba(g)
    host = g.marginalize(0, 50)
    g.close()
    out = []
    for pending in (True, False):
        p = pkg.new_problem(); p.upload_window(w); pkg.protocol.local_ba(p)
        if pending:
            p.marginalize_to_prior(0, 50)
        p.set_prior(host)
        got = p.get_prior()
        assert got["m"] == 0 and got["Ar"] is None and got["br"] is None
        for k in ("vid", "size", "idx", "x0", "J0", "r0"):
            assert np.array_equal(got[k], host[k]), k
        st = p.optimize(5)
        out.append(((st.iterations, st.trials, st.chi2_final), p.get_keyframes()))
        if pending:
            p.set_prior(None)
            with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_STATE"):
                p.get_prior()
        p.close()
    assert out[0][0] == out[1][0]
    _same_results(out[0][1], out[1][1], "set_prior after marginalize_to_prior")


def test_refused_set_prior_leaves_a_device_made_prior_as_it_was(pkg, hip):
    """plba_set_prior validates before it touches anything: a call refused for a bad `size` entry — once while the marginalization
    that makes the prior is still pending, once after it has been resolved — leaves the device-made prior in place.  plba_get_prior and
    the next two-stage BA are those of a twin handle that never made the refused calls, bit for bit."""
    w = pkg.window.make_window(12, 260, 50, imu=True, seed=23)
    bad = dict(n=15, vid=np.array([0, 1], np.int32), size=np.array([9, 7], np.int32), idx=np.array([0, 9], np.int32),
               x0=np.zeros(16), J0=np.eye(15), r0=np.zeros(15))
    out = []
    for refused in (True, False):
        p = pkg.new_problem(); p.upload_window(w); pkg.protocol.local_ba(p)
        p.marginalize_to_prior(0, 50)
        if refused:
            with pytest.raises(pkg.abi.PlbaError, match="Undefined size of marginalization vertex: 7"):
                p.set_prior(bad)
        first = p.get_prior()
        if refused:
            with pytest.raises(pkg.abi.PlbaError, match="Undefined size of marginalization vertex: 7"):
                p.set_prior(bad)
        again = p.get_prior()
        _same_prior(first, again, "read twice")
        assert first["m"] > 0 and first["Ar"] is not None      # still the device-made one
        _restore_robust(p, w)
        r = pkg.protocol.local_ba(p)
        out.append((first, _stats(r), pkg.protocol.results(p)))
        p.close()
    _same_prior(out[0][0], out[1][0], "after the refused set_prior")
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    _same_results(out[0][2], out[1][2], "BA after the refused set_prior")


def test_refusals(pkg, hip):
    w = pkg.window.make_window(8, 150, 40, imu=True, seed=29)
    p = pkg.new_problem(); p.upload_window(w); pkg.protocol.local_ba(p)
    with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_STATE"):
        p.get_prior()                                   # no prior yet
    p.marginalize_to_prior(0, 50)
    before, kf = p.get_prior(), p.get_keyframes()
    for bad in (-1, 8):
        with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_INVALID"):
            p.marginalize_to_prior(bad, 50)
    _same_prior(before, p.get_prior(), "after a refused first_kf")
    _same_results(kf, p.get_keyframes(), "after a refused first_kf")
    assert p.dims["K"] == 8
    p.close()
    s = pkg.new_problem(); s.upload_window(w)
    s.set_shard(0, 2, lambda buf, n, op, stream: None)
    with pytest.raises(pkg.abi.PlbaError, match="PLBA_ERR_STATE"):
        s.marginalize_to_prior(0, 50)
    s.close()


def test_close_with_a_pending_marginalization_then_a_recycled_handle(pkg, hip):
    w = pkg.window.make_window(12, 260, 50, imu=True, seed=37)
    w2 = pkg.window.make_window(12, 300, 60, imu=True, seed=41)

    def run(p):
        p.upload_window(w2)
        r = pkg.protocol.local_ba(p, marginalize="device")
        return _stats(r), pkg.protocol.results(p), p.get_prior()
    ref = run(pkg.new_problem())
    for _ in range(3):      # (every handle parked by the library is re-used: this pends, closes, and the next create recycles it)
        p = pkg.new_problem(); p.upload_window(w); pkg.protocol.local_ba(p)
        p.marginalize_to_prior(0, 50)
        p.close()
    got = run(pkg.new_problem())
    assert got[0] == ref[0]
    _same_results(got[1], ref[1], "recycled handle")
    _same_prior(got[2], ref[2], "recycled handle")


def test_two_threads_each_carrying_its_own_sequence(pkg, hip):
    K, nwin = 12, 3
    seqs = [pkg.window.make_sequence(K, nwin, 300 + 100 * t, 60, seed=0x9A1D70 + t, kf_dt=0.1) for t in range(2)]
    serial = [_carried(pkg, s, K, nwin, {}, True) for s in seqs]
    par, errs = [None, None], []

    def work(t):
        try:
            par[t] = _carried(pkg, seqs[t], K, nwin, {}, True)
        except Exception as e:      # surfaced below
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for t in range(2):
        _same_sequence(par[t], serial[t])
