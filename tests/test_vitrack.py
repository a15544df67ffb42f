"""plba_track_inertial on the device against the wide run of tests/vitrack_ref.py, under track_ref.hold's rule: the states, H, the next
frame's prior information, chi2 and lambda within 8 x the float64 reference's own rounding noise (floor m u |value|, m the active
features), masks, counts, iterations, trials, stop reasons and status exactly.  tests/test_vitrack_cpu.py asserts that every case has the
margin an exact comparison needs and that its noise sample is representative: how the seeds of tests/vitrack_cases.py were chosen."""
import ctypes as C

import numpy as np
import pytest

from . import vitrack_cases as VC
from . import vitrack_ref as VR

pytestmark = pytest.mark.gpu

KEYS = VR.QUANT + VR.EXACT


@pytest.fixture(scope="module")
def prob(pkg, hip):
    p = pkg.new_problem()
    yield p
    p.close()


def _same(a, b, n):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (n, k)
    for x, y in zip(a["pt_inlier"] + a["ln_inlier"], b["pt_inlier"] + b["ln_inlier"]):
        assert np.array_equal(x, y), n


@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_every_case_holds_the_rule(prob, name):
    """the feature counts around the wave (0, 1, 12, 63 / 64 / 65, mixed up to (300, 100)), both anchor modes, the gate with a
    re-admission, a point behind the camera, rejected trials, no round and no iteration, the IMU edge's kernel, SINGULAR"""
    case, r64, rw = VC.runs(name)
    out = VC.call(prob, [case], case["opts"])
    res = VC.as_result(out, 0)
    VR.hold(res, r64, rw, "hip", name, skip=VC.SKIP.get(name, ()))
    assert np.array_equal(res["H"], res["H"].T) and np.array_equal(res["next_prior"], res["next_prior"].T)      # exactly symmetric
    assert res["n_inliers_pt"] == res["pt_in"].sum() and res["n_inliers_ln"] == res["ln_in"].sum()
    if not case["anchor_free"]:      # a fixed anchor comes back bit for bit, its rows and columns of H are zero
        assert np.array_equal(res["state_i"], np.asarray(case["si"], np.float64)) and not res["H"][:15].any() and not res["H"][:, :15].any()
    if name in ("rounds_0", "iters_0"):      # the states bit for bit, H still reported
        assert np.array_equal(res["state_i"], case["si"]) and np.array_equal(res["state_j"], case["sj"]) and res["H"][15:, 15:].any()
    if name == "singular":
        assert res["status"] == VR.SINGULAR and not res["next_prior"].any() and res["H"].any()


def test_chained_frames(prob):
    """frame 2's prior is frame 1's next_prior_info225 and state_j, both as the device returned them"""
    c1 = VC.runs("chain_1")[0]
    first = VC.as_result(VC.call(prob, [c1], c1["opts"]), 0)
    c2 = VC.chain_2(VC.CHAIN_SEED, first)
    _, r64, rw = VC.runs("chain_2")
    VR.hold(VC.as_result(VC.call(prob, [c2], c2["opts"]), 0), r64, rw, "hip", "chain_2")


MIXED = ["fixed_70_30", "free_70_30", "fixed_0_0", "fixed_65_0", "free_300_100"]


def test_batch_of_five_is_the_problems_alone(prob):
    """mixed anchors and sizes in one call: every problem bit-identical to itself called alone"""
    cases = [VC.runs(n)[0] for n in MIXED]
    out = VC.call(prob, cases, VC.OPTS)
    assert list(out["status"]) == [VR.OK] * 5
    for b, (n, c) in enumerate(zip(MIXED, cases)):
        alone = VC.call(prob, [c], VC.OPTS)
        for k in KEYS:
            assert np.array_equal(out[k][b], alone[k][0]), (n, k)
        assert np.array_equal(out["pt_inlier"][b], alone["pt_inlier"][0]) and np.array_equal(out["ln_inlier"][b], alone["ln_inlier"][0]), n


def test_two_calls_give_the_same_bits(prob):
    cases = [VC.runs(n)[0] for n in ("free_300_100", "fixed_70_30", "gate_free")]
    o = VC.runs("gate_free")[0]["opts"]
    _same(VC.call(prob, cases, o), VC.call(prob, cases, o), "twice")


def test_window_state_untouched_and_one_wait(pkg, hip):
    """a resident window's next plba_optimize is bit-identical with and without a plba_track_inertial call in between, and the call
    makes one blocking wait"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imu_small.json")) as f:
        c = json.load(f)["meta"]
    w = pkg.window.make_window(c["K"], c["Np"], c["Nl"], imu=c["imu"], seed=c["seed"])
    case = VC.runs("free_70_30")[0]
    res = []
    for with_call in (False, True):
        p = pkg.new_problem(); p.upload_window(w)
        p.recompute_errors()
        if with_call:
            for _ in range(2):
                before = p.debug_get("host_waits")[0]
                out = VC.call(p, [case], case["opts"])
                assert p.debug_get("host_waits")[0] == before + 1
            assert out["status"][0] == VR.OK
        st = p.optimize(5)
        res.append((p.get_keyframes(), p.get_points(), p.get_lines(), st.chi2_final, st.iterations, [t["chi2_trial"] for t in p.trace()]))
        p.close()
    a, b = res
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]


def test_refusals_leave_the_outputs_untouched(pkg, prob):
    abi = pkg.abi
    case = VC.runs("free_70_30")[0]
    f = lambda k, n: np.ascontiguousarray(np.asarray(case[k], np.float64).reshape(-1, n))
    A = dict(si=f("si", 22), sj=f("sj", 22), pre=f("pre", 142), ip=f("ipvr", 81), ib=f("ibias", 36), pst=f("pst", 22), pi=f("pinfo", 225), gw=f("gw", 3),
             P=f("Pw", 3), uv=f("uv", 2), wp=f("pt_w", 1), pq=f("pq", 6), l3=f("l3", 3), wl=f("ln_w", 1), Rbc=f("Rbc", 9), Pbc=f("Pbc", 3))
    Np, Nl = len(A["P"]), len(A["pq"])
    dp, ip, up = abi._dp, abi._ip, abi._up

    def attempt(B=1, ps=np.array([0, Np], np.int32), ls=np.array([0, Nl], np.int32), af=np.array([1, 1], np.uint8), opt=True, out=True, cam=VC.CAM, o=None, **repl):
        a = dict(A); a.update(repl)
        op = abi.VitrackOptions()
        prob.lib.fn["vitrack_default_options"](C.byref(op))
        for k, v in (o or {}).items():
            setattr(op, k, v)
        res = (abi.VitrackResult * 2)()
        C.memset(res, 0x5A, C.sizeof(res))
        pm, lm = np.full(Np, 7, np.uint8), np.full(Nl, 7, np.uint8)
        rc = prob.lib.fn["track_inertial"](prob._h, C.byref(op) if opt else None, B, up(af), dp(a["si"]), dp(a["sj"]), dp(a["pre"]), dp(a["ip"]), dp(a["ib"]), dp(a["pst"]),
                                           dp(a["pi"]), dp(a["gw"]), ip(ps), dp(a["P"]), dp(a["uv"]), dp(a["wp"]), ip(ls), dp(a["pq"]), dp(a["l3"]), dp(a["wl"]),
                                           *[float(v) for v in cam], dp(a["Rbc"]), dp(a["Pbc"]), up(pm), up(lm), res if out else None)
        assert rc == -1, rc      # PLBA_ERR_INVALID
        assert bytes(res) == b"\x5a" * C.sizeof(res) and (pm == 7).all() and (lm == 7).all()

    def spoiled(k, value=np.nan):
        v = A[k].copy(); v.flat[min(5, v.size - 1)] = value
        return {k: v}
    attempt(B=0)
    attempt(ps=np.array([0, -1], np.int32))
    attempt(ps=np.array([1, Np], np.int32))
    attempt(ls=np.array([0, -3], np.int32))
    for k in ("P", "uv", "wp", "pq", "l3", "wl", "si", "sj", "pre", "ip", "ib", "gw", "Rbc", "Pbc"):
        attempt(**{k: None})
    attempt(out=False)
    attempt(opt=False)
    attempt(pst=None)      # a free anchor without the prior arrays
    attempt(pi=None)
    for k in ("P", "uv", "wp", "pq", "l3", "wl", "si", "sj", "pre", "ip", "ib", "pst", "pi", "gw", "Rbc", "Pbc"):
        attempt(**spoiled(k))
    attempt(**spoiled("wp", -1.0))
    attempt(**spoiled("wl", -1.0))
    attempt(cam=(458.0, float("inf"), 367.0, 248.0))
    for o in (dict(rounds=-1), dict(rounds=9), dict(iters=-1), dict(max_trials=-1), dict(robust_rounds=-1), dict(tau=float("nan")), dict(huber_imu=float("inf")),
              dict(chi2_pt=float("nan")), dict(user_lambda_init=float("nan"))):
        attempt(o=o)
    assert VC.call(prob, [case], case["opts"])["status"][0] == VR.OK      # the handle still works
