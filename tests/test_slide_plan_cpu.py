"""The host half of plba_slide_window — plba::slide_plan of pl-inertial-slam_amd/csrc/plba_window.h — compiled with a plain C++
compiler (csrc/plba_window_hostcheck.cpp) and run without a GPU: every check of the call, the keep / drop maps, the merged observation
lists and the complete next window.  The planned window must EQUAL the one window_at() lists next (integers and doubles exactly: the
merge moves numbers, it computes none); a refused plan must leave the resident window as it was, member by member.  The device half
(copies and two gather kernels into buffers of its own) and the bit-for-bit results are tests/test_slide_window.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-inertial-slam_amd", "csrc")
SO = os.path.join(CSRC, "_obj", "libplba_window_hostcheck.so")

VECTORS = dict(vid_pvr=np.int32, vid_bias=np.int32, kf0=np.float64, fix_pvr=np.uint8, fix_bias=np.uint8, pts=np.float64, lns=np.float64,
               pt_fixed=np.uint8, ln_fixed=np.uint8, po_pt=np.int32, po_kf=np.int32, lo_ln=np.int32, lo_kf=np.int32,
               po_uv=np.float64, po_w=np.float64, lo_l=np.float64, lo_w=np.float64, level=np.uint8,
               imu_i=np.int32, imu_j=np.int32, imu_pre=np.float64, imu_ipvr=np.float64, imu_ibias=np.float64)
PLAN = dict(pmap=np.int32, lmap=np.int32, src_lm=np.int32, src_ob=np.int32, kf_add=np.float64, add_lm=np.float64, add_ob=np.float64)
INTS = ("K", "Np", "Nl", "Ep", "El", "M", "have_cam", "carry_pts", "carry_lns", "carry_kf", "carry_po", "carry_lo")
CARRY = INTS[7:]
ERR_INVALID, ERR_NUMERIC = -1, -4


@pytest.fixture(scope="module")
def wc():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(CSRC, "plba_window_hostcheck.cpp")
    deps = [src, os.path.join(CSRC, "plba_window.h"), os.path.join(CSRC, "plba_math.h"), os.path.join(ROOT, "include", "plba.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        # (no HIP include path and no HIP compiler: the header must be standard-library code)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", SO, src])
    lib = C.CDLL(SO)
    lib.wc_new.restype = C.c_void_p
    lib.wc_free.argtypes = [C.c_void_p]
    lib.wc_put.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_long]; lib.wc_put.restype = C.c_long
    lib.wc_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_long]; lib.wc_get.restype = C.c_long
    lib.wc_put_scalars.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wc_get_scalars.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.wc_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_long, C.c_void_p]
    lib.wc_clear_next_keeps_capacity.argtypes = [C.c_void_p]
    return lib


def _host_window(w, carried=False):
    """The plba::Window the plba_set_* entry points make of a window dict (abi.Problem.upload_window): name -> array or scalar."""
    k = w["kf"]
    K = len(k["vid_pvr"])
    kf0 = np.zeros((K, 24))
    for key, c0, n in (("P", 0, 3), ("V", 3, 3), ("q", 6, 4), ("bg", 10, 3), ("ba", 13, 3), ("dbg", 16, 3), ("dba", 19, 3)):
        kf0[:, c0:c0 + n] = k[key]
    im = w["imu"]
    Ep, El = len(w["po_pt"]), len(w["lo_ln"])
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)      # const float& invSigma2 (plba_set_point_obs)
    out = dict(vid_pvr=k["vid_pvr"], vid_bias=k["vid_bias"], kf0=kf0, fix_pvr=k["fixed_pvr"], fix_bias=k["fixed_bias"],
               pts=w["points"], lns=w["lines"], pt_fixed=np.zeros(len(w["points"]), np.uint8), ln_fixed=np.zeros(len(w["lines"]), np.uint8),
               po_pt=w["po_pt"], po_kf=w["po_kf"], lo_ln=w["lo_ln"], lo_kf=w["lo_kf"], po_uv=w["po_uv"], po_w=f32(w["po_w"]), lo_l=w["lo_l"], lo_w=f32(w["lo_w"]),
               level=np.zeros(Ep + El, np.uint8), imu_i=im["kf_i"], imu_j=im["kf_j"], imu_pre=im["preint"], imu_ipvr=im["info_pvr"], imu_ibias=im["info_bias"])
    out = {n: np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=VECTORS[n]) for n, a in out.items()}
    out.update(K=K, Np=len(w["points"]), Nl=len(w["lines"]), Ep=Ep, El=El, M=len(im["kf_i"]), have_cam=1)
    out.update({f: int(carried) for f in CARRY})
    c = w["cam"]
    out["cam"] = np.concatenate([[c["fx"], c["fy"], c["cx"], c["cy"]], np.asarray(c["Rbc"]).reshape(-1), np.asarray(c["Pbc"]).reshape(-1), np.asarray(w["gw"]).reshape(-1)]).astype(np.float64)
    return out


class Check:
    def __init__(self, lib, host):
        self.lib, self.h = lib, lib.wc_new()
        for n in VECTORS:
            assert lib.wc_put(self.h, n.encode(), host[n].ctypes.data, host[n].nbytes) == host[n].nbytes, n
        i12 = np.array([host[f] for f in INTS], np.int32)
        lib.wc_put_scalars(self.h, i12.ctypes.data, host["cam"].ctypes.data)

    def read(self, which):
        """which: 0 the resident window, 1 the planned one, 2 the plan"""
        out = {}
        for n, dt in (PLAN if which == 2 else VECTORS).items():
            nb = self.lib.wc_get(self.h, which, n.encode(), None, 0)
            assert nb >= 0, n
            a = np.zeros(nb // np.dtype(dt).itemsize, dt)
            assert self.lib.wc_get(self.h, which, n.encode(), a.ctypes.data, a.nbytes) == nb
            out[n] = a
        if which != 2:
            i12, d19 = np.zeros(12, np.int32), np.zeros(19)
            self.lib.wc_get_scalars(self.h, which, i12.ctypes.data, d19.ctypes.data)
            out.update({f: int(v) for f, v in zip(INTS, i12)}); out["cam"] = d19
        return out

    def plan(self, pkg, d):
        s, keep = pkg.abi.make_slide(d)
        err = C.create_string_buffer(512)
        kept = np.zeros(2, np.int32)
        rc = self.lib.wc_plan(self.h, C.addressof(s), err, len(err), kept.ctypes.data)
        del keep
        return rc, err.value.decode(), kept

    def close(self):
        self.lib.wc_free(self.h)


def _measurements(plan, cur, nxt, d):
    """measurements and weights of the planned window through the source lists: >= 0 the old array, -(1 + a) the a-th addition (read from
    the PACKED additions the device stage uploads: [uv | w | l | w])"""
    Ea_p, Ea_l = len(d["po_pt"]), len(d["lo_ln"])
    add = plan["add_ob"]
    assert len(add) == max(3 * Ea_p + 4 * Ea_l, 1)
    a_uv, a_wp = add[:2 * Ea_p], add[2 * Ea_p:3 * Ea_p]
    a_l, a_wl = add[3 * Ea_p:3 * Ea_p + 3 * Ea_l], add[3 * Ea_p + 3 * Ea_l:3 * Ea_p + 4 * Ea_l]
    Ep1, El1 = nxt["Ep"], nxt["El"]
    src = plan["src_ob"]
    assert len(src) == max(Ep1 + El1, 1)
    sp, sl = src[:Ep1], src[Ep1:Ep1 + El1]

    def pick(s, old, new, width):
        old, new = old.reshape(-1, width), new.reshape(-1, width)
        assert (s[s >= 0] < len(old)).all() and (-1 - s[s < 0] < len(new)).all()
        out = np.zeros((len(s), width))
        out[s >= 0] = old[s[s >= 0]]; out[s < 0] = new[-1 - s[s < 0]]
        return out.reshape(-1)
    return dict(po_uv=pick(sp, cur["po_uv"], a_uv, 2), po_w=pick(sp, cur["po_w"], a_wp, 1), lo_l=pick(sl, cur["lo_l"], a_l, 3), lo_w=pick(sl, cur["lo_w"], a_wl, 1))


STALE = ("kf0", "pts", "lns", "po_uv", "po_w", "lo_l", "lo_w")      # the device holds the truth after a slide: right size, carry_* set


def _assert_planned(nxt, plan, cur, want, d, what):
    for f in INTS[:7]:
        assert nxt[f] == want[f], (what, f, nxt[f], want[f])
    assert np.array_equal(nxt["cam"], want["cam"]), what
    for n in VECTORS:
        if n in STALE:
            assert len(nxt[n]) == len(want[n]), (what, n)
        else:
            assert nxt[n].dtype == want[n].dtype and np.array_equal(nxt[n], want[n]), (what, n)
    for n in ("kf0", "pts", "lns"):
        assert not nxt[n].any(), (what, n)
    for n, v in _measurements(plan, cur, nxt, d).items():
        assert np.array_equal(v, want[n]), (what, n)
    assert not nxt["level"].any() and len(nxt["level"]) == nxt["Ep"] + nxt["El"], what
    assert all(nxt[f] == 1 for f in CARRY), what


def _same_window(a, b, what):
    for n in list(VECTORS) + ["cam"]:
        assert np.array_equal(a[n], b[n]), (what, n)
    for f in INTS:
        assert a[f] == b[f], (what, f)


@pytest.mark.parametrize("K,Np,Nl,nwin,extra", [(12, 300, 60, 4, dict(kf_dt=0.1)), (8, 150, 40, 3, dict(kf_dt=0.1)), (20, 2500, 500, 4, {}), (50, 10000, 2000, 3, {})])
def test_planned_windows_equal_the_next_window(pkg, wc, K, Np, Nl, nwin, extra):
    W = pkg.window
    seq = W.make_sequence(K, nwin, Np, Nl, seed=0x511DE + K, **extra)
    w_prev = W.window_at(seq, 0, K)
    for i in range(1, nwin):
        w = W.window_at(seq, i, K, prev=w_prev)
        d = W.slide_delta(w_prev, w)
        cur = _host_window(w_prev, carried=i > 1)
        c = Check(wc, cur)
        rc, msg, kept = c.plan(pkg, d)
        assert rc == 0, msg
        nxt, plan, after = c.read(1), c.read(2), c.read(0)
        _same_window(after, cur, "window %d: the resident window" % i)
        want = _host_window(w)
        _assert_planned(nxt, plan, cur, want, d, "window %d" % i)
        # the maps say where the previous window's landmarks went: exactly the ones the next window lists first
        assert np.array_equal(np.flatnonzero(plan["pmap"] >= 0), np.flatnonzero(np.isin(w_prev["ids"]["points"], w["ids"]["points"])))
        assert np.array_equal(np.flatnonzero(plan["lmap"] >= 0), np.flatnonzero(np.isin(w_prev["ids"]["lines"], w["ids"]["lines"])))
        assert (kept[0], kept[1]) == ((plan["pmap"] >= 0).sum(), (plan["lmap"] >= 0).sum())
        # the device stage's other inputs: landmark sources (old slot, points then Np0 + line | addition) and the packed additions
        Np0, Np1, L1 = cur["Np"], nxt["Np"], nxt["Np"] + nxt["Nl"]
        src = plan["src_lm"]
        assert len(src) == max(L1, 1)
        old_lm = np.concatenate([np.pad(cur["pts"].reshape(-1, 3), ((0, 0), (0, 3))), cur["lns"].reshape(-1, 6)])
        new_lm = np.concatenate([np.pad(want["pts"].reshape(-1, 3), ((0, 0), (0, 3))), want["lns"].reshape(-1, 6)])
        add_lm = plan["add_lm"].reshape(-1, 6)
        got = np.where((src >= 0)[:, None], old_lm[np.maximum(src, 0)], add_lm[np.maximum(-1 - src, 0)])[:L1]
        assert np.array_equal(got, new_lm)      # (the kept ones' estimates are the device's on a GPU; here both windows hold the sequence's initial ones)
        assert (src[:Np1][src[:Np1] >= 0] < Np0).all() and (src[Np1:L1][src[Np1:L1] >= 0] >= Np0).all()
        assert np.array_equal(plan["kf_add"].reshape(-1, 24)[:len(d["kf"]["vid_pvr"])], want["kf0"].reshape(-1, 24)[K - d["n_drop"]:])
        if i == nwin - 1:
            assert wc.wc_clear_next_keeps_capacity(c.h) == 1      # Window::clear(): a new Window's state on the same storage
        c.close()
        w_prev = w


def test_plan_with_drop_masks(pkg, wc):
    """observations dropped by mask (a landmark keeps at least two) and one landmark dropped outright, as
    tests/test_slide_window.py::test_slide_at_the_headline_shape_and_with_drop_masks does on the device"""
    W = pkg.window
    K = 12
    seq = W.make_sequence(K, 4, 300, 60, seed=0x511DE + K, kf_dt=0.1)
    w0 = W.window_at(seq, 0, K); w1 = W.window_at(seq, 1, K, prev=w0); w2 = W.window_at(seq, 2, K, prev=w1)
    d = W.slide_delta(w1, w2)
    rng = np.random.default_rng(0x511DE)

    def thin(bad, ob_lm):
        left = np.bincount(ob_lm[bad == 0], minlength=ob_lm.max() + 1)
        bad = bad.copy(); bad[left[ob_lm] < 2] = 0
        return bad
    bad_p = thin((rng.random(len(w1["po_pt"])) < 0.15).astype(np.uint8), w1["po_pt"])
    bad_l = thin((rng.random(len(w1["lo_ln"])) < 0.15).astype(np.uint8), w1["lo_ln"])
    assert bad_p.sum() > 10 and bad_l.sum() > 3
    victim = int(np.flatnonzero(np.isin(w1["ids"]["points"], w2["ids"]["points"]))[5])      # a point that would stay
    keep_add = d["po_pt"] != victim
    for k in ("po_pt", "po_kf", "po_uv", "po_w"):
        d[k] = d[k][keep_add]
    dp = np.zeros(len(w1["points"]), np.uint8); dp[victim] = 1
    d["drop_point"], d["drop_point_obs"], d["drop_line_obs"] = dp, bad_p, bad_l
    cur = _host_window(w1, carried=True)
    c = Check(wc, cur)
    rc, msg, _ = c.plan(pkg, d)
    assert rc == 0, msg
    nxt, plan = c.read(1), c.read(2)
    assert plan["pmap"][victim] == -1
    # the same window by numpy: w2 minus the victim and the masked observations
    wf = dict(w2)
    vic2 = int(np.flatnonzero(w2["ids"]["points"] == w1["ids"]["points"][victim])[0])
    old_obs_p = {int(o): j for j, o in enumerate(w1["ids"]["points_obs"])}
    old_obs_l = {int(o): j for j, o in enumerate(w1["ids"]["lines_obs"])}
    keep_p = np.array([(wf["po_pt"][j] != vic2) and not (int(o) in old_obs_p and bad_p[old_obs_p[int(o)]]) for j, o in enumerate(w2["ids"]["points_obs"])], bool)
    keep_l = np.array([not (int(o) in old_obs_l and bad_l[old_obs_l[int(o)]]) for o in w2["ids"]["lines_obs"]], bool)
    renum = np.cumsum(np.arange(len(wf["points"])) != vic2) - 1
    wf["points"] = np.delete(wf["points"], vic2, axis=0)
    wf["po_pt"] = renum[wf["po_pt"][keep_p]].astype(np.int32); wf["po_kf"] = wf["po_kf"][keep_p]; wf["po_uv"] = wf["po_uv"][keep_p]; wf["po_w"] = wf["po_w"][keep_p]
    wf["lo_ln"] = wf["lo_ln"][keep_l]; wf["lo_kf"] = wf["lo_kf"][keep_l]; wf["lo_l"] = wf["lo_l"][keep_l]; wf["lo_w"] = wf["lo_w"][keep_l]
    _assert_planned(nxt, plan, cur, _host_window(wf), d, "drop masks")
    _same_window(c.read(0), cur, "drop masks: the resident window")
    c.close()


def test_refused_plans_leave_the_resident_window_as_it_was(pkg, wc):
    W = pkg.window
    seq = W.make_sequence(8, 2, 150, 40, seed=0x511DE08, kf_dt=0.1)
    w0 = W.window_at(seq, 0, 8); w1 = W.window_at(seq, 1, 8, prev=w0)
    d = W.slide_delta(w0, w1)
    cur = _host_window(w0)
    c = Check(wc, cur)
    cases = []
    # an added observation of a point seen from the leaving keyframe
    gone = int(w0["po_pt"][np.flatnonzero(w0["po_kf"] == 0)[0]])
    bad = dict(d); bad["po_pt"] = np.concatenate([[gone], d["po_pt"]]).astype(np.int32); bad["po_kf"] = np.concatenate([[3], d["po_kf"]]).astype(np.int32)
    bad["po_uv"] = np.concatenate([[[1.0, 2.0]], d["po_uv"]]); bad["po_w"] = np.concatenate([[1.0], d["po_w"]])
    o = np.argsort(bad["po_pt"], kind="stable")
    for k in ("po_pt", "po_kf", "po_uv", "po_w"):
        bad[k] = bad[k][o]
    cases.append((bad, ERR_INVALID, "leaves the window"))
    # a second observation of a kept point from a keyframe that already sees it
    dup = dict(d); j = int(np.flatnonzero(d["po_pt"] < len(w0["points"]))[0])
    kf_seen = int(w0["po_kf"][np.flatnonzero(w0["po_pt"] == d["po_pt"][j])[-1]]) - 1
    dup["po_kf"] = d["po_kf"].copy(); dup["po_kf"][j] = kf_seen
    cases.append((dup, ERR_INVALID, "observed twice"))
    for nd in (8, -1):
        b = dict(d); b["n_drop"] = nd
        cases.append((b, ERR_INVALID, "counts out of range"))
    uns = dict(d); uns["lo_ln"] = d["lo_ln"].copy(); uns["lo_ln"][[0, -1]] = uns["lo_ln"][[-1, 0]]
    assert uns["lo_ln"][0] > uns["lo_ln"][1]
    cases.append((uns, ERR_INVALID, "added line observations must be sorted by landmark"))
    nan = dict(d); nan["points"] = d["points"].copy(); nan["points"][0, 1] = np.nan
    cases.append((nan, ERR_NUMERIC, "non-finite landmark or observation"))
    inf = dict(d); inf["kf"] = dict(d["kf"]); inf["kf"]["V"] = d["kf"]["V"].copy(); inf["kf"]["V"][0, 2] = np.inf
    cases.append((inf, ERR_NUMERIC, "non-finite keyframe state"))
    desc = dict(d); desc["kf"] = dict(d["kf"]); desc["kf"]["vid_pvr"] = np.array([w0["kf"]["vid_pvr"][-1]], np.int32)
    cases.append((desc, ERR_INVALID, "keyframe vertex ids must be ascending"))
    nob = dict(d); nob["kf"] = dict(d["kf"]); nob["kf"]["vid_bias"] = np.full(len(d["kf"]["vid_pvr"]), -1, np.int32)
    cases.append((nob, ERR_INVALID, "keyframe without bias vertex"))
    for dd, code, text in cases:
        rc, msg, _ = c.plan(pkg, dd)
        assert rc == code and text in msg, (text, rc, msg)
        _same_window(c.read(0), cur, text)
    # and the valid slide still goes through, on the storage the refused ones wrote into
    rc, msg, _ = c.plan(pkg, d)
    assert rc == 0, msg
    _assert_planned(c.read(1), c.read(2), cur, _host_window(w1), d, "after the refusals")
    c.close()
