"""The references of the marginalization exactness tests, held to their own conditions without a GPU (tests/marg_quad.py states the rule
and conditions (1) - (5); tests/marg_quad_cases.py the windows), and the power of the rule: four corruptions of a passing fp64 result,
each of which hold() rejects, with a record of which of them the comparisons in use accept."""
import os

import numpy as np
import pytest

from . import marg_quad as MQ
from . import marg_quad_cases as MC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIMIT = 159120      # tests/golden/build_exact_prior13.npz, the largest npz committed before these
SMALLEST = "lines_only"      # condition (1): recomputed in full through mpmath
_CACHE = {}


def _case(pkg, orc, name):
    if name not in _CACHE:
        fx, ref = MQ.load(name, GOLDEN)
        case = MC.CASES[name]
        w = case["make"](pkg.window, ref.prior)
        ne, sv = MQ.evaluations(orc, w, case)
        _CACHE[name] = (fx, ref, w, ne, sv)
    return _CACHE[name]


def test_the_case_list(pkg):
    """a fixture for every case and for nothing else, none above the size limit; and each window has the shape it is listed for"""
    have = {f[len("marg_quad_"):-4] for f in os.listdir(GOLDEN) if f.startswith("marg_quad_") and f.endswith(".npz")}
    assert have == set(MC.CASES)
    refs = {}
    for name in MC.CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "marg_quad_%s.npz" % name)) <= LIMIT, name
        refs[name] = MQ.load(name, GOLDEN)[1]
    for name, n in MC.N_EXPECT.items():
        assert refs[name].L.n == n, (name, refs[name].L.n)
    assert refs["m15"].L.m == 15 and refs["noimu"].L.m % 3 == 0 and not (refs["noimu"].size == 6).any()
    kinds = {name: set(r.canon[2].tolist()) for name, r in refs.items()}
    P, L = MQ.KIND["point"], MQ.KIND["line"]
    assert L not in kinds["points_only"] and P in kinds["points_only"] and P not in kinds["lines_only"] and L in kinds["lines_only"]
    assert not kinds["m15"] & {P, L} and MQ.KIND["pvr"] not in kinds["noimu"]
    # the chained windows: the prior's error at the state is not 0; chain_drop's prior holds the dropped keyframe's two vertices;
    # chain_lone's holds a kept vertex that only the prior's rows touch; chain_n105 has n > 100
    for name in ("chain_drop", "chain_lone", "chain_n105"):
        r = refs[name]
        J, rr, k, _ = r.canon
        assert r.prior is not None and np.abs(rr[k == MQ.KIND["prior"]] - r.prior["r0"]).max() > 1e-3, name
    r = refs["chain_drop"]
    dropped_kf = set(r.L.pid[(r.L.drop == 1) & (r.L.pid < MQ.PT0)].tolist())
    assert len(dropped_kf) == 2 and dropped_kf <= set(r.prior["vid"].tolist())
    r = refs["chain_lone"]
    J, _, k, _ = r.canon
    lone = [int(v) for v, o, s in zip(r.L.pid, r.L.off, r.L.size) if v in r.prior["vid"] and not J[k != MQ.KIND["prior"], o:o + s].any() and J[:, o:o + s].any()]
    assert lone, "no vertex that only the old prior touches"
    assert refs["chain_n105"].L.n > 100
    # cap3: the fourth edge of each kind is not the last of its landmark's run
    w = MC.CASES["cap3"]["make"](pkg.window, None)
    for sel, ob_lm in zip(MQ.selected(w, 3), (w["po_pt"], w["lo_ln"])):
        last = np.flatnonzero(sel)[-1]
        assert sel.sum() == 4 and last + 1 < len(ob_lm) and ob_lm[last + 1] == ob_lm[last], "the cut does not fall inside a run"
    # once: a selected point and a selected line with one observation
    w = MC.CASES["once"]["make"](pkg.window, None)
    for sel, ob_lm in zip(MQ.selected(w, 50), (w["po_pt"], w["lo_ln"])):
        assert (np.bincount(ob_lm[sel]) == 1).any()
    # where a formed landmark block does not resolve a kept eigenvalue (the device's certificate then takes the dense path): once and
    # lines_only, and far1e2, which is dense for its eigenvalues at the threshold anyway
    assert {n for n, r in refs.items() if MQ.unresolved_blocks(r)} == {"far1e2", "lines_only", "once"}
    assert refs["eps1e3"].eps == 1e3 and all(refs[n].eps == 1e-8 for n in MC.CASES if n != "eps1e3")


@pytest.mark.parametrize("name", list(MC.CASES))
def test_references(pkg, orc, name):
    fx, ref, w, ne, sv = _case(pkg, orc, name)
    case = MC.CASES[name]
    assert MC.window_sha(w) == str(fx["sha_window"]), "the window generator gives another window than the one the fixture was made from"
    # (1) the inputs of the fixture are what the quad build computes now (and the prior it carries what the fp64 oracle computes now)
    q = MQ.quad_inputs(orc, w, case)
    assert MQ.sha(q["J"], q["J_lo"]) == str(fx["sha_J"]) and MQ.sha(q["r"], q["r_lo"]) == str(fx["sha_r"])
    assert np.array_equal(q["L"].raw, fx["layout"]) and np.array_equal(q["J"], ref.J) and np.array_equal(q["r"], ref.r)
    for k in ("x0", "vid", "size", "idx"):
        assert np.array_equal(q[k], fx[k]), k
    if case["prior_of"]:
        src = MC.CASES[case["prior_of"]]
        pr = MQ.reference_prior(orc, src["make"](pkg.window, None), src)
        assert MQ.sha(*[np.asarray(pr[k]) for k in ("n", "vid", "size", "idx", "x0", "J0", "r0")]) == str(fx["sha_prior"])
        n0 = pr["n"]
        assert np.array_equal(ref.J[ref.L.R - n0:], MQ.prior_rows(pr, ref.L))      # the copied rows, against the J0 that was fed in
    # (2) the caps: what is compared has FACTOR x noise under its cap, and the file says which yardstick applies
    names = [str(s) for s in fx["noise_names"]]
    assert [str(ref.yard(k)) for k in names] == [str(s) for s in fx["yard"]]
    for k in names:
        if ref.yard(k) is not None:
            assert MQ.FACTOR * ref.noise(k) <= (MQ.CAP_R0R0 if k == "r0r0" else MQ.CAP), (name, k, ref.noise(k))
    # (4) no eigenvalue within MARGIN x its noise of the threshold (Amm: or the case is rejected; A': or the prior's quantities are skipped)
    assert MQ.decided(ref.lam_mm, fx["lam_mm_noise"], ref.eps), name
    assert MQ.decided(ref.lam_r, fx["lam_r_noise"], ref.eps) == ref.decided_r
    nm, nr = MQ.lam_noise(sv, ref)
    assert MQ.decided(ref.lam_mm, nm, ref.eps) and MQ.decided(ref.lam_r, nr, ref.eps) == ref.decided_r
    # (3) the fp64 oracle passes where its own noise is the yardstick, the SVD form where its is.  (Where the oracle's noise is the
    # yardstick the SVD form need not be within 8 x of it: the oracle's Jacobi sweeps resolve the projected b' of the full-track windows
    # 45 times finer than LAPACK's SVD does — J0tr0 of k12full: 2.4e3 u against 1.1e5 u.  There it is held to 8 x its own noise.)
    MQ.hold(ne[0], ref, "oracle64", name, skip=[k for k in MQ.SCHUR if ref.yard(k) != "ne"])
    svd = dict(sv[0], vid=ref.vid, size=ref.size, idx=ref.idx)
    fig = MQ.hold(svd, ref, "svd_form", name, skip=[k for k in MQ.SCHUR if ref.yard(k) != "svd"])
    assert set(fig) == {k for k in MQ.SCHUR if ref.yard(k) == "svd"}
    err = MQ.errors(svd, ref, exact=False)
    for k in MQ.SCHUR:
        if ref.yard(k) == "ne":
            assert err[k] <= max(MQ.FACTOR * max(ref.noise_ne[k], ref.noise_svd[k]), max(64, ref.L.R) * MQ.U), (name, k, err[k])


def test_the_smallest_case_recomputed_in_full(pkg, orc):
    """condition (1), second half: quad run, 50-digit evaluation and the oracle's noise, all anew"""
    fx = MQ.load(SMALLEST, GOLDEN)[0]
    now = MQ.generate(SMALLEST, pkg.window, orc, None)
    assert sorted(now) == sorted(fx)
    for k in fx:
        if k in ("noise_svd", "lam_mm_noise", "lam_r_noise"):      # (LAPACK's figures: close, not bit for bit, on another machine)
            assert np.allclose(now[k], fx[k], rtol=0.5, atol=64 * MQ.U), k
        else:
            assert np.array_equal(now[k], fx[k]), k


# ---- (5) the power of the rule -----------------------------------------------------------------------------------------------------------
def _bars(res, ref):
    """what the comparisons in use make of a result: (max-norm distance of A', accepted at 1e-7 (_marg_compare), accepted at 1e-10)"""
    e = float(np.abs(res["Ar"] - ref.Ar).max() / np.abs(ref.Ar).max())
    return e, e < 1e-7, e < 1e-10


def _rejected(res, ref, qs=("Ar", "br")):
    """[(quantity, error / tolerance)] of what the rule rejects of `res` (A' and b': what a recomputation from a corrupted J changes first)"""
    err = MQ.errors(res, ref, exact=False)
    return [(q, err[q] / ref.tol(q)) for q in qs if q in err and ref.yard(q) is not None and not err[q] <= ref.tol(q)]


def _svd_result(J, r, ref):
    return dict(MQ.svd_form(J, r, ref.L.m, ref.eps), vid=ref.vid, size=ref.size, idx=ref.idx)


def _blockwise(J, r, L, eps):
    """the block-by-block pseudo-inverse elimination (landmark blocks one at a time, then the keyframe block), in fp64"""
    A, b = J.T @ J, J.T @ r
    blocks = [np.arange(o, o + s) for v, o, s, d in zip(L.pid, L.off, L.size, L.drop) if d and v >= MQ.PT0]
    blocks.append(np.concatenate([np.arange(o, o + s) for v, o, s, d in zip(L.pid, L.off, L.size, L.drop) if d and v < MQ.PT0]))
    for B in blocks:
        w, V = np.linalg.eigh(A[np.ix_(B, B)])
        k = w > eps
        P = (V[:, k] / w[k]) @ V[:, k].T
        T = A[:, B] @ P
        b = b - T @ b[B]
        A = A - T @ A[B, :]
    return dict(Ar=0.5 * (A[L.m:, L.m:] + A[L.m:, L.m:].T), br=b[L.m:])


def test_the_rule_rejects_what_the_bars_in_use_accept(pkg, orc):
    record = {}
    # (a) one off-diagonal kept block of A' times 1 + 1e-6, on the 12-keyframe window
    fx, ref, w, ne, sv = _case(pkg, orc, "k12full")
    base = _svd_result(ne[0]["J"], ne[0]["r"], ref)
    assert not _rejected(base, ref) and not _rejected(ne[0], ref, MQ.SCHUR)
    # (every off-diagonal vertex-pair block in turn; the one recorded is the median block by its largest entry, as in the issue's figures.
    # Measured: the rule rejects 57 of the 66 nonzero blocks — those it lets through are coupled below 1e-3 of d_i d_j, where 1e-6 of the
    # block is under the fp64 oracle's own noise — and _marg_compare's 1e-7 accepts 40, the median block among them.)
    trials = []
    for a in range(len(ref.vid)):
        for b in range(a):
            i, j, si, sj = int(ref.idx[a]), int(ref.idx[b]), int(ref.size[a]), int(ref.size[b])
            if not ref.Ar[i:i + si, j:j + sj].any():
                continue
            bad = dict(ne[0], Ar=ne[0]["Ar"].copy())      # the fp64 oracle's own result, one block scaled
            bad["Ar"][i:i + si, j:j + sj] *= 1 + 1e-6; bad["Ar"][j:j + sj, i:i + si] *= 1 + 1e-6
            rej = _rejected(bad, ref, MQ.SCHUR)
            assert not rej or rej[0][0] == "Ar"
            trials.append((float(np.abs(ref.Ar[i:i + si, j:j + sj]).max()), _bars(bad, ref) + (rej[0][1] if rej else 0.0,)))
    trials.sort()
    print("block x (1 + 1e-6): %d blocks, the rule rejects %d, 1e-7 accepts %d, 1e-10 accepts %d" % (
        len(trials), sum(t[1][3] > 1 for t in trials), sum(t[1][1] for t in trials), sum(t[1][2] for t in trials)))
    assert 2 * sum(t[1][3] > 1 for t in trials) > len(trials)
    record["block x (1 + 1e-6)"] = trials[len(trials) // 2][1]
    assert record["block x (1 + 1e-6)"][3] > 1, "the median block scaled by 1 + 1e-6 passes the rule"
    # (b) the rotation columns of one point factor rounded to fp32 before A is formed
    J = ne[0]["J"].copy()
    Jc, _, kinds, keys = ref.canon
    row = np.flatnonzero((np.abs(J) > 0)[:, ref.L.owner >= 0].any(axis=1) & (np.arange(ref.L.R) >= 15))[0]      # the first observation row
    kfcols = [c for c in np.flatnonzero(J[row]) if ref.L.pid[ref.L.owner[c]] < MQ.PT0]
    rot = kfcols[-3:]      # a PVR block is (P, V, R): its last three columns
    for rr in (row, row + 1):
        J[rr, rot] = J[rr, rot].astype(np.float32)
    bad = _svd_result(J, ne[0]["r"], ref)
    rej = _rejected(bad, ref)
    assert rej, "fp32 rotation columns pass the rule"
    record["fp32 rotation columns"] = _bars(bad, ref) + (max(x for _, x in rej),)
    # (c) one prior vertex's rows left out, on the chained window where a vertex is held by the prior alone
    fx, ref, w, ne, sv = _case(pkg, orc, "chain_lone")
    assert not _rejected(_svd_result(ne[0]["J"], ne[0]["r"], ref), ref)
    n0, worst = ref.prior["n"], None
    for v in range(len(ref.prior["vid"])):      # every kept vertex of the prior in turn; recorded: the one the max norm is kindest to
        if int(ref.prior["vid"][v]) not in ref.vid:
            continue
        J = ne[0]["J"].copy()
        o = ref.L.off[list(ref.L.pid).index(int(ref.prior["vid"][v]))]
        J[ref.L.R - n0:, o:o + int(ref.prior["size"][v])] = 0
        bad = _svd_result(J, ne[0]["r"], ref)
        rej = _rejected(bad, ref)
        assert rej, "a prior vertex left out passes the rule"
        t = _bars(bad, ref) + (max(x for _, x in rej),)
        worst = t if worst is None or t[0] < worst[0] else worst
    record["prior vertex left out"] = worst
    # (d) the block-wise pseudo-inverse instead of the dense one, where landmarks are far
    fx, ref, w, ne, sv = _case(pkg, orc, "far1e3")
    bad = _blockwise(ne[0]["J"], ne[0]["r"], ref.L, ref.eps)
    rej = _rejected(bad, ref)
    assert rej, "the block-wise pseudo-inverse passes the rule on far landmarks"
    record["block-wise pseudo-inverse, far1e3"] = _bars(bad, ref) + (max(x for _, x in rej),)
    # (and where the GPU test expects the dense path beyond the far windows: marg_eps = 1e3 discards directions that are no block-local
    # null spaces, so the block-wise form is not the reference's there)
    fx, ref, w, ne, sv = _case(pkg, orc, "eps1e3")
    assert _rejected(_blockwise(ne[0]["J"], ne[0]["r"], ref.L, ref.eps), ref), "the block-wise pseudo-inverse passes the rule at marg_eps = 1e3"
    for k, (e, a7, a10, x) in record.items():
        print("%-36s max-norm %.2e  accepted at 1e-7: %s  at 1e-10: %s   rule: error / tolerance %.3g" % (k, e, a7, a10, x))
    # what DESIGN.md 6d records: the 1e-7 bar of _marg_compare accepts the first of these
    assert record["block x (1 + 1e-6)"][1]
