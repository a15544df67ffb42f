"""The harness of the sharded exactness tests (tests/shard_exact.py) held to its conditions on the references alone, without a GPU:
  * the fp64 oracle's own sharded mode, run as W threads through the same in-process exchange and merged by the same merge(), passes
    build_exact.hold() against the same fixtures and noise, for every (case, world, lambda, cut) the device is run at — which checks
    the exchange, the cuts and the merge, and shows that the reference itself stays within the rule when sharded.  What does not pass
    here is recorded in shard_exact.DROPPED by name, before any device runs;
  * merge() of an unsharded result cut into W pieces by hand is that result (numpy only);
  * the explicit cuts partition the landmarks exactly and have the shapes their names promise."""
import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC
from . import shard_exact as SX


def test_the_run_list():
    """every case at world 3; the five cases of worlds 2 and 8; at most two runs left out and no case at every world"""
    assert {r[0] for r in SX.RUNS if r[1] == 3 and r[3] is None} == set(BC.OLD)
    for W in (2, 8):
        assert {r[0] for r in SX.RUNS if r[1] == W} == {"k6", "prior13", "fixed8", "noimu7", "k14_lines"}
        assert {r[2] for r in SX.RUNS if r[1] == W and r[0] == "k6"} == {"init", 5.0, 0.05}
    assert {(r[0], r[3]) for r in SX.RUNS if r[3]} == {(n, k) for n in ("k6", "steps3") for k in SX.EDGE_KINDS}
    assert len(SX.RUNS) == len(set(SX.RUNS)) and set(SX.DROPPED) <= set(SX.RUNS) and len(SX.DROPPED) <= 2
    for name in {r[0] for r in SX.DROPPED}:
        assert {r[1] for r in SX.RUNS if r[0] == name and r not in SX.DROPPED}, name
    for name, W, label, kind in SX.RUNS:
        assert (name, label) not in BC.DROPPED and label in BC.CASES[name]["lambdas"]


@pytest.mark.parametrize("run", SX.RUNS, ids=[SX.run_id(r) for r in SX.RUNS])
def test_the_sharded_oracle_passes_the_rule(pkg, orc, run):
    name, W, label, kind = run
    fx, w = SX.load_case(pkg.window, name)
    i = SX.lambda_index(name, label)
    lam = float(fx["lams"][i])
    ref, tq, _, noise, decided = BX.load(fx, w, i)
    cut = SX.edge_cut(pkg.window, w, kind) if kind else None
    per_rank, shards = SX.run_sharded(orc.new_problem, w, W, lam, cut=cut, window_module=pkg.window, distributed=pkg.distributed)
    merged = SX.merge(per_rank, w, shards)
    if run in SX.DROPPED:      # (the verdict is kept honest: a run recorded as left out does fail here)
        with pytest.raises(AssertionError):
            BX.hold(merged, ref, noise, "oracle64 world %d" % W, SX.run_id(run), trial=(merged["trial"], tq, decided))
        return
    BX.hold(merged, ref, noise, "oracle64 world %d" % W, SX.run_id(run), trial=(merged["trial"], tq, decided))


# ---- merge() ----------------------------------------------------------------------------------------------------------------------------
def _fake_result(w, P, rng):
    """arrays of the shapes build_exact.read() returns for `w`, random"""
    lay = BX.layout(w)
    M = 0 if w.get("imu") is None else len(w["imu"]["kf_i"])
    n = dict(chi2=1, maxdiag=1, err_pt=2 * len(w["po_pt"]), err_ln=3 * len(w["lo_ln"]), err_pvr=9 * M, err_bias=6 * M, err_prior=0,
             hll_pt=9 * lay["Np"], bl_pt=3 * lay["Np"], hll_ln=36 * lay["Nl"], bl_ln=6 * lay["Nl"], bp=P, bschur=P, Hschur=P * P,
             x=P + 3 * int(lay["free_pt"].sum()) + 6 * int(lay["free_ln"].sum()))
    r = {k: rng.standard_normal(v) for k, v in n.items()}
    r["P"] = P
    r["trial"] = rng.standard_normal(4)
    return r, lay


def _cut_by_hand(full, lay, w, shards):
    """what each rank of a sharded run would return if the run computed `full`"""
    out = []
    P = full["P"]
    xp = full["x"][P:P + 3 * int(lay["free_pt"].sum())].reshape(-1, 3)
    xl = full["x"][P + xp.size:].reshape(-1, 6)
    slot_p, slot_l = np.cumsum(lay["free_pt"]) - 1, np.cumsum(lay["free_ln"]) - 1
    for r, s in enumerate(shards):
        pi, li = s["shard"]["pt_index"], s["shard"]["ln_index"]
        mine_p, mine_l = np.isin(w["po_pt"], pi), np.isin(w["lo_ln"], li)
        d = {k: full[k].copy() for k in SX.GLOBAL}
        d["P"], d["trial"] = P, full["trial"].copy()
        for k in SX.RANK0:
            d[k] = full[k].copy() if r == 0 else np.zeros_like(full[k])
        d["err_pt"] = full["err_pt"].reshape(-1, 2)[mine_p].ravel()
        d["err_ln"] = full["err_ln"].reshape(-1, 3)[mine_l].ravel()
        for k, n, idx in (("hll_pt", 9, pi), ("bl_pt", 3, pi), ("hll_ln", 36, li), ("bl_ln", 6, li)):
            d[k] = full[k].reshape(-1, n)[idx].ravel()
        fp, fl = [j for j in pi if lay["free_pt"][j]], [j for j in li if lay["free_ln"][j]]
        d["x"] = np.concatenate([full["x"][:P], xp[slot_p[fp]].ravel() if fp else np.zeros(0), xl[slot_l[fl]].ravel() if fl else np.zeros(0)])
        out.append(d)
    return out


@pytest.mark.parametrize("W", [1, 3, 8])
def test_merge_of_a_result_cut_by_hand_is_the_result(pkg, W):
    w = pkg.window.make_window(6, 101, 23, imu=True, seed=3)
    w["point_fixed"] = np.zeros(101, np.uint8); w["point_fixed"][4::9] = 1
    w["line_fixed"] = np.zeros(23, np.uint8); w["line_fixed"][2::5] = 1
    full, lay = _fake_result(w, 90, np.random.default_rng(W))
    for cut in (None, "by_index"):
        shards = SX.shards_of(pkg.window, w, W, by="index" if cut else "time")
        merged = SX.merge(_cut_by_hand(full, lay, w, shards), w, shards)
        assert set(merged) == set(full)
        for k in full:
            assert np.array_equal(merged[k], full[k]), (W, cut, k)
    # and merge() sees what it is there to see: a global quantity that differs on one rank, a landmark two ranks claim
    if W > 1:
        shards = SX.shards_of(pkg.window, w, W)
        parts = _cut_by_hand(full, lay, w, shards)
        parts[W - 1]["Hschur"][7] = np.nextafter(parts[W - 1]["Hschur"][7], 1.0)
        with pytest.raises(AssertionError, match="Hschur differs"):
            SX.merge(parts, w, shards)
        parts = _cut_by_hand(full, lay, w, shards)
        parts[1]["err_pvr"][0] = 1e-300
        with pytest.raises(AssertionError, match="owns no pose-side edge"):
            SX.merge(parts, w, shards)
        twice = [dict(s) for s in shards]
        twice[1] = dict(shards[1], shard=dict(shards[1]["shard"], pt_index=shards[0]["shard"]["pt_index"][:len(shards[1]["shard"]["pt_index"])]))
        if len(twice[1]["shard"]["pt_index"]) == len(shards[1]["shard"]["pt_index"]):
            with pytest.raises(AssertionError):
                SX.merge(_cut_by_hand(full, lay, w, shards), w, twice)


# ---- the explicit cuts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k6", "steps3"])
@pytest.mark.parametrize("kind", SX.EDGE_KINDS)
def test_the_explicit_cuts_partition_the_landmarks(pkg, name, kind):
    _, w = SX.load_case(pkg.window, name)
    cut = SX.edge_cut(pkg.window, w, kind)
    shards = SX.shards_of(pkg.window, w, 3, cut)
    Np, Nl = len(w["points"]), len(w["lines"])
    assert np.array_equal(np.sort(np.concatenate([s["shard"]["pt_index"] for s in shards])), np.arange(Np))
    assert np.array_equal(np.sort(np.concatenate([s["shard"]["ln_index"] for s in shards])), np.arange(Nl))
    assert sum(len(s["po_pt"]) for s in shards) == len(w["po_pt"]) and sum(len(s["lo_ln"]) for s in shards) == len(w["lo_ln"])
    for s in shards:
        assert s["imu"] is w["imu"] and (np.diff(s["po_pt"]) >= 0).all() and (np.diff(s["lo_ln"]) >= 0).all()
        assert len(s["points"]) == len(s["shard"]["pt_index"]) and len(s["lines"]) == len(s["shard"]["ln_index"])
    n_obs = [len(s["po_pt"]) + len(s["lo_ln"]) for s in shards]
    assert all(n > 0 for n in n_obs) == SX.EVERY_RANK_HAS_OBSERVATIONS[kind]
    if kind == "empty_rank":
        assert len(shards[1]["points"]) == len(shards[1]["lines"]) == 0 and n_obs[0] and n_obs[2]
    elif kind == "rank0_empty":
        assert len(shards[0]["points"]) == len(shards[0]["lines"]) == 0 and n_obs[1] and n_obs[2]
    elif kind == "lines_on_one_rank":
        assert len(shards[1]["lines"]) == Nl and len(shards[1]["points"]) == 0 and len(shards[0]["lines"]) == len(shards[2]["lines"]) == 0
    else:
        first = pkg.window._first_kf(w["po_pt"].astype(np.int64), w["po_kf"].astype(np.int64), Np)
        mine = shards[1]["shard"]["pt_index"]
        assert len(mine) and len(set(first[mine])) == 1 and len(shards[1]["lines"]) == 0
        assert not (first[np.concatenate([shards[0]["shard"]["pt_index"], shards[2]["shard"]["pt_index"]])] == first[mine[0]]).any()


# SHA-256 (first 16 hex digits) over dtype, shape and bytes of a shard's landmark and observation arrays and its two index lists, taken
# from window.shard_window BEFORE it was split into shard_pick and shard_cut: make_window(6, 101, 23, imu=True, seed=3), three ranks
SHARDS_BEFORE_THE_SPLIT = {("time", 0): "cc9be683902350c5", ("time", 1): "d54ab53d73b586da", ("time", 2): "51902accb1a1a173",
                           ("index", 0): "c9c53a27322f5f17", ("index", 1): "1f7d1593cbb3ce7e", ("index", 2): "c12725142b513b1a"}
_SHARD_KEYS = ("points", "lines", "po_pt", "po_kf", "po_uv", "po_w", "lo_ln", "lo_kf", "lo_l", "lo_w")


def _shard_sha(s):
    import hashlib
    h = hashlib.sha256()
    for a in [s[k] for k in _SHARD_KEYS] + [s["shard"]["pt_index"], s["shard"]["ln_index"]]:
        a = np.ascontiguousarray(a)
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()[:16]


def test_shard_window_returns_what_it_returned_before_the_split(pkg):
    """window.shard_window, now shard_pick followed by shard_cut, gives the shards it gave as one function (pinned hashes), replicates
    what it replicated, and its two halves put together by hand give the same"""
    w = pkg.window.make_window(6, 101, 23, imu=True, seed=3)
    for by in ("time", "index"):
        for r in range(3):
            s = pkg.window.shard_window(w, r, 3, by=by)
            assert _shard_sha(s) == SHARDS_BEFORE_THE_SPLIT[(by, r)], (by, r)
            assert s["shard"]["rank"] == r and s["shard"]["world"] == 3 and s["shard"]["by"] == by
            assert set(s) == set(w) | {"shard"} and all(s[k] is w[k] for k in w if k not in _SHARD_KEYS + ("point_fixed", "line_fixed"))
            pi, li = pkg.window.shard_pick(w, r, 3, by)
            assert _shard_sha(pkg.window.shard_cut(w, pi, li, r, 3, by)) == SHARDS_BEFORE_THE_SPLIT[(by, r)]
