"""The rank-k update of the fused Schur pass issues only the MFMAs of tile pairs whose two 16-row blocks hold an observation in the wave
step (lm_schur_group, csrc/plba_lm_dev.h: a ballot of the lanes' observations per window slot; rows 0 - 15 are slots 0 - 2, 16 - 31 slots
2 - 5, 32 - 47 slots 5 - 7).  A wrong mask drops a product that is not zero, so the built system is held stage by stage against the
record-based passes (lm_fused = 0), and the 5 + 10 protocol against the oracle, on the smallest windows where the masks differ:
  short2   6 keyframes, 40 points, every track of length 2: a wave step sees two or three neighbouring slots, most steps one row block;
  mixed    10 keyframes, 60 points + 12 lines, tracks of 2 .. 8 keyframes: one wave step holds units of different masks;
  cross9   9 keyframes, tracks of 2 .. 5: more keyframes than a window has slots, groups that run across first-keyframe buckets."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WINDOWS = {"short2": lambda pkg: pkg.window.make_window(6, 40, 0, imu=True, seed=0xBA1A, track=(2, 2)),
           "mixed": lambda pkg: pkg.window.make_window(10, 60, 12, imu=True, seed=0xBA1B, track=(2, 8)),
           "cross9": lambda pkg: pkg.window.make_window(9, 50, 10, imu=True, seed=0xBA1C, track=(2, 5))}


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def _pose_delta(a, b, pkg):
    dphi = max(np.linalg.norm(pkg.window.log_so3(pkg.window.R_from_quat(qb).T @ pkg.window.R_from_quat(qa))) for qa, qb in zip(a["q"], b["q"]))
    return max(np.abs(a["P"] - b["P"]).max(), np.abs(a["V"] - b["V"]).max(), dphi, np.abs(a["dbg"] - b["dbg"]).max(), np.abs(a["dba"] - b["dba"]).max())


@pytest.mark.parametrize("name", list(WINDOWS))
def test_built_system_against_the_record_based_passes(pkg, hip, name):
    w = WINDOWS[name](pkg)
    g = pkg.new_problem(lm_fused=2); g.upload_window(w)
    r = pkg.new_problem(lm_fused=0); r.upload_window(w)
    g.debug_build(5.0, True); r.debug_build(5.0, True)
    assert g.debug_get("lm_fused")[0] == 1 and r.debug_get("lm_fused")[0] == 0
    if name == "cross9":      # fewer groups than first keyframes with landmarks: some group runs across a bucket boundary
        first_pt = {int(w["po_kf"][w["po_pt"] == i].min()) for i in range(len(w["points"]))}
        first_ln = {int(w["lo_kf"][w["lo_ln"] == i].min()) for i in range(len(w["lines"]))}
        assert g.debug_get("lm_fused")[1] < len(first_pt) + len(first_ln) and len(first_pt) >= 4
    for what in ("chi2", "maxdiag", "err_pt", "err_ln", "hll_pt", "bl_pt", "hll_ln", "bl_ln", "bp", "bschur", "Hschur"):
        d = _rel(g.debug_get(what), r.debug_get(what))
        print(name, what, d)
        assert d < 1e-9, what
    g.close(); r.close()


@pytest.mark.parametrize("name", list(WINDOWS))
def test_protocol_against_the_oracle(pkg, orc, hip, name):
    w = WINDOWS[name](pkg)
    res = {}
    for key, mk in (("fused", lambda: pkg.new_problem(lm_fused=2)), ("oracle", orc.new_problem)):
        q = mk(); q.upload_window(w)
        r = pkg.protocol.local_ba(q)
        res[key] = (r, pkg.protocol.results(q), q.trace(), q.edge_chi2(0)[0].copy()); q.close()
    ro, oo, tro, co = res["oracle"]
    r, out, tr, chi = res["fused"]
    assert r["gated"] == ro["gated"]
    assert [(t["iteration"], t["trial"], t["accepted"]) for t in tr] == [(t["iteration"], t["trial"], t["accepted"]) for t in tro]
    assert r["stage2"].chi2_final == pytest.approx(ro["stage2"].chi2_final, rel=1e-9)
    assert _pose_delta(out, oo, pkg) < 1e-9
    assert np.abs(out["points"] - oo["points"]).max() < 1e-8
    if len(w["lines"]): assert np.abs(out["lines"] - oo["lines"]).max() < 1e-8
    assert _rel(chi, co) < 1e-8
