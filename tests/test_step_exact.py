"""The state plba_optimize leaves behind — the retraction of every keyframe route (update_kf_one from k_update_kf and from the solve
launches, update_kf_vals from the chain segments' back-substitution, the IMU edge blocks' own trial states), the landmark adds, the
publish, the accept and the restore — against the quad-precision run of the oracle, in the coordinates of the step and the scaled norm
of tests/build_exact.py, within 32 x the fp64 oracle's own distance to that run; the decisions and the trace values of every trial; and
the conditions that hold to the bit: what has no free vertex does not move, a call all of whose trials are rejected leaves the upload.
tests/step_exact.py is the rule, tests/step_exact_cases.py the sequences; the references are the fixtures
tests/golden/step_exact_<case>.npz beside build_exact_<case>.npz (tests/golden/make_step_exact.py; tests/test_step_exact_cpu.py holds
them to their conditions without a GPU).  Only the fixtures, the package and numpy are used here.

Three paths: the fused landmark passes (lm_fused = 2, with the lm_group_steps / wide groups the case names), the record-based passes
(lm_fused = 0), and, on the windows with IMU edges, the chain elimination switched off (chain_elim = 0), where k_update_kf writes every
keyframe from the dense solution instead of the chain segments.  DESIGN.md 9o has the measured figures."""
import os

import numpy as np
import pytest

from . import build_exact as BX
from . import build_exact_cases as BC
from . import step_exact as SX
from . import step_exact_cases as SC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = {"fused": dict(lm_fused=2), "records": dict(lm_fused=0), "nochain": dict(lm_fused=0, chain_elim=0)}
IMU = tuple(n for n in BC.CASES if n not in ("noimu7", "noimu_lostkf"))      # (asserted on the windows below)
PARAMS = [(name, path) for name in BC.CASES for path in PATHS if path != "nochain" or name in IMU]
_CACHE = {}


def _case(pkg, name):
    if name not in _CACHE:
        fx = []
        for kind in ("build_exact", "step_exact"):
            with np.load(os.path.join(GOLDEN, "%s_%s.npz" % (kind, name))) as z:
                fx.append({k: z[k] for k in z.files})
        _CACHE[name] = (fx[0], fx[1], BC.CASES[name]["make"](pkg.window, BX.prior_of(fx[0])))
    return _CACHE[name]


@pytest.mark.parametrize("name,path", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_state_trace_and_exact_conditions(pkg, hip, name, path):
    fxb, fx, w = _case(pkg, name)
    assert BC.window_sha(w) == str(fx["sha"]), "the window generator gives another window here than where the fixture was made"
    assert (w.get("imu") is not None) == (name in IMU)
    case = BC.CASES[name]
    seqs = SC.sequences(name)
    assert [str(k) for k in fx["keys"]] == [k for k, _, _, _ in seqs]
    up, failed = SX.upload(w), []
    for j, (key, label, n, opts) in enumerate(seqs):
        s = SX.load(fx, j)
        ref = BX.load(fxb, w, SC.lambda_index(name, label))[0]
        g = pkg.new_problem(user_lambda_init=s["lam"], **PATHS[path], **case["opts"], **opts); g.upload_window(w); BX.apply(g, w)
        res = SX.read(g, g.optimize(n))
        lf = g.debug_get("lm_fused")
        assert lf[0] == (1 if path == "fused" else 0), (name, key, list(lf))
        if path == "fused":
            assert (lf[3] > 0) == case["wide"]      # wide groups exactly where they are meant
        if name in IMU:      # the chain segments write the velocity / bias half of the keyframes exactly where the elimination is on; without it k_update_kf writes all
            assert (g.debug_get("dense_dim")[0] < g.debug_get("pose_dim")[0]) == (path != "nochain"), (name, key)
        try:
            SX.hold(res, s, ref, w, path, "%s %s" % (name, key), dropped=SC.QUANT_DROPPED.get((name, key), ()))
            if key.startswith("rej"):      # the same call again, from what the rejected trial left: the same trial to the bit, and still the upload
                again = SX.read(g, g.optimize(n))
                assert again["trace"].tobytes() == res["trace"].tobytes(), (again["trace"].tolist(), res["trace"].tolist())
                assert not SX.exact(again, up, w, ref.lay)
        except AssertionError as e:      # (the other sequences' figures are printed before the test fails)
            failed.append(e)
        g.close()
    assert not failed, failed
