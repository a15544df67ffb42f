"""The users of a problem's mapped mailbox and of the dense solver's workspace, interleaved on ONE handle: plba_lba_visual,
plba_optimize_pose_graph, plba_optimize, plba_dense_solve and plba_compute_marginals in turn, twice over, each output compared bit for bit
with the same call on a fresh handle.  The one-step-behind loops of the first two continue the handle's sequence numbers where the
calls before them left them (mail_reserve / mail_wait, csrc/plba_problem.h), and every call sizes its solver workspace through
DenseWork: no call may see what another left in the mailbox, the buffer pool or the handle.

options.pgo_solver and options.lm_fused are fixed when a handle is created (include/plba.h has no call that changes them), so the two
pose-graph solvers and the two forms of plba_optimize cannot meet on one handle: two handles run the sequence, one with the dense
pose-graph solve and the fused landmark passes forced, one with the sparse solve and the record-based passes.

Shapes: the smallest that go round each loop more than once, so that the one-behind wait is taken (asserted below)."""
import numpy as np
import pytest

from . import pgo_ref

pytestmark = pytest.mark.gpu

HANDLES = {"dense_fused": dict(pgo_solver=0, lm_fused=2), "sparse_record": dict(pgo_solver=1, lm_fused=0)}


def _ring(nv=6):
    """a ring of nv vertices, one fixed: odometry edges round the ring, noisy measurements, drifted estimates"""
    rng = np.random.default_rng(11)
    T = []
    for k in range(nv):
        a = 2 * np.pi * k / nv
        Rwb = pgo_ref._rot(np.array([0.05 * np.sin(k), 0.04 * np.cos(k), a]))
        T.append(pgo_ref._T(Rwb.T, -Rwb.T @ np.array([4 * np.cos(a), 4 * np.sin(a), 0.2 * np.sin(2 * a)])))
    edges = np.array([(k, (k + 1) % nv) for k in range(nv)], np.int32)
    meas = []
    for i, j in edges:
        Z = np.linalg.inv(T[i]) @ T[j]
        Z[:3, :3] = Z[:3, :3] @ pgo_ref._rot(rng.normal(size=3) * 1e-3); Z[:3, 3] += rng.normal(size=3) * 3e-3
        meas.append(pgo_ref._p12(Z))
    est = [pgo_ref._p12(T[0])] + [pgo_ref._p12(T[k] @ pgo_ref._T(pgo_ref._rot(rng.normal(size=3) * 1e-2), rng.normal(size=3) * 3e-2)) for k in range(1, nv)]
    fixed = np.zeros(nv, np.uint8); fixed[0] = 1
    return dict(pose=np.array(est), ei=edges[:, 0].copy(), ej=edges[:, 1].copy(), meas=np.array(meas), fixed=fixed)


@pytest.fixture(scope="module")
def cases(pkg):
    rng = np.random.default_rng(33)
    B = rng.normal(size=(33, 33))
    return dict(lba=pkg.window.make_visual_window(K=4, Np=20, Nl=4, n_fixed=1, seed=7),      # 3 local keyframes
                ring=_ring(),
                win=pkg.window.make_window(4, 40, 6, imu=True, seed=0x5EED0B0C),
                A=B @ B.T + 33 * np.eye(33), b=rng.normal(size=33))


def _lba(p, c):
    w = c["lba"]
    r = p.lba_visual(w["T_kf_w"], w["kf_loc"], w["xyz"], w["pq"], w["po_pt"], w["po_kf"], w["uv"], w["lo_ln"], w["lo_kf"], w["l3"], w["cam"])
    assert r["iterations"] >= 3, r["iterations"]
    return r


def _pgo(p, c, sparse):
    g = c["ring"]
    X, st, tr = p.pgo(g["pose"], g["ei"], g["ej"], g["meas"], fixed=g["fixed"], iters=10, user_lambda=1e-10)
    assert st["trials"] >= 3 and st["n_trace"] == len(tr), st
    assert p.debug_get("pgo_sparse")[0] == (1 if sparse else 0)
    st = dict(st); del st["ms_total"]
    return dict(X=X, stats=st, trace=tr)


def _ba(p, c, fused):
    p.upload_window(c["win"])
    st = p.optimize(4)
    assert st.trials >= 2 and st.solver_failures == 0
    assert p.debug_get("lm_fused")[0] == (1 if fused else 0)
    kf = p.get_keyframes()
    out = dict(stats=(st.iterations, st.trials, st.stop_reason, st.chi2_initial, st.chi2_final, st.lambda_final), trace=p.trace(),
               points=p.get_points(), lines=p.get_lines(), **{"kf_" + k: v for k, v in kf.items()})
    return out


def _solve(p, c):
    x, ok = p.dense_solve(c["A"], c["b"])
    assert ok
    return dict(x=x)


def _marginals(p, c):
    return p.marginals(pairs=[(0, 1), (1, 3)])


def _sequence(p, c, opts):
    """the calls in turn; plba_compute_marginals works on the window plba_optimize left"""
    return [("lba", _lba(p, c)), ("pgo", _pgo(p, c, opts["pgo_solver"] == 1)), ("optimize", _ba(p, c, opts["lm_fused"] == 2)),
            ("dense_solve", _solve(p, c)), ("marginals", _marginals(p, c))]


def _same_bits(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same_bits(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), "%s: %r != %r" % (where, a, b)
    else:
        assert a == b, "%s: %r != %r" % (where, a, b)


@pytest.fixture(scope="module")
def fresh(pkg, hip, cases):
    """every call on a handle of its own (plba_compute_marginals after the plba_optimize it follows): computed once, compared against, never changed"""
    out = {}
    for name, opts in HANDLES.items():
        ref = {}
        for call, fn in (("lba", _lba), ("pgo", lambda p, c: _pgo(p, c, opts["pgo_solver"] == 1)), ("dense_solve", _solve)):
            p = pkg.new_problem(**opts); ref[call] = fn(p, cases); p.close()
        p = pkg.new_problem(**opts); ref["optimize"] = _ba(p, cases, opts["lm_fused"] == 2); ref["marginals"] = _marginals(p, cases); p.close()
        out[name] = ref
    return out


@pytest.mark.parametrize("name", list(HANDLES))
def test_interleaved_calls_on_one_handle_match_fresh_handles(pkg, hip, cases, fresh, name):
    opts = HANDLES[name]
    p = pkg.new_problem(**opts)
    for rnd in range(2):
        for call, got in _sequence(p, cases, opts):
            _same_bits(got, fresh[name][call], "%s round %d %s" % (name, rnd, call))
    p.close()
