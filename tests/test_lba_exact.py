"""plba_lba_visual (csrc/plba_lba.hip) against the extended-precision reference tests/lba_ref.py, on the smallest windows at which
each loop, chunk and block structure of its kernels can go wrong (PAIR_CHUNK = KF_NT = 256, LM_NT = 128, the 256-wide loops over block
partials), and on the structure edges.  T, xyz, pq, err_first, lam, iterations, updates and the moved flags are compared after one, two
and three passes and for the full run, under the tolerance rule of lba_ref.tolerances; the conditions (i)-(iii) of lba_ref.hold are
asserted for every window (tests/test_lba_exact_cpu.py holds the oracle to the same rule without a GPU).  DESIGN.md 9 has the figures."""
import functools

import numpy as np
import pytest

from . import lba_cases as LC
from . import lba_ref as LR

PASSES = (1, 2, 3, None)


def _run(prob, w, **opts):
    return prob.lba_visual(w["T_kf_w"], w["kf_loc"], w["xyz"], w["pq"], w["po_pt"], w["po_kf"], w["uv"], w["lo_ln"], w["lo_kf"], w["l3"], w["cam"], **opts)


def _hold_all(pkg, w, name, opts=None, passes=PASSES, pose_step=True):
    """one reference run per type (its state after every pass is kept), one device run per pass count"""
    opts = dict(opts or {})
    r64, rw = LR.run(w, np.float64, **opts), LR.run(w, LR.wide(), **opts)
    g = pkg.new_problem()
    try:
        for k in passes:
            o = dict(opts) if k is None else dict(opts, max_iters=k)
            res = _run(g, w, **o)
            LR.hold(res, LR.at(r64, k), LR.at(rw, k), "device", "%s %s passes" % (name, k or "all"), o)
            if k == 1 and pose_step:
                LR.hold_pose_step(res["T"], w, rw, "device", name)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lines", [False, True], ids=["points", "lines"])
@pytest.mark.parametrize("n", LC.CHUNK_N)
def test_device_chunk_and_stride_boundaries(pkg, hip, n, lines):
    """one fixed and two local keyframes, n landmarks seen from all three: exactly n entries per keyframe pair (k_lba_pairs: the 64-lane
    loop at 64 / 65, a second chunk and its atomic accumulation at 257, a third at 513) and n observations per local keyframe (the second
    stride of k_lba_posesys / k_lba_rhs at 257)"""
    _hold_all(pkg, LC.three_keyframes(n, lines), "chunk n=%d%s" % (n, " lines" if lines else ""))


@pytest.mark.gpu
def test_device_generated_multi_chunk_window(pkg, hip):
    """500 entries in one pair, 500 observations on one keyframe"""
    _hold_all(pkg, pkg.window.make_visual_window(K=3, Np=400, Nl=100, n_fixed=1, seed=3, track=3), "generated 400+100")


@pytest.mark.gpu
@pytest.mark.parametrize("Np,Nl", [(127, 2), (128, 1)])
def test_device_landmark_block_boundaries(pkg, hip, Np, Nl):
    """LM_NT = 128: the last block starts with a line (127 + 2: lanes of one block mix 3-wide and 6-wide landmarks) / holds one line only"""
    _hold_all(pkg, LC.block_boundary(Np, Nl), "boundary %d+%d" % (Np, Nl))


@pytest.mark.gpu
def test_device_more_than_256_landmark_blocks(pkg, hip):
    """32 768 points and one line: 257 blocks of partials (the second stride of the `b += 256` loops of k_lba_reduce and k_lba_update),
    about 129 chunks per keyframe pair.  Reference only: the oracle's dense N^2 does not fit."""
    _hold_all(pkg, LC.blocks_257(), "257 blocks")


EDGE_OPTS = dict(identity=dict(lambda_lm=1e-9))
"""identity: the keyframe starts at rotation exactly 0 (the theta < 1e-6 branches of logmap_se3 and expmap_se3).  Under the default
damping its first update would leave it at 2e-4 rad, where the coded acos / (theta - sine) path loses nine digits in fp64 (the
reference's own fp64 evaluation is then 6e-11 off on T); lambda_lm = 1e-9 lets the first step through nearly undamped, to 4e-2 rad."""


@pytest.mark.gpu
@pytest.mark.parametrize("iterate", [0, 1])
@pytest.mark.parametrize("edge", sorted(LC.EDGES))
def test_device_structure_edges(pkg, hip, edge, iterate):
    """a point seen twice from one local keyframe; a landmark seen from fixed keyframes only; a local keyframe whose map rotation is
    exactly the identity; a residual norm below homog_th"""
    _hold_all(pkg, LC.EDGES[edge](), "%s iterate=%d" % (edge, iterate), dict(EDGE_OPTS.get(edge, {}), use_iterate_poses=iterate))


@pytest.mark.gpu
def test_device_structure_edge_gba_variant(pkg, hip):
    eps = 2.0 ** -52
    _hold_all(pkg, LC.edge_duplicate(), "duplicate gba", dict(variant=1, min_error=eps, min_error_change=eps, max_iters=6))


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", [("point", LC.fail_unobserved_point), ("keyframe", LC.fail_unobserved_keyframe)])
def test_device_reports_the_numerical_failure(pkg, orc, hip, name, make):
    """a point index / a local keyframe without observation: a zero pivot clears solver_ok, the update is gated on it, the run stops"""
    w = make()
    g = pkg.new_problem(); o = orc.new_problem()
    a, b = _run(g, w), _run(o, w)
    g.close(); o.close()
    for x in (a, b):
        assert (x["solver_failed"], x["updates"]) == (1, 0)
        assert np.array_equal(x["xyz"], w["xyz"]) and np.array_equal(x["pq"], w["pq"])
        assert np.abs(x["T"] - w["T_kf_w"]).max() <= 64 * LR.U * np.abs(w["T_kf_w"]).max()      # expmap(logmap(T)) of the local keyframes
