"""Windows of the sparse reduced-camera solve of plba_lba_visual (plba_lba_options.solver = 1), from lba_cases.from_tracks: every track is
given, so the covisibility graph, and with it the fronts and levels of the nested dissection, and the entries per block are exact.
SHAPES: name -> (builder(lines), local keyframes, fronts, tree levels)."""
import numpy as np

from . import lba_cases as LC

PER = 6      # points first seen in every keyframe


def _split(tracks, lines):
    """about a fifth of the landmarks are lines"""
    if not lines:
        return tracks, []
    return [t for i, t in enumerate(tracks) if i % 5 != 4], [t for i, t in enumerate(tracks) if i % 5 == 4]


def _band(n_local, n_fixed=2, length=4, per=PER):
    K = n_local + n_fixed
    return [list(range(k, min(K, k + length))) for k in range(K - 1) for _ in range(per)]


def band(n_local, seed, lines=False, extra=()):
    """two fixed keyframes, then n_local local ones; every keyframe is the first to see PER landmarks tracked over 4 consecutive keyframes"""
    pts, lns = _split(_band(n_local) + [list(t) for t in extra], lines)
    return LC.from_tracks(n_local + 2, 2, pts, lns, seed)


def revisit(seed, lines=False):
    """40 local keyframes; keyframes 6, 7 and 33, 34 (local 4, 5 and 31, 32) share four landmarks"""
    return band(40, seed, lines, extra=[[6, 7, 33, 34]] * 4)


def full(seed, lines=False):
    """20 local keyframes, every landmark seen from all 22: one front holds everything"""
    pts, lns = _split([list(range(22))] * 30, lines)
    return LC.from_tracks(22, 2, pts, lns, seed)


def components(seed, lines=False):
    """two trajectories of 12 local keyframes (2 .. 13 behind the fixed 0, 14 .. 25 behind the fixed 1) that share no landmark"""
    tr = []
    for h in range(2):
        loc = [h] + list(range(2 + 12 * h, 14 + 12 * h))
        tr += [[loc[q] for q in range(k, min(13, k + 4))] for k in range(12) for _ in range(PER)]
    pts, lns = _split(tr, lines)
    return LC.from_tracks(26, 2, pts, lns, seed)


def lonely(seed, lines=False):
    """12 local keyframes in a band and a thirteenth (keyframe 14) whose landmarks are otherwise seen from the fixed keyframes only: a
    vertex with a diagonal block and no neighbour"""
    pts, lns = _split(_band(12) + [[0, 1, 14]] * 20, lines)
    return LC.from_tracks(15, 2, pts, lns, seed)


def entries(n, seed=31):
    """two fixed and four local keyframes (2 .. 5): 30 points from 0, 1, 2, 3 and 30 from 0, 1, 4, 5, and n points from 0, 2, 4: the block
    of the local keyframes (0, 2) has exactly n pair entries, their diagonal blocks 30 + n"""
    return LC.from_tracks(6, 2, [[0, 1, 2, 3]] * 30 + [[0, 1, 4, 5]] * 30 + [[0, 2, 4]] * n, [], seed)


ENTRIES_N = (1, 63, 64, 65, 256, 257)

# name -> (builder, local keyframes, fronts, levels): the plan figures are those of pgo_sparse_analyse on these graphs
SHAPES = {
    "band12": (lambda lines: band(12, 41, lines), 12, 1, 1),
    "band17": (lambda lines: band(17, 42, lines), 17, 3, 2),
    "band40": (lambda lines: band(40, 43, lines), 40, 7, 3),
    "revisit40": (lambda lines: revisit(44, lines), 40, 4, 2),
    "full20": (lambda lines: full(45, lines), 20, 1, 1),
    "components": (lambda lines: components(46, lines), 24, 2, 1),
    "lonely": (lambda lines: lonely(47, lines), 13, 2, 1),
}


EPS = 2.0 ** -52
GBA = dict(variant=1, min_error=EPS, min_error_change=EPS, max_iters=6)      # as globalBundleAdjustment calls it (tests/test_lba_exact.py)
# (shape, lines, options): every shape points-only, with a fifth lines, and with the line pass at the iterate; the 40-keyframe band as the GBA variant
RUNS = [(s, lines, dict(use_iterate_poses=it)) for s in SHAPES for lines, it in ((False, 0), (True, 0), (True, 1))] + [("band40", True, GBA)]
SCALE_N, SCALE_OPTS = 1000, dict(max_iters=2)


def run_id(r):
    return "%s-%s-%s" % (r[0], "lines" if r[1] else "points", "gba" if r[2].get("variant") else "iterate%d" % r[2].get("use_iterate_poses", 0))


_REF = {}


def reference(key, make, opts, sparse=False):
    """(window, fp64 run, wide run) of the reference, computed once per session and shared"""
    if key not in _REF:
        from . import lba_ref as LR
        from . import lba_sparse_ref as LS
        w = make()
        run = (lambda dt: LS.run(w, dt, **opts)) if sparse else (lambda dt: LR.run(w, dt, **opts))
        _REF[key] = (w, run(np.float64), run(LR.wide()))
    return _REF[key]


def run_reference(r):
    return reference(run_id(r), lambda: SHAPES[r[0]][0](r[1]), r[2])


def entries_reference(n):
    return reference("entries%d" % n, lambda: entries(n), {})


def scale_reference(pkg):
    return reference("scale", lambda: pkg.window.make_map_window(SCALE_N, revisits=3), SCALE_OPTS, sparse=True)


def all_fixed(seed=48):
    w = band(12, seed)
    w["kf_loc"] = np.full(len(w["kf_loc"]), -1, np.int32)
    return w
