"""Time of plba_bow_insert_keyframes for ONE keyframe (600 point + 200 line descriptors, vocabularies of k = 10, L = 5: 100 000 words each)
against a database of 300 / 1 000 / 5 000 / 20 000 stored keyframes: the whole call (upload, transform, append, scores, decision, read-back
of the four score columns and the candidate), against the plain-C++ drop-in of include/plba_g2o/bow.h on one core (built -O2 without
sanitizers from csrc/plba_bow_hostcheck.cpp, timed inside the program so that process start and file I/O stay out).  The stored keyframes
are a pool of 250 distinct ones (leaf descriptors with a few flipped bits, 50 places), inserted again and again in calls of B = 250 that
read no score column back; the device call is timed at the C ABI on arrays laid out beforehand: best of `reps` wall-clock calls after a
warm-up (every repetition appends one more keyframe); the host column is the mean of `reps` insertions.
python tools/time_bow.py [reps]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, '.')
import __graft_entry__ as ge  # noqa: E402

import torch  # noqa: E402,F401  (torch's HIP runtime first, as in the tests)

from tests import bow_ref as BR  # noqa: E402

pkg = ge.load_package()
abi = pkg.abi
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
POOL, SIZES = 250, (300, 1000, 5000, 20000)
exe = BR.build_hostcheck(os.path.join(ge.ROOT, "tools", "_build_bow_hostcheck"), sanitize=False)


def vocabulary(k, L, seed):
    """make_vocabulary's tree, vectorised: children are their parent with 12 % / 6 % / 3 % / 1.5 % of the bits flipped by level"""
    rng = np.random.default_rng(seed)
    parent, desc = [np.array([-1])], [np.zeros((1, 32), np.uint8)]
    first, count = 0, 1
    for lev in range(1, L + 1):
        par = np.repeat(np.arange(first, first + count), k)
        if lev == 1:
            d = rng.integers(0, 256, (len(par), 32), dtype=np.uint8)
        else:
            d = desc[-1][par - first] ^ np.packbits(rng.random((len(par), 256)) < 0.24 / (1 << (lev - 1)), axis=1)
        parent.append(par); desc.append(d)
        first, count = first + count, len(par)
    parent, desc = np.concatenate(parent).astype(np.int32), np.concatenate(desc)
    n = len(parent)
    word = np.full(n, -1, np.int32); word[first:] = rng.permutation(count)
    weight = rng.uniform(0.2, 9.0, n); weight[rng.random(n) < 0.1] = 0.0
    return dict(k=k, L=L, parent=parent, desc=desc, weight=weight, word_id=word), np.arange(first, n)


def keyframe(vp, lp, vl, ll, seed, place):
    rng, prng = np.random.default_rng(seed), np.random.default_rng(7000 + place)
    kf = {}
    for key, pos, w, voc, leaves, n in (("pdesc", "pl", 2, vp, lp, 600), ("ldesc", "spl_epl", 4, vl, ll, 200)):
        pick = np.where(rng.random(n) < 0.3, leaves[rng.integers(0, len(leaves), n)], leaves[prng.integers(0, len(leaves), n)])
        kf[key] = voc["desc"][pick] ^ np.packbits(rng.random((n, 256)) < 0.01, axis=1)
        kf[pos] = rng.uniform(0.0, 640.0, (n, w))
    return kf


(vp, lp), (vl, ll) = vocabulary(10, 5, 1), vocabulary(10, 5, 2)
pool = [keyframe(vp, lp, vl, ll, 100 + i, i % 50) for i in range(POOL)]
query = keyframe(vp, lp, vl, ll, 99, 7)
p = pkg.new_problem()
p.bow_set_vocabulary(0, vp); p.bow_set_vocabulary(1, vl)
fn, dp, ip, up = p.lib.fn, abi._dp, abi._ip, abi._up
res = {}
with tempfile.TemporaryDirectory() as tmp:
    s = dict(voc=(vp, vl), weighting=(0, 0), kfs=pool + [query], removed=[], opts={}, cov=[np.zeros(i, np.int32) for i in range(POOL + 1)])
    pin = os.path.join(tmp, "in.bin")
    BR.write_host_input(pin, s)
    stored = 0
    for N in SIZES:
        while stored < N:
            m = min(POOL, N - stored)
            p.bow_insert_keyframes(pool[:m], want_scores=False)
            stored += m
        o = abi.BowOptions(); fn["bow_default_options"](C.byref(o))
        ps, ls = np.array([0, 600], np.int32), np.array([0, 200], np.int32)
        dP, dL, pl, se = (np.ascontiguousarray(query[k]) for k in ("pdesc", "ldesc", "pl", "spl_epl"))
        cap = N + reps + 8
        cov, cs = np.zeros(cap, np.int32), np.zeros(2, np.int32)
        sp, sl, sc, sf = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, np.float32)
        cand = (abi.BowCandidate * 1)()
        r = abi.BowResult()
        r.score_cap = cap; r.score_p, r.score_l, r.score, r.score_f32, r.cand = dp(sp), dp(sl), dp(sc), sf.ctypes.data_as(C.POINTER(C.c_float)), cand
        wall = 1e9
        for rep in range(reps + 1):
            cs[1] = stored
            t0 = time.perf_counter()
            rc = fn["bow_insert_keyframes"](p._h, C.byref(o), 1, ip(ps), up(dP), dp(pl), ip(ls), up(dL), dp(se), ip(cs), ip(cov), C.byref(r))
            dt = time.perf_counter() - t0
            assert rc == 0 and r.first_index == stored, (rc, r.first_index, stored)
            stored += 1
            if rep:
                wall = min(wall, dt)
        host = subprocess.check_output([exe, pin, "-", str(max(reps, 2)), str(N)]).split()
        res[N] = dict(device_ms=round(wall * 1e3, 4), host_ms=round(float(host[0]), 3), host_stored=int(host[2]), best_score=round(float(cand[0].best_score), 4),
                      kf_prev=int(cand[0].kf_prev), db_bytes=int(p.debug_get("bow_db")[4]))
        print("stored %6d: device %.3f ms, bow.h on one core %.2f ms (%d stored)" % (N, res[N]["device_ms"], res[N]["host_ms"], res[N]["host_stored"]), flush=True)
p.close()
print(json.dumps(dict(what="one keyframe, 600 + 200 descriptors, k = 10, L = 5", reps=reps, stored=res)))
