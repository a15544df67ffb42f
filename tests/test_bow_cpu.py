"""Place recognition without a GPU: known answers by hand, the literal cases of the cited text, the host program (csrc/plba_bow_hostcheck.cpp
over include/plba_g2o/bow.h and the kernels' shared header) against the restatement of tests/bow_ref.py within the derived tolerances, the
conditions under which tests/test_bow.py may compare with the restatement (its own error inside the tolerance on every scenario; the
decision margins), the ABI surface, and the loud failure without a device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from . import bow_ref as BR

ROOT = BR.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return BR.build_hostcheck(str(tmp_path_factory.mktemp("bow_hostcheck")))


def _tiny_voc(descs, weights, parent=None):
    n = len(descs) + 1
    parent = np.array([-1] + ([0] * len(descs) if parent is None else list(parent)), np.int32)
    desc = np.zeros((n, 32), np.uint8)
    desc[1:] = np.asarray(descs, np.uint8).reshape(len(descs), 32)
    has_child = np.zeros(n, bool); has_child[parent[1:]] = True
    word = np.full(n, -1, np.int32); word[~has_child] = np.arange((~has_child).sum())
    return dict(k=2, L=1, parent=parent, desc=desc, weight=np.array([0.0] + list(weights), np.float64), word_id=word)


def _scn(voc, kfs, weighting=BR.TF_IDF, mode=BR.POINTS, **opts):
    full = []
    for rows in kfs:
        rows = np.asarray(rows, np.uint8).reshape(-1, 32)
        full.append(dict(pdesc=rows, pl=np.arange(2.0 * len(rows)).reshape(-1, 2), ldesc=np.zeros((0, 32), np.uint8), spl_epl=np.zeros((0, 4))))
    o = dict(mode=mode, lc_kf_dist=0, lc_kf_max_dist=0, lc_nkf_closest=0, topk=4); o.update(opts)
    return dict(voc=(voc, voc), weighting=(weighting, weighting), kfs=full, removed=[], opts=o, cov=BR.cov_columns(len(full), 3))


A, Bd = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)


def test_known_answers_by_hand(exe, tmp_path):
    """two words of weight 1: v = (1/2, 1/2), w = (1): the score is 1/2 and every self-score is 1"""
    voc = _tiny_voc([A, Bd], [1.0, 1.0])
    out, _ = BR.host_run(exe, str(tmp_path), _scn(voc, [[A], [A, Bd]]))
    assert list(out[1]["id0"]) == [0, 1] and list(out[1]["val0"]) == [0.5, 0.5] and list(out[0]["val0"]) == [1.0]
    assert list(out[1]["score_p"]) == [0.5, 1.0] and list(out[0]["score_p"]) == [1.0] and list(out[1]["score_f32"]) == [0.5, 1.0]
    v = BR.Voc(voc)
    _, i1, v1 = v.transform(np.array([A, Bd]))
    _, i0, v0 = v.transform(np.array([A]))
    assert BR.score_l1(i1, v1, i0, v0) == 0.5 and BR.score_l1(i1, v1, i1, v1) == 1.0


def test_literal_cases(exe, tmp_path):
    one = A.copy(); one[0] = 1
    # a Hamming tie between children takes the first: both children are one bit from the query
    two = A.copy(); two[5] = 16
    tie = _tiny_voc([one, two], [2.0, 3.0])
    out, _ = BR.host_run(exe, str(tmp_path), _scn(tie, [[A]]))
    assert list(out[0]["word0"]) == [0] and list(BR.Voc(tie).transform(np.array([A]))[0]) == [0]
    # a zero-weight word is skipped: no entry, the word reported as -1
    stop = _tiny_voc([A, Bd], [0.0, 3.0])
    out, _ = BR.host_run(exe, str(tmp_path), _scn(stop, [[A, Bd, A]]))
    assert list(out[0]["word0"]) == [-1, 1, -1] and list(out[0]["id0"]) == [1] and list(out[0]["val0"]) == [1.0]
    # addWeight against addIfNotExist: three times word 0 (weight 2) and once word 1 (weight 3)
    voc = _tiny_voc([A, Bd], [2.0, 3.0])
    rows = [[A, A, Bd, A]]
    acc, _ = BR.host_run(exe, str(tmp_path), _scn(voc, rows, weighting=BR.TF_IDF))
    once, _ = BR.host_run(exe, str(tmp_path), _scn(voc, rows, weighting=BR.BINARY))
    assert list(acc[0]["val0"]) == [6.0 / 9.0, 3.0 / 9.0] and list(once[0]["val0"]) == [2.0 / 5.0, 3.0 / 5.0]
    for w, want in ((BR.TF, [6.0 / 9.0, 3.0 / 9.0]), (BR.IDF, [0.4, 0.6])):
        assert BR.Voc(voc, w).transform(np.array(rows[0]))[2] == want


def test_empty_kind_is_nan_in_combined_mode_and_no_candidate(exe, tmp_path):
    voc = _tiny_voc([A, Bd], [1.0, 1.0])
    s = _scn(voc, [[A], [A, Bd], [A]], mode=BR.COMBINED)      # no line segments at all: 0 / 0
    out, _ = BR.host_run(exe, str(tmp_path), s)
    for idx in range(3):
        assert np.isnan(out[idx]["score"]).all() and np.isnan(out[idx]["score_f32"]).all() and not np.isnan(out[idx]["score_p"]).any()
        c = out[idx]["cand"]
        assert c["is_candidate"] == 0 and c["kf_prev"] == -1 and c["n_eligible"] == idx and c["n_closest"] == 0 and c["lc_min_score"] == 1.0
        # the pinned scan: a NaN at its start stays, so the order is the index order
        assert list(c["topk"][:idx]) == list(range(idx))
        assert BR.same_decision({k: [v] for k, v in c.items()}, 0, BR.decide_ref(out[idx]["score_f32"][:idx], s["cov"][idx], np.ones(idx), idx, **s["opts"])) is None
    assert math.isnan(BR.combined(0.5, 0.0, 2, 0, 1.0, float("nan")))


def test_malformed_trees_are_refused(exe, tmp_path):
    good = _tiny_voc([A, Bd], [1.0, 1.0])
    bad = []
    v = dict(good); v["parent"] = np.array([-1, 0, 2], np.int32); bad.append(v)                 # parent[i] >= i
    v = dict(good); v["word_id"] = np.array([-1, 0, -1], np.int32); bad.append(v)                # a leaf without a word id
    v = dict(good); v["word_id"] = np.array([-1, 1, 1], np.int32); bad.append(v)                 # a duplicate word id
    for v in bad:
        pin = str(tmp_path / "bad.bin")
        BR.write_host_input(pin, _scn(v, [[A]]))
        assert subprocess.call([exe, pin, str(tmp_path / "bad.out")], stderr=subprocess.DEVNULL) == 3


NAMES = sorted(BR.SCENARIOS)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_inside_the_tolerances(name):
    """the condition of every comparison tests/test_bow.py makes with the restatement, by the reference alone: its own sequential fp64
    values lie inside the derived tolerances of the exact ones, on every scenario the GPU tests use"""
    ref = BR.reference(name)
    worst = (0.0, 0.0)
    for idx, r in enumerate(ref):
        for k in (0, 1):
            for v, x in zip(r["val%d" % k], r["xval%d" % k]):
                assert BR.exact_err(v, x) <= BR.tol_value(max(r["n"][k], 1)) * float(x)
        w = BR.column_errors(name, idx, r["score_p"], r["score_l"], r["score"])
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print("%s: restatement / tolerance: single %.4f, chosen %.4f" % (name, worst[0], worst[1]))
    assert worst[0] < 1.0 and worst[1] < 1.0


@pytest.mark.parametrize("name", NAMES)
def test_host_program_against_the_restatement(exe, tmp_path, name):
    """bow.h on the shared header: words and nnz for equality, values and scores within the tolerances of the exact ones, and the decision
    it makes from ITS float column equal to the restatement's decision from that column"""
    s, ref = BR.scenario(name), BR.reference(name)
    out, _ = BR.host_run(exe, str(tmp_path), s)
    o = dict(BR.DEFAULTS); o.update(s["opts"])
    for idx, (h, r) in enumerate(zip(out, ref)):
        for k in (0, 1):
            if (k == 0 and o["mode"] == BR.LINES) or (k == 1 and o["mode"] == BR.POINTS):
                continue      # a mode reads only the kinds it uses
            assert np.array_equal(h["word%d" % k], r["word%d" % k]) and list(h["id%d" % k]) == r["id%d" % k], (idx, k)
            for v, x in zip(h["val%d" % k], r["xval%d" % k]):
                assert BR.exact_err(v, x) <= BR.tol_value(max(r["n"][k], 1)) * float(x)
        w = BR.column_errors(name, idx, h["score_p"], h["score_l"], h["score"])
        assert w[0] < 1.0 and w[1] < 1.0, (idx, w)
        assert np.array_equal(h["score_f32"], h["score"].astype(np.float32), equal_nan=True)
        dead = np.flatnonzero(r["live"] == 0)
        assert not h["score"][dead].any() and not h["score_p"][dead].any()
        assert BR.same_decision({k: [v] for k, v in h["cand"].items()}, 0, BR.decide_ref(h["score_f32"][:idx], s["cov"][idx], r["live"], idx, **o)) is None, idx
        if BR.margins_ok(name, idx):
            assert BR.same_decision({k: [v] for k, v in h["cand"].items()}, 0, r["cand"]) is None, idx


def test_margins_and_planted_revisits():
    """by the reference alone: the scenarios hold decisions with safe margins, among them candidates found at their planted revisits, and
    the special cases the GPU tests lean on are what they are meant to be"""
    for name in ("loop80", "loop80_points", "loop80_lines", "removed", "db258"):
        ref = BR.reference(name)
        n = len(ref)
        safe = [idx for idx in range(n) if BR.margins_ok(name, idx)]
        assert len(safe) > n // 2 and any(ref[idx]["cand"]["is_candidate"] for idx in safe) and any(not ref[idx]["cand"]["is_candidate"] for idx in safe), name
    # a revisit: the second half of the trajectory returns to the places of the first, two keyframes to a place
    ref = BR.reference("loop80")
    hits = [idx for idx in range(50, 80) if BR.margins_ok("loop80", idx) and ref[idx]["cand"]["is_candidate"] and abs(ref[idx]["cand"]["kf_prev"] - (idx - 40)) <= 2]
    assert len(hits) >= 20, hits
    s, ref = BR.scenario("removed"), BR.reference("removed")
    for a, kf in s["removed"]:
        for idx in range(a, len(ref)):
            assert ref[idx]["score"][kf] == 0 and kf not in ref[idx]["cand"]["topk"] and ref[idx]["cand"]["kf_prev"] != kf
    few = BR.reference("few_eligible")
    assert all(0 < r["cand"]["n_eligible"] < 16 and r["cand"]["topk"][r["cand"]["n_eligible"]] == -1 for r in few[7:])
    assert all(r["cand"]["topk"] == [-1] * 16 and r["cand"]["n_eligible"] > 0 for r in BR.reference("topk0")[4:])
    assert any(len(r["id0"]) < r["n"][0] for r in BR.reference("sizes"))      # words that repeat: the run-length path


def test_abi_surface(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct sizes as a C compiler lays out include/plba.h, and the defaults of the reference's configuration"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    names = ("bow_default_options", "bow_set_vocabulary", "bow_transform", "bow_insert_keyframes", "bow_remove_keyframe", "bow_reset")
    for n in names:
        assert hasattr(lib, "plba_" + n), n
    assert set(names) <= set(abi.SIGNATURES) and set(names) <= abi.PRODUCT_ONLY
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(plba_bow_options), '
                   'sizeof(plba_bow_candidate), sizeof(plba_bow_result), offsetof(plba_bow_candidate, topk_score), offsetof(plba_bow_result, cand), '
                   'offsetof(plba_bow_result, score_f32)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    so, sc, sr, o1, o2, o3 = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert (so, sc, sr) == (C.sizeof(abi.BowOptions), C.sizeof(abi.BowCandidate), C.sizeof(abi.BowResult))
    assert (o1, o2, o3) == (abi.BowCandidate.topk_score.offset, abi.BowResult.cand.offset, abi.BowResult.score_f32.offset)
    o = abi.BowOptions()
    f = lib.plba_bow_default_options
    f.restype = None; f.argtypes = [C.POINTER(abi.BowOptions)]
    f(C.byref(o))
    assert (o.mode, o.topk, o.min_lm_cov_graph, o.min_kf_local_map, o.lc_kf_dist, o.lc_kf_max_dist, o.lc_nkf_closest) == (0, 8, 75, 3, 50, 50, 4)
    assert {k: getattr(o, k) for k in BR.DEFAULTS} == BR.DEFAULTS
    for m in ("bow_set_vocabulary", "bow_transform", "bow_insert_keyframes", "bow_remove_keyframe", "bow_reset"):
        assert hasattr(abi.Problem, m)


def test_calls_fail_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        # with a device the refusal is the library's: a null handle is an error, not a fallback
        lib = pkg.hip_lib()
        assert lib.fn["bow_reset"](None) != 0 and lib.fn["bow_remove_keyframe"](None, 0) != 0
        assert lib.fn["bow_transform"](None, 0, 1, None, None, None, None, None, None) != 0
        return
    with pytest.raises(pkg.abi.PlbaError, match="no HIP device|no CPU fallback"):
        pkg.new_problem().bow_set_vocabulary(0, _tiny_voc([A, Bd], [1.0, 1.0]))
