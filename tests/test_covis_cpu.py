"""The covisibility graph without a GPU: the recount against a replay of the reference's increments, the host header
(include/plba_g2o/covis.h over the kernels' shared csrc/plba_covis_dev.h) through the stand-alone host program under ASan / UBSan on
every map the GPU tests use, with exact equality; three mutations of the shared header, each caught; the struct layout and the ABI
surface; and the loud failure without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import covis_ref as CR

ROOT = CR.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return CR.build_hostcheck(str(tmp_path_factory.mktemp("covis_hostcheck")))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recount_equals_the_increment_replay(seed):
    """on a map without removals the recount is what the reference's increments maintain: points and lines, landmarks re-observed by the
    same keyframe; then a removed keyframe, whose row and column :3033-3038 clears"""
    K = 14
    ev = CR.insertion_sequence(K, seed)
    assert any(e[0] == "obs" for e in ev) and any(e[1] == 1 for e in ev)
    G, pts, lns = CR.replay_increments(K, ev)
    assert any(len(l) != len(set(l)) for l in pts + lns), "no landmark was observed twice by one keyframe"
    m = CR.make_map(K, pts, lns)
    Cm = CR.recount_dense(m)
    assert np.array_equal(Cm, G) and np.array_equal(Cm, Cm.T) and not np.diag(Cm).any() and Cm.max() > 1
    i, j, c = CR.recount_keys(m)
    S = np.zeros((K, K), np.int64); S[i, j] = c
    assert np.array_equal(S, G)
    # a removal after the last insertion
    CR.remove_keyframe(G, 5)
    lv = np.ones(K, np.uint8); lv[5] = 0
    md = CR.make_map(K, pts, lns, lv)
    assert np.array_equal(CR.recount_dense(md), G)
    i, j, c = CR.recount_keys(md)
    S = np.zeros((K, K), np.int64); S[i, j] = c
    assert np.array_equal(S, G)


def test_known_answers_by_hand():
    m = CR.case("multiplicity")
    Cm = CR.recount_dense(m)
    # [3, 0, 3]: m(3) m(0) = 2; [4, 0, 4, 4]: 3; [2, 2, 2, 0, 0]: 6; lines [1, 3, 1, 3]: 4; [0, 0]: only the diagonal
    assert Cm[0, 3] == 2 and Cm[0, 4] == 3 and Cm[0, 2] == 6 and Cm[1, 3] == 4 and Cm[1, 2] == 2 and Cm[0, 1] == 0
    th = CR.case("thresholds")
    ei, ej = CR.edge_loop(CR.recount_dense(th), CR.live_of(th), th["K"])
    got = set(zip(ei.tolist(), ej.tolist()))
    assert (0, 2) not in got and (0, 3) in got and (0, 4) in got and (1, 5) in got and (1, 6) in got and (1, 7) in got and (2, 9) in got and (7, 9) in got
    assert all((a, a + 1) in got for a in range(9)) and len(got) == 9 + 7
    ei, ej = CR.edge_loop(CR.recount_dense(th), CR.live_of(th), th["K"], dict(min_lm_ess_graph=150, min_lm_cov_graph=200))
    got = set(zip(ei.tolist(), ej.tolist()))
    assert (1, 5) not in got and (1, 6) in got and (1, 7) in got and (7, 9) in got and len(got) == 9 + 3
    dead = CR.case("dead")
    ei, ej = CR.edge_loop(CR.recount_dense(dead), CR.live_of(dead), dead["K"])
    for k in (7, 20, 21, 59):
        assert k not in ei and k not in ej
    assert not any((a, b) == (6, 8) for a, b in zip(ei, ej)) or CR.recount_dense(dead)[6, 8] >= 75      # nothing bridges a gap by index alone


@pytest.mark.parametrize("name", CR.CASES)
def test_host_header_against_the_reference(exe, tmp_path, name):
    """covis.h on the shared header under the host sanitizers: rows, column, edges and flags equal to the numpy reference, and the
    measurements inside the issue's bound of the wide evaluation"""
    from . import lba_ref
    m = CR.case(name)
    q = CR.queries(m, name)
    P = CR.poses(m["K"])
    for opts in (CR.OPTION_SETS if m["K"] <= 400 else CR.OPTION_SETS[:1]):
        got = CR.host_run(exe, str(tmp_path), m, q, opts, P)
        assert got is not None
        want = CR.expected(m, q, opts)
        assert CR.same(got, want) is None, (name, opts, CR.same(got, want))
        n_cov = len(got["ei"]) - len(q["loops"])
        if m["K"] <= 400 and n_cov:
            dt = lba_ref.wide()
            Zw = CR.relative_pose(P, got["ei"][:n_cov], got["ej"][:n_cov], dt)
            err = np.array(np.abs(got["meas"][:n_cov].astype(np.longdouble if dt != "mp" else object) - Zw), dtype=np.float64)
            assert (err <= CR.meas_bound(P, got["ei"][:n_cov], got["ej"][:n_cov])).all(), (name, err.max())
        if q["loops"]:
            assert np.array_equal(got["meas"][n_cov:], CR.loop_meas(P, q["loops"]))


MUTATIONS = {
    "greater_for_greater_equal": ("c >= min_lm_ess_graph || c >= min_lm_cov_graph", "c > min_lm_ess_graph || c > min_lm_cov_graph"),
    "multiplicity_ignored": ("if (j != i && j >= lo && j < hi) add(j - lo);", "if (j != i && !(x > b && kf[x - 1] == j) && j >= lo && j < hi) add(j - lo);"),
    "dead_keyframe_test_dropped": ("return live_i && live_j && (c >= min_lm_ess_graph", "return (c >= min_lm_ess_graph"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutations_of_the_shared_header_are_caught(tmp_path, which):
    old, new = MUTATIONS[which]
    txt = open(CR.DEV_HEADER).read()
    assert txt.count(old) == 1, "the mutation's anchor is gone from plba_covis_dev.h"
    hdr = tmp_path / "hdr"
    hdr.mkdir()
    (hdr / "plba_covis_dev.h").write_text(txt.replace(old, new))
    bad = CR.build_hostcheck(str(tmp_path / "bin"), sanitize=False, header_dir=str(hdr))
    caught = []
    for name in ("thresholds", "multiplicity", "dead"):
        m = CR.case(name)
        q = CR.queries(m, name)
        got = CR.host_run(bad, str(tmp_path), m, q, None, CR.poses(m["K"]))
        if got is None or CR.same(got, CR.expected(m, q, None)) is not None:
            caught.append(name)
    print(which, "caught by", caught)
    assert caught, which


def test_host_header_refuses_what_the_call_refuses(exe, tmp_path):
    m = CR.case("points_only")
    q = CR.queries(m, "points_only")
    P = CR.poses(m["K"])
    bad = dict(m); bad["pt_kf"] = m["pt_kf"].copy(); bad["pt_kf"][1] = m["K"]
    assert CR.host_run(exe, str(tmp_path), bad, q, None, P) is None
    bad = dict(m); bad["pt_kf"] = m["pt_kf"].copy(); bad["pt_kf"][0] = -1
    assert CR.host_run(exe, str(tmp_path), bad, q, None, P) is None
    assert CR.host_run(exe, str(tmp_path), m, q, dict(min_lm_cov_graph=-1), P) is None
    q2 = dict(q); q2["loops"] = [(1, 1)]
    assert CR.host_run(exe, str(tmp_path), m, q2, None, P) is None
    Pn = P.copy(); Pn[2, 10] = np.inf
    assert CR.host_run(exe, str(tmp_path), m, q, None, Pn) is None
    assert CR.host_run(exe, str(tmp_path), m, q, None, P) is not None


def test_abi_surface(pkg, hip_lib_path, tmp_path):
    """the symbols, the struct as a C compiler lays out include/plba.h, and the defaults of the reference's configuration"""
    abi = pkg.abi
    lib = C.CDLL(hip_lib_path)
    names = ("covis_default_options", "covis_set_map", "covis_reset", "covis_rows", "covis_column", "covis_pose_graph", "covis_local_map")
    for n in names:
        assert hasattr(lib, "plba_" + n), n
    assert set(names) <= set(abi.SIGNATURES) and set(names) <= abi.PRODUCT_ONLY
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plba.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(plba_covis_options), '
                   'offsetof(plba_covis_options, min_lm_ess_graph), offsetof(plba_covis_options, min_lm_cov_graph), offsetof(plba_covis_options, min_kf_local_map), '
                   'offsetof(plba_covis_options, reserved)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sz, o0, o1, o2, o3 = (int(v) for v in subprocess.check_output([str(exe)]).split())
    O = abi.CovisOptions
    assert (sz, o0, o1, o2, o3) == (C.sizeof(O), O.min_lm_ess_graph.offset, O.min_lm_cov_graph.offset, O.min_kf_local_map.offset, O.reserved.offset)
    o = O()
    f = lib.plba_covis_default_options
    f.restype = None; f.argtypes = [C.POINTER(O)]
    f(C.byref(o))
    assert (o.min_lm_ess_graph, o.min_lm_cov_graph, o.min_kf_local_map) == (150, 75, 3)
    assert {k: getattr(o, k) for k in CR.DEFAULTS} == CR.DEFAULTS
    for mth in ("covis_set_map", "covis_rows", "covis_column", "covis_pose_graph", "covis_local_map", "covis_reset"):
        assert hasattr(abi.Problem, mth)


def test_calls_fail_loudly_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        # with a device the refusal is the library's: a null handle is an error, not a fallback
        lib = pkg.hip_lib()
        assert lib.fn["covis_reset"](None) != 0 and lib.fn["covis_column"](None, 0, None) != 0
        return
    with pytest.raises(pkg.abi.PlbaError, match="no HIP device|no CPU fallback"):
        m = CR.case("k2")
        pkg.new_problem().covis_set_map(m["K"], m["pt_start"], m["pt_kf"], m["ln_start"], m["ln_kf"])
