"""IMU preintegration producer: KeyFrame::ComputeIMUPreIntSinceLastFrame + IMUPreintegrator::update
(src/keyFrame.cpp:139-172, IMU/IMUPreintegrator.cpp:47-139) — oracle vs an independent schedule, HIP vs oracle, and the kernel
through plba_preintegrate against the independent 40-digit fixture tests/golden/preint_exact.json (make_preint_exact.py), per 3 x 3
block; mixed waves and the call's plumbing (chunked read-back, staging overflow, re-use of a handle) bit for bit against small calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import preint_cases as PC  # noqa: E402

LD = np.longdouble
U = 2.0 ** -53


def _stream(pkg, M, rng, t0=LD("1403636579.763555527"), rate=200.0, kf_dt=0.25, jitter=True):
    """EuRoC-shaped stream: ns-resolution stamps around 1.4e9 s (a double cannot hold them: long double matters),
    every interval owning the samples from a little before its first image to a little after its second."""
    t_prev = t0 + LD(kf_dt) * np.arange(M, dtype=LD)
    t_curr = t_prev + LD(kf_dt)
    ts, starts = [], [0]
    for m in range(M):
        n_before = int(rng.integers(0, 3))            # samples older than prev_t (skipped by the reference loop)
        n_after = int(rng.integers(0, 3))             # samples past curr_t (the first one takes the last partial step)
        n_in = int(kf_dt * rate)
        k = np.arange(-n_before, n_in + n_after, dtype=LD)
        off = LD(0.0007) if jitter else LD(0.0)
        tt = t_prev[m] + off + k / LD(rate) + (LD(1e-6) * rng.normal(size=len(k)).astype(LD) if jitter else 0)
        ts.append(np.sort(tt))
        starts.append(starts[-1] + len(tt))
    t = np.concatenate(ts)
    S = len(t)
    gyr = rng.normal(size=(S, 3)) * 0.3
    acc = rng.normal(size=(S, 3)) * 2.0 + np.array([0, 0, 9.81])
    bg = rng.normal(size=(M, 3)) * 1e-3
    ba = rng.normal(size=(M, 3)) * 1e-2
    return dict(sample_start=np.array(starts, dtype=np.int32), t=t, gyr=gyr, acc=acc, t_prev=t_prev, t_curr=t_curr, bg=bg, ba=ba)


def _schedule(s, m):
    """src/keyFrame.cpp:147-170 restated on its own (index, dt) — independent of the C implementations."""
    lo, hi = int(s["sample_start"][m]), int(s["sample_start"][m + 1])
    t, prev, curr = s["t"], s["t_prev"][m], s["t_curr"][m]
    i = lo
    while i < hi and t[i] < prev:
        i += 1
    out = []
    if i >= hi:
        return out
    out.append((i, float(t[i] - prev))); i += 1
    while i < hi and t[i] <= curr:
        out.append((i, float(t[i] - t[i - 1]))); i += 1
    if i < hi:
        out.append((i, float(curr - t[i])))
    return out


def _call(prob, pkg, s):
    return prob.preintegrate(s["sample_start"], s["t"], s["gyr"], s["acc"], s["t_prev"], s["t_curr"], s["bg"], s["ba"],
                             pkg.window.GYR_MEAS_COV, pkg.window.ACC_MEAS_COV)


def test_oracle_driver_follows_the_reference_schedule(pkg, orc):
    rng = np.random.default_rng(11)
    s = _stream(pkg, 6, rng)
    p = orc.new_problem()
    got = _call(p, pkg, s)
    gc, ac = pkg.window.GYR_MEAS_COV, pkg.window.ACC_MEAS_COV
    n_neg = 0
    for m in range(6):
        pre = np.zeros(142); pre[[6, 10, 14]] = 1.0
        for i, dt in _schedule(s, m):
            n_neg += dt < 0
            pre = orc.preint_update(pre, s["gyr"][i] - s["bg"][m], s["acc"][i] - s["ba"][m], dt, gc, ac)
        assert np.array_equal(got[m], pre)
    assert n_neg > 0          # the literal `dt = curr_t - t[i]` step of keyFrame.cpp:162-167 was exercised
    p.close()


def test_oracle_driver_against_the_window_generator(pkg, orc):
    """uniform 200 Hz samples ending exactly on the second image: the numpy generator's recurrence is the same thing"""
    rng = np.random.default_rng(12)
    M, S, dt = 3, 50, 0.005
    omega = rng.normal(size=(M, S, 3)) * 0.3
    acc = rng.normal(size=(M, S, 3)) * 2.0 + np.array([0, 0, 9.81])
    ref = pkg.window.preintegrate(omega, acc, dt)
    t_prev = LD(10.0) + LD(0.25) * np.arange(M, dtype=LD)
    t = np.concatenate([t_prev[m] + LD(dt) * np.arange(1, S + 1, dtype=LD) for m in range(M)])
    s = dict(sample_start=np.arange(M + 1, dtype=np.int32) * S, t=t, gyr=omega.reshape(-1, 3), acc=acc.reshape(-1, 3),
             t_prev=t_prev, t_curr=t.reshape(M, S)[:, -1].copy(), bg=np.zeros((M, 3)), ba=np.zeros((M, 3)))
    p = orc.new_problem()
    got = _call(p, pkg, s)
    p.close()
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-16)


def test_empty_and_degenerate_intervals(pkg, orc):
    p = orc.new_problem()
    s = dict(sample_start=np.array([0, 0, 2], dtype=np.int32), t=np.array([1.0, 1.005], dtype=LD), gyr=np.zeros((2, 3)), acc=np.zeros((2, 3)),
             t_prev=np.array([0.0, 2.0], dtype=LD), t_curr=np.array([0.5, 2.5], dtype=LD), bg=np.zeros((2, 3)), ba=np.zeros((2, 3)))
    got = _call(p, pkg, s)     # interval 0 owns no samples, interval 1 only samples older than its first image
    p.close()
    ident = np.zeros(142); ident[[6, 10, 14]] = 1.0
    assert np.array_equal(got[0], ident) and np.array_equal(got[1], ident)


@pytest.mark.gpu
def test_hip_preintegration_matches_the_oracle(pkg, orc, hip):
    rng = np.random.default_rng(13)
    for M in (1, 49, 130):
        s = _stream(pkg, M, rng)
        g, o = pkg.new_problem(), orc.new_problem()
        a, b = _call(g, pkg, s), _call(o, pkg, s)
        g.close(); o.close()
        # fp64 with fused multiply-adds against the oracle's unfused arithmetic: relative to each block's own scale
        for lo, hi in ((0, 3), (3, 6), (6, 15), (15, 24), (24, 33), (33, 42), (42, 51), (51, 60), (60, 141), (141, 142)):
            sc = np.abs(b[:, lo:hi]).max()
            assert np.abs(a[:, lo:hi] - b[:, lo:hi]).max() <= 1e-11 * sc, (M, lo)
        # ... and every 3 x 3 block of every interval on its own scale (the whole-matrix measure above lets cov_phiphi be off by 1e-7):
        # two fp64 evaluations of sums of ~50 same-order terms, 16 n 2^-53 each from the exact value (tests/test_preint_exact_cpu.py)
        for m in range(M):
            n = len(_schedule(s, m))
            for name, e in PC.block_errors(a[m], b[m]).items():
                assert e <= 2 * 16 * n * U, (M, m, name, e)


@pytest.mark.gpu
def test_hip_preintegration_degenerate(pkg, orc, hip):
    g = pkg.new_problem()
    s = dict(sample_start=np.array([0, 0, 2], dtype=np.int32), t=np.array([1.0, 1.005], dtype=LD), gyr=np.zeros((2, 3)), acc=np.zeros((2, 3)),
             t_prev=np.array([0.0, 2.0], dtype=LD), t_curr=np.array([0.5, 2.5], dtype=LD), bg=np.zeros((2, 3)), ba=np.zeros((2, 3)))
    got = _call(g, pkg, s)
    ident = np.zeros(142); ident[[6, 10, 14]] = 1.0
    assert np.array_equal(got[0], ident) and np.array_equal(got[1], ident)
    assert _call(g, pkg, dict(s, sample_start=np.array([0], dtype=np.int32))).shape == (0, 142)
    g.close()


# ---- the kernel against the independent 40-digit fixture ---------------------------------------------------------------------------
FIX = PC.fixture()
NAMES = [e["name"] for e in FIX["cases"]]


def _case_call(prob, c):
    s = PC.as_stream([c])
    return prob.preintegrate(s["sample_start"], s["t"], s["gyr"], s["acc"], s["t_prev"], s["t_curr"], s["bg"], s["ba"], c["gcov"], c["acov"])[0]


@pytest.mark.gpu
def test_hip_preintegration_matches_the_exact_fixture(pkg, orc, hip, capsys):
    """every case of the fixture, per block: |HIP - exact| <= max(4 |oracle - exact|, 8 n 2^-53); the oracle's distance is computed
    here.  A block that is exactly zero in the fixture must be exactly zero.  The distances are printed (pytest -s) for DESIGN.md 1."""
    g, o = pkg.new_problem(), orc.new_problem()
    bad = []
    for e in FIX["cases"]:
        c = PC.load(e)
        exact = np.array(e["expected"])
        n = max(e["n_steps"], 1)
        got, ref = _case_call(g, c), _case_call(o, c)
        eh, eo = PC.block_errors(got, exact), PC.block_errors(ref, exact)
        with capsys.disabled():
            print("preint_exact %-15s n=%-6d worst block, units of n 2^-53: oracle %-8s %8.3f   hip %-8s %8.3f" % (
                e["name"], e["n_steps"], max(eo, key=eo.get), max(eo.values()) / (n * U), max(eh, key=eh.get), max(eh.values()) / (n * U)))
            print("   hip per block: " + " ".join("%s %.2f" % (k, v / (n * U)) for k, v in eh.items()))
        for name in PC.BLOCKS:
            if not eh[name] <= max(4.0 * eo[name], 8.0 * n * U):
                bad.append((e["name"], name, eh[name], eo[name]))
        assert got[141] == ref[141]
    g.close(); o.close()
    assert not bad, bad


def _mixed(M, seed):
    """M intervals whose kinds -- empty, one step, the negative step only, 50 steps, 2000 steps, tiny angles, large rotation -- and
    biases change from lane to lane without a period, so that neighbours in a wave differ in schedule length by three orders of magnitude"""
    rng = np.random.default_rng(seed)
    kinds = ["empty", "one_sample", "negative_only", "euroc_1_1", "long_2000", "tiny_angle", "spin6_y"]
    base = {k: PC.load(FIX["cases"][NAMES.index(k)]) for k in kinds}
    order = [int(x) for x in rng.integers(0, len(kinds), size=M)]
    if M >= 7:
        order[:7] = [int(x) for x in rng.permutation(7)]      # every kind is present, the first wave holds all of them
    out = []
    for m in range(M):
        c = dict(base[kinds[order[m]]])
        v = int(rng.integers(0, 5))
        c["bg"] = c["bg"] + v * 1e-4; c["ba"] = c["ba"] - v * 1e-3
        c["key"] = (order[m], v)
        out.append(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 63, 64, 65, 130, 1000])
def test_hip_preintegration_mixed_waves_equal_the_intervals_alone(pkg, hip, M):
    """one call with all kinds of interval side by side: every row is, BIT FOR BIT, what that interval gives when submitted alone.
    What it finds: a lane that reads a neighbour's schedule or bias, an index past sched_start[M], aliasing of the private 142-double
    array.  E.g. a kernel that took `sched_start[m] + 50` for the end of lane m's schedule: an empty or one-step lane would run into
    its neighbours' steps (different samples and dt than the zero-filled tail it meets when alone) and a 2001-step lane, cut at 50 in
    both submissions, fails the fixture test above; only the 51-step lanes would survive."""
    cases = _mixed(M, 1000 + M)
    g = pkg.new_problem()
    s = PC.as_stream(cases)
    got = g.preintegrate(s["sample_start"], s["t"], s["gyr"], s["acc"], s["t_prev"], s["t_curr"], s["bg"], s["ba"], PC.GYR_COV, PC.ACC_COV)
    g.close()
    alone = {}
    h = pkg.new_problem()
    for c in cases:
        if c["key"] not in alone:
            alone[c["key"]] = _case_call(h, c)
    h.close()
    lens = sorted({len(PC.schedule(c)) for c in cases})
    assert M < 7 or (lens[0] == 0 and lens[-1] >= 2000)
    for m, c in enumerate(cases):
        assert np.array_equal(got[m], alone[c["key"]]), (M, m, c["key"])


def _short_stream(M, per, seed):
    """M intervals of `per` samples each at 200 Hz, all inside the interval (per steps each); stamps near 1.4e9 s"""
    rng = np.random.default_rng(seed)
    t_prev = LD("1403636579.763555527") + LD(per) * LD("0.005") * np.arange(M, dtype=LD)
    t = (t_prev[:, None] + LD("0.005") * np.arange(1, per + 1, dtype=LD)[None, :]).reshape(-1)
    S = M * per
    return dict(sample_start=(np.arange(M + 1) * per).astype(np.int32), t=t, gyr=rng.normal(size=(S, 3)) * 0.3, acc=rng.normal(size=(S, 3)) * 2.0 + np.array([0, 0, 9.81]),
                t_prev=t_prev, t_curr=t_prev + LD(per) * LD("0.005"), bg=rng.normal(size=(M, 3)) * 1e-3, ba=rng.normal(size=(M, 3)) * 1e-2)


def _slice(s, m0, m1):
    a, b = int(s["sample_start"][m0]), int(s["sample_start"][m1])
    return dict(sample_start=(s["sample_start"][m0:m1 + 1] - a).astype(np.int32), t=s["t"][a:b], gyr=s["gyr"][a:b], acc=s["acc"][a:b],
                t_prev=s["t_prev"][m0:m1], t_curr=s["t_curr"][m0:m1], bg=s["bg"][m0:m1], ba=s["ba"][m0:m1])


def _in_small_calls(pkg, s, chunk):
    h = pkg.new_problem()
    M = len(s["t_prev"])
    out = np.concatenate([_call(h, pkg, _slice(s, m0, min(m0 + chunk, M))) for m0 in range(0, M, chunk)])
    h.close()
    return out


@pytest.mark.gpu
def test_hip_preintegration_chunked_read_back(pkg, hip):
    """M = 4000 intervals: the output (4000 * 142 * 8 = 4.5 MB) exceeds the 4 MiB bounce buffer of the blocking device-to-host copy
    (StageArea::XFER, plba_problem.h), so it comes back in two pieces; bit for bit what calls of 250 intervals on a fresh handle give"""
    s = _short_stream(4000, 4, 21)
    assert 4000 * 142 * 8 > (4 << 20)
    g = pkg.new_problem()
    got = _call(g, pkg, s)
    g.close()
    assert np.array_equal(got, _in_small_calls(pkg, s, 250))
    assert np.abs(got[-1, 60:141]).max() > 0 and got[-1, 141] > 0


@pytest.mark.gpu
def test_hip_preintegration_uploads_beyond_the_staging_area(pkg, hip):
    """The queued uploads of one call go through the pinned staging area the context allocates in plba_create (plba_api.hip: 64 MiB, of
    which the last 4 MiB are the bounce buffer: 60 MiB for uploads), in the order schedule starts, schedule indices (4 B / step),
    schedule dt (8 B / step), gyro table (24 B / sample), accelerometer table (24 B / sample), biases.  With 4400 intervals of 250
    samples (1.1 M samples, all of them steps) the first four take 39.6 MB and the ACCELEROMETER table (26.4 MB) no longer fits: it is
    copied from the caller's pageable memory, the biases after it are staged again.  The smallest stream that overflows has 1.05 M
    samples; building this one takes well under a second of host time.  Bit for bit what calls of 200 intervals on a fresh handle give."""
    M, per = 4400, 250
    up = (64 << 20) - (4 << 20)
    S = M * per
    assert 4 * (M + 1) + 12 * S + 24 * S + 4 * 256 <= up < 4 * (M + 1) + 12 * S + 48 * S
    s = _short_stream(M, per, 22)
    g = pkg.new_problem()
    got = _call(g, pkg, s)
    again = _call(g, pkg, _slice(s, 10, 75))      # the same handle after the overflow: the staging area starts over
    g.close()
    small = _in_small_calls(pkg, s, 200)
    assert np.array_equal(got, small)
    assert np.array_equal(again, small[10:75])


@pytest.mark.gpu
def test_hip_preintegration_twice_on_one_handle(pkg, hip):
    """two calls in a row on one handle, the second with fewer intervals: nothing of the first call's tables or output is left in it"""
    a, b = _short_stream(130, 50, 23), _short_stream(37, 20, 24)
    g = pkg.new_problem()
    first, second = _call(g, pkg, a), _call(g, pkg, b)
    g.close()
    assert np.array_equal(first, _in_small_calls(pkg, a, 130)) and np.array_equal(second, _in_small_calls(pkg, b, 37))


@pytest.mark.gpu
def test_hip_preintegration_between_upload_and_optimize(pkg, hip):
    """plba_preintegrate starts the context's staging area over (DArrStreamScope).  Called on a handle between the upload of a window
    and its optimize(), and between the two optimize() stages of the local BA, it leaves the optimisation bit-identical -- trace and
    final states -- and returns what it returns on a fresh handle."""
    w = pkg.window.make_window(12, 260, 50, imu=True, seed=77)
    s = _short_stream(11, 50, 25)
    want = _in_small_calls(pkg, s, 11)

    def run(interleave):
        g = pkg.new_problem(); g.upload_window(w)
        pre = []
        if interleave: pre.append(_call(g, pkg, s))
        g.optimize(pkg.protocol.STAGE1_ITERS)
        tr = [g.trace()]
        gated = g.gate_outliers(pkg.window.CHI2_GATE)
        if interleave: pre.append(_call(g, pkg, s))
        g.optimize(pkg.protocol.STAGE2_ITERS)
        tr.append(g.trace())
        res = pkg.protocol.results(g)
        g.close()
        return tr, gated, res, pre
    tr0, gated0, res0, _ = run(False)
    tr1, gated1, res1, pre = run(True)
    assert len(tr0[0]) > 0 and len(tr0[1]) > 0 and tr0 == tr1 and gated0 == gated1
    for k in res0:
        assert np.array_equal(res0[k], res1[k]), k
    assert np.array_equal(pre[0], want) and np.array_equal(pre[1], want)
