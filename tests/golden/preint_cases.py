"""Inputs of the 40-digit IMU preintegration fixture (tests/golden/preint_exact.json), shared by its generator
(make_preint_exact.py) and by the tests.  numpy only; nothing here computes a preintegration.

A case is ONE keyframe interval: decimal time stamps (strings: a double cannot hold a ns stamp near 1.4e9 s), the raw gyro /
accelerometer samples, the biases and the two noise densities.  Short cases are written into the JSON in full; a long stream is
stored as (kind, parameters, seed) and rebuilt by `build()`, and the JSON keeps the SHA-256 of the rebuilt arrays."""
import hashlib

import numpy as np

GYR_COV = 1.7e-4 * 1.7e-4 / 0.005            # IMU/imudata.cpp:27
ACC_COV = 2.0e-3 * 2.0e-3 / 0.005 * 100      # IMU/imudata.cpp:28
LD = np.longdouble


def stamp(ns):
    """integer nanoseconds -> exact decimal string of seconds"""
    return "%d.%09d" % (ns // 10**9, ns % 10**9)


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _grid(t0_ns, n_before, n_in, n_after, rng=None, jitter_ns=0, period_ns=5_000_000, offset_ns=700_000):
    """sample stamps of one interval [t0, t0 + n_in * period]: n_before samples older than the first image, n_after past the second"""
    k = np.arange(-n_before, n_in + n_after)
    ns = t0_ns + offset_ns + k * period_ns
    if jitter_ns:
        ns = np.sort(ns + rng.integers(-jitter_ns, jitter_ns + 1, size=len(k)))
    return [stamp(int(x)) for x in ns], stamp(t0_ns), stamp(t0_ns + n_in * period_ns)


def build(kind, seed=0, **p):
    """-> dict(t=[str], t_prev=str, t_curr=str, gyr (S,3), acc (S,3), bg (3,), ba (3,), gcov, acov)"""
    rng = np.random.default_rng(seed)
    gcov, acov = p.get("gcov", GYR_COV), p.get("acov", ACC_COV)
    grav = np.array([0.0, 0.0, 9.81])
    if kind == "euroc":          # ns stamps near 1.4e9 s, jitter, non-zero biases, samples outside the interval on both sides
        t, tp, tc = _grid(1403636579_763555527, p["n_before"], p.get("n_in", 50), p["n_after"], rng, jitter_ns=p.get("jitter_ns", 1000))
        S = len(t)
        gyr = rng.normal(size=(S, 3)) * 0.3; acc = rng.normal(size=(S, 3)) * 2.0 + grav
        bg = rng.normal(size=3) * 1e-3; ba = rng.normal(size=3) * 1e-2
    elif kind == "tiny":         # |w dt| at and around the 1e-10 (Expmap) and 1e-5 (JacobianR) thresholds; gyr == bg bit for bit on some steps
        per = 3_906_250          # 2^-8 s: every stamp is a binary fraction, so every dt is exactly one period (a uniform case)
        t, tp, tc = _grid(100_000_000_000, 0, 28, 1, offset_ns=0, period_ns=per)
        t = t[1:]                # first sample one period after the first image, the last one on the second
        S = len(t)
        bg = np.array([1.25e-3, -2.5e-3, 0.75e-3]); ba = rng.normal(size=3) * 1e-2
        acc = rng.normal(size=(S, 3)) * 2.0 + grav
        targets = [0.0, 5e-11, 2e-10, 5e-6, 2e-5, 9.9e-6, 1.1e-5]
        gyr = np.empty((S, 3))
        for s in range(S):
            d = _unit(rng.normal(size=3))
            th = targets[s % 7] if s % 8 != 7 else 1.5e-3
            gyr[s] = bg + d * (th / (per * 1e-9))
            if th == 0.0: gyr[s] = bg
    elif kind == "spin":         # constant rate about a skew axis: accumulated rotation runs through pi (q.w < 0, R_to_q's three trace <= 0 branches)
        t, tp, tc = _grid(250_000_000_000, 1, p["n_in"], 1)
        S = len(t)
        bg = rng.normal(size=3) * 1e-3; ba = rng.normal(size=3) * 1e-2
        gyr = bg + _unit(p["axis"]) * p["rate"] + rng.normal(size=(S, 3)) * p.get("wobble", 0.0)
        acc = rng.normal(size=(S, 3)) * 1.0 + grav
    elif kind == "stamps":       # degenerate schedules, stamps given literally (seconds offsets in ns from t_prev)
        base = 1403636600_000000000
        t = [stamp(base + x) for x in p["t_ns"]]; tp, tc = stamp(base), stamp(base + p["curr_ns"])
        S = len(t)
        gyr = rng.normal(size=(S, 3)) * 0.3; acc = rng.normal(size=(S, 3)) * 2.0 + grav
        bg = rng.normal(size=3) * 1e-3; ba = rng.normal(size=3) * 1e-2
    elif kind == "long":         # tracking lost for seconds: n steps at 200 Hz, smooth motion plus sensor noise
        n = p["n"]
        t, tp, tc = _grid(1403636700_000000000, 1, n, 1, rng, jitter_ns=1000)
        S = len(t)
        x = np.arange(S)[:, None] * 0.005
        gyr = 0.4 * np.sin(x * np.array([0.7, 1.1, 0.5]) + np.array([0.1, 1.0, 2.0])) + rng.normal(size=(S, 3)) * 0.01
        acc = grav + 1.5 * np.sin(x * np.array([0.9, 0.6, 1.3]) + np.array([2.0, 0.3, 1.1])) + rng.normal(size=(S, 3)) * 0.05
        bg = rng.normal(size=3) * 1e-3; ba = rng.normal(size=3) * 1e-2
        gyr = gyr + bg; acc = acc + ba
    elif kind == "scale":        # sample magnitudes from 1e-4 to 150, biases of the samples' own size
        t, tp, tc = _grid(1403636800_000000000, 1, 50, 1, rng, jitter_ns=1000)
        S = len(t)
        gs, as_ = p["gyr_scale"], p["acc_scale"]
        bg = rng.normal(size=3) * (gs if p.get("big_bg") else 1e-3); ba = rng.normal(size=3) * (as_ if p.get("big_ba") else 1e-2)
        gyr = bg + rng.normal(size=(S, 3)) * gs; acc = ba + rng.normal(size=(S, 3)) * as_
    else:
        raise ValueError(kind)
    return dict(t=t, t_prev=tp, t_curr=tc, gyr=np.ascontiguousarray(gyr), acc=np.ascontiguousarray(acc), bg=np.ascontiguousarray(bg),
                ba=np.ascontiguousarray(ba), gcov=float(gcov), acov=float(acov))


# name, family, kind, parameters.  Cases with more than STORE_MAX samples are stored as parameters + hash only.
STORE_MAX = 64
CASES = [
    ("euroc_0_0", "euroc", "euroc", dict(seed=101, n_before=0, n_after=0)),
    ("euroc_1_1", "euroc", "euroc", dict(seed=102, n_before=1, n_after=1)),
    ("euroc_2_2", "euroc", "euroc", dict(seed=103, n_before=2, n_after=2)),
    ("tiny_angle", "threshold", "tiny", dict(seed=111)),
    ("spin6_x", "rotation", "spin", dict(seed=121, n_in=200, axis=[0.8, 0.45, -0.4], rate=6.0)),
    ("spin6_y", "rotation", "spin", dict(seed=122, n_in=200, axis=[-0.35, 0.85, 0.4], rate=6.0)),
    ("spin6_z", "rotation", "spin", dict(seed=123, n_in=200, axis=[0.4, -0.3, 0.87], rate=6.0)),
    ("cross_pi", "rotation", "spin", dict(seed=124, n_in=50, axis=[0.5, 0.6, 0.62], rate=15.0, wobble=0.5)),
    ("repeated_stamp", "degenerate", "stamps", dict(seed=131, t_ns=[4_000_000, 9_000_000, 9_000_000, 14_000_000, 19_000_000, 19_000_000, 24_000_000, 31_000_000], curr_ns=30_000_000)),
    ("one_sample", "degenerate", "stamps", dict(seed=132, t_ns=[-3_000_000, 2_000_000], curr_ns=250_000_000)),
    ("negative_only", "degenerate", "stamps", dict(seed=133, t_ns=[0, 253_000_000], curr_ns=250_000_000)),
    ("empty", "degenerate", "stamps", dict(seed=134, t_ns=[-7_000_000, -2_000_000], curr_ns=250_000_000)),
    ("long_2000", "long", "long", dict(seed=141, n=2000)),
    ("long_20000", "long", "long", dict(seed=142, n=20000)),
    ("acc_1e-3", "scale", "scale", dict(seed=151, gyr_scale=0.3, acc_scale=1e-3, big_ba=True)),
    ("acc_150", "scale", "scale", dict(seed=152, gyr_scale=0.3, acc_scale=150.0, big_ba=True)),
    ("gyr_1e-4", "scale", "scale", dict(seed=153, gyr_scale=1e-4, acc_scale=2.0, big_bg=True)),
    ("gyr_30", "scale", "scale", dict(seed=154, gyr_scale=30.0, acc_scale=2.0, big_bg=True)),
    ("noise_custom", "noise", "euroc", dict(seed=161, n_before=1, n_after=1, gcov=3.0e-5, acov=2.0e-2)),
    ("noise_gyr_zero", "noise", "euroc", dict(seed=162, n_before=1, n_after=1, gcov=0.0, acov=2.0e-2)),
    ("noise_acc_zero", "noise", "euroc", dict(seed=163, n_before=1, n_after=1, gcov=3.0e-5, acov=0.0)),
]


def digest(c):
    h = hashlib.sha256()
    h.update("|".join(c["t"] + [c["t_prev"], c["t_curr"]]).encode())
    for k in ("gyr", "acc", "bg", "ba"):
        h.update(np.ascontiguousarray(c[k], dtype="<f8").tobytes())
    h.update(np.array([c["gcov"], c["acov"]], dtype="<f8").tobytes())
    return h.hexdigest()


def load(entry):
    """the inputs of one JSON entry: stored in full, or rebuilt from (kind, params) and checked against the stored hash"""
    if "gyr" in entry:
        c = dict(t=list(entry["t"]), t_prev=entry["t_prev"], t_curr=entry["t_curr"], gyr=np.array(entry["gyr"], float).reshape(-1, 3),
                 acc=np.array(entry["acc"], float).reshape(-1, 3), bg=np.array(entry["bg"], float), ba=np.array(entry["ba"], float),
                 gcov=float(entry["gcov"]), acov=float(entry["acov"]))
    else:
        c = build(entry["kind"], **entry["params"])
    if digest(c) != entry["sha256"]:
        raise AssertionError("inputs of fixture case %s do not hash to the stored value" % entry["name"])
    return c


def schedule(c):
    """src/keyFrame.cpp:147-170 on long double stamps: [(sample index, dt as double)]"""
    t = np.array([LD(s) for s in c["t"]], dtype=LD)
    prev, curr = LD(c["t_prev"]), LD(c["t_curr"])
    n, i, out = len(t), 0, []
    while i < n and t[i] < prev:
        i += 1
    if i >= n:
        return out
    out.append((i, float(t[i] - prev))); i += 1
    while i < n and t[i] <= curr:
        out.append((i, float(t[i] - t[i - 1]))); i += 1
    if i < n:
        out.append((i, float(curr - t[i])))
    return out


def as_stream(cases):
    """several cases side by side as one plba_preintegrate call (M = len(cases))"""
    starts = np.cumsum([0] + [len(c["t"]) for c in cases]).astype(np.int32)
    cat = lambda k: np.concatenate([c[k].reshape(-1, 3) for c in cases]) if sum(len(c["t"]) for c in cases) else np.zeros((0, 3))
    return dict(sample_start=starts, t=np.array([LD(s) for c in cases for s in c["t"]], dtype=LD), gyr=cat("gyr"), acc=cat("acc"),
                t_prev=np.array([LD(c["t_prev"]) for c in cases], dtype=LD), t_curr=np.array([LD(c["t_curr"]) for c in cases], dtype=LD),
                bg=np.stack([c["bg"] for c in cases]), ba=np.stack([c["ba"] for c in cases]))


# ---- the error measure of every comparison with the fixture: per 3 x 3 block ---------------------------------------------------------
def _blocks():
    b = {"dP": np.arange(0, 3), "dV": np.arange(3, 6), "dR": np.arange(6, 15), "JPg": np.arange(15, 24), "JPa": np.arange(24, 33),
         "JVg": np.arange(33, 42), "JVa": np.arange(42, 51), "JRg": np.arange(51, 60)}
    for i, ni in enumerate("PVR"):
        for j, nj in enumerate("PVR"):
            b["cov_" + ni + nj] = np.array([60 + (3 * i + r) * 9 + 3 * j + c for r in range(3) for c in range(3)])
    return b


BLOCKS = _blocks()      # name -> indices into the 142-double payload (R = the rotation block phi)


def block_errors(got, exact):
    """name -> max |got - exact| / max |exact| of that block; a block that is exactly zero in `exact` gives inf unless `got` is zero too"""
    out = {}
    for name, ix in BLOCKS.items():
        den = np.abs(exact[ix]).max()
        num = np.abs(got[ix] - exact[ix]).max()
        out[name] = (0.0 if num == 0.0 else np.inf) if den == 0.0 else float(num / den)
    return out


def fixture():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "preint_exact.json")) as f:
        return json.load(f)
