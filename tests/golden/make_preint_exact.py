#!/usr/bin/env python
"""Independent 40-digit values of the IMU preintegration producer, written to tests/golden/preint_exact.json.
      python tests/golden/make_preint_exact.py            (a few minutes: the 20 000-step case dominates)

The payload [dP dV dR JPg JPa JVg JVa JRg cov81 dt] that every IMU edge consumes is produced by four implementations of one
author (oracle/plba_oracle.c, window.preintegrate, plba_math.h::preint_update on host and device).  This script is a restatement
that shares no code with any of them: mpmath at 40 digits, written from the reference's text alone --
    IMU/IMUPreintegrator.cpp:56-75    reset
    IMU/IMUPreintegrator.cpp:80-139   update: DENSE 9 x 9 A, 9 x 3 Bg, Ca exactly as written there, cov = A cov A^T + Bg Sg Bg^T + Ca Sa Ca^T
    IMU/IMUPreintegrator.h:85-90      Expmap (identity below |v| < 1e-10)
    IMU/IMUPreintegrator.h:93-110     JacobianR (= IMU/so3.cpp:32-49; identity below theta < 1e-5)
    IMU/IMUPreintegrator.h:164-178    normalizeRotationQ / normalizeRotationM
    IMU/imudata.h:18-19, .cpp:27-28   the two noise matrices are multiples of the identity
    src/keyFrame.cpp:139-172          the step schedule, on long double stamps, every dt assigned to a double
-- with the SO(3) helpers of make_mp_vectors.py (itself independent: IMU/so3.cpp, Eigen's quaternion conversions).  Inputs come from
preint_cases.py (numpy only).  Doubles enter exactly; a decimal stamp is rounded to the 64-bit significand of a long double, differences
of stamps to 64 and then to 53 bits, as the reference's `double dt = imu._t - prev_t` does; results are rounded to double at the end.

The script checks ITSELF by two identities that do not restate the recurrences (both printed and stored per case):
  * bias Jacobians by central differences of the delta recurrence (dP, dV, dR only) in bg +- h e_k, ba +- h e_k;
  * cov = sum_k G_k diag(Sg, Sa) G_k^T, G_k = d(dP, dV, phi)/d(sample k), phi = Log(dR0^T dR), again by central differences.  The final
    state after perturbing sample k is obtained by composing the perturbed step with the unperturbed motion of the later steps
    ((P, V, R) o (p, v, r, T) = (P + V T + R p, V + R v, R r): the recurrence of cpp:115-117 is exactly this composition, checked against
    a plain re-run on the first case), so the sum costs O(n) steps, not O(n^2).
h = 1e-12.  A central difference at 40 digits is off by h^2 / 6 times the ratio of third to first derivative; every further derivative
in a sample brings at most one factor S = max(T, |w|max T, |a|max T^2) (sensitivity of the final state to a unit change of a sample), so
the identities are asserted to  h^2 (1 + S)^2  relative to each block's largest entry -- 1e-14 at worst (100 s), far below fp64.
The differences are taken of the SMOOTH map (Expmap without its identity shortcut, a change of the state below 1e-10); where the reference
takes JacobianR = I (theta < 1e-5) its covariance and JRg are NOT the derivative of its own map but off by theta / 2 relative on that step
(SURVEY App. B-Q16): on a case with such steps the bound is widened by the largest such theta, both sides are stored, and the
fixture follows the reference's text."""
import json
import os
import sys
from multiprocessing import Pool

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_mp_vectors as so3      # noqa: E402  (SO(3) / quaternion helpers; sets mp.dps = 40)
import preint_cases as PC          # noqa: E402

mp.mp.dps = 40
H = mp.mpf("1e-12")
I3 = mp.eye(3)


def ld_stamp(s):      # decimal string -> long double (64-bit significand, round to nearest even)
    return mp.mpf(s, prec=64, rounding="n")


def as_double(x):      # `double dt = <long double expression>`
    return mp.mpf(mp.mpf(x, prec=64, rounding="n"), prec=53, rounding="n")


def schedule(c):      # src/keyFrame.cpp:147-170; a bound check where the reference has none (:150) -- an interval without samples takes no step
    t = [ld_stamp(s) for s in c["t"]]
    prev, curr = ld_stamp(c["t_prev"]), ld_stamp(c["t_curr"])
    n, i, out = len(t), 0, []
    while i < n and t[i] < prev:      # :150-152
        i += 1
    if i >= n:
        return out
    out.append((i, as_double(t[i] - prev))); i += 1      # :153-157
    while i < n and t[i] <= curr:      # :158-164
        out.append((i, as_double(t[i] - t[i - 1]))); i += 1
    if i < n:      # :165-170, dt = curr_t - t[i] as written (negative)
        out.append((i, as_double(curr - t[i])))
    return out


def expmap(v, smooth=False):      # IMU/IMUPreintegrator.h:85-90
    if not smooth and so3.vnorm(v) < mp.mpf("1e-10"):
        return mp.eye(3)
    return so3.quat_to_R(so3.so3_exp(v))      # SO3::exp(v).matrix(), IMU/so3.cpp:171-175, 257-280


def normalize_rotation(R):      # IMU/IMUPreintegrator.h:164-178
    q = so3.R_to_quat(R)      # Quaterniond qr(R)
    if q[3] < 0:
        q = [-x for x in q]
    return so3.quat_to_R(so3.quat_normalized(q))


def vec(m):
    return [m[0], m[1], m[2]]


def delta_step(P, V, R, w, a, dt, smooth=False):      # cpp:84, 115-117
    dR = expmap([w[0] * dt, w[1] * dt, w[2] * dt], smooth)
    Ra = R * so3.col(a)
    dt2 = dt * dt
    P = P + V * dt + Ra * dt2 / 2
    V = V + Ra * dt
    return P, V, normalize_rotation(R * dR)


def delta_run(steps, smooth=False):
    P, V, R = mp.zeros(3, 1), mp.zeros(3, 1), mp.eye(3)
    for w, a, dt in steps:
        P, V, R = delta_step(P, V, R, w, a, dt, smooth)
    return P, V, R


def full_run(steps, gcov, acov):      # IMU/IMUPreintegrator.cpp:56-75 then :80-139 per step
    P, V, R = mp.zeros(3, 1), mp.zeros(3, 1), mp.eye(3)
    JPg, JPa, JVg, JVa, JRg = (mp.zeros(3) for _ in range(5))
    cov = mp.zeros(9)
    T = mp.mpf(0)
    T_double = mp.mpf(0)
    Sg, Sa = I3 * gcov, I3 * acov      # getGyrMeasCov / getAccMeasCov
    for w, a, dt in steps:
        dt2 = dt * dt      # :82
        wdt = [w[0] * dt, w[1] * dt, w[2] * dt]
        dR = expmap(wdt)      # :84
        Jr = so3.so3_Jr(wdt)      # :85
        RS = R * so3.hat(a)
        A = mp.eye(9)      # :90-94
        A[6:9, 6:9] = dR.T
        A[3:6, 6:9] = -RS * dt
        A[0:3, 6:9] = -RS * dt2 / 2
        A[0:3, 3:6] = I3 * dt
        Bg = mp.zeros(9, 3); Bg[6:9, 0:3] = Jr * dt      # :95-96
        Ca = mp.zeros(9, 3); Ca[3:6, 0:3] = R * dt; Ca[0:3, 0:3] = R * dt2 / 2      # :97-99
        cov = A * cov * A.T + Bg * Sg * Bg.T + Ca * Sa * Ca.T      # :100-102
        JPa = JPa + JVa * dt - R * dt2 / 2      # :107
        JPg = JPg + JVg * dt - RS * JRg * dt2 / 2      # :108
        JVa = JVa - R * dt      # :109
        JVg = JVg - RS * JRg * dt      # :110
        JRg = dR.T * JRg - Jr * dt      # :111
        Ra = R * so3.col(a)
        P = P + V * dt + Ra * dt2 / 2      # :115
        V = V + Ra * dt      # :116
        R = normalize_rotation(R * dR)      # :117
        T = T + dt      # :137
        T_double = mp.mpf(T_double + dt, prec=53, rounding="n")      # _delta_time is a double: the step-by-step rounded sum
    return dict(dP=P, dV=V, dR=R, JPg=JPg, JPa=JPa, JVg=JVg, JVa=JVa, JRg=JRg, cov=cov, dt=T_double, T=T)


def log_near_identity(R):      # rotation vector of a rotation within pi / 2 of the identity
    v = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]
    s = so3.vnorm(v)
    f = mp.mpf(1) if s == 0 else mp.asin(s) / s
    return [f * x for x in v]


def relblock(got, ref):
    den = max(abs(x) for x in ref)
    num = max(abs(x - y) for x, y in zip(got, ref))
    return (num / den) if den != 0 else num


def check_jacobians(steps_of, out):
    """central differences of (dP, dV, Log(dR0^T dR)) in the two biases against JPg JPa JVg JVa JRg"""
    _, _, R0 = delta_run(steps_of(None, None), smooth=True)
    cols = {k: [] for k in ("JPg", "JPa", "JVg", "JVa", "JRg")}
    for which in ("g", "a"):
        for k in range(3):
            e = [mp.mpf(0)] * 3; e[k] = H
            lo = delta_run(steps_of(*(([-x for x in e], None) if which == "g" else (None, [-x for x in e]))), smooth=True)
            hi = delta_run(steps_of(*((e, None) if which == "g" else (None, e))), smooth=True)
            cols["JP" + which].append(vec((hi[0] - lo[0]) / (2 * H)))
            cols["JV" + which].append(vec((hi[1] - lo[1]) / (2 * H)))
            if which == "g":
                ph, pl = log_near_identity(R0.T * hi[2]), log_near_identity(R0.T * lo[2])
                cols["JRg"].append([(x - y) / (2 * H) for x, y in zip(ph, pl)])
    res = {}
    for name, cs in cols.items():
        fd = [cs[c][r] for r in range(3) for c in range(3)]
        res[name] = relblock(fd, [out[name][r, c] for r in range(3) for c in range(3)])
    return res


def compose(a, b):      # (P, V, R) then the motion (p, v, r, T) of the later steps
    P, V, R = a
    p, v, r, T = b
    return P + V * T + R * p, V + R * v, R * r


def check_covariance(steps, gcov, acov, out, cross_check):
    n = len(steps)
    states = [(mp.zeros(3, 1), mp.zeros(3, 1), mp.eye(3))]
    for w, a, dt in steps:
        states.append(delta_step(*states[-1], w, a, dt, smooth=True))
    Pf, Vf, Rf = states[-1]
    suffix = [None] * (n + 1)      # suffix[k] = motion of steps k .. n-1 relative to the state before step k
    suffix[n] = (mp.zeros(3, 1), mp.zeros(3, 1), mp.eye(3), mp.mpf(0))
    for k in range(n - 1, -1, -1):
        w, a, dt = steps[k]
        p1, v1, r1 = delta_step(mp.zeros(3, 1), mp.zeros(3, 1), mp.eye(3), w, a, dt, smooth=True)
        p, v, r, T = suffix[k + 1]
        suffix[k] = (p1 + v1 * T + r1 * p, v1 + r1 * v, r1 * r, dt + T)
    acc_cov = mp.zeros(9)
    for k in range(n):
        w, a, dt = steps[k]
        for src, var in ((0, gcov), (1, acov)):
            G = mp.zeros(9, 3)
            for c in range(3):
                ends = []
                for sg in (1, -1):
                    ww, aa = list(w), list(a)
                    if src == 0: ww[c] = ww[c] + sg * H
                    else: aa[c] = aa[c] + sg * H
                    fin = compose(delta_step(*states[k], ww, aa, dt, smooth=True), suffix[k + 1])
                    if cross_check and k in (0, n // 2):      # the composition against a plain re-run of every later step
                        st = list(steps); st[k] = (ww, aa, dt)
                        plain = delta_run(st, smooth=True)
                        dev = max(max(abs(x) for x in (fin[i] - plain[i])) for i in range(3))
                        assert dev < mp.mpf("1e-36"), ("composition", k, dev)
                    ends.append(vec(fin[0]) + vec(fin[1]) + log_near_identity(Rf.T * fin[2]))
                for r in range(9):
                    G[r, c] = (ends[0][r] - ends[1][r]) / (2 * H)
            acc_cov += G * G.T * var
    res = [[None] * 3 for _ in range(3)]
    for bi in range(3):
        for bj in range(3):
            ref = [out["cov"][3 * bi + r, 3 * bj + c] for r in range(3) for c in range(3)]
            got = [acc_cov[3 * bi + r, 3 * bj + c] for r in range(3) for c in range(3)]
            res[bi][bj] = relblock(got, ref)
    return res


def payload(out):
    f = lambda m: [float(m[r, c]) for r in range(m.rows) for c in range(m.cols)]
    return f(out["dP"]) + f(out["dV"]) + f(out["dR"]) + f(out["JPg"]) + f(out["JPa"]) + f(out["JVg"]) + f(out["JVa"]) + f(out["JRg"]) + f(out["cov"]) + [float(out["dt"])]


def run_case(idx):
    name, family, kind, params = PC.CASES[idx]
    c = PC.build(kind, **params)
    sched = schedule(c)
    bg, ba = so3.mpv(c["bg"]), so3.mpv(c["ba"])
    raw = [(so3.mpv(c["gyr"][i]), so3.mpv(c["acc"][i]), dt) for i, dt in sched]

    def steps_of(dbg, dba):      # gyr = imu._g - bg, acc = imu._a - ba (keyFrame.cpp:154-155); the subtraction is a double operation in the
        # reference, so the unperturbed samples are rounded to double; a perturbed bias is applied on top at 40 digits
        out = []
        for g, a, dt in raw:
            w = [mp.mpf(g[q] - bg[q], prec=53, rounding="n") - (dbg[q] if dbg else 0) for q in range(3)]
            x = [mp.mpf(a[q] - ba[q], prec=53, rounding="n") - (dba[q] if dba else 0) for q in range(3)]
            out.append((w, x, dt))
        return out
    steps = steps_of(None, None)
    gcov, acov = mp.mpf(c["gcov"]), mp.mpf(c["acov"])
    out = full_run(steps, gcov, acov)
    n = len(steps)
    entry = dict(name=name, family=family, n_steps=n, sha256=PC.digest(c), gcov=c["gcov"], acov=c["acov"])
    if len(c["t"]) <= PC.STORE_MAX:
        entry.update(t=c["t"], t_prev=c["t_prev"], t_curr=c["t_curr"], gyr=c["gyr"].tolist(), acc=c["acc"].tolist(), bg=c["bg"].tolist(), ba=c["ba"].tolist(),
                     sched_idx=[i for i, _ in sched], sched_dt=[float(dt) for _, dt in sched])
    else:
        entry.update(kind=kind, params=params)
    entry["expected"] = payload(out)
    if n:
        thetas = [so3.vnorm([w[q] * dt for q in range(3)]) for w, _, dt in steps]
        small = [th for th in thetas if 0 < th < mp.mpf("0.00001")]
        T = sum(abs(dt) for _, _, dt in steps)
        S = max([T] + [so3.vnorm(w) * T for w, _, _ in steps] + [so3.vnorm(a) * T * T for _, a, _ in steps])
        bound = H * H * (1 + S) ** 2 + (max(small) if small else 0)
        jac = check_jacobians(steps_of, out)
        cov = check_covariance(steps, gcov, acov, out, cross_check=(idx == 0))
        worst = max(list(jac.values()) + [x for r in cov for x in r])
        entry["selfcheck"] = dict(bound=float(bound), jac={k: float(v) for k, v in jac.items()}, cov=[[float(x) for x in r] for r in cov],
                                  steps_with_Jr_identity=len(small), largest_such_theta=float(max(small)) if small else 0.0)
        assert worst <= bound, (name, float(worst), float(bound))
    return entry


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        entries = pool.map(run_case, range(len(PC.CASES)), chunksize=1)
    for e in entries:
        sc = e.get("selfcheck")
        if sc:
            print("%-15s n=%-6d bound %.1e  jac %s  cov max %.1e" % (e["name"], e["n_steps"], sc["bound"], " ".join("%s %.1e" % kv for kv in sc["jac"].items()),
                                                                      max(x for r in sc["cov"] for x in r)))
        else:
            print("%-15s n=0" % e["name"])
    doc = dict(note="mpmath 40 digits from the reference's text, rounded to double; see make_preint_exact.py", digits=40, h=float(H),
               layout="dP3 dV3 dR9 JPg9 JPa9 JVg9 JVa9 JRg9 cov81 dt", cases=entries)
    with open(os.path.join(HERE, "preint_exact.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote preint_exact.json:", len(entries), "cases")


if __name__ == "__main__":
    main()
