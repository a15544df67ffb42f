#!/usr/bin/env python
"""40-digit values of single observations of the pre-init visual-only local BA, written to tests/golden/lba_obs_exact.json.
      python tests/golden/make_lba_obs_exact.py            (a second)

The per-observation residual norm n, weight w, pose row Jp and landmark row Jl of MapHandler::levMarquardtOptimizationLBA are restated
by the oracle, the device kernels and tests/lba_ref.py.  This script shares no code with any of them: mpmath scalars at 40 digits, term
by term from the reference's text --
    src/mapHandler.cpp:1479-1516      point observation (Tiw = inverse_se3(T_kf_w); Xwi; projection; gz2; the six terms; the landmark row
                                      rotated by Tiw's rotation; both divided by max(homogTh, norm))
    src/mapHandler.cpp:1558-1625      line observation: both end points' six / three terms from fx l_err(0) and fy l_err(1) AS WRITTEN
                                      (:1580-1581 set fxlx, fyly once; :1604-1614 reuse them for the end point), landmark rows scaled by
                                      l_err(0) and l_err(1), the pose row (Jij_Piw l_err(0) + Jij_Qiw l_err(1)) / max(homogTh, norm)
    stvo-pl/src/auxiliar.cpp:113-122  inverse_se3,     :556-559 robustWeightCauchy
    the camera's projection           (cx + fx X / Z, cy + fy Y / Z)
The line rows are not the derivative of the line residual, so no finite difference can pin them: this restatement does.
Inputs are doubles and enter exactly; results are written with 30 significant digits.  The file holds data only."""
import json
import os

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 40
CAM = [458.654, 457.296, 367.215, 248.375]
HOMOG_TH = 1e-7


def D(x):      # a double, exactly
    return mp.mpf(float(x))


def pose(rv, t):      # camera-to-world pose from a rotation vector (Rodrigues at 40 digits), ROUNDED to doubles: the rounded matrix is the input
    w = [D(v) for v in rv]
    th = mp.sqrt(sum(v * v for v in w))
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = mp.eye(3) if th == 0 else mp.eye(3) + K * (mp.sin(th) / th) + K * K * ((1 - mp.cos(th)) / th ** 2)
    return [[float(R[i, j]) for j in range(3)] + [float(t[i])] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]


def inverse_se3(T):      # auxiliar.cpp:113-122
    R = mp.matrix(3, 3); t = mp.matrix(3, 1)
    for i in range(3):
        t[i] = D(T[i][3])
        for j in range(3):
            R[i, j] = D(T[i][j])
    Rt = R.T
    return Rt, -(Rt * t)


def project(X):
    fx, fy, cx, cy = (D(v) for v in CAM)
    return cx + fx * X[0] / X[2], cy + fy * X[1] / X[2]


def six_terms(g, a, b):      # :1491-1506: gz2 and the row for (fxdx, fydy) = (a, b)
    gx, gy, gz = g[0], g[1], g[2]
    gz2 = gz * gz
    gz2 = 1 / max(D(HOMOG_TH), gz2)
    return [+gz2 * a * gz,
            +gz2 * b * gz,
            -gz2 * (a * gx + b * gy),
            -gz2 * (a * gx * gy + b * gy * gy + b * gz * gz),
            +gz2 * (a * gx * gx + a * gz * gz + b * gx * gy),
            +gz2 * (b * gx * gz - a * gy * gz)]


def row_times_R(v3, R):      # Jij_Xwj.transpose() * Tiw.block(0,0,3,3)
    return [sum(v3[i] * R[i, c] for i in range(3)) for c in range(3)]


def cauchy(n):      # auxiliar.cpp:556-559
    return 1 / (1 + n * n)


def point_observation(T, X, uv):
    R, t = inverse_se3(T)                                  # :1481
    Xwi = R * mp.matrix([D(v) for v in X]) + t             # :1482
    pu, pv = project(Xwi)                                  # :1483
    dx, dy = D(uv[0]) - pu, D(uv[1]) - pv                  # :1485
    n = mp.sqrt(dx * dx + dy * dy)                         # :1486
    fx, fy = D(CAM[0]), D(CAM[1])
    J = six_terms(Xwi, fx * dx, fy * dy)
    dn = max(D(HOMOG_TH), n)
    Jp = [v / dn for v in J]                               # :1507
    Jl = [v / dn for v in row_times_R(J[:3], R)]           # :1513
    return n, cauchy(n), Jp, Jl


def line_observation(T, PQ, l):
    R, t = inverse_se3(T)                                  # :1560
    Pwi = R * mp.matrix([D(v) for v in PQ[:3]]) + t
    Qwi = R * mp.matrix([D(v) for v in PQ[3:]]) + t
    pu, pv = project(Pwi)
    qu, qv = project(Qwi)
    l0, l1, l2 = (D(v) for v in l)
    e0 = l0 * pu + l1 * pv + l2                            # :1567
    e1 = l0 * qu + l1 * qv + l2                            # :1568
    n = mp.sqrt(e0 * e0 + e1 * e1)
    fxlx, fyly = D(CAM[0]) * e0, D(CAM[1]) * e1            # :1580-1581
    dn = max(D(HOMOG_TH), n)
    JP = six_terms(Pwi, fxlx, fyly)                        # :1584-1589
    JlP = [v * e0 / dn for v in row_times_R(JP[:3], R)]    # :1595
    JQ = six_terms(Qwi, fxlx, fyly)                        # :1604-1609 (fxlx, fyly unchanged)
    JlQ = [v * e1 / dn for v in row_times_R(JQ[:3], R)]    # :1615
    Jp = [(a * e0 + b * e1) / dn for a, b in zip(JP, JQ)]  # :1618
    return n, cauchy(n), Jp, JlP + JlQ, (e0, e1)


def exact_uv(T, X):      # the double nearest to the projection
    R, t = inverse_se3(T)
    return [float(v) for v in project(R * mp.matrix([D(v) for v in X]) + t)]


def cases():
    Ta = pose([0.02, -0.05, 0.01], [0.25, 0.03, 0.05])
    Tb = pose([-0.013, 0.04, 0.03], [0.75, -0.02, 0.15])
    Tc = pose([0.0, 0.0, 0.0], [0.5, 0.01, 0.1])            # identity rotation
    Td = pose([0.3, -0.2, 0.45], [1.5, -0.4, 0.3])
    out = []

    def point(name, T, X, uv, fixed=False):
        out.append(dict(name=name, kind="point", fixed=fixed, T=T, X=[float(v) for v in X], z=[float(v) for v in uv]))

    def line(name, T, PQ, l, fixed=False):
        out.append(dict(name=name, kind="line", fixed=fixed, T=T, X=[float(v) for v in PQ], z=[float(v) for v in l]))
    X1, X2, X3 = [0.8, -0.4, 6.5], [-1.9, 1.1, 4.2], [2.4, 0.9, 9.7]
    point("point_ordinary", Ta, X1, [v + d for v, d in zip(exact_uv(Ta, X1), (0.61, -0.37))])
    point("point_far_corner", Tb, X3, [v + d for v, d in zip(exact_uv(Tb, X3), (-1.9, 2.3))])
    point("point_identity_rotation", Tc, X2, [v + d for v, d in zip(exact_uv(Tc, X2), (0.05, 0.02))])
    point("point_large_rotation_large_residual", Td, X3, [v + d for v, d in zip(exact_uv(Td, X3), (14.0, -9.0))])
    point("point_below_homog_th", Ta, X2, [v + d for v, d in zip(exact_uv(Ta, X2), (3e-8, -2e-8))])
    point("point_residual_of_rounding_only", Tb, X1, exact_uv(Tb, X1))
    point("point_fixed_keyframe", Tb, X2, [v + d for v, d in zip(exact_uv(Tb, X2), (-0.4, 0.8))], fixed=True)

    def image_line(T, P, Q, dp, dq):      # normalised line through the two projections displaced by dp, dq pixels along the normal
        a, b = exact_uv(T, P), exact_uv(T, Q)
        ux, uy = b[0] - a[0], b[1] - a[1]
        nn = (ux * ux + uy * uy) ** 0.5
        nx, ny = -uy / nn, ux / nn
        a = [a[0] + dp * nx, a[1] + dp * ny]; b = [b[0] + dq * nx, b[1] + dq * ny]
        l = [a[1] - b[1], b[0] - a[0], a[0] * b[1] - a[1] * b[0]]
        h = (l[0] * l[0] + l[1] * l[1]) ** 0.5
        return [v / h for v in l]
    L1, L2 = X1 + [1.5, -0.1, 6.9], X2 + [-1.2, 1.8, 4.5]
    line("line_ordinary", Ta, L1, image_line(Ta, L1[:3], L1[3:], 0.7, 0.4))
    line("line_opposite_signs", Tb, L1, image_line(Tb, L1[:3], L1[3:], 0.9, -0.6))
    line("line_large_rotation", Td, L2, image_line(Td, L2[:3], L2[3:], -3.0, -5.5))
    line("line_below_homog_th", Ta, L2, image_line(Ta, L2[:3], L2[3:], 4e-8, -3e-8))
    line("line_fixed_keyframe", Tc, L2, image_line(Tc, L2[:3], L2[3:], 0.3, 1.1), fixed=True)
    return out


def main():
    s = lambda v: mp.nstr(v, 30)
    doc = []
    for c in cases():
        if c["kind"] == "point":
            n, w, Jp, Jl = point_observation(c["T"], c["X"], c["z"])
        else:
            n, w, Jp, Jl, e = line_observation(c["T"], c["X"], c["z"])
            if "opposite" in c["name"]:
                assert e[0] * e[1] < 0
        if "below" in c["name"] or "rounding_only" in c["name"]:
            assert n < HOMOG_TH
        else:
            assert n > HOMOG_TH
        c["expected"] = dict(n=s(n), w=s(w), Jp=[s(v) for v in Jp], Jl=[s(v) for v in Jl])
        doc.append(c)
        print("%-38s n = %s" % (c["name"], mp.nstr(n, 8)))
    with open(os.path.join(HERE, "lba_obs_exact.json"), "w") as f:
        json.dump(dict(note="mpmath 40 digits from the reference's text, 30 digits written; see make_lba_obs_exact.py", digits=40, cam=CAM, homog_th=HOMOG_TH,
                       cases=doc), f, indent=0)
        f.write("\n")
    print("wrote lba_obs_exact.json:", len(doc), "cases")


if __name__ == "__main__":
    main()
