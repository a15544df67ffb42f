// plba_pgo_edge_body.inc — the body of one edge's evaluation, included as text by k_pgo_edges (plba_pgo.hip) and by pgo_edge_eval
// (plba_pgo_dev.h): EdgeSE3::computeError, then (JAC) linearizeOplus and the weighted blocks of buildHost.  Text and not a call, because
// the compiler pairs the products of this body into FMAs differently once it reaches the kernel through an inlined function, and the
// kernel's results are pinned bit for bit.  The includer provides: JAC (a constant), Xi, Xj, Zi (Iso), and the macros PGO_EDGE_OM (the
// edge's 36 information entries), PGO_EDGE_CHI (where e^T O e goes) and PGO_EDGE_REC (the edge's record of PGO_REC doubles).
    const double* om = PGO_EDGE_OM;
    const Iso E = iso_mul(iso_mul(Zi, iso_inv(Xi)), Xj);
    const Q4 qe = unit_q(E.R);
    const double e[6] = {E.t.x, E.t.y, E.t.z, qe.x, qe.y, qe.z};
    double we[6], chi = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) t += om[i * 6 + j] * e[j];
        we[i] = t;
        chi += e[i] * t;
    }
    PGO_EDGE_CHI = chi;
    if (!JAC) return;
    // linearizeOplus: E = Z^-1 (Xi^-1 Xj) = Zi B, q its unit quaternion; derivation next to EdgeSE3::linearizeOplus
    const Iso B = iso_mul(iso_inv(Xi), Xj), E2 = iso_mul(Zi, B);
    const Q4 q = unit_q(E2.R);
    const M3 RZt = Zi.R, V = hat(v3(q.x, q.y, q.z)), TB = hat(B.t), RZtTB = mul(RZt, TB);
    M3 Qm, Qp;
#pragma unroll
    for (int i = 0; i < 9; ++i) { const double dg = (i % 4 == 0) ? q.w : 0.0; Qm.a[i] = dg - V.a[i]; Qp.a[i] = dg + V.a[i]; }
    const M3 QmRZt = mul(Qm, RZt);
    double J0[36], J1[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) { J0[i] = 0.0; J1[i] = 0.0; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            J0[r * 6 + c] = -RZt.a[r * 3 + c];
            J0[r * 6 + 3 + c] = 2.0 * RZtTB.a[r * 3 + c];
            J0[(3 + r) * 6 + 3 + c] = -QmRZt.a[r * 3 + c];
            J1[r * 6 + c] = E2.R.a[r * 3 + c];
            J1[(3 + r) * 6 + 3 + c] = Qp.a[r * 3 + c];
        }
    double* rec = PGO_EDGE_REC;
    // g_a = J_a^T O e  (b -= g_a in the sum)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) { t0 += J0[r * 6 + c] * we[r]; t1 += J1[r * 6 + c] * we[r]; }
        rec[108 + c] = t0; rec[114 + c] = t1;
    }
    // O J0 -> A00 = J0^T (O J0), A10 = J1^T (O J0); then O J1 -> A11
    double OJ[36];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { double t = 0.0;
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2) t += om[r * 6 + q2] * J0[q2 * 6 + c];
            OJ[r * 6 + c] = t; }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2) { t0 += J0[q2 * 6 + r] * OJ[q2 * 6 + c]; t1 += J1[q2 * 6 + r] * OJ[q2 * 6 + c]; }
            rec[r * 6 + c] = t0; rec[72 + r * 6 + c] = t1;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) { double t = 0.0;
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2) t += om[r * 6 + q2] * J1[q2 * 6 + c];
            OJ[r * 6 + c] = t; }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double t = 0.0;
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2) t += J1[q2 * 6 + r] * OJ[q2 * 6 + c];
            rec[36 + r * 6 + c] = t;
        }
