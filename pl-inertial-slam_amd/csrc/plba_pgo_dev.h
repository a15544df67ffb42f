// plba_pgo_dev.h — the per-thread arithmetic of the pose-graph kernels (plba_pgo.hip): what one thread of k_pgo_edges does for its edge
// (EdgeSE3::computeError, linearizeOplus and the weighted blocks of buildHost: the 120-double record) and what one thread of
// k_pgo_update does for its vertex (VertexSE3::oplusImpl with its counter and re-orthogonalisation), as include/plba_g2o/types_slam3d.h
// restates them.  PLBA_HD, so that csrc/plba_pgo_hostcheck.cpp runs the same text on the CPU against the extended-precision reference
// (tests/pgo_exact.py); the product only ever runs these functions inside the kernels.
#pragma once
#include <stddef.h>

#include "plba_math.h"

namespace plba {
namespace pgo_dev {

constexpr int PGO_REC = 120;       // per-edge record: A00 = J0^T O J0 | A11 = J1^T O J1 | A10 = J1^T O J0 | g0 = J0^T O e | g1 = J1^T O e
constexpr int ORTHO_AFTER = 1000;  // VertexSE3::orthogonalizeAfter

struct Iso { M3 R; V3 t; };
PLBA_HD Iso iso_load(const double* p) {
    Iso a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.R.a[i] = p[i];
    a.t = v3(p[9], p[10], p[11]);
    return a;
}
PLBA_HD void iso_store(const Iso& a, double* p) {
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = a.R.a[i];
    p[9] = a.t.x; p[10] = a.t.y; p[11] = a.t.z;
}
// slam3d_detail::mul / inv / from_mqt / unit_q of include/plba_g2o/types_slam3d.h, on the plba_math.h helpers
PLBA_HD Iso iso_mul(const Iso& a, const Iso& b) { Iso r; r.R = mul(a.R, b.R); r.t = mul(a.R, b.t) + a.t; return r; }
PLBA_HD Iso iso_inv(const Iso& a) { Iso r; r.R = transpose(a.R); const V3 x = mul(r.R, a.t); r.t = v3(-x.x, -x.y, -x.z); return r; }
PLBA_HD Iso iso_from_mqt(const double* u) {
    Iso r;
    r.t = v3(u[0], u[1], u[2]);
    const double w2 = 1.0 - (u[3] * u[3] + u[4] * u[4] + u[5] * u[5]);
    if (w2 < 0) r.R = eye3();
    else { Q4 q; q.x = u[3]; q.y = u[4]; q.z = u[5]; q.w = sqrt(w2); r.R = q_to_R(q); }
    return r;
}
PLBA_HD Q4 unit_q(const M3& R) {
    Q4 q = q_normalized(R_to_q(R));
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    return q;
}

// EdgeSE3::computeError (+ linearizeOplus and the weighted blocks of buildHost when JAC): *echi = e^T O e, rec[PGO_REC] written when JAC.
// The host's entry to the text k_pgo_edges includes (plba_pgo_edge_body.inc).
template <bool JAC>
PLBA_HD void pgo_edge_eval(const Iso& Xi, const Iso& Xj, const Iso& Zi, const double* om_in, double* echi, double* rec_out) {
#define PGO_EDGE_OM om_in
#define PGO_EDGE_CHI (*echi)
#define PGO_EDGE_REC rec_out
#include "plba_pgo_edge_body.inc"
#undef PGO_EDGE_OM
#undef PGO_EDGE_CHI
#undef PGO_EDGE_REC
}

// One entry of a block's sum from one source of k_pgo_sum: slot 0 A00, 1 A11, 2 A10, 3 A10^T (the edge's vertex 1 has the lower free rank)
PLBA_HD double pgo_block_term(const double* rec, int slot, int r, int c) {
    return slot == 3 ? rec[72 + c * 6 + r] : rec[slot * 36 + r * 6 + c];
}

// VertexSE3::oplusImpl on the pose at xp: X <- X fromVectorMQT(u); the counter counts every call, rejected trials included
PLBA_HD void pgo_vertex_oplus(double* xp, const double* u, int* cnt) {
    Iso X = iso_mul(iso_load(xp), iso_from_mqt(u));
    if (++*cnt > ORTHO_AFTER) {      // approximateNearestOrthogonalMatrix: R -= 0.5 R (R^T R - I)
        *cnt = 0;
        M3 E = mulAtB(X.R, X.R);
        E.a[0] -= 1; E.a[4] -= 1; E.a[8] -= 1;
        const M3 RE = mul(X.R, E);
#pragma unroll
        for (int i = 0; i < 9; ++i) X.R.a[i] -= 0.5 * RE.a[i];
    }
    iso_store(X, xp);
}

}  // namespace pgo_dev
}  // namespace plba
