// plba_pgo_sparse_dev.h — the device side of the multifrontal solve of plba_pgo_sparse.h (the analysis, the layout and the kernel
// sequence are described there): what the kernels read, who owns it, and the launchers of plba_pgo_sparse.hip.
#pragma once
#include "plba_pgo_sparse.h"
#include "plba_problem.h"

namespace plba {

// what the kernels read (device pointers)
struct PgoSparseDev {
    const int32_t *f_m, *f_np, *f_row0, *rows, *umap, *ch_start, *ch, *as_start, *as, *lv;
    const long long *f_off, *f_roff;
    double* F;                  // frontal matrices
    double* R;                  // their right-hand sides
    const double* Hblk;         // nblk x 36, undamped
    const double* b;            // P
    double* x;                  // P, free-vertex order
    Ctrl* c;                    // lambda in, solver_ok out
    const int* done;            // PgoCtl::done
};

// The device image of a PgoSparsePlan and the fronts, and the PgoSparseDev fields that name them: every caller of the launchers holds
// one.  Hblk, b, x, c and done stay with the caller, who comes by them in its own way.
struct PgoSparseWork {
    DArr<int32_t> f_m, f_np, f_row0, rows, umap, ch_start, ch, as_start, as, lv;
    DArr<long long> f_off, f_roff;
    DArr<double> F, R;
    // under the caller's DArrStreamScope: the copies are queued and nothing waits, so `pl` stays alive and unchanged until the caller has
    // waited for the stream.  The empty `ch` of a one-front plan becomes DArr::upload's one zeroed element; F and R are not cleared.
    hipError_t upload(const PgoSparsePlan& pl) {
        hipError_t e;
        if ((e = f_m.upload(pl.f_m)) || (e = f_np.upload(pl.f_np)) || (e = f_row0.upload(pl.f_row0)) || (e = rows.upload(pl.rows)) || (e = umap.upload(pl.umap)) ||
            (e = ch_start.upload(pl.ch_start)) || (e = as_start.upload(pl.as_start)) || (e = as.upload(pl.as)) || (e = lv.upload(pl.lv)) ||
            (e = f_off.upload(pl.f_off)) || (e = f_roff.upload(pl.f_roff)) || (e = ch.upload(pl.ch)) || (e = F.alloc((size_t)pl.fsize, false))) return e;
        return R.alloc((size_t)pl.rsize, false);
    }
    void bind(PgoSparseDev& d) const {
        d.f_m = f_m.p; d.f_np = f_np.p; d.f_row0 = f_row0.p; d.rows = rows.p; d.umap = umap.p; d.ch_start = ch_start.p; d.ch = ch.p;
        d.as_start = as_start.p; d.as = as.p; d.lv = lv.p; d.f_off = f_off.p; d.f_roff = f_roff.p; d.F = F.p; d.R = R.p;
    }
    size_t bytes() const {      // of the fourteen buffers, for the callers' records
        return (f_m.n + f_np.n + f_row0.n + rows.n + umap.n + ch_start.n + ch.n + as_start.n + as.n + lv.n) * sizeof(int32_t) +
               (f_off.n + f_roff.n) * sizeof(long long) + (F.n + R.n) * sizeof(double);
    }
};

void pgo_sparse_launch(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s);      // one trial's solve
// its first two stages on their own (plba_pose_graph_marginals factors and then inverts): k_sps_assemble over every front; k_sps_factor
// level by level, bottom-up; k_sps_factor over the fronts lv[l0 .. l0 + count) of one level
void pgo_sparse_launch_assemble(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s);
void pgo_sparse_launch_factor_levels(const PgoSparseDev& d, const PgoSparsePlan& pl, hipStream_t s);
void pgo_sparse_launch_factor(const PgoSparseDev& d, int l0, int count, hipStream_t s);

}  // namespace plba
