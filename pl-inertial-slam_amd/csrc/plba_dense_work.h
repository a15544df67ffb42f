// plba_dense_work.h — the dense solver's workspace in numbers: how a dimension is padded, how many elements each buffer that launch_cholesky / launch_trsv_back
// work in holds, and when the explicit inverse is kept.  struct DenseWork (plba_problem.h) owns the buffers and names them in a DevBuf.  Standard library only
// (no HIP header): csrc/plba_dense_work_hostcheck.cpp compiles it with a plain C++ compiler under the host sanitizers (tests/test_dense_work_cpu.py).
#pragma once
#include <cstddef>

namespace plba {
constexpr int TILE = 64;          // dense tile edge (wavefront-wide)
constexpr int NINV_MAX_T = 32;    // explicit-inverse back-substitution up to this many 32-wide block steps (longer sums would outlast the pivot sweep)
inline int dense_ppad(int P) { const int r = (P + TILE - 1) / TILE * TILE; return r > TILE ? r : TILE; }      // up to the 64-wide tile, one at the least
inline bool ninv_fits(int Ppad) { return Ppad / 32 <= NINV_MAX_T; }      // N = L^-T rides through the factorisation (DevBuf::Ninv / Nwork); longer systems are back-substituted

// element counts for a system of Ppad rows (a multiple of 32; of 64 everywhere but the small compact system) at row stride ld
struct DenseCounts {
    size_t sys_len, x, Linv, LT32, rd32;   // augmented system and the factor of the same shape, (Ppad + 64) x ld | solution | 64 x 64 inverses of the diagonal tiles | transposed
                                           // diagonal blocks (the 32 x 32 inverses, DevBuf::Linv32, share the storage) | reciprocal diagonal
    size_t flow_flags, chol_flags, ninv;   // one flag per 64-wide tile | (T32 + 1) x T32 tile flags + T32 inverse flags | Ninv and Nwork, Ppad x ld each
};
inline DenseCounts dense_counts(int Ppad, int ld) {
    const size_t T64 = (size_t)(Ppad + TILE - 1) / TILE, T32 = (size_t)Ppad / 32;
    return {(size_t)(Ppad + TILE) * ld, (size_t)ld, T64 * TILE * TILE, (size_t)Ppad * 64, (size_t)Ppad, T64, (T32 + 2) * T32, (size_t)2 * Ppad * ld};
}
}  // namespace plba
