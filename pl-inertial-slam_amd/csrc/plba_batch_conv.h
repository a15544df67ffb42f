// plba_batch_conv.h — the pure parts of a batched front-end call (plba_batch_call.h): the layout of its one device block, the check of
// a CSR start array, and the small conversions between the caller's arrays and the kernels'.
//
// Standard library only (no HIP header): csrc/plba_batch_call_hostcheck.cpp compiles it with a plain C++ compiler under the host
// sanitizers (tests/test_batch_call_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace plba {

// sections of one block in declaration order, each on a 16-byte boundary; `off` is the end of what has been taken
struct Layout {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 15) & ~(size_t)15; return o; }
};

// what is wrong with a CSR start array over B sets (B + 1 entries) of at most max_rows rows each, or null; `too_many` is the text for a
// set over the cap
inline const char* check_starts(int B, const int32_t* st, int max_rows = INT32_MAX, const char* too_many = "a set has more rows than the call takes") {
    if (st[0] != 0) return "a start array does not begin at 0";
    for (int b = 0; b < B; ++b) {
        if (st[b + 1] < st[b]) return "a start array descends";
        if (st[b + 1] - st[b] > max_rows) return too_many;
    }
    return nullptr;
}

// a row-major 4 x 4 pose -> the kernels' 12 numbers (R row-major, then t), and back with the fixed last row
inline void pose_pack12(const double* m16, double* q12) {
    for (int i = 0; i < 3; ++i) { q12[i * 3] = m16[i * 4]; q12[i * 3 + 1] = m16[i * 4 + 1]; q12[i * 3 + 2] = m16[i * 4 + 2]; q12[9 + i] = m16[i * 4 + 3]; }
}
inline void pose_unpack16(const double* q12, double* m16) {
    for (int i = 0; i < 3; ++i) { m16[i * 4] = q12[i * 3]; m16[i * 4 + 1] = q12[i * 3 + 1]; m16[i * 4 + 2] = q12[i * 3 + 2]; m16[i * 4 + 3] = q12[9 + i]; }
    m16[12] = m16[13] = m16[14] = 0.0; m16[15] = 1.0;
}

// the 21 upper entries of a symmetric 6 x 6, row by row -> the full matrix
inline void sym6_expand(const double* u21, double* m36) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { m36[i * 6 + j] = u21[k]; m36[j * 6 + i] = u21[k]; ++k; }
}

// a caller's inlier mask as the kernels read it: 1 for every nonzero byte, all ones when the caller passed none
inline void mask_normalise(const uint8_t* in, size_t n, uint8_t* out) {
    if (!in) { if (n) memset(out, 1, n); return; }
    for (size_t i = 0; i < n; ++i) out[i] = in[i] ? 1 : 0;
}

}  // namespace plba
