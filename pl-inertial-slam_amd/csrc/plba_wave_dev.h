// plba_wave_dev.h — the cross-lane steps of the one-wave-per-problem kernels (k_relpose, k_track): the fixed 64-lane butterfly sum and
// the broadcast of lane 0's verdict and pose.
//
// The butterfly is a contract with the host checks (relpose::tree_sum spells the same tree out): quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror and row_mirror inside a DPP row of 16, then lanes ^ 16 and ^ 32 across the rows.  Every step adds the two
// operands of a pair in both of its lanes, so all 64 lanes end with the same bits.  The control words and their order are fixed: a
// device result is compared with the host's for equality.
#pragma once
#include <hip/hip_runtime.h>

namespace plba {

template <int CTRL>
__device__ __forceinline__ double wave_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, the same bits in all of them
__device__ __forceinline__ double wave_sum64(double v) {
    v += wave_dpp<0xB1>(v);
    v += wave_dpp<0x4E>(v);
    v += wave_dpp<0x141>(v);
    v += wave_dpp<0x140>(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int wave_sum64_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// lane 0's pose (R row-major, t) and flag to every lane; returns the flag
__device__ __forceinline__ int wave_lead(int go, double (&R)[9], double (&t)[3]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = __shfl(R[i], 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = __shfl(t[i], 0);
    return __shfl(go, 0);
}

}  // namespace plba
