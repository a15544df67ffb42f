// plba_relpose_launch.h — what plba_relpose.hip lends to plba_match.hip (plba_verify_loop_candidates): the argument block of k_relpose,
// its launch, and the host code that turns a candidate's read-back into a plba_relpose_result.  The kernel itself stays in
// plba_relpose.hip; both entries run the same code object and the same host assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plba.h"
#include "plba_relpose_dev.h"

namespace plba {

constexpr int RP_OUT_D = 12 + 21 + 1 + 6 + 6;      // per candidate: T_inc (R, t), H (upper), e, logmap(T_inc), pose_inc
constexpr int RP_OUT_I = 4;                        // n_inliers, iters[2], status

struct RelposeDev {
    relpose::Opt o;
    const int32_t *pt_start, *ln_start;            // device, B + 1 each
    const double *P3, *uv2, *pq6, *l3, *T0;        // T0: B x 12 or null
    uint8_t *pt_in, *ln_in;
    double* out_d;                                 // B x RP_OUT_D
    int32_t* out_i;                                // B x RP_OUT_I
};

// null, or why plba_relative_pose refuses these options
const char* relpose_check_options(const plba_relpose_options& opt, double fx, double fy, double cx, double cy);
void relpose_set_options(const plba_relpose_options& opt, double fx, double fy, double cx, double cy, relpose::Opt& o);
// k_relpose for B candidates on stream s: one wave per candidate
hipError_t relpose_launch(const RelposeDev& d, int B, hipStream_t s);
// candidate's out_d / out_i (as read back) -> its result: rank, cov_eig and the decision bits, on the host
void relpose_assemble(const plba_relpose_options& opt, int n_features, const double* out_d, const int32_t* out_i, plba_relpose_result& r);

}  // namespace plba
