// Host-compiled wrapper around plba_twin_plan.h used ONLY by tests/test_twin_plan_cpu.py: the layout of a variant, the launch count
// the segment-length choice asks for, and a built plan read back table by table.  That this file compiles without any HIP header is
// the check that plba_twin_plan.h is standard-library code.  Not linked into libplba_hip.so and never used by the product path.
#include <string.h>
#include <string>
#include "plba_twin_plan.h"
using namespace plba;

static_assert(sizeof(TwinTile) == 12, "six int16_t: k_chol32_list reads the list as uploaded");

extern "C" {
// out12 = [nch, nC, w0, w1, w2, stage1, sep0, lenA, lenB, final0, launches, 0]; returns valid
int tp_layout(int T, int hbt, int variant, int32_t* out12) {
    const TwinLayout L = twin_layout(T, hbt, variant);
    const int32_t v[12] = {L.nch, L.nC, L.w[0], L.w[1], L.w[2], L.stage1, L.sep0, L.lenA, L.lenB, L.final0, L.launches, 0};
    memcpy(out12, v, sizeof v);
    return L.valid ? 1 : 0;
}
int tp_launches(int T, int hbt) { return twin_plan_launches(T, hbt); }
void* tp_new() { return new TwinPlan; }
void tp_free(void* h) { delete (TwinPlan*)h; }
int tp_build(void* h, int T, int hbt) { return twin_plan_build(T, hbt, *(TwinPlan*)h) ? 1 : 0; }
// [T, final0, sep0, nchains, nlaunch] and summary[5] of the plan built last
void tp_scalars(void* h, int32_t* i5, double* summary5) {
    const TwinPlan& pl = *(TwinPlan*)h;
    const int32_t v[5] = {pl.T, pl.final0, pl.sep0, pl.nchains, pl.nlaunch};
    memcpy(i5, v, sizeof v); memcpy(summary5, pl.summary, sizeof pl.summary);
}
// bytes of table <name>, copied to out when it has room; -1: no such table
long tp_get(void* h, const char* name, void* out, long cap) {
    const TwinPlan& pl = *(TwinPlan*)h;
    const std::string n = name;
    long bytes = -1;
    auto take = [&](const auto& v) {
        bytes = (long)(v.size() * sizeof(v[0]));
        if (out && bytes && bytes <= cap) memcpy(out, v.data(), (size_t)bytes);
    };
    if (n == "perm") take(pl.perm); else if (n == "xmap") take(pl.xmap); else if (n == "fac") take(pl.fac);
    else if (n == "off") take(pl.off); else if (n == "list") take(pl.list); else if (n == "cs_order") take(pl.cs_order);
    return bytes;
}
}
