// plba_batch_call_hostcheck.cpp — a stand-alone program over plba_batch_conv.h, the HIP-free part of the batched calls' scaffold:
// the block layout, the CSR start check and the conversions, each against its statement in the header.  Built with a plain C++
// compiler under the address and undefined-behaviour sanitizers and run directly by tests/test_batch_call_cpu.py; every buffer is
// exactly as long as the function under test may touch, so a write past an end is a sanitizer report.
// Prints one line per group, `ok <group>`, and exits 0; the first failed check prints its text and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plba_batch_conv.h"

using namespace plba;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void layout() {
    const size_t sizes[] = {1, 0, 15, 16, 17, 0, 4 * 66, 32 * 3, 7};
    const size_t n = sizeof sizes / sizeof *sizes;
    Layout L;
    CHECK(L.off == 0);
    size_t prev_end = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t before = L.off, o = L.take(sizes[i]);
        CHECK(o == before);                      // declaration order: a section begins where the ones before it end
        CHECK(o % 16 == 0 && L.off % 16 == 0);
        CHECK(o >= prev_end);                    // disjoint
        CHECK(L.off >= o + sizes[i] && L.off - (o + sizes[i]) < 16);
        if (sizes[i] == 0) CHECK(L.off == before);      // a zero-byte section consumes nothing
        prev_end = o + sizes[i];
    }
    printf("ok layout\n");
}

static void starts() {
    { const std::vector<int32_t> st{0}; CHECK(check_starts(0, st.data()) == nullptr); }
    { const std::vector<int32_t> st{0, 0, 3, 3, 3, 9}; CHECK(check_starts(5, st.data()) == nullptr); }      // empty sets
    { const std::vector<int32_t> st{1, 2, 3}; CHECK(check_starts(2, st.data()) != nullptr); }               // a nonzero first entry
    { const std::vector<int32_t> st{0, 2, 5, 4}; CHECK(check_starts(3, st.data()) != nullptr); }            // a descent at the last set
    { const std::vector<int32_t> st{0, 2, 5, 4}; CHECK(check_starts(2, st.data()) == nullptr); }            // ... which B = 2 does not read
    const int cap = 8192;
    const char* text = "too many rows";
    { const std::vector<int32_t> st{0, 5, 5 + cap}; CHECK(check_starts(2, st.data(), cap, text) == nullptr); }
    { const std::vector<int32_t> st{0, 5, 5 + cap + 1}; CHECK(check_starts(2, st.data(), cap, text) == text); }
    { const std::vector<int32_t> st{0, cap + 1, cap + 1}; CHECK(check_starts(2, st.data(), cap, text) == text); }
    { const std::vector<int32_t> st{0, 5, 5 + cap + 1}; CHECK(check_starts(2, st.data()) == nullptr); }     // no cap given
    printf("ok starts\n");
}

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

static void poses() {
    // values whose bits a lossy path would change: a denormal, a negative zero, 1 + one ulp, a large and a tiny magnitude
    std::vector<double> m(16);
    const double vals[12] = {5e-324, -0.0, 1.0000000000000002, -3.5e300, 7.25e-300, 0.1, -0.2, 0.3, 1.0 / 3.0, -2.0 / 3.0, 123456.789, -1e-17};
    for (int i = 0; i < 12; ++i) m[i] = vals[i];
    m[12] = 9.0; m[13] = 8.0; m[14] = 7.0; m[15] = 6.0;      // a last row the pack must not read into the 12 numbers
    std::vector<double> q(12), back(16, 55.0);
    pose_pack12(m.data(), q.data());
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) CHECK(bits(q[3 * i + j]) == bits(m[4 * i + j]));      // R row-major
        CHECK(bits(q[9 + i]) == bits(m[4 * i + 3]));                                      // then t
    }
    pose_unpack16(q.data(), back.data());
    for (int i = 0; i < 12; ++i) CHECK(bits(back[i]) == bits(m[i]));
    CHECK(bits(back[12]) == bits(0.0) && bits(back[13]) == bits(0.0) && bits(back[14]) == bits(0.0) && bits(back[15]) == bits(1.0));
    printf("ok poses\n");
}

static void sym6() {
    std::vector<double> u(21), m(36, -1.0);
    for (int k = 0; k < 21; ++k) u[k] = 100.0 + k;
    sym6_expand(u.data(), m.data());
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            const int k = i * 6 - i * (i - 1) / 2 + (j - i);      // row-major upper index of (i, j)
            CHECK(m[i * 6 + j] == u[k] && m[j * 6 + i] == u[k]);
        }
    printf("ok sym6\n");
}

static void masks() {
    const std::vector<uint8_t> in{0, 1, 2, 255};
    std::vector<uint8_t> out(4, 7);
    mask_normalise(in.data(), 4, out.data());
    CHECK(out[0] == 0 && out[1] == 1 && out[2] == 1 && out[3] == 1);
    std::vector<uint8_t> ones(5, 7);
    mask_normalise(nullptr, 5, ones.data());
    for (uint8_t v : ones) CHECK(v == 1);
    mask_normalise(nullptr, 0, nullptr);      // nothing to write, nothing touched
    mask_normalise(in.data(), 0, nullptr);
    printf("ok masks\n");
}

int main() {
    layout();
    starts();
    poses();
    sym6();
    masks();
    return 0;
}
