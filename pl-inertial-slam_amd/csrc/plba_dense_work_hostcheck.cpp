// plba_dense_work_hostcheck.cpp — a stand-alone program over the two HIP-free contracts of the host side: plba_dense_work.h (the dense
// solver's padding rule, the element counts of its workspace, when the explicit inverse is kept) and plba_mailbox.h (the overlay the
// other optimisers lay over the problem's mapped mailbox).  Built with a plain C++ compiler under the address and undefined-behaviour
// sanitizers and run directly by tests/test_dense_work_cpu.py.  Every expected number is exact: it is what the call sites computed by
// hand before the header existed.
// Prints one line per group, `ok <group>`, and exits 0; the first failed check prints its text and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "plba_dense_work.h"
#include "plba_mailbox.h"

using namespace plba;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void ppad() {
    CHECK(dense_ppad(0) == 64 && dense_ppad(1) == 64 && dense_ppad(64) == 64 && dense_ppad(65) == 128);
    printf("ok ppad\n");
}

static void counts() {
    {
        const DenseCounts n = dense_counts(64, 64);
        CHECK(n.sys_len == 8192 && n.x == 64 && n.Linv == 4096 && n.LT32 == 4096 && n.rd32 == 64 && n.flow_flags == 1 && n.chol_flags == 8);
        CHECK(ninv_fits(64) && n.ninv == 8192);
    }
    {   // a multiple of 32 alone (the small compact system): the tile counts round up
        const DenseCounts n = dense_counts(96, 96);
        CHECK(n.sys_len == 15360 && n.x == 96 && n.Linv == 8192 && n.LT32 == 6144 && n.rd32 == 96 && n.flow_flags == 2 && n.chol_flags == 15);
        CHECK(ninv_fits(96) && n.ninv == 18432);
    }
    {   // the longest system that keeps the explicit inverse, and the first that does not
        const DenseCounts n = dense_counts(1024, 1024);
        CHECK(n.chol_flags == 1088 && ninv_fits(1024) && n.ninv == 2097152);
        const DenseCounts m = dense_counts(1088, 1088);
        CHECK(m.Linv == 69632 && m.chol_flags == 1224 && !ninv_fits(1088));
    }
    printf("ok counts\n");
}

struct Head16 { int a, b, c, d; };
struct HeadFull { char bytes[sizeof(Ctrl)]; };

template <class Head>
static void overlay_of() {
    CHECK(sizeof(MailOver<Head>) == sizeof(Mailbox));
    CHECK(offsetof(MailOver<Head>, seq) == offsetof(Mailbox, seq));
    CHECK(offsetof(MailOver<Head>, c) == 0);
    // a write of every byte the overlay owns stays inside a mailbox (the sanitizers watch the heap block's ends)
    Mailbox* mb = new Mailbox();
    MailOver<Head>* o = reinterpret_cast<MailOver<Head>*>(mb);
    memset(static_cast<void*>(o), 0xa5, sizeof *o);
    o->seq = 0x0123456789abcdefULL;
    CHECK(mb->seq == 0x0123456789abcdefULL);
    delete mb;
}

static void overlay() {
    static_assert(sizeof(Head16) == 16, "the small head");
    overlay_of<Head16>();
    overlay_of<HeadFull>();
    printf("ok overlay\n");
}

int main() {
    ppad();
    counts();
    overlay();
    return 0;
}
