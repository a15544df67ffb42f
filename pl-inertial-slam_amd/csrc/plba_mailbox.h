// plba_mailbox.h — the LM control block, the mapped mailbox the device delivers it through, and the overlay the other optimisers lay over that mailbox; the host side
// (mail_reserve, mail_wait) is in plba_problem.h.  No HIP header: csrc/plba_dense_work_hostcheck.cpp checks the overlay's layout with a plain C++ compiler.
#pragma once
#include <cstddef>
#include "plba.h"

namespace plba {
// LM control block, device-resident; copied back once per trial.
struct Ctrl {
    double lambda, ni, current_chi, temp_chi, scale, rho, maxdiag, pad0;
    int accepted, solver_ok, iteration, trial, n_gate_pt, n_gate_ln, n_fail, sync_fail /* an in-launch wait ran into its bound */;
};
// Pinned, device-mapped host memory k_decide writes the control block into at the end of every LM trial: the host
// polls `seq` instead of paying for a device-to-host copy launch plus a stream synchronisation per trial.
struct Mailbox {
    Ctrl c;
    unsigned long long seq;
    plba_trace_row row;      // the trial's trace row (also appended to the device-side trace): the host keeps the trace from here, no read-back at the end of a call
};

// What another optimiser delivers through the problem's mailbox, laid over it: its own head `c` where the LM control block is, `seq`
// where the host polls it.  (The members sit in a base so that the checks can stand in the template: a class is incomplete in its own body.)
template <class Head>
struct MailOverLayout {
    Head c;
    char pad_[sizeof(Ctrl) - sizeof(Head)];      // (none for a head as large as the control block: a zero-length array, which both compilers take)
    unsigned long long seq;
    char row_[sizeof(Mailbox) - sizeof(Ctrl) - sizeof(unsigned long long)];
};
template <class Head>
struct MailOver : MailOverLayout<Head> {
    static_assert(sizeof(Head) <= sizeof(Ctrl), "the head has to fit where the LM control block is");
    static_assert(sizeof(MailOverLayout<Head>) == sizeof(Mailbox), "the overlay covers the problem's mapped mailbox exactly");
    static_assert(offsetof(MailOverLayout<Head>, seq) == offsetof(Mailbox, seq), "the host polls `seq` where the LM trials leave it");
};
}  // namespace plba
