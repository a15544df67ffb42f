"""Writes tests/golden/marg_quad_<case>.npz for the cases of tests/marg_quad_cases.py: the marginalization step evaluated with mpmath at
50 digits (tests/golden/marg_mp.py, shared with make_marg_exact.py) from the stacked Jacobian and residual of the quad-precision oracle
(oracle/make_quad.py: orcq_marginalize, orcq_debug_get + orcq_debug_get_lo) — no device anywhere — and the noise of the two fp64
yardsticks against it; tests/marg_quad.py says what the figures are and how they are used.  CPU only; a case takes seconds to minutes.

    python tests/golden/make_marg_quad.py [--reuse] [case ...]

--reuse keeps the 50-digit part of a fixture that exists and whose inputs (the quad J and r) are unchanged, and makes the rest anew.

Prints, per case, the noise of every quantity under both yardsticks in units of u = 2^-53, which yardstick applies, the eigenvalues of Amm
and A' within a decade of the threshold, and the file size."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g                      # noqa: E402
from oracle import oracle as orc                 # noqa: E402
from tests import marg_quad as MQ                # noqa: E402
from tests import marg_quad_cases as MC          # noqa: E402

LIMIT = 159120      # no fixture above the largest npz committed before these (build_exact_prior13.npz)


def main():
    W = g.load_package().window
    orc.build()
    args = [a for a in sys.argv[1:] if a != "--reuse"]
    for name in args or list(MC.CASES):
        t0 = time.time()
        path = os.path.join(ROOT, "tests", "golden", "marg_quad_%s.npz" % name)
        old = None
        if "--reuse" in sys.argv and os.path.exists(path):
            with np.load(path) as z:
                old = {k: z[k] for k in z.files}
        out = MQ.generate(name, W, orc, old)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        ref = MQ.Ref(out)
        eps = ref.eps
        print("%-11s m %d n %d R %d  decided_r %d  %.0f s  %d bytes" % (name, ref.L.m, ref.L.n, ref.L.R, ref.decided_r, time.time() - t0, size))
        for q in [str(s) for s in out["noise_names"]]:
            print("    %-8s ne %12.1f u  svd %12.1f u   -> %s" % (q, ref.noise_ne[q] / MQ.U, ref.noise_svd[q] / MQ.U, ref.yard(q) or "NOT COMPARED"))
        for nm, lam in (("Amm", ref.lam_mm), ("A'", ref.lam_r)):
            near = np.sort(lam[(lam > eps / 10) & (lam < eps * 10)])
            if len(near):
                print("    eigenvalues of %s within a decade of eps = %g: %s" % (nm, eps, near))
        assert size <= LIMIT, (name, size)


if __name__ == "__main__":
    main()
