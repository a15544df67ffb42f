"""Writes tests/golden/build_exact_<case>.npz for the cases of tests/build_exact_cases.py: the built system of the quad-precision oracle
(oracle/make_quad.py: orcq_debug_build / orcq_debug_get), the fp64 oracle's noise against it and the first trial of optimize(1), per
lambda; tests/build_exact.py says what the figures are and how they are used.  A case that carries levels, robust switches or a
replaced state (the gated cases) is built with them: build_exact.apply after every upload; the stage2 cases store the state and levels
of the quad oracle's own optimize(5) + gate_outliers.  CPU only, seconds per case.

    python tests/golden/make_build_exact.py [case ...]

Prints, per case and lambda, the noise of every quantity in units of u = 2^-53 and the file size."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g                      # noqa: E402
from oracle import oracle as orc                 # noqa: E402
from tests import build_exact as BX              # noqa: E402
from tests import build_exact_cases as BC        # noqa: E402

LIMIT = 199235      # no fixture above the largest file committed before these


def main():
    W = g.load_package().window
    orc.build()
    for name in sys.argv[1:] or list(BC.CASES):
        out = BX.generate(name, W, orc)
        path = os.path.join(ROOT, "tests", "golden", "build_exact_%s.npz" % name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        for i, lam in enumerate(out["lams"]):
            noise = dict(zip(out["%d/noise_names" % i], out["%d/noise" % i]))
            over = [q for q, n in noise.items() if BX.factor(q) * n > BX.cap(q)]      # condition (ii): such a (case, lambda) belongs in DROPPED
            print("%-12s lambda %-10.4g decided %d  " % (name, lam, out["%d/decided" % i]) + " ".join("%s %.0fu" % (q, n / BX.U) for q, n in noise.items())
                  + ("   OVER THE CAP: %s" % over if over else ""))
        print("%-12s %d bytes" % (name, size))
        assert size <= LIMIT, (name, size)


if __name__ == "__main__":
    main()
