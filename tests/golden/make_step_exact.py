"""Writes tests/golden/step_exact_<case>.npz for the sequences of tests/step_exact_cases.py: the state of the quad-precision oracle after
each optimize(n), rounded to fp64 on the way out, the quad and fp64 traces, the fp64 oracle's noise against the quad run per quantity
and whether the sequence is decided; tests/step_exact.py says what the figures are and how they are used.  The scales and the window's
carried prior or state come from the case's build_exact fixture (tests/golden/make_build_exact.py, run first).  CPU only, seconds per case.

    python tests/golden/make_step_exact.py [--planned] [case ...]

Prints, per sequence, the noise of every quantity in units of u = 2^-53, the state's tolerance in absolute units per kind, and names what
misses a condition: such a sequence belongs in step_exact_cases.SHORTENED or DROPPED.  --planned judges every planned sequence at three
and at two iterations without writing anything."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g                      # noqa: E402
from oracle import oracle as orc                 # noqa: E402
from tests import build_exact as BX              # noqa: E402
from tests import build_exact_cases as BC        # noqa: E402
from tests import step_exact as SX               # noqa: E402
from tests import step_exact_cases as SC         # noqa: E402

LIMIT = 199235      # no fixture above the largest file committed before these
GOLDEN = os.path.join(ROOT, "tests", "golden")


def judge(w, ref, q, noise, decided, margin):
    """what a sequence misses ([] where it meets (ii) and (iv)) and its tolerance in absolute units per kind"""
    if not decided:
        return ["UNDECIDED (margin %.3g)" % margin], {}
    over, quantities, ab = SX.misses(noise, q, SX.upload(w), ref, w)
    return (["%s %.3g" % kv for kv in over.items()] + ["->"] + sorted(quantities) if over else []), ab


def line(name, key, n, q, noise, over, ab):
    return ("%-16s %-9s n %d trials %d rejected %d  " % (name, key, n, len(q["trace"]), int((q["trace"][:, 2] == 0).sum()))
            + " ".join("%s %.0fu" % (qn, v / SX.U) for qn, v in noise.items()) + "  |  " + " ".join("%s %.1e" % kv for kv in ab.items())
            + ("   MISSES: %s" % over if over else ""))


def main():
    args = [a for a in sys.argv[1:] if a != "--planned"]
    W = g.load_package().window
    orc.build()
    for name in args or list(BC.CASES):
        with np.load(os.path.join(GOLDEN, "build_exact_%s.npz" % name)) as z:
            fxb = {k: z[k] for k in z.files}
        w = BC.CASES[name]["make"](W, BX.prior_of(fxb))
        if "--planned" in sys.argv:
            for key, label, n, opts in SC.planned(name):
                i = SC.lambda_index(name, label)
                ref = BX.load(fxb, w, i)[0]
                for m in sorted({n, min(n, 2)}, reverse=True):
                    q, _, noise, decided, margin = SX.references(orc, w, float(fxb["lams"][i]), m, opts, ref)
                    over, ab = judge(w, ref, q, noise, decided, margin)
                    print(line(name, key, m, q, noise, over, ab))
                    if not over:
                        break
            continue
        out = SX.generate(name, W, orc, fxb)
        path = os.path.join(GOLDEN, "step_exact_%s.npz" % name)
        np.savez_compressed(path, **out)
        for j, (key, label, n, opts) in enumerate(SC.sequences(name)):
            s = SX.load(out, j)
            ref = BX.load(fxb, w, SC.lambda_index(name, label))[0]
            over, ab = judge(w, ref, s["q"], s["noise"], s["decided"], s["margin"])
            print(line(name, key, n, s["q"], s["noise"], over, ab))
        size = os.path.getsize(path)
        print("%-16s %d bytes" % (name, size))
        assert size <= LIMIT, (name, size)


if __name__ == "__main__":
    main()
