"""Writes tests/golden/gate_exact_<case>.npz for the cases of tests/gate_exact.py: the quad-precision oracle's run of the gate / cull
sequence (oracle/make_quad.py: orcq_recompute_errors, orcq_get_edge_chi2, orcq_gate_outliers, orcq_get_levels, orcq_set_levels,
orcq_cull_observations), the state and planted observations a case carries, and the fp64 oracle's noise against the quad run;
tests/gate_exact.py says what the figures are and how they are used.  CPU only, seconds per case.

    python tests/golden/make_gate_exact.py [case ...]

Prints, per case, the noise figures in units of u = 2^-53, the smallest |chi2 - threshold| / (MARGIN x bound) over the edges and the
smallest |z| / |X - C|, and the file size."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g                      # noqa: E402
from oracle import oracle as orc                 # noqa: E402
from tests import gate_exact as GX               # noqa: E402

LIMIT = 199235


def main():
    W = g.load_package().window
    orc.build()
    for name in sys.argv[1:] or list(GX.CASES):
        out = GX.generate(name, W, orc)
        path = os.path.join(ROOT, "tests", "golden", "gate_exact_%s.npz" % name)
        np.savez_compressed(path, **out)
        carried, ref, noise = GX.load(out)
        w = GX.window(name, W, carried); wb = GX.at_b(W, w)
        bnd = GX.bounds(ref, w, noise)
        room = min(float((np.abs(ref[k] - GX.THRESH) / (GX.MARGIN * bnd[k])).min(initial=np.inf)) for k in bnd if k[:4] in ("chi0", "chiA", "chiB") and k[5:] in ("pt", "ln"))
        depth = min(float(np.abs(r).min(initial=np.inf)) for ww in (w, wb) for r in GX.depth_ratio(ww))
        print("%-13s " % name + " ".join("%s %.0fu" % (q, n / GX.U) for q, n in noise.items()))
        print("%-13s gate %s cull (a) %s (b) %s; smallest margin / (MARGIN x bound) %.3g, smallest |z| / |X - C| %.3g; %d bytes"
              % (name, list(ref["gate"]), list(ref["cullA"]), list(ref["cullB"]), room, depth, os.path.getsize(path)))
        assert os.path.getsize(path) <= LIMIT, name


if __name__ == "__main__":
    main()
