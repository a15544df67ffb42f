"""The sequences of the state exactness tests (tests/step_exact.py is the rule, tests/golden/make_step_exact.py writes the fixtures,
tests/test_step_exact_cpu.py holds the references to their conditions, tests/test_step_exact.py holds the device).

The windows are those of tests/build_exact_cases.py, all of them: every one is at most 16 keyframes and 300 landmarks, and the fixture of
each already holds the scales d = sqrt(diag Hschur) and dl = sqrt(diag Hll) of the quad build at the uploaded state, per lambda.

A sequence is one optimize(n) call from the uploaded state with user_lambda_init = lambda:
  n1-<lambda>    n = 1 at each lambda the case keeps (build_exact_cases.lambdas_of, its DROPPED left out)
  n3-5, n3-init  n = 3 at lambda = 5 and at the protocol's own first lambda (where the case keeps it)
  rej-<lambda>   n = 1 with max_trials = 1 where the quad run rejects the first trial with margin: a call all of whose trials are
                 rejected, after which the whole state is the upload's, byte for byte.  There are four such (window, lambda) among the
                 kept ones; three have IMU edges, one of those lines as well.
The key of a sequence is that label; SHORTENED maps (case, key) to the iterations it keeps where three miss a condition, DROPPED names
what misses them at two as well (or, for n = 1, on its keyframes), QUANT_DROPPED the quantities a sequence of one iteration leaves out."""
from . import build_exact_cases as BC

REJECTED = {"gated_short2": 5.0, "stage2_cross9": 5.0, "noimu7": 0.05, "points_only": 0.05}

# What conditions (ii) and (iv) of tests/step_exact.py removed, judged on the references alone before any device ran
# (tests/golden/make_step_exact.py prints every figure and names what is over; tests/test_step_exact_cpu.py recomputes each entry and
# asserts that it misses its condition now).  DESIGN.md 9o has the figures.
# Three iterations miss (ii), two meet it:
SHORTENED = {(c, "n3-5"): 2 for c in ("mixed", "cross9", "k6", "levels_robust_on", "biasfirst")}
# Two iterations miss (ii) as well (n3-*), or the single one misses it on the keyframes (n1-*):
DROPPED = {(c, "n3-5") for c in ("lines_only", "k16_all", "k14_lines", "noimu7", "steps3", "prior13", "fixed8", "gated_mixed", "gated_steps3", "gated_k16",
                                 "noimu_lostkf", "stage2_mixed")}
DROPPED |= {("behind", "n3-init"), ("cross9", "n1-0.05"), ("k6", "n1-0.05"), ("noimu7", "n1-0.05"), ("steps3", "n1-0.05"), ("levels_robust_on", "n1-0.05")}
# One iteration, the keyframes within every cap: the quantities named are over theirs (a landmark kind in absolute units, or the trial's
# chi2) and are not compared; everything else of the sequence is.
QUANT_DROPPED = {
    ("lines_only", "n1-5"): ("state_ln",), ("k14_lines", "n1-5"): ("state_ln",), ("steps3", "n1-5"): ("state_ln",), ("gated_mixed", "n1-5"): ("state_ln",),
    ("gated_steps3", "n1-5"): ("state_pt", "state_ln"), ("gated_k16", "n1-5"): ("state_pt", "state_ln"), ("fixed8", "n1-0.05"): ("state_pt", "state_ln"),
    ("lines_all_gated", "n1-0.05"): ("state_pt",), ("behind", "n1-init"): ("state_pt",),
    ("points_only", "n1-0.05"): ("chi2_trial",), ("points_only", "rej-0.05"): ("chi2_trial",), ("noimu7", "rej-0.05"): ("chi2_trial",),
}


def _key(kind, label):
    return "%s-%s" % (kind, "init" if label == "init" else "%g" % label)


def planned(name):
    """[(key, lambda label, iterations asked for, options)] of a case before anything is shortened or dropped"""
    kept = [l for l in BC.CASES[name]["lambdas"] if (name, l) not in BC.DROPPED]
    out = [(_key("n1", l), l, 1, {}) for l in kept]
    out += [(_key("n3", l), l, 3, {}) for l in (5.0, "init") if l in kept]
    if name in REJECTED:
        assert REJECTED[name] in kept, name
        out.append((_key("rej", REJECTED[name]), REJECTED[name], 1, dict(max_trials=1)))
    return out


def sequences(name):
    """[(key, lambda label, iterations, options)] of the sequences a case keeps"""
    return [(k, l, SHORTENED.get((name, k), n), o) for k, l, n, o in planned(name) if (name, k) not in DROPPED]


def lambda_index(name, label):
    """the number of lambda `label` among the case's kept lambdas: the index of its scales in the build_exact fixture"""
    return [l for l in BC.CASES[name]["lambdas"] if (name, l) not in BC.DROPPED].index(label)
