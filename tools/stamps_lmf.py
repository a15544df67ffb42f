"""cycle stamps of three workgroups of k_lm_schur<0> (diagnostic build: PLBA_EXTRA_FLAGS=-DPLBA_STAMPS_LMF)

python tools/stamps_lmf.py [config]         the phases of the first, middle and last group
python tools/stamps_lmf.py --wg [config]    where the launches end: every workgroup of the last k_lm_schur<0> and k_lm_trial<true> of the
                                            call with its compute unit (HW_ID / XCC_ID) and its start / end on the 100 MHz real-time counter"""
import sys, numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as ge
pkg = ge.load_package()
args = [a for a in sys.argv[1:] if not a.startswith("--")]
cfg = int(args[0]) if args else 3
w = pkg.window.make_config(cfg)
g = pkg.new_problem(); g.upload_window(w)
g.optimize(4)
print("fused:", g.debug_get("lm_fused"))
v = g.debug_get("dbgbuf")


def kind_name(k):
    k = int(k)
    return {-1: "chain segment", -2: "IMU edge block", -3: "prior block"}.get(k, "%s group, %d steps" % ("line" if k >= 100 else "point", k % 100))


def wg_table(v):
    BASE, REC, MAX, US = 128, 5, 1024, 0.01      # (plba_internal.h: DBG_WG_*; one tick of the real-time counter = 10 ns)
    if len(v) < BASE + 2 * REC * MAX:
        sys.exit("this library was not built with -DPLBA_STAMPS_LMF")
    for launch, name in ((0, "k_lm_schur<0>"), (1, "k_lm_trial<true>")):
        n = min(int(v[126 + launch]), MAX)
        r = v[BASE + REC * MAX * launch:BASE + REC * MAX * (launch + 1)].reshape(MAX, REC)[:n]
        hw, xcc = r[:, 2].astype(np.int64), r[:, 3].astype(np.int64) & 15
        cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)      # XCC | SE | SH | CU
        t0 = r[:, 0].min()
        start, end = (r[:, 0] - t0) * US, (r[:, 1] - t0) * US
        ids, inv, cnt = np.unique(cu, return_inverse=True, return_counts=True)
        cu_end = np.array([end[inv == i].max() for i in range(len(ids))])
        print("\n%s: %d workgroups on %d compute units, launch ends at %.2f us (first start = 0)" % (name, n, len(ids), end.max()))
        print("  workgroups per compute unit: " + ", ".join("%d x %d" % ((cnt == c).sum(), c) for c in sorted(set(cnt))))
        for c in sorted(set(cnt)):
            e = cu_end[cnt == c]
            print("  compute units with %d workgroup%s end at   median %.2f [%.2f .. %.2f] us" % (c, "" if c == 1 else "s", np.median(e), e.min(), e.max()))
        for k in sorted(set(r[:, 4].astype(int))):
            m = r[:, 4].astype(int) == k
            for c in sorted(set(cnt[inv[m]])):
                mm = m & (cnt[inv] == c)
                dur = (end - start)[mm]
                print("  %-24s on a unit of %d: %4d, run time median %.2f [%.2f .. %.2f] us" % (kind_name(k), c, mm.sum(), np.median(dur), dur.min(), dur.max()))
        print("  the last ten workgroups to end:")
        for b in np.argsort(end)[::-1][:10]:
            print("    block %4d  %-24s start %6.2f end %6.2f us  xcc %d se %d cu %2d simd %d, %d workgroup(s) on its unit" % (
                b, kind_name(r[b, 4]), start[b], end[b], xcc[b], (hw[b] >> 13) & 7, (hw[b] >> 8) & 15, (hw[b] >> 4) & 3, cnt[inv[b]]))


if "--wg" in sys.argv:
    wg_table(v)
    sys.exit(0)
names = ["start", "staged+first loads", "eval done", "hll reduced", "operand written", "mfma done", None, "step 0 end", "loop end", "waves combined", "outputs drained"]
for name, o in (("first group", 0), ("middle group", 16), ("last group", 32)):
    print(name, "steps", int(v[o + 11]))
    prev = 0.0
    for q in range(1, 11):
        if names[q] is None: continue
        print("   %-28s %8.0f  (+%.0f)" % (names[q], v[o + q], v[o + q] - prev)); prev = v[o + q]
h = g.debug_get("lm_groups")
print("groups by steps, points:", [int(x) for x in h[:8]], "lines:", [int(x) for x in h[8:16]], "mean window %.2f" % (h[16] / max(sum(h[:16]), 1)), "workgroup steps", int(h[17]))
