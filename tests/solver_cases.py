"""The window sweep of the solver-accuracy tests (tests/test_solver_accuracy_cpu.py pins the oracle on these inputs, tests/test_solver_accuracy.py
holds the device to them).  Landmark counts are small (12 points and 3 lines per keyframe): the pose system's size and band come from the
keyframes and the track lengths alone, and the oracle stays cheap.

A SHAPE is a window and a damping (what the oracle solves once); a CASE is a shape, the options the device problem is created with and the
plan the case is there for: `form` as debug_get("solver_plan")[0] reports it (0 the pose system itself, 1 the compact system with one
launch per tile, 2 multi-chain, 3 in-LDS band) plus further fields of the descriptor that must hold."""

SEED = 0x50C0


def shape(K, track=(2, 8), lam=3.0, kf_dt=None, revisit=0.0, extra=""):
    return (K, track, lam, kf_dt, revisit, extra)


def make_shape_window(pkg, orc, sh):
    K, track, lam, kf_dt, revisit, extra = sh
    kw = dict(imu=True, seed=SEED + K, track=track, revisit=revisit)
    if revisit:      # a place seen again tens of keyframes later; "far": from the window's last keyframes, which leaves no band at all
        kw["revisit_gap"] = (K - 16, K - 6) if extra == "far" else (K // 3, K // 2)
    if kf_dt is not None:
        kw["kf_dt"] = kf_dt
    w = pkg.window.make_window(K, 12 * K, 3 * K, **kw)
    if extra == "prior":      # the marginalization prior of the window's own first BA: its kept keyframes widen the band at the old end
        o = orc.new_problem(); o.upload_window(w); o.optimize(3); pr = o.marginalize(0, 50); o.close()
        w = pkg.window.make_window(K, 12 * K, 3 * K, **kw)
        w["prior"] = pr
    if extra == "fixed":      # two fixed keyframes inside the window: the IMU chain falls into three
        kf = w["kf"]
        kf["fixed_pvr"] = kf["fixed_pvr"].copy(); kf["fixed_bias"] = kf["fixed_bias"].copy()
        for k in (K // 3, (2 * K) // 3):
            kf["fixed_pvr"][k] = 1; kf["fixed_bias"][k] = 1
    return w


# plan kinds the sweep must reach (test_every_plan_kind_was_reached)
def plan_kinds(plan):
    form, T, ninv, hbt, nch, nested, s0, s1, s2, nA, nB = [int(v) for v in plan[:11]]
    kinds = set()
    if form in (0, 1):
        kinds.add("dense, explicit inverse" if ninv else "dense, triangular solves")
    if form == 2:
        kinds.add("twin, four chains" if nch == 4 else "twin, two chains")
        if nested:
            kinds.add("twin, nested second stage")
        if any(s > hbt for s in (s0, s1, s2)[:nch - 1]):
            kinds.add("twin, separators widened by leftover tiles")
    if form == 3:
        kinds.add("band, T even" if T % 2 == 0 else "band, T odd")      # (odd: cannot happen, see REQUIRED_KINDS)
        if nA != nB:
            kinds.add("band, nA != nB")
    if form in (2, 3) and 1 <= hbt <= 3:
        kinds.add("band half-width %d" % hbt)
    return kinds


# No "band, T odd": a compact system of 8 tiles or more is padded to a multiple of 64 columns (dense_pad, csrc/plba_api.hip), so every
# multi-chain or band plan has an even tile count and the in-LDS sweeps always differ by one tile (nA = (T - 3) / 2 rounded down, nB the
# rest).  test_every_plan_kind_was_reached asserts that this still holds, so that an odd T, once it can happen, is noticed as uncovered.
REQUIRED_KINDS = {"dense, explicit inverse", "dense, triangular solves", "twin, two chains", "twin, four chains", "twin, nested second stage",
                  "twin, separators widened by leftover tiles", "band, T even", "band, nA != nB",
                  "band half-width 1", "band half-width 2", "band half-width 3"}

# (name, shape, options, expected).  expected: `form`, and further fields of the descriptor where the case is there for them
_L = (1e-4, 3.0, 1e3)
SIZES = (12, 26, 33, 34, 36, 41, 50, 64, 77, 80, 100, 110, 128, 170, 200, 260, 300)
CASES = []


def _lam(K):
    """the damping of a size: 1e-4, 3, 1e3 in turn, so that every option case shares its oracle run with the default case of its size"""
    return _L[SIZES.index(K) % 3]


def _case(name, sh, opts=None, **expected):
    CASES.append((name, sh, opts or {}, expected))


# sizes: the default plan from under 8 tiles to beyond TWIN_MAX_TILES = 64 (about 7 compact dims a keyframe) and both sides of NINV_MAX_T = 32;
# BAND_MIN_TILES = 24 only decides once the multi-chain form is refused (twin_max_tiles below)
for K in SIZES:
    _case("K%d" % K, shape(K, lam=_lam(K)), form=1 if K <= 12 else 2 if K <= 260 else 3)
# track lengths: short tracks (the band stays two tiles wide: a chain segment's column window alone spans 30 + 6 x its length dims),
# long tracks (three tiles), places seen again (a band wider than the in-LDS solver takes: separators nine tiles wide) and no band at all
_case("K50_short", shape(50, track=(2, 4)), form=2, hbt=2)
_case("K128_short", shape(128, track=(2, 4), lam=1e-4), form=2, hbt=2)
_case("K260_short", shape(260, track=(2, 4), lam=1e3), form=2, hbt=2)
_case("K300_short", shape(300, track=(2, 4)), form=3)
# ... one tile: tracks of two or three keyframes at 40 keyframes, where the host's choice of one-keyframe segments keeps every window inside
# two neighbouring tiles (found by listing the plans of 40 / 48 / 64 keyframes x chain_seg 0 .. 3: only this size gives it)
_case("K40_narrow", shape(40, track=(2, 3)), form=2, hbt=1)
_case("K40_narrow_lds", shape(40, track=(2, 3)), dict(chain_seg=1, band_solve=2), form=3, hbt=1)
_case("K64_long", shape(64, track=(6, 12), kf_dt=0.1), form=2, hbt=3)
_case("K100_long", shape(100, track=(6, 12), kf_dt=0.1, lam=1e-4), form=2, hbt=3)
_case("K64_revisit", shape(64, revisit=0.2), form=2, hbt_min=4)
_case("K64_revisit_far", shape(64, revisit=0.2, extra="far"), form=1)
# a marginalization prior / fixed keyframes
_case("K33_prior", shape(33, extra="prior"), form=2)
_case("K77_prior", shape(77, extra="prior", lam=1e-4), form=2)
_case("K128_prior", shape(128, extra="prior", lam=1e3), form=2)
_case("K50_fixed", shape(50, extra="fixed", lam=1e-4), form=2)
_case("K110_fixed", shape(110, extra="fixed"), form=2)
# options
_case("K100_noband", shape(100, lam=_lam(100)), dict(band_solve=0), form=1, ninv=1)
_case("K200_noband", shape(200, lam=_lam(200)), dict(band_solve=0), form=1, ninv=0)
_case("K41_lds", shape(41, lam=_lam(41)), dict(band_solve=2), form=3)
_case("K50_lds", shape(50, lam=_lam(50)), dict(band_solve=2), form=3)
_case("K64_lds_long", shape(64, track=(6, 12), kf_dt=0.1), dict(band_solve=2), form=3, hbt=3)
_case("K110_twin_low", shape(110, lam=_lam(110)), dict(twin_max_tiles=8), form=3)      # past BAND_MIN_TILES, the multi-chain form refused: in LDS
_case("K80_twin_low", shape(80, lam=_lam(80)), dict(twin_max_tiles=8), form=1)         # under BAND_MIN_TILES: one launch per tile
_case("K300_twin_high", shape(300, lam=_lam(300)), dict(twin_max_tiles=128), form=2)
for seg in (1, 3, 8):
    _case("K64_seg%d" % seg, shape(64, lam=_lam(64)), dict(chain_seg=seg), form=2)
_case("K36_nochain", shape(36, lam=_lam(36)), dict(chain_elim=0), form=0, ninv=1)
_case("K80_nochain", shape(80, lam=_lam(80)), dict(chain_elim=0), form=0, ninv=0)
_case("K41_nochain_valu", shape(41, lam=_lam(41)), dict(chain_elim=0, use_mfma=0), form=0)      # (use_mfma / factor_block act on the pose system's
_case("K41_nochain_fb64", shape(41, lam=_lam(41)), dict(chain_elim=0, factor_block=64), form=0)  # own factorisation only: chain_elim = 0 with them)
_case("K77_records", shape(77, lam=_lam(77)), dict(lm_fused=0), form=2)
_case("K77_fused", shape(77, lam=_lam(77)), dict(lm_fused=2), form=2)

SHAPES = sorted({c[1] for c in CASES}, key=lambda s: (s[0], str(s)))


def shape_id(sh):
    K, track, lam, kf_dt, revisit, extra = sh
    return "K%d-t%d_%d-lam%g%s%s%s" % (K, track[0], track[1], lam, "-dt%g" % kf_dt if kf_dt else "", "-revisit" if revisit else "", "-" + extra if extra else "")


_REF = {}


def oracle_reference(pkg, orc, sh):
    """the oracle on the shape (cached for the session): its system, its solution's E_D against the refined solution of ITS system, the bound"""
    from tests import solver_ref as R
    if sh not in _REF:
        w = make_shape_window(pkg, orc, sh)
        o = orc.new_problem(); o.upload_window(w); o.debug_build(sh[2], True)
        P = int(o.debug_get("pose_dim")[0])
        H = o.debug_get("Hschur").reshape(P, P).copy(); b = o.debug_get("bschur").copy(); x = o.debug_get("x")[:P].copy()
        o.close()
        xref, om = R.refine(H, b)
        _REF[sh] = dict(w=w, P=P, omega=om, E=R.scaled_error(x, xref, H), kappa_s=R.kappa_s(H), cpu=R.cpu_solvers(H, b, xref))
    return _REF[sh]
