"""The market lists of tests/wide_markets.py without a GPU: the strata are covered, every market passes the library's input checks,
the shapes of tests/test_gpu_wide_markets.py keep the families' near and kink caps and exercise their payoffs and barriers, and the
lists have POWER: each wrong restatement of wide_markets.MUTATIONS moves, on some wide market, at least 90 % of the paths with a
non-zero value beyond the fp32 bound -- the project's existing condition -- while the families' old fixed cases cannot see some
of them (printed by the same test, recorded in HISTORY.md).  For local vol and the Heston level the whole row of a mutation is
printed, the weak markets too: the level's fp32 power is small where |Y| itself is under the fp32 bound (the small-volatility
market over days), and a mutation is judged on its best market.  Local vol's power is the better of two of its shapes, (8, 2, 2, 65)
and (15, 5, 5, 4), both run on every market by the GPU test: a wrong interval is another volatility only on a coarse grid.  Sight, for
the two: calls and puts each have a value on 10 % of the paths of half the markets; Y = P_fine - P_coarse is non-zero on half the
paths of ten of the twelve level markets and, in fp64, above its bound there.  On every wide surface mc_localvol_sigma_* is
localvol_ref.sigma_at from below y_lo to above y_hi: the host's lookup on one-sided grids, without a GPU.

All of it on numpy's generator behind the Engine's draw calls (wide_markets.NumpyEngine): the models alone, on exactly the shapes
(market, date count, precision, antithetic, switch) the GPU test runs.

The input checks (mc_*_check_* of csrc/mc_hostmath_impl.h) are hidden symbols: they are reached through the public host functions
that run them first -- mc_merton_thresholds_* (mc_merton_check, and with the barrier payoff mc_barrier_check), mc_lookback_closed_form_*,
mc_heston_closed_form_*, mc_american_lattice_*, mc_rainbow_closed_form_*, mc_asian_control_mean_*, mc_localvol_sigma_* (mc_localvol_check
on the market's own struct, every payoff, right and barrier kind; it accepts k <= 0).  A refusal whose text names the
formula ("... closed form: needs k > 0", "lattice: ...", "asian control variate: needs k > 0" on the two Asian markets with k <= 0) is
the formula's own and comes after the check: the check has then passed.  The conditions are taken per market on the mean over its
calls (date counts, switches, precisions); the least and the most of a single call are printed beside them.  The
exponent-range guards of the GPU entry points (mc_api.hip) are met by the GPU test, where any McError fails."""
import math

import numpy as np
import pytest

import wide_markets as wm
from wide_markets import IN_MATURITY, IN_SPOT, IN_VOL

PRECISIONS = ["f32", "f64"]
POWER = 0.9                       # the share of non-zero paths a mutation must move beyond the bound
POWER_DATES = dict({f: 8 for f in wm.FAMILIES}, heston_path=(8, 1), localvol=(8, 2, 2, 65), heston_level=(8, 4))
LV_COARSE = (15, 5, 5, 4)         # local vol's second power shape: four nodes, where a wrong interval is another volatility
assert POWER_DATES["localvol"] in wm.LV_SHAPES and LV_COARSE in wm.LV_SHAPES and POWER_DATES["heston_level"] in wm.LEVEL_SHAPES
NEW = ("localvol", "heston_level")
UNSEEN_BY_OLD = {}


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def at_least_two(markets, pick, strata, what):
    for name, inside in strata.items():
        hit = [i for i, mk in enumerate(markets) if inside(pick(mk))]
        assert len(hit) >= 2, (what, name, hit)


def vol_of(family, mk):
    if "model" in mk:
        return math.sqrt(mk["model"]["v0"] if mk["model"]["v0"] > 0 else mk["model"]["theta"])
    return mk["o"]["v"]


# ---- 1. strata ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", wm.SINGLE)
def test_single_asset_strata_are_covered(family):
    mks = wm.markets(family)
    assert 2 <= len(mks) <= 16
    assert all(IN_SPOT[mk["strata"][0]](mk["o"]["s"]) and IN_MATURITY[mk["strata"][2]](mk["o"]["t"]) for mk in mks)   # the table's rows are what they say
    at_least_two(mks, lambda mk: mk["o"]["s"], IN_SPOT, (family, "spot"))
    at_least_two(mks, lambda mk: vol_of(family, mk), IN_VOL, (family, "volatility"))
    at_least_two(mks, lambda mk: mk["o"]["t"], IN_MATURITY, (family, "maturity"))
    assert sum(mk["o"]["r"] < 0 for mk in mks) >= 2 and sum(mk["o"]["r"] > 0.15 for mk in mks) >= 2
    if "model" not in mks[0]:
        a = [mk["o"]["r"] - 0.5 * mk["o"]["v"] ** 2 for mk in mks]
        assert sum(x == 0.0 for x in a) >= 2, a                      # exactly zero, in floating point
        rest = [x for x, mk in zip(a, mks) if x != 0.0 and not mk["o"]["r"] < 0 and not mk["o"]["r"] > 0.15]    # outside the three named strata
        assert any(x > 0 for x in rest) and any(x < 0 for x in rest), rest
    qs = [mk["q"] for mk in mks]
    assert min(qs) <= -1.0 and max(qs) >= 1.0 and min(qs) <= -2.0 and max(qs) >= 2.0
    if family == "heston_level":      # struck for a difference: at most at the money, but for the two markets that meet the kink between the legs
        qk = [mk["qk"] for mk in mks]
        assert sorted(i for i, q in enumerate(qk) if q > 0) == sorted(wm.LEVEL_OTM) and all(qk[i] == 0.5 for i in wm.LEVEL_OTM) and min(qk) <= -2.0
        assert all(mk["o"]["k"] > 0 for i, mk in enumerate(mks) if i in wm.LEVEL_OTM)
        assert all(s[1] % 2 == 0 for s in wm.LEVEL_SHAPES) and {s[0] * s[1] % 4 for s in wm.LEVEL_SHAPES} == {0, 2} and any(s[1] == 2 for s in wm.LEVEL_SHAPES)
    non_positive = sum(mk["o"]["k"] <= 0 for mk in mks)
    assert non_positive == (0 if family in ("lookback", "american") else 2), (family, non_positive)
    assert {mk["first"] for mk in mks} == set(wm.FIRSTS) and wm.FIRSTS[-1] < (1 << 32) < wm.FIRSTS[-1] + wm.N_PATHS
    if family in ("barrier", "merton"):
        assert all(mk["up"] == (mk["B"] > mk["o"]["s"]) and mk["B"] != mk["o"]["s"] for mk in mks)
        ups, downs = [mk["p"] for mk in mks if mk["up"]], [mk["p"] for mk in mks if not mk["up"]]
        assert len(ups) >= 2 and len(downs) >= 2 and min(ups + downs) <= 0.05 and max(ups) >= 2.0 and max(downs) >= 2.0
    if family == "localvol":
        for name, inside in wm.IN_PLACEMENT.items():
            hit = [i for i, mk in enumerate(mks) if mk["placement"] == name and inside(mk["grid"])]
            assert len(hit) >= 3, (name, hit)
        assert all(wm.IN_PLACEMENT[mk["placement"]](mk["grid"]) and mk["grid"][0] != -mk["grid"][1] for mk in mks)
        assert any(max(abs(g) for g in mk["grid"]) >= 2 * min(abs(g) for g in mk["grid"]) for mk in mks if mk["placement"] == "straddle")
        assert all(mk["B"] != mk["o"]["s"] and (mk["B"] > mk["o"]["s"]) == mk["up"] and (mk["B2"] < mk["o"]["s"]) == mk["up"] and mk["B2"] > 0 for mk in mks)
        assert {kind for mk in mks[:1] for _, kind in wm.lv_barriers(mk)} == set(wm.lv.KINDS) and min(mk["p"] for mk in mks) <= 0.05 and max(mk["p"] for mk in mks) >= 2.0
        for mk in mks:                # the surfaces: float32 values, rows and intervals all differ, one reaches exactly 0 at its first node
            for shape in wm.LV_SHAPES:
                a = wm.surface_of(mk, shape)["sigma"]
                assert a.shape == shape[1::2] and np.array_equal(a, a.astype(np.float32)) and np.all(a[:, 1:] > 0)
                assert bool(np.all(a[:, 0] == 0)) == mk["zero_node"] and np.all(a[:, 0] >= 0)
                inner = a[:, 1:] if mk["zero_node"] else a
                assert len(set(inner.ravel().tolist())) == inner.size and len(set(np.diff(a, axis=1).ravel().tolist())) == a.size - a.shape[0]
                assert shape[0] % shape[1] == 0 and shape[0] % shape[2] == 0
        assert sum(mk["zero_node"] for mk in mks) == 1
        odd = [s for s in wm.LV_SHAPES if (s[0] // s[1]) % 2 and s[2] % 2 and s[0] // s[1] != s[2] and s[2] > 1 and s[0] // s[1] > 1]
        assert odd and {1, 3, 8, 17} <= {s[0] for s in wm.LV_SHAPES}
    if family in ("heston", "heston_path", "heston_level"):
        models = [mk["model"] for mk in mks]
        assert {md["rho"] for md in models} == {-1.0, -0.9, 0.0, 0.9, 1.0}
        assert sum(md["v0"] == 0 for md in models) >= 2 and sum(md["kappa"] == 0 for md in models) >= 2
        assert any(md["theta"] >= 9 * md["v0"] > 0 for md in models) and any(0 < md["theta"] <= 0.11 * md["v0"] for md in models)
        assert any(md["xi"] <= 2e-3 for md in models) and any(md["xi"] >= 0.9 for md in models)
        feller = [2 * md["kappa"] * md["theta"] >= md["xi"] ** 2 for md in models]
        assert sum(feller) >= 2 and len(feller) - sum(feller) >= 2
    if family == "heston_path":
        assert all(mk["B_up"] > mk["o"]["s"] > mk["B_down"] for mk in mks) and min(mk["p"] for mk in mks) <= 0.05 and max(mk["p"] for mk in mks) >= 2.0
    if family == "merton":
        jumps = [mk["jumps"] for mk in mks]
        assert any(j["mu_j"] > 0 for j in jumps) and any(j["mu_j"] < 0 for j in jumps)
        assert any(j["delta"] == 0 for j in jumps) and any(j["delta"] >= 0.4 for j in jumps)
        p = [mk["jumps"]["lambda"] * mk["o"]["t"] / m for mk in mks for m in wm.DATES]
        assert min(p) < 0.01 and 5.5 < max(p) < 6.23        # the 64-bit threshold table's cap is reached at 6.23
    if family == "american":
        assert sum(mk["kind"] == "put" for mk in mks) >= 2 and sum(mk["kind"] == "call" for mk in mks) >= 2


@pytest.mark.parametrize("family", wm.MULTI)
def test_basket_strata_are_covered(family):
    mks = wm.markets(family)
    assert len(mks) == 16 and sorted(mk["n"] for mk in mks) == sorted(list(range(1, 9)) * 2)
    assert {mk["first"] for mk in mks} == set(wm.FIRSTS)
    spots = np.concatenate([mk["b"]["s"] for mk in mks])
    assert spots.min() < 0.1 and spots.max() > 1e4
    t_class = lambda t: min(range(3), key=lambda i: abs(math.log(t / wm.BASKET_T[i])))
    assert {t_class(mk["b"]["t"]) for mk in mks} == {0, 1, 2} and all(mk["b"]["t"] != 1.0 for mk in mks)
    assert any(mk["b"]["r"] < 0 for mk in mks) and any(mk["b"]["r"] > 0 for mk in mks)
    for mk in mks:
        b, n = mk["b"], mk["n"]
        assert len(set(b["s"])) == n and np.all(b["w"] > 0) and np.all(b["d"] == 0)     # a non-zero d is refused by the library
        assert np.all((b["v"] >= 0.05) & (b["v"] <= 0.8))
        if n > 1:
            assert len(set(b["w"])) == n and np.all(np.abs(b["w"] * b["s"] - 1.0) > 1e-3)
            assert (b["p"] @ b["p"].T).min() < 0
        if n > 2:
            assert not np.all(np.diff(b["v"]) > 0) and not np.all(np.diff(b["v"]) < 0)
        ph = 4 // math.gcd(n, 4)
        assert {(n * m) % 4 for m in wm.dates_of(family, mk)} == {(n * j) % 4 for j in range(ph)}, (n, "every phase of the fp32 unroll")
    # per market, hence per n (6 and 7 included): the calls of one test meet every switch, antithetic off and on
    eng = wm.NumpyEngine()
    for mk in mks:
        tags = {c.tag[3:] for c in wm.cases(family, mk, 1, "f32", eng)}
        if family == "rainbow":
            assert tags == {(kind, bk, anti) for kind in wm.rr.KINDS for bk in [None] + wm.rr.BARRIER_KINDS for anti in (False, True)}, (mk["n"], tags)
            for kind, k, barriers in mk["contracts"]:
                lv = mk["b"]["w"] * mk["b"]["s"]
                ext = lv.max() if kind.endswith("max") else lv.min()
                assert barriers[False] < ext < barriers[True] and k > 0
        else:
            assert tags == {(ki, memory, anti) for ki, memory in wm.KI_MODES for anti in (False, True)}, (mk["n"], tags)
            assert 0 < mk["B"] < (mk["b"]["w"] * mk["b"]["s"]).min()
    assert len(set(wm.KI_MODES)) == 6 and {ki for ki, _ in wm.KI_MODES} == {"dates", "maturity", None}
    if family == "rainbow":
        assert min(mk["p"] for mk in mks) <= 0.05 and max(mk["p"] for mk in mks) >= 2.0


# ---- 2. every market is accepted ----------------------------------------------------------------------------------------
def passes_the_check(mc, call):
    try:
        call()
    except mc.McError as e:
        assert " closed form: " in str(e) or " lattice: " in str(e), str(e)


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("family", wm.FAMILIES)
def test_every_market_passes_the_input_checks(mc, family, X):
    import ctypes as C
    from montecarlocuda_amd import engine
    L = mc._lib

    def merton_check(o, jp, m, payoff="european", B=None, kind=None):
        out, n = np.zeros(L.MAX_MERTON_JUMPS, dtype=np.uint64), C.c_int()
        L.check(getattr(L.lib(), f"mc_merton_thresholds_{X}")(C.byref(engine._as_merton(X, o, jp, m, payoff, B, kind)),
                                                               out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))

    no_jumps = dict([("lambda", 0.0), ("mu_j", 0.0), ("delta", 0.0)])
    for mk in wm.markets(family):
        for m in wm.dates_of(family, mk):
            if family == "asian":     # k <= 0: refused by the control's own condition, AFTER the inputs' checks that the call shares
                try:
                    assert math.isfinite(mc.asian_control_mean(mk["o"], m, X)) and mk["o"]["k"] > 0
                except mc.McError as e:
                    assert "asian control variate: needs k > 0" in str(e) and not mk["o"]["k"] > 0, str(e)
            elif family in ("barrier", "merton"):
                jp = mk.get("jumps", no_jumps)
                merton_check(mk["o"], jp, m)
                for kind in wm.kinds_of(mk):
                    merton_check(mk["o"], jp, m, "barrier", mk["B"], kind)
            elif family == "lookback":
                for kind in wm.lr.KINDS:
                    assert math.isfinite(mc.lookback_closed_form(mk["o"], kind, X))
            elif family == "localvol":          # mc_localvol_sigma_* runs mc_localvol_check_* first, the barrier's conditions and k <= 0 included
                for payoff, B, kind in [("european", None, None), ("asian", None, None)] + [("barrier", B, kind) for B, kind in wm.lv_barriers(mk)]:
                    for right in ("call", "put"):
                        h = engine._LocalVolHolder(X, mk["o"], wm.surface_of(mk, m), m[0] // m[2], m[2], payoff, right, B, kind)
                        out = C.c_double()
                        L.check(getattr(L.lib(), f"mc_localvol_sigma_{X}")(C.byref(h.struct), 1, 0.0, C.byref(out)))
                        assert math.isfinite(out.value) and out.value >= 0
            elif family in ("heston", "heston_path", "heston_level"):
                passes_the_check(mc, lambda: mc.heston_closed_form(mk["o"], mk["model"], X))
                if family == "heston_path":     # the barrier's own conditions, by mc_barrier_check
                    o = dict(mk["o"], v=0.2)
                    merton_check(o, no_jumps, m[0], "barrier", mk["B_up"], "up-and-out"), merton_check(o, no_jumps, m[0], "barrier", mk["B_down"], "down-and-in")
            elif family == "american":
                passes_the_check(mc, lambda: mc.american_lattice(mk["o"], m, 1, mk["kind"], X))
            elif family == "rainbow":
                for kind, k, barriers in mk["contracts"]:
                    for B, bk in [(None, None)] + [(barriers[side], bk) for side in barriers for bk in wm.rr.kinds_of(side)]:
                        passes_the_check(mc, lambda: mc.rainbow_closed_form(dict(mk["b"], k=k), kind, B, bk, X))
            elif family == "autocall":
                con = wm.contract(mk, wm.AUTOCALL_OBS[m], "dates", True)    # the modes differ in ki and memory alone
                passes_the_check(mc, lambda: mc.rainbow_closed_form(mk["b"], "put-on-min", con["barrier"], None if con["ki"] is None else "down-and-in", X))
                # the note's own conditions, as the header states them
                A, Cb = con["autocall"], con["coupon_barrier"]
                assert np.all(A > 0) and np.all(Cb >= 0) and np.all(np.isfinite(Cb)) and con["coupon"] >= 0 and con["gearing"] >= 0 and mk["b"]["k"] > 0
                assert mk["n"] * m + 3 * A.size <= wm.ac.MAX_TABLE and m % A.size == 0


# ---- 3. the shapes of the GPU test: caps and exercise -----------------------------------------------------------------------
@pytest.mark.parametrize("family", wm.FAMILIES)
def test_caps_hold_and_the_markets_exercise_the_payoffs(family):
    eng = wm.NumpyEngine()
    mks = wm.markets(family)
    worst = {X: [0.0, 0.0] for X in PRECISIONS}
    live, knocked, least, extremes = [], [], [], []
    by_right, beyond = {"call": [], "put": []}, []
    for i, mk in enumerate(mks):
        share, kn, rights, above = [], [], {"call": [], "put": []}, []
        for m, X in ((m, X) for m in wm.dates_of(family, mk) for X in PRECISIONS):
            for c in wm.cases(family, mk, m, X, eng):
                near, kink = float(c.near.mean()), float(c.kink.mean())
                assert near <= wm.NEAR_CAP and kink <= wm.KINK_CAP, (family, i, c.tag, X, near, kink)
                if family in NEW:     # every path has a bound the model can follow, at volatility above 1 over decades too
                    assert np.all(c.bound > 0) and np.all(np.isfinite(c.bound[~c.kink])), (family, i, c.tag, X)
                worst[X] = [max(worst[X][0], near), max(worst[X][1], kink)]
                share.append(float((c.value != 0).mean()))
                if c.knocked is not None and not c.anti:
                    kn.append(float(c.knocked.mean()))
                if family == "localvol":
                    rights[c.tag[3]].append(share[-1])
                if family == "heston_level" and X == "f64" and share[-1] > 0:     # in fp64 a non-zero Y is above its bound: the test sees it
                    above.append(float((np.abs(c.value) > c.bound)[c.value != 0].mean()))
        if family == "localvol":
            for right in by_right:
                by_right[right].append(float(np.mean(rights[right])))
        if family == "heston_level":
            beyond.append(min(above))
        live.append(float(np.mean(share)))
        least.append(min(share))
        if kn:
            knocked.append(float(np.mean(kn)))
            extremes.append((round(min(kn), 2), round(max(kn), 2)))
    print(f"{family}: worst share of near / kink paths fp32 {worst['f32'][0]:.4f} / {worst['f32'][1]:.4f}, fp64 {worst['f64'][0]:.4f} / {worst['f64'][1]:.4f}")
    print(f"{family}: share of paths with a non-zero value per market, mean over its calls {np.round(live, 2).tolist()}, least of a call {np.round(least, 2).tolist()}")
    assert sum(x >= 0.10 for x in live) * 2 >= len(mks), live
    if family == "localvol":          # calls and puts each
        print(f"localvol: share of paths with a non-zero value per market, calls {np.round(by_right['call'], 2).tolist()}, puts {np.round(by_right['put'], 2).tolist()}")
        assert all(sum(x >= 0.10 for x in v) * 2 >= len(mks) for v in by_right.values()), by_right
    if family == "heston_level":      # Y = P_fine - P_coarse is exactly 0 where both legs end out of the money: the strikes are chosen against that
        print(f"heston_level: least share, over a market's fp64 calls, of the non-zero Y above their bound {np.round(beyond, 3).tolist()}")
        seen = [x >= 0.50 and b == 1.0 for x, b in zip(live, beyond)]
        assert sum(seen) >= 10, (live, beyond)
    if family in wm.BARRIER_FAMILIES:
        print(f"{family}: share of knocked paths per market, mean over its calls {np.round(knocked, 2).tolist()}, (least, most) of a call {extremes}")
        assert sum(0.05 <= x <= 0.95 for x in knocked) * 2 >= len(knocked) > 0, knocked


# ---- 4. power ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", wm.FAMILIES)
def test_every_mutation_is_caught_on_some_wide_market(family):
    m = POWER_DATES[family]
    names = [name for name, (families, _, _) in wm.MUTATIONS.items() if family in families]
    assert names

    def share(mk, name):
        """Local vol: the better of the two power shapes, both run by the GPU test on every market -- a mutation of the lookup shows on
        the coarse grid, one of the walk on the fine one."""
        if family != "localvol":
            return wm.moved_share(family, mk, m, name)
        got = [x for x in (wm.moved_share(family, mk, shape, name) for shape in (m, LV_COARSE)) if x is not None]
        return max(got) if got else None

    for name in names:
        wide = [share(mk, name) for mk in wm.markets(family)]
        old = [share(mk, name) for mk in wm.old_markets(family)]
        best = max(x for x in wide if x is not None)
        seen_by_old = [x for x in old if x is not None and x >= POWER]
        applies = [x for x in old if x is not None]
        verdict = "caught on every old case" if applies and len(seen_by_old) == len(applies) else \
            f"caught on {len(seen_by_old)} of {len(applies)} old cases" if seen_by_old else "NOT SEEN by any old case"
        print(f"{family}: {name}: best wide market moves {best:.3f} of its non-zero paths; old cases {[None if x is None else round(x, 3) for x in old]}: {verdict}")
        if family in NEW:             # the whole row, the weak markets too (the level where |Y| is under the fp32 bound, row 11's rate over days)
            print(f"{family}: {name}: per wide market {[None if x is None else round(x, 3) for x in wide]}")
        if not seen_by_old:
            UNSEEN_BY_OLD.setdefault(family, []).append(name)
        assert best >= POWER, (family, name, wide)
    print(f"{family}: mutations no old case can see: {UNSEEN_BY_OLD.get(family, [])}")


# ---- 5. the host's interpolant on the wide surfaces -----------------------------------------------------------------------------
@pytest.mark.parametrize("X", PRECISIONS)
def test_the_hosts_interpolant_is_the_models_on_every_wide_surface(mc, X):
    """mc_localvol_sigma_* against localvol_ref.sigma_at at 200 y from below y_lo to above y_hi, at every slice of every shape of
    every market, under the tolerance of tests/test_localvol_ref.py's lookup test: (y - y_lo) / h on grids that lie wholly on one side of
    0 and on one with unequal arms, where y_hi for -y_lo or |y_lo| for y_lo is another number."""
    NP = {"f32": np.float32, "f64": np.float64}[X]
    for i, mk in enumerate(wm.markets("localvol")):
        for shape in wm.LV_SHAPES:
            m, nt = shape[:2]
            surf = wm.surface_of(mk, shape)
            lo, hi = surf["y_lo"], surf["y_hi"]
            ys = np.linspace(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), 200)
            assert (ys < lo).sum() >= 20 and (ys > hi).sum() >= 20
            for q in range(nt):
                step = q * (m // nt) + 1
                got = np.array([mc.localvol_sigma(surf, m, step, float(y), X) for y in ys])
                want = np.array([wm.lv.sigma_at(surf, m, step, float(y), NP) for y in ys])
                assert got == pytest.approx(want, rel=1e-13, abs=1e-15), (i, shape, q)
                assert got[0] == surf["sigma"][q, 0] and len(set(got.tolist())) > 100      # flat below the grid, and not flat inside
