"""MC_RNG_XORWOW, every path against the float64 models on asymmetric markets: the kernels compiled for this mode only --
vanilla_f32_kernel<ANTI, GenXorwow>, vanilla_kernel<..., double, ANTI, GenXorwow>, the masked vanilla kernel in both precisions,
basket_dyn_kernel<Real, ANTI, GenXorwow> (its <float, true> exists under no other generator) and cva_kernel<Real, ANTI, GenXorwow>.

Why: tests/test_gpu_xorwow.py compares them with the oracle's XORWOW twin -- the same formulas in the same precision, the lane
bookkeeping restated by the same hand -- on the symmetric markets that cannot see an index error, under absolute constants, at
five basket sizes and four grids, never with the control variate.  And XORWOW is the one generator with STATE: a lane's sequence
must move on by whole blocks for every unit, used or not, or every later path of that lane is another sample -- an error the first
grid-stride trip cannot show.

Here the sample is xorwow_ref.py's, written from the header's sentence (include/mc_mi355x.h, mc_context_set_generator): the words
are Engine.xorwow_words (pinned word for word to rocRAND by tests/test_rocrand_xcheck.py), the lanes L = grid x 256 are read from
Engine.last_launch (never restated from the grid rule), the words become normals through the device's own inline functions
(Engine.math_probe: "f32_block", "pair"), and the values are greeks_ref.vanilla, basket_ref.value and cva_ref.price on the inputs
as the entry point of the precision reads them.  Every path stays within greeks_ref.bound(p, TOL[X]["pay"]); no path is left out
(these payoffs have no step).  tests/test_xorwow_ref.py shows on the CPU that this bound rejects every wrong assignment of
xorwow_ref.MUTATIONS on at least 90 % of the later-trip paths it reaches.

Engines (xorwow_ref.UNITS): blocks = 1 prices 256 x 3 + 77 units (three full trips, a partial wave and a partial workgroup),
blocks = 2 prices 512 x 2 + 77, the default engine 2121 (one trip).  Every call is first held to grid <= blocks (every lane has a
start state) and on the small engines to grid x 256 x 2 <= units, so that a changed grid rule fails the test instead of turning it
into a one-trip test.  Both seeds and the three subsequence bases (0, 1000, 2^40 + 5) rotate over the engines of every test.

Sums: {sum, sum2, n} of the run form against the same call's dump (greeks_ref.check_sums; the fp32 vanilla dump is the kernel's
value times the call's scale ROUNDED to float, which the run form's sums never are: its bound carries that rounding, 2^-24 of every
dumped value).  Whole-unit vanilla ranges run the hot kernels and have no dump: their sums are held to the model's, the sum of the
per-path bounds as tolerance, on the many-trip engines; the masked form's sums are held to the model's the same way.  A test of sums
sees HOW MANY words a unit consumes, never the order in which a lane hands its blocks to its units: every unit of a call is priced
alike, so a permutation leaves the multiset of payoffs unchanged (HISTORY.md: the mutation trial's case B).

Wall time on the MI355X: the module's 64 tests take 4.6 s together, the slowest (the 64-asset basket: 48 calls on three engines)
0.31 s.  Worst err/bound as printed (fp32, fp64): vanilla masked 0.085, 0.031; hot-kernel sums over the summed bounds 0.016, 0.011;
basket 0.201, 0.129; CVA 0.030, 0.656 (31 dates ending intrinsic: the model's Hastings-step term; every other grid below 0.03).
"""
import math

import numpy as np
import pytest

import xorwow_ref as xr
from greeks_ref import check_sums
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

U64 = np.uint64
ENGINES = (1, 2, 0)              # blocks; 0 = the default engine
FIRSTS = {1: 4242, 2: (5 << 32) + 123, 0: (1 << 32) - 2121 - 9}     # (the last range ends nine paths below a multiple of 2^32 units)


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def engines(mc):
    engs = {b: mc.Engine(0, blocks=b) for b in ENGINES}
    assert engs[1].blocks == 1 and engs[2].blocks == 2 and engs[0].blocks * xr.GROUP >= 4 * xr.UNITS[0]
    yield engs
    for e in engs.values():
        e.close()


def setting(e, seed_base, anti=False, control=False, date_lanes=0):
    e.set_generator("xorwow", seed_base[1])
    e.set_antithetic(anti), e.set_control_variate(control), e.set_cva_date_lanes(date_lanes)


def lanes_of_last_launch(e, bk, n_units):
    """L of the call just made, from the launch itself; on the small engines the call is held to at least two full trips."""
    grid, group = e.last_launch()
    assert group == xr.GROUP and 1 <= grid <= e.blocks, (grid, group, e.blocks)
    if bk:
        assert e.blocks == bk and grid * group * 2 <= n_units, (bk, grid, group, n_units)
    else:
        assert grid * group >= n_units, (grid, group, n_units)       # the default engine: one trip
    return grid * group


def probe_normals(eng):
    """The device's own words-to-normals step: words_to_normals of four words (fp32), pair_normals_f64 of three (fp64)."""
    def f(blocks, X):
        b = np.ascontiguousarray(blocks, dtype=U64)
        if X == "f32":
            out = eng.math_probe("f32_block", b)
            return np.ascontiguousarray(out[:, :4]).astype(np.uint32).view(np.float32).astype(np.float64)
        out = eng.math_probe("pair", b.reshape(-1, 3))
        return np.ascontiguousarray(out[:, :2]).view(np.float64).reshape(-1, 8)
    return f


def model_normals(engines, c, seed_base, n_paths):
    seed, base = seed_base
    words_of = lambda lanes, K: engines[0].xorwow_words(seed, base, lanes, K)     # noqa: E731
    return xr.product_normals(xr.draw(c, words_of, probe_normals(engines[0])), c, n_paths)


def check_paths(got, c, p, what):
    """Every path within the bound; returns the worst err/bound."""
    v, bnd = p.value[0], xr.bound(c, p, TOL)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == v.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - v)
    r = xr.ratio(err, bnd)
    i = int(np.argmax(r))
    assert np.all(err <= bnd), (what, i, got[i], v[i], err[i], bnd[i], int((err > bnd).sum()), float(r[i]))
    return float(r[i])


def check_model_sums(est, c, p, n, what):
    """{sum, sum2, n} against the model's, the sum of the per-path bounds as tolerance; returns |sum - model| over that tolerance."""
    v, bnd = p.value[0], xr.bound(c, p, TOL)
    assert est.n == n, what
    assert abs(est.sum - v.sum()) <= bnd.sum(), (what, est.sum, v.sum(), bnd.sum())
    assert abs(est.sum2 - (v * v).sum()) <= (2 * np.abs(v) * bnd + bnd * bnd).sum(), (what, est.sum2, (v * v).sum())
    return abs(est.sum - v.sum()) / bnd.sum() if bnd.sum() > 0 else 0.0


def check_sums_of_rounded_dump(est, got, n, what):
    """greeks_ref.check_sums for the fp32 vanilla dump: out = fl32(p x scale) while the sums are (sum of p) x scale in fp64, so every
    dumped value is within 2^-24 of itself of the summand: the additions' bound plus that rounding, term by term."""
    u, r = 2.0 ** -53, 2.0 ** -24
    p = [float(x) for x in got]
    assert est.n == n, what
    s_abs, q = math.fsum(abs(x) for x in p), math.fsum(x * x for x in p)
    assert abs(est.sum - math.fsum(p)) <= (n * u + r) * s_abs, (what, est.sum, math.fsum(p))
    assert abs(est.sum2 - q) <= ((n + 1) * u + 2 * r + r * r) * q, (what, est.sum2, q)


def tag_of(anti, control):
    return ("anti" if anti else "plain") + ("+cv" if control else "")


# ---- vanilla: the masked kernel per path, the hot kernels by their sums ---------------------------------------------------------
@pytest.mark.parametrize("X", xr.PRECISIONS)
def test_vanilla_masked_every_path(engines, X):
    """Ranges that start and end inside a unit, first != 0: one masked launch over every unit the range touches; the partly live
    first unit moves its lane on by a whole block."""
    npb, worst = xr.NPB[X], {}
    for j, bk in enumerate(ENGINES):
        e, units = engines[bk], xr.UNITS[bk]
        for i, head in enumerate(xr.VANILLA_HEADS[X]):
            sb = xr.rotation(i + j)
            first = (FIRSTS[bk] // npb + 7 * i) * npb + head
            n = units * npb - head - (1 + i)                     # ends inside the last unit
            o = xr.vanilla_market((i + j) % xr.N_VANILLA_MARKETS)
            z = None
            for m, mtag in ((o, ""), (xr.vanilla_in_the_money(o), " itm")):
                for anti in (False, True):
                    setting(e, sb, anti)
                    got = e.vanilla_paths(m, n, sb[0], first, X)
                    c = xr.vanilla_call(X, e.blocks, lanes_of_last_launch(e, bk, units), first, n)
                    assert (c.n_units, c.head) == (units, head)
                    if z is None:
                        z = model_normals(engines, c, sb, n)
                    p = xr.value(c, m, z, anti)
                    what = (X, bk, head, sb, mtag, anti)
                    key = f"{tag_of(anti, False)}{mtag}"
                    worst[key] = max(worst.get(key, 0.0), check_paths(got, c, p, what))
                    est = e.vanilla(m, n, sb[0], first, X)
                    assert lanes_of_last_launch(e, bk, units) == c.lanes
                    (check_sums if X == "f64" else check_sums_of_rounded_dump)(est, got, n, what)
                    check_model_sums(est, c, p, n, what)
    print(f"xorwow_ref vanilla masked {X}: worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("X", xr.PRECISIONS)
def test_vanilla_hot_kernels_sums_of_many_trips(engines, X):
    """Whole-unit ranges run vanilla_f32_kernel / vanilla_kernel under GenXorwow: no dump, so {sum, sum2, n} against the model's sums on
    the engines where every lane takes several trips (fp32: the peeled partial trip after three full ones)."""
    npb, worst = xr.NPB[X], 0.0
    for j, bk in enumerate((1, 2)):
        e, units = engines[bk], xr.UNITS[bk]
        for i in range(3):
            sb = xr.rotation(i + j + 1)
            first, n = (FIRSTS[bk] // npb + 11 * i + 1) * npb, units * npb
            o = xr.vanilla_market((i + j + 2) % xr.N_VANILLA_MARKETS)
            z = None
            for m, mtag in ((o, ""), (xr.vanilla_in_the_money(o), " itm")):
                for anti in (False, True):
                    setting(e, sb, anti)
                    est = e.vanilla(m, n, sb[0], first, X)
                    c = xr.vanilla_call(X, e.blocks, lanes_of_last_launch(e, bk, units), first, n)
                    assert (c.n_units, c.head) == (units, 0)
                    if z is None:
                        z = model_normals(engines, c, sb, n)
                    worst = max(worst, check_model_sums(est, c, xr.value(c, m, z, anti), n, (X, bk, i, sb, mtag, anti)))
    print(f"xorwow_ref vanilla hot {X}: worst |sum - model| / summed bounds {worst:.4f}")


# ---- basket: basket_dyn_kernel under GenXorwow, four estimators ---------------------------------------------------------------------
@pytest.mark.parametrize("X", xr.PRECISIONS)
@pytest.mark.parametrize("n_assets", xr.BASKET_SIZES)
def test_basket_every_path_every_estimator(mc, engines, X, n_assets):
    b = xr.basket_market(mc, n_assets)
    i, worst = xr.BASKET_SIZES.index(n_assets), {}
    for j, bk in enumerate(ENGINES):
        e, n, sb, first = engines[bk], xr.UNITS[bk], xr.rotation(i + j), FIRSTS[bk] + 1000 * n_assets * (bk != 0)
        g = None
        for m, mtag in ((b, ""), (xr.br.in_the_money(b), " itm")):
            for anti, control in xr.br.ESTIMATORS:
                setting(e, sb, anti, control)
                got = e.basket_paths(m, n, sb[0], first, X)
                c = xr.Call("basket", X, e.blocks, lanes_of_last_launch(e, bk, n), n, n_assets, 0)
                if g is None:
                    g = model_normals(engines, c, sb, n)
                    assert g.shape == (n, n_assets)
                what = (X, n_assets, bk, sb, mtag, anti, control)
                key = f"{tag_of(anti, control)}{mtag}"
                worst[key] = max(worst.get(key, 0.0), check_paths(got, c, xr.value(c, m, g, anti, control), what))
                est = e.basket(m, n, sb[0], first, X)
                assert lanes_of_last_launch(e, bk, n) == c.lanes
                check_sums(est, got, n, what)
    print(f"xorwow_ref basket {X} n_assets={n_assets}: worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ---- CVA: cva_kernel under GenXorwow ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", xr.PRECISIONS)
@pytest.mark.parametrize("n_dates", xr.CVA_DATES)
def test_cva_every_path_and_forced_date_lanes(engines, X, n_dates):
    """Every ending (xorwow_ref.cva_schedules), plain and antithetic; and with set_cva_date_lanes forced the call keeps one lane per
    path (the header says so for XORWOW): the same launch, the same bits."""
    m0 = xr.cva_market(X, n_dates)
    assert xr.cr.schedule(m0, X).n_dates == n_dates
    i, worst = xr.CVA_DATES.index(n_dates), {}
    for j, bk in enumerate(ENGINES):
        e, n, sb, first = engines[bk], xr.UNITS[bk], xr.rotation(i + j), FIRSTS[bk] + 3000 * n_dates * (bk != 0)
        z = None
        for m, mtag in ((m0, ""), (xr.cva_in_the_money(m0), " itm")):
            for anti in (False, True):
                setting(e, sb, anti)
                got = e.cva_paths(m, n, sb[0], first, X)
                c = xr.Call("cva", X, e.blocks, lanes_of_last_launch(e, bk, n), n, n_dates, 0)
                if z is None:
                    z = model_normals(engines, c, sb, n)
                what = (X, n_dates, xr.cva_schedules(X)[n_dates], bk, sb, mtag, anti)
                key = f"{tag_of(anti, False)}{mtag}"
                worst[key] = max(worst.get(key, 0.0), check_paths(got, c, xr.value(c, m, z, anti), what))
                est = e.cva(m, n, sb[0], first, X)
                assert lanes_of_last_launch(e, bk, n) == c.lanes
                check_sums(est, got, n, what)
                try:
                    setting(e, sb, anti, date_lanes=(8, 64, 2)[j])
                    forced = e.cva_paths(m, n, sb[0], first, X)
                    assert lanes_of_last_launch(e, bk, n) == c.lanes
                finally:
                    e.set_cva_date_lanes(0)
                assert np.array_equal(forced.view(np.uint8), got.view(np.uint8)), what
    ending = xr.cva_schedules(X)[n_dates][2]
    print(f"xorwow_ref cva {X} n_dates={n_dates} ({ending}): worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))

