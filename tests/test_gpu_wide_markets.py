"""The eleven dated families on wide, asymmetric markets (tests/wide_markets.py): every path of every compiled instantiation of
asian_kernel, barrier_kernel, lookback_kernel, merton_kernel, heston_kernel, heston_path_kernel, american_kernel, localvol_kernel (twelve),
heston_level_kernel, rainbow_kernel<Real, 1 ... 8>
and autocall_kernel<Real, 1 ... 8> against the family's independent float64 model, by the family's own per-path rule and tolerance
(imported by wide_markets.cases from where each lives; TOL[X]["pay"] of tests/test_gpu_parity.py per unit of the model's scale; a path
near a barrier, a trigger or an exercise boundary must match one of the values it can take; near and kink paths under the families'
caps, which tests/test_wide_markets.py holds as conditions on these very shapes).  No path is left out.

Why: the families' own modules run on one narrow box of markets (spot 36 to 120, volatility 0.2 to 0.45, maturity 0.5 to 2, rates at or
above 0 but for one call, Heston's |rho| = 1, v0 = 0 and kappa = 0 never, every rainbow asset at log level 0), and no per-path test
reaches rainbow_kernel<Real, 6>, <Real, 7>, autocall_kernel<Real, 6> and <Real, 7>.  tests/test_wide_markets.py shows what that
box hides: |ln S0| for ln S0 and a rate clamped at 0 pass every old case of every family.  The two families merged after that work sat
in the same box again: local vol on one market (s = 87, r = 0.02, t = 0.75) and two grids symmetric about y = 0, where fabs(log s),
max(r, 0) and u0 = y_hi / h are the bits of the correct constants; the Heston level on heston_ref.CASES (s = 100, r = 0.05, t = 1).

One test per (family, market, precision): 2121 paths from one of the three usual first paths (the market's; the last crosses the
2^32-unit seam), and inside it antithetic off and on, the family's switches (Asian control; barrier and lookback monitoring and
kinds; Merton payoffs; Heston-path payoff, kinds and steps_per_date 1 and 2; rainbow: all four types, each without a barrier and with
the four barrier kinds; autocall: the three knock-in modes with memory on and off -- on EVERY market, so every n meets every switch) and the date counts 1, 3, 8, 17 that reach every end of the date loops -- for the
baskets also 6 where n is odd, so that n n_dates takes every phase of the fp32 unroll.  Local vol: the five shapes (n_steps, n_times,
steps_per_date, n_nodes) of wide_markets.LV_SHAPES, each with calls and puts, the European and the Asian payoff and the four barrier
kinds (the market's barrier and a second one on the other side), on grids that straddle 0 with unequal arms or lie wholly above or
below it: 120 calls per market.  Heston level: the six shapes (n_dates, steps_per_date) of LEVEL_SHAPES.  On two markets of each of
these two families every call also runs in the run form, {sum, sum2, n} against the same call's dump (greeks_ref.check_sums).  Any
McError fails the test: every market is inside the domain the header states.

Wall time on the MI355X: the module's 280 tests take 12.6 s together, the slowest 0.21 s (an eight-asset rainbow market: 200 calls; a
local-vol market, 120 calls, 0.13 s; a Heston-path or Heston-level market 0.05 s): the numpy models dominate.  Worst err/bound as printed
(fp32, fp64): Asian 0.025, 0.014; barrier 0.023, 0.016; lookback 0.015, 0.011; Merton 0.024, 0.011; Heston 0.018, 0.0056; Heston path
0.014, 0.0055; Bermudan 0.127, 0.105; local vol 0.012, 0.0076; Heston level 0.0095, 0.0039; rainbow 0.032, 0.015; autocall 0.031, 0.020.
"""
import numpy as np
import pytest

import greeks_ref as gr
import wide_markets as wm

pytestmark = pytest.mark.gpu

COUNTS = {f: 16 if f in wm.MULTI else 12 for f in wm.FAMILIES}   # markets per family (asserted: the lists are built on first use)
WORST = {}
# the markets whose every call also runs in the run form, {sum, sum2, n} against the same call's dump (greeks_ref.check_sums): local vol
# at spot 0.05 and at a huge spot, the level at k < 0 with rho = 1 (Y != 0 on every path) and at v0 = 0 out of the money
SUMS = {("localvol", 2), ("localvol", 10), ("heston_level", 9), ("heston_level", 7)}


@pytest.fixture(scope="module")
def eng():
    import montecarlocuda_amd as mc
    e = mc.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("family,i", [(f, i) for f in wm.FAMILIES for i in range(COUNTS[f])], ids=lambda v: str(v))
def test_every_path_on_a_wide_market(eng, family, i, X):
    mks = wm.markets(family)
    assert len(mks) == COUNTS[family]
    mk = mks[i]
    worst, calls, nears, kinks, antis, summed = 0.0, 0, 0, 0, set(), 0
    try:
        for m in wm.dates_of(family, mk):
            for c in wm.cases(family, mk, m, X, eng):
                eng.set_antithetic(c.anti), eng.set_control_variate(c.control)
                got = np.asarray(c.run(eng), dtype=np.float64)
                assert got.shape == (wm.N_PATHS,), c.tag
                try:
                    w = c.check(got)
                except AssertionError as e:
                    raise AssertionError(f"{c.tag} {X} market {i}: {e}") from e
                if (family, i) in SUMS:
                    gr.check_sums(c.sums(eng), got, wm.N_PATHS, (c.tag, X, i))
                    summed += 1
                worst, calls, nears, kinks = max(worst, w), calls + 1, nears + int(c.near.sum()), kinks + int(c.kink.sum())
                antis.add(c.anti)
    finally:
        eng.set_antithetic(False), eng.set_control_variate(False)
    assert antis == {False, True} and calls >= 2 * len(wm.dates_of(family, mk)) and summed == (calls if (family, i) in SUMS else 0)
    if family == "localvol":
        assert calls == len(wm.LV_SHAPES) * 2 * 2 * 6
    WORST[family, X] = max(WORST.get((family, X), 0.0), worst)
    print(f"wide {family} {X} market {i} first={mk['first']}: {calls} calls of {wm.N_PATHS} paths, worst err/bound {worst:.3g}, {nears} near and {kinks} kink "
          f"paths; worst of the family so far {WORST[family, X]:.3g}")
