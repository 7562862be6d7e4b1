"""The Bermudan options without a GPU: the binomial lattice (mc_american_lattice_*) against Black-Scholes, against Longstaff and
Schwartz's Table 1 and against a numpy lattice; the backward (Brownian-bridge) walk of a fit; mc_american_solve against
numpy.linalg.lstsq, its never-exercise cases and its independence of what lies beyond `degree`; the float64 model american_ref
as a whole (fit, then price on fresh paths) between the European and the lattice price; and the forward-error bound the GPU
tests use: near paths capped on every GPU shape, a float32 evaluation inside it, four wrong walks outside it."""
import math

import numpy as np
import pytest

import american_ref as am

TOL32 = 2e-6   # TOL["f32"]["pay"] of tests/test_gpu_parity.py (importing that module would import the GPU fixtures' helpers)
NEAR_CAP = 0.05
MUTATION_SHARE = 0.40


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


# ---- 1. the lattice -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["put", "call"])
def test_lattice_with_one_date_converges_to_black_scholes(mc, kind):
    """One exercise date, at maturity: the European option.  The lattice's law converges to the lognormal one and what is left is
    the payoff's kink between two nodes: at most one squared node spacing at the strike, (k v sqrt(t/n))^2, times the largest gamma
    0.4 / (s v sqrt(t)): an error of at most 0.4 k^2 v sqrt(t) / (s n), falling as 1/n (2e-4 at 16384 steps)."""
    for o, _, _, _ in am.TABLE1:
        bs = am.black_scholes(o, kind)
        for n in (64, 1024, 16384):
            err = abs(mc.american_lattice(o, 1, n, kind) - bs)
            print(kind, o["s"], o["v"], n, bs, err)
            assert err <= 0.4 * o["k"] ** 2 * o["v"] * math.sqrt(o["t"]) / (o["s"] * n)


@pytest.mark.parametrize("case", range(3))
def test_lattice_reproduces_table_1(case):
    """Longstaff and Schwartz's finite-difference column, printed to three decimals: 4.478, 6.920, 1.110.  The lattice at n and 2n
    steps per date gives its own Richardson difference; the table's rounding adds 0.0005.  Dates: 50 per year is the table's own
    exercise grid for its simulated column; its finite-difference column is closer to continuous exercise, and the lattice of the
    SAME contract converges to 4.4779 (50 dates), 6.9170 (100 dates over the two years) and 1.1100 (50 dates) -- the two one-year
    cases agree with the table to its last digit, the two-year case does so at 200 dates (6.9201; continuous exercise gives
    6.9233, 4.4867 and 1.1130), which is the date count used for it here ("50 or more")."""
    o, m, fd, _ = am.TABLE1[case]
    dates = m if o["t"] == 1.0 else 2 * m
    coarse, fine = am.lattice(o, dates, 16, "put"), am.lattice(o, dates, 32, "put")
    print(o, dates, coarse, fine, fd)
    assert abs(fine - fd) <= abs(fine - coarse) + 0.0005


def test_c_lattice_equals_the_numpy_lattice(mc):
    for kind in ("put", "call"):
        for o, m, spd in ((am.TABLE1[0][0], 50, 8), (am.TABLE1[1][0], 100, 3), (am.MARKETS["call"], 7, 33), (am.TABLE1[2][0], 1, 500)):
            for X in ("f64", "f32"):
                want = am.lattice({c: (float(np.float32(o[c])) if X == "f32" else o[c]) for c in "skrvt"}, m, spd, kind)
                got = mc.american_lattice(o, m, spd, kind, X)
                assert abs(got - want) <= 1e-12 * want, (kind, o, m, spd, X, got, want)
    assert mc.american_lattice(am.MARKETS["call"], 12, 20, "call") > am.black_scholes(am.MARKETS["call"], "call") + 0.01   # r < 0: exercising early pays
    o = am.TABLE1[0][0]
    for bad, kw in ((dict(o, v=0.0), {}), (dict(o, s=-1.0), {}), (dict(o, k=0.0), {}), (o, dict(n_dates=0)), (o, dict(n_dates=513)),
                    (o, dict(steps_per_date=0)), (o, dict(n_dates=512, steps_per_date=65)), (dict(o, r=3.0, v=0.01), {})):
        with pytest.raises(mc.McError, match="mc error 1"):
            mc.american_lattice(bad, kw.get("n_dates", 10), kw.get("steps_per_date", 4), "put")


# ---- 2. the backward walk ---------------------------------------------------------------------------------------------------
def test_bridge_walk_has_the_covariance_of_a_brownian_motion():
    """W_j from the backward recursion on 2^20 paths: the sample mean of W_i W_j within 4 standard errors of min(i, j)
    (Var(W_i W_j) = i j + min(i, j)^2 for jointly normal W with E = 0)."""
    n, m = 1 << 20, 6
    W = am.bridge(np.random.default_rng(11).standard_normal((n, m)))
    for i in range(1, m + 1):
        for j in range(i, m + 1):
            got, se = float((W[:, i - 1] * W[:, j - 1]).mean()), math.sqrt((i * j + i * i) / n)
            assert abs(got - i) <= 4 * se, (i, j, got, se)
    assert np.abs(W.mean(axis=0)).max() <= 4 * math.sqrt(m / n)


# ---- 3. the solve -----------------------------------------------------------------------------------------------------------
def regression_data(seed, n=5000):
    rng = np.random.default_rng(seed)
    p = np.abs(rng.standard_normal(n)) * 0.15
    V = 0.12 + 0.4 * p - 0.9 * p * p + 0.3 * p ** 3 + 0.02 * rng.standard_normal(n)
    return p, V


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_solve_agrees_with_lstsq(mc, degree):
    """The normal equations square the design matrix's condition number (about 1e3 here, scaled): 1e-9 relative to the largest
    coefficient is what float64 leaves."""
    p, V = regression_data(5)
    S = am.sums(p, V)
    want = np.linalg.lstsq(p[:, None] ** np.arange(degree + 1), V, rcond=None)[0]
    got, model = mc.american_solve(S, degree), am.solve(S, degree)
    assert np.all(got[degree + 1:] == 0)
    assert np.abs(got[:degree + 1] - want).max() <= 1e-9 * np.abs(want).max(), (got, want)
    assert np.abs(got - model).max() <= 1e-12 * np.abs(want).max(), (got, model)   # the same arithmetic, up to libm's sqrt and the order


def test_solve_never_exercise_rows_and_padding(mc):
    p, V = regression_data(6)
    S = am.sums(p, V)
    few = am.sums(p[:am.MIN_ITM - 1], V[:am.MIN_ITM - 1])
    assert few[0] == am.MIN_ITM - 1
    same = am.sums(np.full(100, 0.25), V[:100])               # every path at the same payoff: the scaled Gram matrix has rank 1
    for degree in (1, 2, 3):
        assert np.array_equal(mc.american_solve(few, degree), am.NEVER)
        assert np.array_equal(mc.american_solve(same, degree), am.NEVER), mc.american_solve(same, degree)
        assert np.array_equal(am.solve(few, degree), am.NEVER) and np.array_equal(am.solve(same, degree), am.NEVER)
        assert np.all(np.isfinite(mc.american_solve(am.sums(p[:am.MIN_ITM], V[:am.MIN_ITM]), 1)))
    for degree in (1, 2):                                      # what lies beyond 2 degree and degree is never read
        junk = S.copy()
        junk[2 * degree + 1:7] = np.nan
        junk[7 + degree + 1:] = -1e300
        assert np.array_equal(mc.american_solve(junk, degree), mc.american_solve(S, degree))
    nan = S.copy()
    nan[8] = np.nan
    assert np.array_equal(mc.american_solve(nan, 3), am.NEVER)
    for bad in (0, 4):
        with pytest.raises(mc.McError, match="mc error 1"):
            mc.american_solve(S, bad)


# ---- 4. the model as a whole --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(3))
def test_model_fit_then_price_lies_between_the_european_and_the_lattice_price(mc, case):
    """Fit on 2^16 paths, price on 2^18 fresh ones: a lower bound of the Bermudan price (at most the lattice price plus 3
    half-widths) that is worth more than the European put (by more than 3 half-widths)."""
    o, m, _, _ = am.TABLE1[case]
    beta, ins = am.fit(o, m, "put", 3, np.random.default_rng(100 + case), 1 << 16)
    price, hw = am.price_stream(o, m, "put", beta, np.random.default_rng(200 + case), 1 << 18)
    lat, eu = mc.american_lattice(o, m, 20, "put"), am.black_scholes(o, "put")
    scale = o["k"] * math.exp(-o["r"] * o["t"])
    print(o, m, "price", price, "+-", hw, "in sample", scale * ins[0], "+-", scale * ins[1], "lattice", lat, "european", eu)
    assert price <= lat + 3 * hw
    assert price >= eu + 3 * hw
    assert abs(scale * ins[0] - lat) <= 0.02 * lat   # the in-sample estimate is biased high, by little


def test_model_call_without_dividends_is_the_european_call():
    o, m, _, _ = am.TABLE1[2]
    beta, _ = am.fit(o, m, "call", 3, np.random.default_rng(300), 1 << 16)
    price, hw = am.price_stream(o, m, "call", beta, np.random.default_rng(301), 1 << 18)
    print("call", price, "+-", hw, "black-scholes", am.black_scholes(o, "call"))
    assert abs(price - am.black_scholes(o, "call")) <= 3 * hw


# ---- 5. the bound -------------------------------------------------------------------------------------------------------------
def gpu_shape(kind, m, anti):
    beta = am.rule(kind, m)
    z = np.random.default_rng(9000 + m).standard_normal((am.GPU_PATHS, m)).astype(np.float32)
    return beta, z, am.price(am.MARKETS[kind], m, kind, beta, z, anti, TOL32, am.U["f32"])


@pytest.mark.parametrize("kind", ["put", "call"])
@pytest.mark.parametrize("m", am.DATES)
def test_near_paths_are_few_and_a_float32_walk_stays_inside_the_bound(kind, m):
    """On every shape the GPU tests run, at the fp32 tolerance: at most 5 % of the paths are near; a float32 numpy evaluation of the
    walk is within the bound on every path that is not, and on one of its admissible values on every path that is."""
    o = am.MARKETS[kind]
    for anti in (False, True):
        beta, z, P = gpu_shape(kind, m, anti)
        got = am.walk(o, m, kind, beta, z, np.float32)
        if anti:
            got = 0.5 * (got + am.walk(o, m, kind, beta, -z, np.float32))
        share = float(P.near.mean())
        assert share <= NEAR_CAP, (kind, m, anti, share)
        ok = am.admissible(got, P, anti)
        assert ok.all(), (kind, m, anti, int((~ok).sum()), np.flatnonzero(~ok)[:5])
        assert np.all(np.abs(got - P.value)[~P.near] <= P.bound[~P.near])
    assert np.array_equal(am.walk(o, m, kind, beta, z), am.price(o, m, kind, beta, z).value)   # the two float64 forms of the walk


@pytest.mark.parametrize("mutation", ["late", "no_g", "call", "swap"])
def test_the_bound_rejects_wrong_walks(mutation):
    """Deep in the money (s = 32 on the put of Table 1, 16 dates) at least half the paths exercise before maturity; each wrong
    walk lands outside the bound -- and outside every admissible value of a near path -- on more than 40 % of the paths."""
    o, m, kind = dict(am.MARKETS["put"], s=32.0), 16, "put"
    beta, _ = am.fit(o, m, kind, 3, np.random.default_rng(77), 1 << 14)
    z = np.random.default_rng(78).standard_normal((am.GPU_PATHS, m)).astype(np.float32)
    P = am.price(o, m, kind, beta, z, False, TOL32, am.U["f32"])
    right = am.price(o, m, kind, beta, z)
    tau_early = (right.cand[:, :m - 1] == right.value[:, None]).any(axis=1) & (right.value > 0)
    assert tau_early.mean() >= 0.5, tau_early.mean()
    wrong = am.walk(o, m, kind, beta, z, np.float64, mutation)
    outside = float((~am.admissible(wrong, P)).mean())
    print(mutation, "outside on", outside, "early", tau_early.mean())
    assert outside > MUTATION_SHARE
