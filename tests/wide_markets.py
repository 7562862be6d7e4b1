"""Wide, asymmetric markets for the eleven dated families (not a test module): the market lists and the helpers that
tests/test_wide_markets.py (no GPU: conditions on the lists, power) and tests/test_gpu_wide_markets.py (every path of every
instantiation against the family's float64 model) share.

Why: the families' own cases (barrier_ref.CASES, lookback_ref.CASES, merton_ref.CASES, heston_ref.CASES, american_ref.MARKETS,
rainbow_ref.market) sit in one narrow box -- spot 36 to 120, volatility 0.2 to 0.45, maturity 0.5 to 2 (1.0 in every Heston case but
one), rates at or above 0 but for one call, every rainbow asset at log level 0 -- where a constant folded with |ln S0|, a T dropped
at T = 1, a rate clamped at 0 or a per-date addend one date off while a = 0 pass.  Here every family gets at most 16 markets, drawn
once by a seeded generator ON A FIXED TABLE OF STRATA (the rows of `_single`'s table and of `basket`; numpy's Generator streams are
stable, so the lists are frozen: a market that breaks a condition of tests/test_wide_markets.py is replaced by editing its row, within
its stratum), every value rounded to a float32 so that the model and the kernels of both precisions read the same number:

  single-asset families (Asian, barrier, lookback, Merton, Heston, Heston path, Bermudan, local vol, Heston level), 12 markets each:
    spot        near 0.05, exactly 1.0 (ln S0 = 0), tens, above 1e4
    volatility  near 0.03, near 0.2, above 1               (Heston: sqrt(v0))
    maturity    days (near 0.01), about 1 but not 1, decades (near 20)
    rate        negative; exactly v^2/2 (v a multiple of 2^-10, so that v^2/2 is a float32 and a = (r - v^2/2) dt is exactly 0 in the
                model and on the host); near 0.2; and, outside these three, 0.01 to 0.05 at v near 0.03 (a > 0) and below 0.01 at v near 0.2 (a < 0)
    strike      k = s exp(a m + q v sqrt t), q from -2.5 (deep in the money for a call) to 2.5; k = 0 and k < 0 where the header
                accepts them (Asian without the control variate, barrier, Merton, Heston, Heston path)
    barrier     h = ln s + b p v sqrt t (+ a m when the drift points at the barrier, so that not every path is knocked by the drift
                alone), b = +1 up / -1 down, p from 0.05 to 2.5
    Heston      rho in {-1, -0.9, 0, 0.9, 1}; v0 = 0; kappa = 0; theta 10 times and a tenth of v0; xi 1e-3 and up to 1; Feller held and
                violated
    Merton      mu_j of both signs, delta = 0 and 0.4, lambda t from 0.05 to 6 (lambda dt = 6 at one date: the 64-bit table's cap is
                reached at 6.23)
    Bermudan    puts and calls; the rule of (market, dates) is american_ref.fit on 2^13 paths of a fixed numpy stream, cached
    local vol   the row plus a surface scaled to the row's v and t (the product ignores the option's v).  Grid [y_lo, y_hi] =
                c + (lo, hi) v sqrt t, (lo, hi) rotating over (-2.2, 1.1) (straddling 0, unequal arms), (0.3, 2.0) (wholly above 0: every
                path starts in the lower clamp) and (-1.8, -0.2) (wholly below: in the upper clamp); c = drift / 2, held inside the
                interval that keeps the placement where the drift dwarfs v sqrt t (LV_CENTRE).  Values v (1 + 0.15 q / n_times - 0.35 x
                + 0.25 x^2 + 0.1 / (n_nodes - 1) cos(2.3 i + 0.7 q)), x from -1 to 1 over the nodes: rows and intervals all differ, the
                slope in y times sqrt(dt) z stays of order 1 at any v and t; one market's values are multiplied by (1 + x) / 2 and reach
                exactly 0 at the first node.  A second barrier p standard deviations on the other side: every market runs the four
                kinds.  Calls and puts, the three payoffs, shapes (n_steps, n_times, steps_per_date, n_nodes) LV_SHAPES
    Heston level  the Heston row with a strike chosen for a DIFFERENCE Y = P_fine - P_coarse: q at most 0 (both legs in the money on
                half the paths and more; far out of the money Y is exactly 0), k = 0 and k < 0 on two markets (Y = A_fine - A_coarse
                on every path), q = 0.5 on two (the kink between the legs); shapes (n_dates, steps_per_date) LEVEL_SHAPES
  rainbow and autocall, n = 1 ... 8, two markets each: greeks_ref.random_basket's manner -- distinct spots over 0.05 to 3e4, unequal
    absolute weights (not 1 / s_i), volatilities 0.05 to 0.8 in random order, a random correlation with a negative entry factored by
    mc.chol, t in {0.08, 1.3, 7}, r of both signs; strike, barrier, triggers and coupon levels in standard deviations of the initial
    worst (best) level; EVERY market runs the four types, each without a barrier and with the four barrier kinds, and the six pairs of
    a knock-in mode with memory on or off: every size n meets every switch.
    basket.d stays ZERO: mc_rainbow_run_* and mc_autocall_run_* refuse a non-zero d ("a shift of the terminal normals has no meaning
    on a walk"), so no accepted market can carry one.

`cases(family, market, m, X, eng)` yields every call the GPU test makes on one market at one date count -- antithetic off and on, the
family's switches -- as a Case: how to run it, the model's values, and the family's OWN per-path rule (imported from where it
lives: test_gpu_barrier.check_paths, test_gpu_lookback.check_paths, merton_ref.check_paths, test_gpu_heston.check,
heston_path_ref.check_asian / check_barrier, test_gpu_american.check_paths, test_gpu_rainbow.check_paths, autocall_ref.check,
localvol_ref.check / check_barrier, heston_level_ref.check).  `eng` is
an Engine, or a NumpyEngine: the same call signature for normals and words, numpy's generator behind it, so that the CPU test
walks exactly the shapes of the GPU test.
"""
import itertools
import math
from types import SimpleNamespace as V

import numpy as np

import american_ref as am
import asian_ref as ar
import autocall_ref as ac
import barrier_ref as br
import greeks_ref as gr
import heston_level_ref as hl
import heston_path_ref as hp
import heston_ref as hr
import localvol_ref as lv
import lookback_ref as lr
import merton_ref as mr
import rainbow_ref as rr
from test_gpu_american import check_paths as american_check_paths
from test_gpu_barrier import check_paths as barrier_check_paths
from test_gpu_heston import check as heston_check
from test_gpu_lookback import check_paths as bound_check_paths
from test_gpu_parity import SEED, TOL
from test_gpu_rainbow import check_paths as rainbow_check_paths

N_PATHS = 2121                                  # eight workgroups and a partial wave
FIRSTS = (0, 12345, (1 << 32) - 1000)           # the last range crosses the 2^32-unit seam
DATES = [1, 3, 8, 17]                           # the ends of the date loops (fp32 4 dates per trip; fp64 8, then 2): TRIP_DATES and one date
SINGLE = ["asian", "barrier", "lookback", "merton", "heston", "heston_path", "american", "localvol", "heston_level"]
MULTI = ["rainbow", "autocall"]
FAMILIES = SINGLE + MULTI
BARRIER_FAMILIES = ["barrier", "merton", "heston_path", "rainbow", "autocall", "localvol"]
NEAR_CAP = KINK_CAP = 0.05
assert hp.NEAR_CAP == NEAR_CAP and hr.KINK_CAP == KINK_CAP and lv.NEAR_CAP == NEAR_CAP
NPX = {"f32": np.float32, "f64": np.float64}
# local vol, (n_steps, n_times, steps_per_date, n_nodes): the ends of both precisions' step loops (fp32 four steps per block; fp64 eight
# per trip, then two), one slice and one per step, 2 nodes and the 65 of the family's own test, and an odd number of steps per slice (3)
# and per date (5) that differ
LV_SHAPES = [(1, 1, 1, 2), (3, 3, 1, 3), (8, 2, 2, 65), (17, 1, 1, 9), (15, 5, 5, 4)]
LV_GRIDS = [("straddle", -2.2, 1.1), ("above", 0.3, 2.0), ("below", -1.8, -0.2)]
LV_CENTRE = {"straddle": (-0.8, 1.5), "above": (-0.2, math.inf), "below": (-math.inf, 0.1)}   # the centre c in units of v sqrt t: the placement holds
IN_PLACEMENT = {"straddle": lambda g: g[0] < 0 < g[1], "above": lambda g: g[0] > 0, "below": lambda g: g[1] < 0}
LV_ZERO_NODE = 6                                # the market whose surface is 0 at its first node
# Heston level, (n_dates, steps_per_date): m = 2 (mod 4) and m = 0 (mod 4), one coarse step per date, a date inside an fp64 trip and in the remainder
LEVEL_SHAPES = [(1, 2), (3, 2), (1, 6), (2, 10), (8, 4), (17, 2)]
LEVEL_OTM = (7, 10)                             # the two markets kept out of the money, q = 0.5


def f32(x):
    return float(np.float32(x))


# ---- the single-asset strata ------------------------------------------------------------------------------------------------
# one row per market: spot, volatility, maturity, rate stratum, q (strike, in standard deviations), barrier side and distance p
_TABLE = [
    ("low",  "small", "year",    "neg",    -0.5, +1, 1.0),
    ("low",  "mid",   "decades", "zero_a",  0.0, -1, 0.3),
    ("low",  "big",   "days",    "large",   1.0, +1, 2.0),
    ("one",  "small", "decades", "pos",     0.25, +1, 1.0),
    ("one",  "mid",   "days",    "neg",    -2.5, +1, 0.05),
    ("one",  "big",   "year",    "zero_a", -1.0, -1, 2.5),
    ("tens", "small", "days",    "zero_a",  0.5, +1, 0.3),
    ("tens", "mid",   "year",    "large",   1.5, -1, 0.05),
    ("tens", "big",   "decades", "neg",     0.0, -1, 1.0),
    ("huge", "small", "year",    "large",  -0.25, -1, 2.0),
    ("huge", "mid",   "decades", "small",   2.5, +1, 0.5),
    ("huge", "big",   "days",    "neg",    -1.5, -1, 0.3),
]
SPOT = {"low": lambda g: 0.05 * g.uniform(0.8, 1.3), "one": lambda g: 1.0, "tens": lambda g: g.uniform(20, 90), "huge": lambda g: g.uniform(1.2e4, 3e4)}
VOL = {"small": lambda g: 0.03 * g.uniform(0.95, 1.2), "mid": lambda g: 0.2 * g.uniform(0.8, 1.3), "big": lambda g: g.uniform(1.02, 1.3)}
MATURITY = {"days": lambda g: 0.01 * g.uniform(0.8, 1.5), "year": lambda g: g.choice([g.uniform(0.7, 0.95), g.uniform(1.1, 1.4)]),
            "decades": lambda g: g.uniform(15, 22)}
IN_SPOT = {"low": lambda s: s < 0.1, "one": lambda s: s == 1.0, "tens": lambda s: 10 <= s < 100, "huge": lambda s: s > 1e4}
IN_VOL = {"small": lambda v: v < 0.05, "mid": lambda v: 0.1 < v < 0.3, "big": lambda v: v > 1}
IN_MATURITY = {"days": lambda t: t < 0.02, "year": lambda t: 0.5 < t < 1.5 and t != 1.0, "decades": lambda t: t > 10}


def _single(seed, rows=None):
    """The markets of one family from the table: dicts with the option's fields, the strata's names, the strike's q, a barrier."""
    out = []
    for i, (sp, vo, ma, ra, q, side, p) in enumerate(_TABLE if rows is None else [_TABLE[i] for i in rows]):
        g = np.random.default_rng([seed, i])
        s, t = f32(SPOT[sp](g)), f32(MATURITY[ma](g))
        v = round(VOL[vo](g) * 1024) / 1024          # a multiple of 2^-10: v and v^2/2 are float32 numbers
        r = {"neg": -g.uniform(0.005, 0.04), "zero_a": 0.5 * v * v, "large": g.uniform(0.17, 0.22), "pos": g.uniform(0.01, 0.05), "small": g.uniform(0.002, 0.01)}[ra]
        r = f32(r)
        assert ra != "zero_a" or r - 0.5 * v * v == 0.0
        drift, sd = (r - 0.5 * v * v) * t, v * math.sqrt(t)
        k = f32(s * math.exp(drift + q * sd))
        B = f32(s * math.exp(side * p * sd + (drift if drift * side > 0 else 0.0)))
        out.append(dict(o=dict(s=s, k=k, r=r, v=v, t=t), B=B, up=side > 0, p=p, q=q, strata=(sp, vo, ma, ra), first=FIRSTS[i % 3]))
    return out


def _non_positive_strikes(markets, rows=(4, 9)):
    """k = 0 on one market and k < 0 on another: the families whose header accepts them."""
    for row, k in zip(rows, (0.0, -0.5)):
        o = markets[row]["o"]
        o["k"] = f32(k * o["s"])
    return markets


def _heston(seed, rows=None):
    """Heston markets: the table's volatility stratum is sqrt(v0); the model's own strata rotate over the rows."""
    RHO = [-1.0, -0.9, 0.0, 0.9, 1.0]
    out = _single(seed, rows)
    for i, mk in enumerate(out):
        g = np.random.default_rng([seed, 100 + i])
        o = mk["o"]
        v0 = f32(o.pop("v") ** 2)
        t = o["t"]
        theta = f32(v0 * (10.0 if i % 2 else 0.1))
        kappa = f32(g.uniform(0.5, 3.0) / min(max(t, 0.5), 2.0))
        # xi: tiny, moderate, or as large as keeps sqrt(V) from exploding over t (xi^2 t <= 1)
        xi = f32([1e-3, 0.3 * math.sqrt(max(v0, 1e-3)), min(1.0, 1.0 / math.sqrt(t))][i % 3])
        if i in (2, 7):
            v0 = 0.0
            theta = f32(0.04 if i == 2 else 1.2)
        if i in (5, 10):
            kappa = 0.0
        mk["model"] = dict(v0=v0, kappa=kappa, theta=theta, xi=xi, rho=RHO[i % 5])
        w = 0.5 * (v0 + theta) if kappa > 0 else v0
        sd = math.sqrt(w * t)
        o["k"] = f32(o["s"] * math.exp(o["r"] * t - 0.5 * w * t + mk["q"] * sd))
        mk["B_up"], mk["B_down"] = f32(o["s"] * math.exp(mk["p"] * sd + max(o["r"] * t, 0.0))), f32(o["s"] * math.exp(-mk["p"] * sd + min(o["r"] * t - 0.5 * w * t, 0.0)))
    return out


def _localvol(seed):
    """The row plus a grid and a second barrier on the other side; the surface of a shape is surface_of(mk, shape)."""
    out = _non_positive_strikes(_single(seed))
    for i, mk in enumerate(out):
        o = mk["o"]
        drift, sd = (o["r"] - 0.5 * o["v"] ** 2) * o["t"], o["v"] * math.sqrt(o["t"])
        name, lo, hi = LV_GRIDS[i % 3]
        c = min(max(0.5 * drift, LV_CENTRE[name][0] * sd), LV_CENTRE[name][1] * sd)
        side = -1 if mk["up"] else 1
        mk.update(placement=name, grid=(f32(c + lo * sd), f32(c + hi * sd)), zero_node=i == LV_ZERO_NODE,
                  B2=f32(o["s"] * math.exp(side * mk["p"] * sd + (drift if drift * side > 0 else 0.0))))
    return out


def surface_of(mk, shape):
    """The surface of a local-vol market at a shape, every value a float32 (module docstring); a market may carry its own rule
    (`surface`: the old fixed cases, the mirrored grid of the power test)."""
    if "surface" in mk:
        return mk["surface"](shape)
    _, nt, _, nn = shape
    q, i = np.arange(nt)[:, None], np.arange(nn)[None, :]
    x = np.linspace(-1.0, 1.0, nn)[None, :]
    a = mk["o"]["v"] * (1.0 + 0.15 * q / nt - 0.35 * x + 0.25 * x * x + 0.1 / (nn - 1) * np.cos(2.3 * i + 0.7 * q))
    if mk["zero_node"]:
        a = a * (0.5 * (1.0 + x))
    return lv.make_surface(a.astype(np.float32).astype(np.float64), *mk["grid"])


def _heston_level(seed):
    """The Heston rows, struck for a difference: q at most 0, but 0.5 on LEVEL_OTM; k = 0 and k < 0 on two more."""
    out = _heston(seed)
    for i, mk in enumerate(out):
        o, md = mk["o"], mk["model"]
        mk["qk"] = 0.5 if i in LEVEL_OTM else min(mk["q"], 0.0)
        w = 0.5 * (md["v0"] + md["theta"]) if md["kappa"] > 0 else md["v0"]
        o["k"] = f32(o["s"] * math.exp(o["r"] * o["t"] - 0.5 * w * o["t"] + mk["qk"] * math.sqrt(w * o["t"])))
    return _non_positive_strikes(out)


def _merton(seed):
    out = _non_positive_strikes(_single(seed))
    LT = [0.05, 0.5, 2.0, 6.0]                     # lambda t: lambda dt at one date
    for i, mk in enumerate(out):
        t = mk["o"]["t"]
        mk["jumps"] = dict([("lambda", f32(LT[i % 4] / t)), ("mu_j", f32((-1) ** i * [0.02, 0.1, 0.3][i % 3])), ("delta", f32([0.0, 0.15, 0.4][(i // 2) % 3]))])
    return out


def _american(seed):
    out = _single(seed)
    for i, mk in enumerate(out):
        mk["kind"] = "put" if i % 2 == 0 else "call"
        o = mk["o"]
        q = min(max(mk["q"], -1.0), 1.0) * (1.0 if mk["kind"] == "put" else -1.0)    # at most one standard deviation out of the money
        o["k"] = f32(o["s"] * math.exp((o["r"] - 0.5 * o["v"] ** 2) * o["t"] - q * o["v"] * math.sqrt(o["t"])))
    return out


_RULES = {}


def rule(mk, m):
    """The exercise rule of (market, dates): the model's own fit on numpy normals, as american_ref.rule does for MARKETS."""
    key = (mk["kind"], m) + tuple(sorted(mk["o"].items()))
    if key not in _RULES:
        _RULES[key] = am.fit(mk["o"], m, mk["kind"], 3, np.random.default_rng(7000 + m), 1 << 13)[0]
    return _RULES[key]


# ---- baskets ----------------------------------------------------------------------------------------------------------------
BASKET_T = [0.08, 1.3, 7.0]
RAINBOW_DATES = {n: DATES + ([6] if n % 2 else []) for n in range(1, 9)}   # n n_dates takes every phase of the fp32 unroll 4 / gcd(n, 4)
AUTOCALL_OBS = {1: 1, 3: 3, 6: 3, 8: 4, 17: 17}                            # observations of a date count
KI_MODES = [("dates", True), ("maturity", False), (None, True), ("dates", False), ("maturity", True), (None, False)]


def _chol():
    import montecarlocuda_amd as mc
    return mc.chol


def basket(n, j):
    """Market j (0 or 1) of n assets, in greeks_ref.random_basket's manner on the wide box."""
    g = np.random.default_rng([4100, n, j])
    while True:
        s = np.exp(g.uniform(math.log(0.05), math.log(3e4), n))
        w = g.uniform(0.2, 1.5, n)
        if n == 1 or np.abs(np.diff(np.sort(np.log(w * s)))).min() > 0.05:
            break
    v = g.uniform(0.05, 0.8, n)
    while n > 2 and (np.all(np.diff(v) > 0) or np.all(np.diff(v) < 0)):
        v = g.permutation(v)
    while True:
        A = g.normal(size=(n, n + 2))
        C = A @ A.T
        C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
        if n == 1 or C.min() < -0.05:
            break
    L, bad = _chol()(C)
    assert bad == 0
    r32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    t = f32(BASKET_T[(n + j) % 3] * g.uniform(0.9, 1.1))
    r = f32(g.uniform(0.01, 0.06) * (-1 if (n + j) % 2 else 1))
    return dict(s=r32(s), v=r32(v), p=r32(np.asarray(L, dtype=np.float64)), d=np.zeros(n), w=r32(w), k=1.0, t=t, r=r)


def _extreme(b, use_max):
    """(the initial best or worst weighted level, the standard deviation over t of the asset that holds it)."""
    lv = b["w"] * b["s"]
    i = int(np.argmax(lv) if use_max else np.argmin(lv))
    return float(lv[i]), float(b["v"][i]) * math.sqrt(b["t"])


def _rainbow():
    """Every market carries all four types, each with its own strike and a barrier on either side of the level it reads: q and p
    standard deviations of the initial worst (min types) or best (max types) level."""
    out = []
    for i, (n, j) in enumerate(itertools.product(range(1, 9), (0, 1))):
        b = basket(n, j)
        q, p = [-1.0, -0.3, 0.0, 0.4, 1.0][i % 5], [0.05, 0.5, 1.0, 2.0][i % 4]
        contracts = []
        for kind in rr.KINDS:
            L0, sd = _extreme(b, kind.endswith("max"))
            k = f32(L0 * math.exp(q * sd * (1 if kind.startswith("call") else -1)))
            contracts.append((kind, k, {True: f32(L0 * math.exp(p * sd)), False: f32(L0 * math.exp(-p * sd))}))
        out.append(dict(b=b, n=n, contracts=contracts, p=p, first=FIRSTS[i % 3]))
    return out


def _autocall():
    """Every market runs all six (knock-in mode, memory) pairs of KI_MODES on one knock-in level."""
    out = []
    for i, (n, j) in enumerate(itertools.product(range(1, 9), (0, 1))):
        b = basket(n, j)
        L0, sd = _extreme(b, False)
        b["k"] = f32(L0)
        p = [0.3, 1.0, 2.0][i % 3]
        out.append(dict(b=b, n=n, L0=L0, sd=sd, modes=KI_MODES, B=f32(L0 * math.exp(-p * sd)), p=p, first=FIRSTS[(i + 1) % 3]))
    return out


def contract(mk, n_obs, ki, memory):
    """The note of an autocall market on n_obs observations in one knock-in mode: triggers stepping down from 0.3 standard deviations above the initial
    worst level, the first not callable when there are three or more, coupon levels 0.4 standard deviations below (unconditional
    on every third market), the standard gearing 1 / k."""
    L0, sd = mk["L0"], mk["sd"]
    A = np.array([f32(L0 * math.exp((0.3 - 0.15 * k) * sd * math.sqrt((k + 1) / n_obs))) for k in range(n_obs)])
    if n_obs >= 3:
        A[0] = math.inf
    C = 0.0 if mk["n"] % 3 == 0 else f32(L0 * math.exp(-0.4 * sd))
    return ac.contract(A, C, f32(0.02), barrier=None if ki is None else mk["B"], ki=ki, gearing=None, memory=memory, n_obs=n_obs, k=mk["b"]["k"])


_MARKETS = {}


def markets(family):
    if family not in _MARKETS:
        _MARKETS[family] = {
            "asian": lambda: _non_positive_strikes(_single(1)), "barrier": lambda: _non_positive_strikes(_single(2)), "lookback": lambda: _single(3),
            "merton": lambda: _merton(4), "heston": lambda: _non_positive_strikes(_heston(5)),
            "heston_path": lambda: _non_positive_strikes(_heston(6)),
            "american": lambda: _american(7), "localvol": lambda: _localvol(8), "heston_level": lambda: _heston_level(9),
            "rainbow": _rainbow, "autocall": _autocall}[family]()
        assert len(_MARKETS[family]) <= 16
    return _MARKETS[family]


def dates_of(family, mk):
    """The date counts of one market, Heston path and Heston level: (dates, steps per date), local vol: LV_SHAPES."""
    if family == "heston_path":
        return [(nd, spd) for nd in DATES for spd in (1, 2)]
    if family == "localvol":
        return LV_SHAPES
    if family == "heston_level":
        return LEVEL_SHAPES
    return RAINBOW_DATES[mk["n"]] if family in MULTI else DATES


# ---- numpy behind the Engine's draw calls ----------------------------------------------------------------------------------------
class NumpyEngine:
    """Engine.normals and Engine.words on numpy's generator: a block of a unit range is a function of its arguments, so two walks of
    one market (the model and a mutant) read the same draws."""

    def normals(self, seed, domain, first_unit, n_units, block=0, precision="f64"):
        g = np.random.default_rng([1, domain, block, first_unit & 0xFFFFFFFF, first_unit >> 32])
        return g.standard_normal((n_units, gr.NPB[precision]))

    def words(self, seed, domain, first_unit, n_units, first_block=0, n_blocks=1):
        g = np.random.default_rng([2, domain, first_block, first_unit & 0xFFFFFFFF, first_unit >> 32])
        return g.integers(0, 1 << 32, (n_units, n_blocks, 4), dtype=np.uint64).astype(np.uint32)


# ---- every call of the GPU test on one market ---------------------------------------------------------------------------------
def _ratio(err, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / b)


def _case(tag, anti, run, check, value, bound, near=None, kink=None, knocked=None, control=False, sums=None):
    """run(engine) -> the per-path values (float64); check(got) -> the worst err / bound, asserting the family's rule; value and
    bound (n,): the model's values and per-path bounds (the power test); near, kink: masks; knocked: the plain direction's mask;
    sums(engine) -> the run form's Estimate of the same call (local vol and Heston level)."""
    n = value.size
    z = np.zeros(n, dtype=bool)
    return V(tag=tag, anti=anti, control=control, run=run, check=check, value=value, bound=bound, near=z if near is None else near,
             kink=z if kink is None else kink, knocked=knocked, sums=sums)


def _draw(eng, X):
    return lambda domain, u0, c, block: eng.normals(SEED, domain, u0, c, block, X)


def kinds_of(mk):
    """The two barrier types of a single-asset market: by the side its barrier was placed on, not by a (mutated) spot."""
    return br.KINDS[:2] if mk["up"] else br.KINDS[2:]


def cases(family, mk, m, X, eng, mutate=None):
    """Every call on market mk at m dates in precision X.  mutate: "up_as_down" (the barrier's direction read from |gap|) or
    "no_compensator" (Merton), or a name of localvol_ref.MUTATIONS / heston_level_ref.MUTATIONS (those two families); every other
    mutation of the power test is a change of the market itself."""
    return list(globals()["_" + family + "_cases"](mk, m, X, eng, mutate))


def _asian_cases(mk, m, X, eng, mutate):
    o, first, n, tol = mk["o"], mk["first"], N_PATHS, TOL[X]["pay"]
    z = ar.asian_normals(_draw(eng, X), first, n, m, gr.NPB[X])
    for anti, control in itertools.product((False, True), repeat=2):
        if control and not o["k"] > 0:      # the control variate needs k > 0 (mc_asian_run_*)
            continue
        p = ar.asian(o, m, z, control, anti)
        yield _case(("asian", m, anti, control), anti, lambda e: e.asian_paths(o, m, n, SEED, first, X).astype(np.float64),
                    lambda got, p=p: bound_check_paths(got, p, tol), p.value[0], gr.bound(p, tol)[0], control=control)


def _barrier_cases(mk, m, X, eng, mutate):
    o, B, first, n, tol = mk["o"], mk["B"], mk["first"], N_PATHS, TOL[X]["pay"]
    z = br.barrier_normals(_draw(eng, X), first, n, m, gr.NPB[X])
    up = True if mutate == "up_as_down" else mk["up"]
    for monitoring, anti in itertools.product(br.MONITORINGS, (False, True)):
        sides = br.walk(o, B, m, z, up, monitoring, anti)
        for kind in kinds_of(mk):
            p = br.value(sides, kind.endswith("in"))
            yield _case(("barrier", m, kind, monitoring, anti), anti,
                        lambda e, kind=kind, monitoring=monitoring: e.barrier_paths(o, B, m, n, SEED, first, X, kind, monitoring).astype(np.float64),
                        lambda got, sides=sides, kind=kind, monitoring=monitoring: barrier_check_paths(got, sides, kind.endswith("in"), monitoring, tol)[0],
                        p.value[0], gr.bound(p, tol)[0], near=p.edge <= tol, knocked=None if monitoring == "continuous" else sides[0]["P"] == 0)


def _lookback_cases(mk, m, X, eng, mutate):
    o, first, n, tol = mk["o"], mk["first"], N_PATHS, TOL[X]["pay"]
    assert tol == lr.EPS[X]
    z, u = lr.lookback_draws(_draw(eng, X), lambda domain, u0, c, b0, nb: eng.words(SEED, domain, u0, c, b0, nb), first, n, m, X)
    for monitoring in lr.MONITORINGS:
        both = {side: lr.walk(o, m, z, u, side, monitoring, True, tol) for side in (True, False)}
        for anti, kind in itertools.product((False, True), lr.KINDS):
            sides = both[lr.ON_MAX[kind]]
            p = lr.value(sides if anti else sides[:1], kind, o["k"])
            yield _case(("lookback", m, kind, monitoring, anti), anti,
                        lambda e, kind=kind, monitoring=monitoring: e.lookback_paths(o, m, n, SEED, first, X, kind, monitoring).astype(np.float64),
                        lambda got, p=p: bound_check_paths(got, p, tol), p.value[0], gr.bound(p, tol)[0])


def _merton_run(e, o, jp, B, m, n, first, X, payoff, kind):
    if payoff == "european":
        return e.merton_paths(o, jp, m, n, SEED, first, X)
    if payoff == "asian":
        return e.merton_asian_paths(o, jp, m, n, SEED, first, X)
    return e.merton_barrier_paths(o, jp, B, m, n, SEED, first, X, kind)


def _merton_cases(mk, m, X, eng, mutate):
    import montecarlocuda_amd as mc
    o, B, jp, first, n, tol = mk["o"], mk["B"], mk["jumps"], mk["first"], N_PATHS, TOL[X]["pay"]
    z, N = mr.merton_draws(eng, SEED, X, first, n, m, mc.merton_thresholds(o, jp, m, X))
    up = True if mutate == "up_as_down" else mk["up"]
    for anti in (False, True):
        c, sides = mr.walk(o, jp, m, z, N, B, up, anti, "no_compensator" if mutate == "no_compensator" else None)
        for payoff, kind in [("european", None), ("asian", None)] + [("barrier", kd) for kd in kinds_of(mk)]:
            knock_in = bool(kind) and kind.endswith("in")
            p = mr.value(c, sides, payoff, knock_in)
            yield _case(("merton", m, payoff, kind, anti), anti,
                        lambda e, payoff=payoff, kind=kind: _merton_run(e, o, jp, B, m, n, first, X, payoff, kind).astype(np.float64),
                        lambda got, c=c, sides=sides, payoff=payoff, knock_in=knock_in: mr.check_paths(got, c, sides, payoff, knock_in, tol)[0],
                        p.value[0], gr.bound(p, tol)[0], near=p.edge <= tol, knocked=sides[0]["P"] == 0 if payoff == "barrier" else None)


def _heston_cases(mk, m, X, eng, mutate):
    o, model, first, n, tol = mk["o"], mk["model"], mk["first"], N_PATHS, TOL[X]["pay"]
    z1, z2 = hr.heston_normals(_draw(eng, X), first, n, m, hr.NPB[X])
    both = hr.walk(o, model, m, z1, z2, anti=True)
    for anti, p in ((False, hr.plain_of(both)), (True, both)):
        b, kink = hr.bound(p, tol)

        def check(got, p=p, anti=anti):
            worst, kinks = heston_check(got, p, tol, ("heston", m, anti))
            assert kinks <= KINK_CAP * n, (m, anti, kinks)
            return worst

        yield _case(("heston", m, anti), anti, lambda e: e.heston_paths(o, model, m, n, SEED, first, X), check, p.value[0], b, kink=kink)


def _heston_path_cases(mk, shape, X, eng, mutate):
    o, model, first, n, tol = mk["o"], mk["model"], mk["first"], N_PATHS, TOL[X]["pay"]
    nd, spd = shape
    z1, z2 = hp.heston_path_normals(_draw(eng, X), first, n, nd * spd, hp.NPB[X])
    both = hp.walk(o, model, nd, spd, z1, z2, anti=True)
    for anti in (False, True):
        sides = both if anti else both[:1]
        b, kink = hp.asian_bound(sides, tol)
        yield _case(("heston_path", shape, "asian", anti), anti, lambda e: e.heston_asian_paths(o, model, nd, spd, n, SEED, first, X),
                    lambda got, sides=sides, anti=anti: hp.check_asian(got, sides, tol, ("asian", shape, anti))[0], hp.asian(sides), b, kink=kink)
        for B, kind in [(mk["B_up"], k) for k in hp.KINDS[:2]] + [(mk["B_down"], k) for k in hp.KINDS[2:]]:
            b, near, kink = hp.barrier_bound(sides, B, kind, tol)
            live = hp._barrier_side(sides[0], B, kind.startswith("up") != (mutate == "up_as_down"), None)[0]
            yield _case(("heston_path", shape, kind, anti), anti,
                        lambda e, B=B, kind=kind: e.heston_barrier_paths(o, model, B, nd, spd, n, SEED, first, X, kind),
                        lambda got, sides=sides, B=B, kind=kind, anti=anti: hp.check_barrier(got, sides, B, kind, tol, (shape, anti))[0],
                        hp.barrier(sides, B, kind, up_as_down=mutate == "up_as_down"), b, near=near, kink=kink, knocked=~live)


def _american_cases(mk, m, X, eng, mutate):
    o, kind, first, n, tol = mk["o"], mk["kind"], mk["first"], N_PATHS, TOL[X]["pay"]
    beta = mk.get("beta", {}).get(m)
    beta = rule(mk, m) if beta is None else beta
    z = am.american_normals(_draw(eng, X), first, n, m, gr.NPB[X])
    for anti in (False, True):
        P = am.price(o, m, kind, beta, z, anti, tol, am.U[X])

        def check(got, P=P, anti=anti):
            american_check_paths(got, P, anti, f"wide {X} {kind} m={m} first={first} anti={anti}")
            far = ~P.near
            return float(_ratio(np.abs(got - P.value)[far], P.bound[far]).max()) if far.any() else 0.0

        yield _case(("american", m, kind, anti), anti, lambda e: e.american_paths(o, m, beta, n, SEED, first, X, kind).astype(np.float64), check,
                    P.value, P.bound, near=P.near)


def lv_barriers(mk):
    """(barrier, kind) of a local-vol market: its own barrier with its side's two kinds, the second barrier with the other side's."""
    own = kinds_of(mk)
    return [(mk["B"], k) for k in own] + [(mk["B2"], k) for k in lv.KINDS if k not in own]


def _localvol_cases(mk, shape, X, eng, mutate):
    """mutate: one of localvol_ref.MUTATIONS, or "up_as_down" (dk = sgn |ln(B / s)|: a down barrier read as an up barrier)."""
    o, first, n, tol = mk["o"], mk["first"], N_PATHS, TOL[X]["pay"]
    m, nt, spd, nn = shape
    nd = m // spd
    surf = surface_of(mk, shape)
    z = lv.localvol_normals(_draw(eng, X), first, n, m, gr.NPB[X])
    in_walk = mutate if mutate in ("slice_late", "round_nearest", "no_half", "clamp_n", "date_late") else None
    in_pay = mutate if mutate in ("one_more", "put_as_call") else None
    both = lv.walk(o, surf, nd, spd, z, anti=True, tol=tol, table=NPX[X], mutation=in_walk)
    for anti in (False, True):
        sides = both if anti else both[:1]
        for right in ("call", "put"):
            what = ("localvol", shape, right, anti)
            value, b = lv.european(sides, right, in_pay), lv.european_bound(sides, right)
            yield _case(("localvol", shape, "european", right, None, anti), anti,
                        lambda e, right=right: e.localvol_paths(o, surf, m, n, right, SEED, first, X).astype(np.float64),
                        lambda got, value=value, b=b, what=what: lv.check(got, value, b, what + ("european",)), value, b,
                        sums=lambda e, right=right: e.localvol(o, surf, m, n, right, SEED, first, X))
            value, b = lv.asian(sides, right, in_pay), lv.asian_bound(sides, right)
            yield _case(("localvol", shape, "asian", right, None, anti), anti,
                        lambda e, right=right: e.localvol_asian_paths(o, surf, nd, spd, n, right, SEED, first, X).astype(np.float64),
                        lambda got, value=value, b=b, what=what: lv.check(got, value, b, what + ("asian",)), value, b,
                        sums=lambda e, right=right: e.localvol_asian(o, surf, nd, spd, n, right, SEED, first, X))
            for B, kind in lv_barriers(mk):
                up = kind.startswith("up")
                read = "up" + kind[kind.index("-"):] if mutate == "up_as_down" else kind
                parts = [lv._barrier_side(s, B, up, right, True) for s in sides]
                b = sum(p[3] for p in parts) / len(sides) + tol * np.abs(lv.barrier(sides, B, kind, right))
                near = np.logical_or.reduce([p[1] for p in parts])
                yield _case(("localvol", shape, "barrier", right, kind, anti), anti,
                            lambda e, right=right, B=B, kind=kind: e.localvol_barrier_paths(o, surf, B, nd, spd, n, right, SEED, first, X, kind).astype(np.float64),
                            lambda got, sides=sides, B=B, kind=kind, right=right, what=what: lv.check_barrier(got, sides, B, kind, right, what)[0],
                            lv.barrier(sides, B, read, right, in_pay), b, near=near, knocked=~lv._barrier_side(sides[0], B, read.startswith("up"), right, False)[0],
                            sums=lambda e, right=right, B=B, kind=kind: e.localvol_barrier(o, surf, B, nd, spd, n, right, SEED, first, X, kind))


def _heston_level_cases(mk, shape, X, eng, mutate):
    """mutate: one of heston_level_ref.MUTATIONS (the coarse leg's)."""
    o, model, first, n, tol = mk["o"], mk["model"], mk["first"], N_PATHS, TOL[X]["pay"]
    nd, spd = shape
    z1, z2 = hl.level_normals(_draw(eng, X), first, n, nd * spd, hl.NPB[X])
    both = hl.walk(o, model, nd, spd, z1, z2, anti=True, mutation=mutate, prec=NPX[X])      # prec: as tests/test_gpu_heston_level.py sets it
    for anti, level in ((False, hl.plain_of(both)), (True, both)):
        b, kink = hl.bound(level, tol)
        yield _case(("heston_level", shape, anti), anti, lambda e: e.heston_level_paths(o, model, nd, spd, n, SEED, first, X).astype(np.float64),
                    lambda got, level=level, anti=anti: hl.check(got, level, tol, ("heston_level", shape, anti))[0], hl.value(level), b, kink=kink,
                    sums=lambda e: e.heston_level(o, model, nd, spd, n, SEED, first, X))


def _rainbow_cases(mk, m, X, eng, mutate):
    first, n, tol = mk["first"], N_PATHS, TOL[X]["pay"]
    z = rr.rainbow_normals(_draw(eng, X), first, n, mk["n"], m, gr.NPB[X])
    for kind, k, barriers in mk["contracts"]:
        b = dict(mk["b"], k=k)
        for si, side in enumerate(sorted(barriers)):
            B = barriers[side]
            both = rr.walk(b, m, z, kind, B, True if mutate == "up_as_down" else side, anti=True)
            for anti in (False, True):
                sides = both if anti else both[:1]
                for bk in ([None] if si == 0 else []) + rr.kinds_of(side):       # without a barrier: once per type
                    p = rr.value(sides, bk)
                    yield _case(("rainbow", mk["n"], m, kind, bk, anti), anti,
                                lambda e, b=b, kind=kind, B=B, bk=bk: e.rainbow_paths(b, m, n, kind, None if bk is None else B, bk, SEED, first, X).astype(np.float64),
                                lambda got, sides=sides, bk=bk: rainbow_check_paths(got, sides, bk, tol)[0], p.value[0], gr.bound(p, tol)[0],
                                near=p.edge <= tol, knocked=None if bk is None else sides[0]["P"] == 0)


def _autocall_cases(mk, m, X, eng, mutate):
    b, first, n, tol = mk["b"], mk["first"], N_PATHS, TOL[X]["pay"]
    z = ac.autocall_normals(_draw(eng, X), first, n, mk["n"], m, gr.NPB[X])
    both = ac.walk(b, m, z, anti=True)
    for ki, memory in mk["modes"]:
        con = ac.contract_a(AUTOCALL_OBS[m]) if mk.get("old") else contract(mk, AUTOCALL_OBS[m], ki, memory)
        for anti in (False, True):
            sides = both if anti else both[:1]
            p, cands = ac.value(b, m, con, sides, tol, full=True)
            knocked = None
            if con["ki"] is not None:
                knocked = ac._knock_in(b, m, con, sides[0][0], sides[0][1], None)[0] > 0
            yield _case(("autocall", mk["n"], m, con["ki"], con["memory"], anti), anti,
                        lambda e, con=con: e.autocall_paths(b, m, n, con["autocall"], con["coupon_barrier"], con["coupon"], con["barrier"], con["ki"],
                                                            con["gearing"], con["memory"], SEED, first, X).astype(np.float64),
                        lambda got, p=p, cands=cands: ac.check(got, p, cands, tol)[0], p.value[0], gr.bound(p, tol)[0], near=p.edge <= tol, knocked=knocked)


# ---- the wrong restatements of the power test -----------------------------------------------------------------------------------
def _opt(mk, **changes):
    return dict(mk, o=dict(mk["o"], **changes))


def _a_dt(mk, m):
    """The per-date addend a = (r - v^2/2) dt of a constant-volatility market (Merton: with the compensator)."""
    o = mk["o"]
    comp = 0.0
    if "jumps" in mk:
        jp = mk["jumps"]
        comp = jp["lambda"] * math.expm1(jp["mu_j"] + 0.5 * jp["delta"] ** 2)
    return (o["r"] - comp - 0.5 * o["v"] ** 2) * o["t"] / m


def _abs_ln_s0(family, mk, m):
    if family in MULTI:       # |ln(w_i s_i)| for ln(w_i s_i)
        lv = mk["b"]["w"] * mk["b"]["s"]
        return dict(mk, b=dict(mk["b"], w=np.where(lv < 1, 1.0 / (lv * mk["b"]["s"]), mk["b"]["w"])))
    s = math.exp(abs(math.log(mk["o"]["s"])))
    if family == "localvol":      # x0 = |ln s| alone: dk = sgn ln(B / s) is folded apart from it, so the barriers keep their distance
        return dict(_opt(mk, s=s), B=mk["B"] * s / mk["o"]["s"], B2=mk["B2"] * s / mk["o"]["s"])
    return _opt(mk, s=s)


def _rate_clamped(family, mk, m):
    if family in MULTI:
        return dict(mk, b=dict(mk["b"], r=max(mk["b"]["r"], 0.0)))
    return _opt(mk, r=max(mk["o"]["r"], 0.0))


def _t_dropped(family, mk, m):
    """dt = 1 / m in the volatility step only: bx = v sqrt(1 / m), a unchanged (baskets: M = diag(v sqrt(1 / m)) L, by the factor)."""
    if family in MULTI:
        return dict(mk, b=dict(mk["b"], p=mk["b"]["p"] / math.sqrt(mk["b"]["t"])))
    o = mk["o"]
    v = o["v"] / math.sqrt(o["t"])
    return _opt(mk, v=v, r=o["r"] - 0.5 * o["v"] ** 2 + 0.5 * v * v)


def _addend_late(family, mk, m):
    """The per-date addend taken at j - 1: ln S0 + (j - 1) a (Heston path: the per-date constant ln S0 + r t_{d-1})."""
    if family == "heston_path":
        return _opt(mk, s=mk["o"]["s"] * math.exp(-mk["o"]["r"] * mk["o"]["t"] / m[0]))
    if family in MULTI:
        b = mk["b"]
        a = (b["r"] - 0.5 * b["v"] ** 2) * b["t"] / m
        return dict(mk, b=dict(b, w=b["w"] * np.exp(-a)))
    return _opt(mk, s=mk["o"]["s"] * math.exp(-_a_dt(mk, m)))


def _rows_exchanged(family, mk, m):
    """The initial rows ln(w_i s_i) of assets 0 and 1 exchanged; volatilities and the factor stay."""
    b = mk["b"]
    s, w = b["s"].copy(), b["w"].copy()
    s[[0, 1]], w[[0, 1]] = s[[1, 0]], w[[1, 0]]
    return dict(mk, b=dict(b, s=s, w=w))


def _grid_mirrored(family, mk, m):
    """u0 = y_hi / h for -y_lo / h: the grid [-y_hi, -y_lo] under the same values."""
    def mirrored(shape):
        s = surface_of(mk, shape)
        return dict(s, y_lo=-s["y_hi"], y_hi=-s["y_lo"])
    return dict(mk, surface=mirrored)


def _dt_without_t(family, mk, m):
    """dt = 1 / m.  Local vol: in r dt, dt / 2 and sqrt(dt) -- the model at t = 1 on the same surface.  Heston level: heston_args' dt,
    in kdt, ktdt, c1, c2, av and aw, while x0 and the per-date table keep r t -- the model at t = 1 with the rate r t."""
    if family == "localvol":
        return _opt(mk, t=1.0)             # the grid is the market's own, frozen: the surface stays
    return _opt(mk, t=1.0, r=mk["o"]["r"] * mk["o"]["t"])


CONSTANT_VOL = ["asian", "barrier", "lookback", "merton", "american"]
# name -> (the families it applies to, market -> market or None, the `mutate` switch of cases())
MUTATIONS = {
    "|ln S0| for ln S0": (FAMILIES, _abs_ln_s0, None),
    "rate clamped at 0": ([f for f in FAMILIES if f != "heston_level"], _rate_clamped, None),
    "T dropped in the volatility step": (CONSTANT_VOL + MULTI, _t_dropped, None),
    "addend of date j - 1": (CONSTANT_VOL + ["heston_path"] + MULTI, _addend_late, None),
    "gap's sign from |gap|": (["barrier", "merton", "heston_path", "rainbow", "localvol"], None, "up_as_down"),
    "|rho| for rho": (["heston", "heston_path", "heston_level"], lambda f, mk, m: dict(mk, model=dict(mk["model"], rho=abs(mk["model"]["rho"]))), None),
    "kappa theta dt with T = 1": (["heston", "heston_path"], lambda f, mk, m: dict(mk, model=dict(mk["model"], theta=mk["model"]["theta"] / mk["o"]["t"])), None),
    "sign of mu_j": (["merton"], lambda f, mk, m: dict(mk, jumps=dict(mk["jumps"], mu_j=-mk["jumps"]["mu_j"])), None),
    "compensator dropped": (["merton"], None, "no_compensator"),
    "initial rows of assets 0 and 1 exchanged": (MULTI, _rows_exchanged, None),
    "u0 from y_hi (a mirrored grid)": (["localvol"], _grid_mirrored, None),
    "dt without T (T = 1)": (["localvol", "heston_level"], _dt_without_t, None),
    "|r| for r": (["heston_level"], lambda f, mk, m: _opt(mk, r=abs(mk["o"]["r"])), None),
}
MUTATIONS.update({f"localvol_ref: {name}": (["localvol"], None, name) for name in lv.MUTATIONS})
MUTATIONS.update({f"heston_level_ref: {name}": (["heston_level"], None, name) for name in hl.MUTATIONS})


def moved_share(family, mk, m, name, eng=None):
    """The largest share, over the calls on market mk at m dates, of the paths with a non-zero value that the mutation moves beyond
    the fp32 bound; None when the mutation cannot apply to this market (it leaves the market as it is)."""
    families, change, switch = MUTATIONS[name]
    assert family in families
    eng = NumpyEngine() if eng is None else eng
    if family in MULTI and name.startswith("initial rows") and mk["n"] < 2:
        return None
    mutant = mk if change is None else change(family, mk, m)
    if family == "american":      # both walks under the rule of the unchanged market
        mk = dict(mk, beta={m: rule(mk, m)})
        mutant = dict(mutant, beta=mk["beta"])
    if switch == "up_as_down" and _is_up(family, mk):
        return None
    true, wrong = cases(family, mk, m, "f32", eng), cases(family, mutant, m, "f32", eng, switch)
    best = 0.0
    for c, w in zip(true, wrong):
        assert c.tag == w.tag
        live = c.value != 0
        if live.sum() >= 20:
            best = max(best, float((np.abs(w.value - c.value) > c.bound)[live & ~c.near].sum() / live.sum()))
    return best


def _is_up(family, mk):
    """No down barrier on this market: reading the direction from |gap| changes nothing."""
    if family in ("heston_path", "localvol"):
        return False              # every market carries both barriers
    if family == "rainbow":
        return all(side for _, _, barriers in mk["contracts"] for side in barriers)
    return mk["up"]


# ---- the families' old fixed cases, in this module's market form (the power test runs every mutation on them too) ---------------
def old_markets(family):
    if family == "asian":
        return [dict(o=o, first=0) for o in ar.CASES]
    if family == "barrier":
        return [dict(o=o, B=B, up=B > o["s"], first=0) for o, B in br.CASES]
    if family == "lookback":
        return [dict(o=o, first=0) for o in lr.CASES]
    if family == "merton":
        return [dict(o=o, B=B, up=B > o["s"], jumps=jp, first=0) for o, B, jp in mr.CASES + [mr.HEAVY]]
    if family in ("heston", "heston_path", "heston_level"):
        return [dict(o=o, model=model, B_up=hp.UP, B_down=hp.DOWN, first=0) for _, o, model in hr.CASES]
    if family == "localvol":      # lv.MKT on the two symmetric grids of tests/test_gpu_localvol.py, one barrier per side
        return [dict(o=lv.MKT, B=lv.UP, B2=lv.DOWN, up=True, first=0, surface=lambda shape, grid=grid: lv.surface_for(shape, grid)) for grid in (lv.WIDE, lv.NARROW)]
    if family == "american":
        return [dict(o=o, kind=kind, first=0) for kind, o in am.MARKETS.items()]
    if family == "rainbow":
        return [dict(b=b, n=n, contracts=[(kind, b["k"], {up: B})], first=0) for n in rr.ASSETS for b, kind, B, up in rr.cases(n)] + \
            [dict(b=rr.ABSOLUTE[0], n=3, contracts=[(rr.ABSOLUTE[1], rr.ABSOLUTE[0]["k"], {rr.ABSOLUTE[3]: rr.ABSOLUTE[2]})], first=0)]
    out = []
    for n in ac.ASSETS:
        b = rr.market(n)
        out.append(dict(b=b, n=n, L0=1.0, sd=float(b["v"][0]) * math.sqrt(b["t"]), modes=[("dates", True)], B=0.6, first=0, old=True))
    return out
