"""The XORWOW mode's sample definition in numpy (not a test module).

Written from the one sentence of include/mc_mi355x.h (mc_context_set_generator): lane l of a launch starts at rocRAND's
(seed, subsequence_base + l), keeps ONE sequence for the whole launch, and draws four words per block of normals.  With
L = grid x 256 lanes of the launch (Engine.last_launch on the GPU -- never restated from the grid rule) a call is one segment
whose unit u (0-based) is priced by lane u mod L as that lane's (u div L)-th unit, ascending, and a unit consumes WHOLE blocks,
used or not (a block is 4 words = 4 normals in fp32, 12 words = 4 Box-Muller pairs = 8 normals in fp64):
  vanilla  one block per unit of 4 (fp32) or 8 (fp64) paths, a unit only partly inside [first, first + n) included;
  basket   ceil(4 ceil(n / 4) / NPB) blocks per path, normal k of the path = entry k of those blocks;
  CVA      ceil(d / NPB) blocks per path, d = the dates the schedule prices (cva_ref.schedule); fp64 draws them pair by pair,
           three words a pair, and skips to the end of the block of four pairs after the last date.
(ceil(4 ceil(n / 4) / NPB) = ceil(n / NPB) for every n -- nested ceilings -- so a kernel that pads the basket to whole blocks
only draws the same sample: test_xorwow_ref.py holds that identity instead of listing it as an error.)

`unit_words(words[L, K], n_units, words_per_unit)` cuts the lanes' words into the units' words; `normals_of_words` turns them
into normals through a caller-supplied words-to-normals step -- on the GPU the device's own inline functions through
Engine.math_probe, on the CPU `cpu_normals` (math_ref's long-double Box-Muller) -- and `vanilla_z`, `basket_g`, `cva_z` pick a
product's normals.  The values are greeks_ref.vanilla, basket_ref.value and cva_ref.price: nothing here prices anything.

MUTATIONS are wrong assignments a kernel could plausibly implement, stated as changes of (lanes, words a unit moves on by,
order of the trips).  test_xorwow_ref.py holds the model to the oracle's XORWOW twin and shows that every mutation moves
almost every later-trip path it can reach beyond the bound; test_gpu_xorwow_ref.py holds the kernels to the model.
"""
import math
from collections import namedtuple

import numpy as np

import basket_ref as br
import cva_ref as cr
import greeks_ref as gr
import math_ref as mr

GROUP = 256
NPB = {"f32": 4, "f64": 8}     # normals per block
WPB = {"f32": 4, "f64": 12}    # words per block
PRECISIONS = ["f32", "f64"]
U64 = np.uint64


# ---- words a unit consumes ---------------------------------------------------------------------------------------------
def vanilla_blocks(X):
    return 1


def basket_blocks(n_assets, X):
    return -(-(4 * (-(-n_assets // 4))) // NPB[X])


def cva_blocks(n_dates, X):
    return -(-n_dates // NPB[X])


# ---- a call -------------------------------------------------------------------------------------------------------------------
# family: "vanilla" | "basket" | "cva"; blocks: the context's; lanes: grid x 256 of the launch; n_units: units of the segment;
# size: assets or dates (vanilla: 0); head: paths of unit 0 below `first` (vanilla only)
Call = namedtuple("Call", "family X blocks lanes n_units size head")


def blocks_per_unit(c):
    return {"vanilla": lambda: vanilla_blocks(c.X), "basket": lambda: basket_blocks(c.size, c.X), "cva": lambda: cva_blocks(c.size, c.X)}[c.family]()


def words_per_unit(c):
    return blocks_per_unit(c) * WPB[c.X]


def trips(c, lanes=None):
    return -(-c.n_units // (lanes or c.lanes))


def words_needed(c, lanes=None):
    """K: the words the busiest lane draws."""
    return trips(c, lanes) * words_per_unit(c)


def later_trips(c):
    """Mask over the units: those a lane prices after its first."""
    return np.arange(c.n_units) >= c.lanes


# ---- the assignment -----------------------------------------------------------------------------------------------------------
def unit_words(words, n_units, words_per_unit, advance=None, order=None):
    """The words of every unit, (n_units, words_per_unit): unit u reads words_per_unit words of lane u mod L from where that lane's
    earlier units left its sequence.  `advance` (per unit; default words_per_unit) is what a unit moves the sequence on by and
    `order` the order in which the trips draw (default ascending): both exist for MUTATIONS only."""
    words = np.asarray(words)
    L, K = words.shape
    u = np.arange(n_units)
    lane, trip = u % L, u // L
    adv = np.broadcast_to(np.asarray(words_per_unit if advance is None else advance, dtype=np.int64), (n_units,))
    start, cursor = np.zeros(n_units, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for t in (range(-(-n_units // L)) if order is None else order):
        sel = u[trip == t]
        start[sel] = cursor[lane[sel]]
        cursor[lane[sel]] += adv[sel]
    idx = start[:, None] + np.arange(words_per_unit)[None, :]
    assert idx.max() < K, (int(idx.max()), K)
    return words[lane[:, None], idx]


def normals_of_words(w, X, to_normals):
    """(n_units, blocks x NPB) float64: every block of the units' words through to_normals((m, WPB) words) -> (m, NPB)."""
    n, k = w.shape
    assert k % WPB[X] == 0
    z = np.asarray(to_normals(np.ascontiguousarray(w).reshape(-1, WPB[X]), X), dtype=np.float64)
    assert z.shape == (n * k // WPB[X], NPB[X])
    return z.reshape(n, -1)


def cpu_normals(blocks, X):
    """The words-to-normals step from the definitions (math_ref, long double): fp32 words (x, y, z, w) -> cos, sin of (x, y), cos, sin
    of (z, w); fp64 pair p of a block = words 3p, 3p + 1, 3p + 2 -> cos, sin."""
    b = np.asarray(blocks, dtype=U64)
    if X == "f32":
        pairs = [mr.normals_f32(b[:, 0], b[:, 1]), mr.normals_f32(b[:, 2], b[:, 3])]
    else:
        pairs = [mr.normals_J(*mr.pair_J(b[:, 3 * p], b[:, 3 * p + 1], b[:, 3 * p + 2])) for p in range(4)]
    return np.stack([np.asarray(v, dtype=np.float64) for zc, zs in pairs for v in (zc, zs)], axis=1)


def vanilla_z(z_units, c, n_paths):
    """Path p of the range: entry (head + p) mod NPB of unit (head + p) div NPB."""
    return z_units[:, :NPB[c.X]].reshape(-1)[c.head:c.head + n_paths]


def unit_of_path(c, n_paths):
    """The unit every path of the range belongs to (vanilla: NPB paths a unit; the others: one)."""
    p = np.arange(n_paths)
    return (c.head + p) // NPB[c.X] if c.family == "vanilla" else p


def product_normals(z_units, c, n_paths):
    if c.family == "vanilla":
        return vanilla_z(z_units, c, n_paths)
    return z_units[:, :c.size]


def vanilla_call(X, blocks, lanes, first, n_paths):
    u0, u1 = first // NPB[X], -(-(first + n_paths) // NPB[X])
    return Call("vanilla", X, blocks, lanes, u1 - u0, 0, first - u0 * NPB[X])


def draw(c, words_of, to_normals, mutation=None):
    """The normals of every unit of call c, (n_units, blocks x NPB): words_of(lanes, K) -> the first K words of lanes 0 .. lanes - 1
    of the call's (seed, subsequence base).  `mutation`: a key of MUTATIONS."""
    lanes, advance, order = c.lanes, None, None
    if mutation is not None:
        assert applies(mutation, c), (mutation, c)
        lanes, advance, order = MUTATIONS[mutation].change(c)
    wpu = words_per_unit(c)
    w = unit_words(words_of(lanes, trips(c, lanes) * wpu + wpu), c.n_units, wpu, advance, order)
    return normals_of_words(w, c.X, to_normals)


# ---- the values (a one-row greeks_ref.Paths each) ---------------------------------------------------------------------------
def vanilla_value(o, z, X, anti=False):
    """The call's payoff per path on the market as precision X receives it; the payoff is continuous: no jump, no path left out."""
    o = mr.as_given(o, X)
    p = gr.vanilla(o, z)
    value, scale = p.value[:1], p.scale[:1]
    if anti:
        q = gr.vanilla(o, -np.asarray(z, dtype=np.float64))
        value, scale = 0.5 * (value + q.value[:1]), 0.5 * (scale + q.scale[:1])
    n = value.shape[1]
    return gr.Paths(value, scale, np.zeros((1, n)), np.full(n, np.inf))


def value(c, market, z, anti=False, control=False):
    if c.family == "vanilla":
        return vanilla_value(market, z, c.X, anti)
    if c.family == "basket":
        return br.value(br.as_seen(market, c.X), z, anti, control)
    return cr.price(market, z, c.X, anti)


def bound(c, p, tol):
    """greeks_ref.bound with the project's TOL[X]["pay"] (cva_ref.bound is the same expression)."""
    return gr.bound(p, tol[c.X]["pay"])[0]


# ---- wrong assignments ------------------------------------------------------------------------------------------------------------
def _pair_words(X):
    return 2 if X == "f32" else 3     # words per Box-Muller pair


def _lanes_from_context(c):
    return c.blocks * GROUP, None, None


def _partial_unit_skips_dead_paths(c):
    adv = np.full(c.n_units, words_per_unit(c), dtype=np.int64)
    live = NPB[c.X] - c.head
    adv[0] = -(-live // 2) * _pair_words(c.X)      # the pairs of its live paths only
    return c.lanes, adv, None


def _no_round_up_to_blocks(c):
    """fp64: the pairs the unit needs (basket: of its 4 ceil(n / 4) normals; CVA: of its dates), not whole blocks of four pairs."""
    need = 4 * (-(-c.size // 4)) if c.family == "basket" else c.size
    return c.lanes, np.full(c.n_units, -(-need // 2) * 3, dtype=np.int64), None


def _partial_trip_first(c):
    t = trips(c)
    return c.lanes, None, [t - 1] + list(range(t - 1))


Mutation = namedtuple("Mutation", "what applies reach change")
# reach(c): the units whose draws the mutation can move (the power condition counts the later-trip ones among them)
MUTATIONS = {
    "lanes_from_context_blocks": Mutation(
        "L taken from the context's blocks instead of from the launch",
        lambda c: c.blocks * GROUP != c.lanes and c.n_units > c.lanes,
        lambda c: np.arange(c.n_units) >= c.lanes, _lanes_from_context),
    "partial_vanilla_unit_skips_dead_paths": Mutation(
        "a partly live first vanilla unit consumes nothing for the pairs of its dead paths",
        lambda c: c.family == "vanilla" and c.head >= 2 and c.n_units > c.lanes,
        lambda c: np.arange(c.n_units) % c.lanes == 0, _partial_unit_skips_dead_paths),
    "fp64_basket_without_whole_blocks": Mutation(
        "an fp64 basket draws the pairs of its 4 ceil(n / 4) normals and not whole blocks of four pairs",
        lambda c: c.family == "basket" and c.X == "f64" and (4 * (-(-c.size // 4))) % 8 != 0 and c.n_units > c.lanes,
        lambda c: np.ones(c.n_units, dtype=bool), _no_round_up_to_blocks),
    "fp64_cva_without_round_up_after_last_pair": Mutation(
        "the fp64 CVA does not skip to the end of the block after its last pair",
        lambda c: c.family == "cva" and c.X == "f64" and (-(-c.size // 2)) % 4 != 0 and c.n_units > c.lanes,
        lambda c: np.ones(c.n_units, dtype=bool), _no_round_up_to_blocks),
    "partial_last_trip_drawn_first": Mutation(
        "the lanes of the partial last trip draw that unit before their others",
        lambda c: c.n_units > c.lanes and c.n_units % c.lanes != 0,
        lambda c: np.arange(c.n_units) % c.lanes < c.n_units % c.lanes, _partial_trip_first),
}


def applies(name, c):
    return bool(MUTATIONS[name].applies(c))


def reach(name, c):
    return MUTATIONS[name].reach(c) & later_trips(c)


# ---- the shapes of both test modules ----------------------------------------------------------------------------------------
# (blocks of the engine; 0 = the default engine) -> units of the call
UNITS = {1: GROUP * 3 + 77, 2: 2 * GROUP * 2 + 77, 0: 2121}     # three trips, a partial wave and a partial workgroup; two; one
SEEDS = [0x4D435F4D49333535, 20261020]
BASES = [0, 1000, (1 << 40) + 5]
BASKET_SIZES = [1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 33, 64]      # every padding and block boundary of both precisions
CVA_DATES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65]
ENDINGS = ("full", "cut", "intrinsic")
VANILLA_HEADS = {"f32": [1, 2, 3], "f64": [1, 2, 5, 6]}                # paths of the first unit below `first`: odd, and whole pairs
N_VANILLA_MARKETS = 6

# markets whose first seed missed the power condition of test_xorwow_ref.py: the seed moves on by 100 000 per step, the condition stays
RESEEDED = {}


def _rng(tag, i):
    return np.random.default_rng(31000 + 1000 * ["vanilla", "basket", "cva"].index(tag) + i + 100_000 * RESEEDED.get((tag, i), 0))


def rotation(i):
    """(seed, base) of case i: both seeds and the three bases, rotated over the cases."""
    return SEEDS[i % 2], BASES[i % 3]


def vanilla_market(i):
    return gr.random_vanilla(_rng("vanilla", i))


def vanilla_in_the_money(o):
    return dict(o, k=0.2 * o["s"])


def basket_market(mc, n_assets):
    """Every weight positive: the control variate runs on it."""
    return br.random_market(_rng("basket", n_assets), n_assets, lambda c: mc.chol(c, "f64"), positive_weights=True)


_T_CANDIDATES = [1.0, 0.7321, 2.0, 0.9, 1.3, 0.37, 2.71, 1.7, 0.61, 2.3]


def cva_schedules(X):
    """{d: (t, n_grid, ending)}: for every date count of CVA_DATES a grid whose schedule prices exactly d dates in precision X; the
    endings rotate over the counts (a count without the wanted ending -- a power of two always ends intrinsic -- takes the next)."""
    out = {}
    for i, d in enumerate(CVA_DATES):
        found = None
        for e in range(3):
            want = ENDINGS[(i + e) % 3]
            if want == "intrinsic":
                cands = [(d / 8.0, d)]                      # dt = 1/8 exactly: tau reaches an exact 0 at date d
            else:
                cands = [(t, d + (want == "cut")) for t in _T_CANDIDATES]
            for t, g in cands:
                s = cr.schedule(dict(t=t, n_grid=g, defint=0.0), X)
                if s.n_dates == d and s.ending == want:
                    found = (t, g, want)
                    break
            if found:
                break
        assert found, (X, d)
        out[d] = found
    return out


def cva_market(X, d):
    t, g, _ = cva_schedules(X)[d]
    return dict(gr.random_cva(_rng("cva", d)), t=t, n_grid=g)


def cva_in_the_money(c):
    return dict(c, k=0.3 * c["s"])


def ratio(err, bnd):
    """err / bound per path; 0 where both are exactly 0."""
    return np.where(err > 0, err / np.where(bnd > 0, bnd, math.ldexp(1.0, -1074)), 0.0)
