"""The launch-geometry (compatibility) mode's sample definition in numpy (not a test module).

Written from the paragraph "compatibility mode" of include/mc_mi355x.h and from nothing else: thread (b, t) of a G x T launch
owns the normal stream of rocRAND's XORWOW (seed b + G, subsequence t, offset 0) -- two words a Box-Muller pair, the sine member
first, the cosine member kept for the next draw; thread t of a block prices the block's paths t, t + T, ... < paths_per_block one
after the other, so path p = b * paths_per_block + i is priced by thread i mod T as that thread's (i div T)-th path; a path takes
`draws` CONSECUTIVE normals of its thread's stream (the kept member of an odd path's last pair is the next path's first normal):
  vanilla  1;    basket  n, one per asset;
  CVA      one per date whose `t -= dt` is still >= 0 in the precision's own arithmetic (`cva_draws`); the later dates read 0.
Both precisions take the float normal, widened.  The sample does not depend on how a kernel cuts a thread's stream into pieces, so
the model knows nothing about pieces: `arrange(streams[G, T, count], c)` picks every path's normals out of the per-thread streams
(Engine.grid_normals on the GPU, pyoracle.grid_normals on the CPU).

It prices nothing itself: `value` is greeks_ref.vanilla (through xorwow_ref.vanilla_value), basket_ref.value on
basket_ref.as_seen(market, X) and cva_ref.price (which carries the Hastings step as a jump); `bound` is
greeks_ref.bound(p, TOL[X]["pay"]) as everywhere else.  No path is left out.

MUTATIONS are wrong samples a kernel could plausibly implement, each a change of the Plan (which seed a block has, which thread
prices a path, where in that thread's stream the path starts, which member of a pair comes first) with the set of paths it can
reach; the two about pieces take the piece count `sub` and the 8-aligned piece length `seg` as parameters.  test_grid_ref.py
shows that the unmutated arrangement is pyoracle.grid_path_normals bit for bit and that every mutation moves at least 90 % of the
paths it reaches beyond the fp32 bound on the markets and geometries below; test_gpu_grid_ref.py holds the kernels to the model.
"""
from collections import namedtuple

import numpy as np

import basket_ref as br
import cva_ref as cr
import greeks_ref as gr
import xorwow_ref as xr
from test_gpu_parity import TOL

PRECISIONS = ["f32", "f64"]
NP = {"f32": np.float32, "f64": np.float64}

# family: "vanilla" | "basket" | "cva"; draws: normals a path takes; size: assets (basket), dates of the grid (CVA), 0 (vanilla)
Call = namedtuple("Call", "family G T per_block draws size")
# seeds (G,): the seed of every block's streams; thread, start (per_block,): the thread that prices local path i and the position
# in that thread's stream of the path's first normal; cosine_first: the two members of every pair exchanged
Plan = namedtuple("Plan", "seeds thread start cosine_first")


# ---- the rules of the header ----------------------------------------------------------------------------------------------------
def cva_draws(c, X):
    """Dates of a CVA path that draw: those whose `t -= dt` is still >= 0, t and dt = t / n_grid in the precision's arithmetic."""
    R = NP[X]
    t = R(c["t"])
    dt = R(t / R(c["n_grid"]))
    draws = 0
    for _ in range(int(c["n_grid"])):
        t = R(t - dt)
        if not t >= 0:
            break
        draws += 1
    return draws


def call(family, geom, market, X):
    G, T, per_block = geom
    if family == "vanilla":
        return Call(family, G, T, per_block, 1, 0)
    if family == "basket":
        return Call(family, G, T, per_block, len(market["s"]), len(market["s"]))
    return Call(family, G, T, per_block, cva_draws(market, X), int(market["n_grid"]))


def thread_paths(c):
    """(T,): how many paths of a block every thread prices -- the paths t, t + T, ... < per_block."""
    t = np.arange(c.T)
    return np.where(t < c.per_block, (c.per_block - t + c.T - 1) // c.T, 0)


def plan(c, mutation=None, sub=1, seg=0):
    i = np.arange(c.per_block)
    p = Plan(np.arange(c.G) + c.G, i % c.T, (i // c.T) * c.draws, False)
    if mutation is None:
        return p
    assert applies(mutation, c, sub, seg), (mutation, c, sub, seg)
    return MUTATIONS[mutation].change(c, p, sub, seg)


def count_needed(c, p=None):
    """Normals of a stream the plan reads, rounded up to whole pairs."""
    p = p or plan(c)
    return (int(p.start.max()) + c.draws + 1) // 2 * 2


def arrange(streams, c, p=None):
    """(G * per_block, draws): every path's normals, path b * per_block + i in row order; streams[g] = the (T, count) streams of seed
    p.seeds[g]."""
    p = p or plan(c)
    streams = np.asarray(streams)
    assert streams.shape[:2] == (c.G, c.T) and streams.shape[2] >= count_needed(c, p), (streams.shape, c, count_needed(c, p))
    idx = p.start[:, None] + np.arange(c.draws)[None, :]
    if p.cosine_first:
        idx = idx ^ 1
    return streams[:, p.thread[:, None], idx].reshape(c.G * c.per_block, c.draws)


def normals_of(z, c):
    """What the values take: the vanilla path's one normal as a vector, the others' (n, draws)."""
    return z[:, 0] if c.family == "vanilla" else z


def box_muller(words):
    """rocrand_normal's Box-Muller (rocrand_normal.h) on (..., 2 m) XORWOW words, float64 (..., 2 m): words (x, y) make
    u = 2^-32 + x 2^-32 and v = c + y c, c = fl32(2 pi 2^-32), both IN FLOAT as the header forms them (x and y converted to float,
    the multiply-add rounded once: a contracted build; an uncontracted one differs by an ulp of v on some pairs, 5e-7 |s| at most),
    then s = sqrt(-2 ln u), sin(v) s first, cos(v) s second, in float64."""
    w = np.asarray(words, dtype=np.uint32)
    assert w.shape[-1] % 2 == 0
    x, y = w[..., 0::2].astype(np.float32).astype(np.float64), w[..., 1::2].astype(np.float32).astype(np.float64)
    c1, c2 = float(np.float32(2.3283064e-10)), float(np.float32(1.46291807e-09))
    u = (c1 + x * c1).astype(np.float32).astype(np.float64)
    v = (c2 + y * c2).astype(np.float32).astype(np.float64)
    s = np.sqrt(-2.0 * np.log(u))
    out = np.empty(w.shape, dtype=np.float64)
    out[..., 0::2], out[..., 1::2] = np.sin(v) * s, np.cos(v) * s
    return out


# ---- the values (a one-row greeks_ref.Paths each) ------------------------------------------------------------------------------
def value(c, market, z, X):
    z = normals_of(np.asarray(z, dtype=np.float64), c)
    if c.family == "vanilla":
        return xr.vanilla_value(market, z, X)
    if c.family == "basket":
        return br.value(br.as_seen(market, X), z)
    return cr.price(market, z, X)


def bound(p, X):
    return gr.bound(p, TOL[X]["pay"])[0]


# ---- wrong samples ------------------------------------------------------------------------------------------------------------------
def compiled_size(n):
    """The fused basket kernels exist for 4, 8 and 16 assets; a smaller basket runs the next size zero-padded."""
    return next(na for na in (4, 8, 16) if n <= na)


def _k(c):
    return np.arange(c.per_block) // c.T      # which of its thread's paths a local path is


def _per_block_chunk(c):
    return -(-c.per_block // c.T)


def _contiguous(c, p, sub, seg):
    i, chunk = np.arange(c.per_block), _per_block_chunk(c)
    return p._replace(thread=i // chunk, start=(i % chunk) * c.draws)


def _kept_dropped(c, p, sub, seg):
    return p._replace(start=_k(c) * (c.draws + 1))


def _cosine_first(c, p, sub, seg):
    return p._replace(cosine_first=True)


def _seed_is_block(c, p, sub, seg):
    return p._replace(seeds=np.arange(c.G))


def _advance_by_size(c, p, sub, seg):
    """A path uses its first `draws` normals but moves its stream on by the grid's dates (CVA)."""
    return p._replace(start=_k(c) * c.size)


def _advance_by_compiled_size(c, p, sub, seg):
    return p._replace(start=_k(c) * compiled_size(c.size))


def _piece_of_unaligned_start(c, sub):
    """(piece, paths per piece) of every local path when piece s starts at path s ceil(n_t / sub) of its thread."""
    per = np.maximum(-(-thread_paths(c) // sub), 1)[np.arange(c.per_block) % c.T]
    return _k(c) // per, per


def _piece_unaligned(c, p, sub, seg):
    """The start states stand at s seg draws words; piece s begins pricing at path s ceil(n_t / sub) instead of s seg."""
    s, per = _piece_of_unaligned_start(c, sub)
    return p._replace(start=(s * seg + (_k(c) - s * per)) * c.draws)


def _piece_state_by_paths(c, p, sub, seg):
    s = _k(c) // seg
    return p._replace(start=s * seg + (_k(c) - s * seg) * c.draws)


def _n_max(c):
    return -(-c.per_block // c.T)


Mutation = namedtuple("Mutation", "what applies reach change")
# applies(c, sub, seg); reach(c, sub, seg) -> (per_block,) bool: the local paths (of every block) whose normals it can change
MUTATIONS = {
    "block_contiguous_map": Mutation(
        "thread t prices the contiguous paths t ceil(N / T) ... of its block instead of t, t + T, ...",
        lambda c, sub, seg: c.T > 1 and c.per_block > c.T,
        lambda c, sub, seg: (np.arange(c.per_block) // _per_block_chunk(c) != np.arange(c.per_block) % c.T)
        | (np.arange(c.per_block) % _per_block_chunk(c) != _k(c)), _contiguous),
    "kept_member_dropped_between_paths": Mutation(
        "every path starts on a fresh Box-Muller pair: the kept member of an odd path's last pair is dropped",
        lambda c, sub, seg: c.draws % 2 == 1 and _n_max(c) > 1,
        lambda c, sub, seg: _k(c) >= 1, _kept_dropped),
    "cosine_member_first": Mutation(
        "the cosine member of a pair is returned first, the sine member kept",
        lambda c, sub, seg: True,
        lambda c, sub, seg: np.ones(c.per_block, dtype=bool), _cosine_first),
    "block_seeded_without_grid_size": Mutation(
        "block b seeded with b instead of b + G",
        lambda c, sub, seg: True,
        lambda c, sub, seg: np.ones(c.per_block, dtype=bool), _seed_is_block),
    "cva_draws_for_every_grid_date": Mutation(
        "a CVA path of a cut schedule draws for every date of the grid",
        lambda c, sub, seg: c.family == "cva" and c.draws < c.size and _n_max(c) > 1,
        lambda c, sub, seg: _k(c) >= 1, _advance_by_size),
    "padded_basket_draws_compiled_size": Mutation(
        "a basket run zero-padded inside a compiled size draws that size's normals instead of n",
        lambda c, sub, seg: c.family == "basket" and c.size <= 16 and compiled_size(c.size) != c.size and _n_max(c) > 1,
        lambda c, sub, seg: _k(c) >= 1, _advance_by_compiled_size),
    "piece_starts_unaligned": Mutation(
        "piece s starts at path s ceil(n_t / sub) of its thread instead of at the 8-aligned s seg",
        lambda c, sub, seg: sub > 1 and bool(np.any(MUTATIONS["piece_starts_unaligned"].reach(c, sub, seg))),
        lambda c, sub, seg: (_piece_of_unaligned_start(c, sub)[0] >= 1) & (_piece_of_unaligned_start(c, sub)[1] != seg), _piece_unaligned),
    "piece_state_advanced_by_paths": Mutation(
        "a piece's start state advanced by seg words instead of seg draws",
        lambda c, sub, seg: sub > 1 and c.draws > 1 and _n_max(c) > seg,
        lambda c, sub, seg: _k(c) >= seg, _piece_state_by_paths),
}


def applies(name, c, sub=1, seg=0):
    return bool(MUTATIONS[name].applies(c, sub, seg))


def reach(name, c, sub=1, seg=0):
    """(G * per_block,) bool, in path order."""
    return np.tile(MUTATIONS[name].reach(c, sub, seg), c.G)


# ---- the shapes of both test modules ------------------------------------------------------------------------------------------
# (G, T, paths_per_block) -> the pieces the fused kernels cut every thread's stream into: READ from the launch on the GPU
# (Engine.last_launch()[0] // G) and asserted there; test_grid_ref.py holds the list to the conditions it was chosen for with the
# piece rule restated.  T = 1, odd T below 64, 64, 100 (a partial wave), 512 and 1024; G > 1; paths_per_block no multiple of T in
# six, and below T in the last (63 threads of each block price nothing); every piece count 1 ... 32; empty pieces in the first five.
GEOMS = {(1, 1, 545): 32, (3, 5, 2653): 32, (2, 3, 900): 16, (2, 7, 1001): 8, (2, 100, 6437): 4, (1, 64, 2117): 2,
         (1, 512, 1100): 1, (1, 1024, 2148): 1, (2, 100, 37): 1}
SMALL_GEOM = (2, 3, 900)               # the long cut CVA schedule runs on this one only: 16 pieces, 257 draws a path

N_VANILLA_MARKETS = xr.N_VANILLA_MARKETS
BASKET_FUSED = [1, 2, 3, 4, 5, 7, 8, 9, 13, 16]
BASKET_STAGED_ONLY = [17, 33]
CVA_DATES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 65]      # of xorwow_ref.CVA_DATES: every ending in both precisions, 1 date, odd and even
CVA_LONG = cr.CUT_LONG[0]


def vanilla_markets(i):
    o = xr.vanilla_market(i)
    return [("drawn", o), ("itm", xr.vanilla_in_the_money(o))]


def basket_markets(mc, n_assets):
    b = xr.basket_market(mc, n_assets)
    return [("drawn", b), ("itm", br.in_the_money(b))]


def cva_markets(X, d):
    """d: a date count of CVA_DATES (xorwow_ref.cva_market) or "long" (cva_ref.CUT_LONG)."""
    c = cr.market(CVA_LONG) if d == "long" else xr.cva_market(X, d)
    return [("drawn", c), ("itm", xr.cva_in_the_money(c))]


def cva_geoms(d):
    return [SMALL_GEOM] if d == "long" else list(GEOMS)


def ratio(err, bnd):
    return xr.ratio(err, bnd)
