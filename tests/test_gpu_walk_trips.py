"""The dated products whose lanes take SEVERAL grid-stride trips: asian_kernel, barrier_kernel, lookback_kernel, heston_kernel,
heston_path_kernel and merton_kernel, every compiled instantiation (both precisions, plain and antithetic, and the family's
compile-time switch: 48 kernels), per path.

Why: a dated product launches min(ceil(n / 256), blocks * 3 / 2) workgroups per segment, 3072 on the default engine, so below
786 432 paths every lane prices one path and the back-edge of `for (i = ...; i < w.n_units; i += stride)` is never taken.  The
per-path tests of the six families' own modules run 329 to 5500 paths there: what a lane carries from one path into the next (the
running sums, extrema, the bridge product and its lagged distance, the variance, the jump state, the fp64 pair cursor, the
coefficient registers behind the empty-asm ties), the hand-placed wait states next to other neighbours, the idle lanes of a
partial last trip and out[i] for i beyond the stride are seen by nothing but 1e7-path prices at three half-widths.  Here small
engines (greeks_ref.TRIP_RANGES: 16 blocks = 6144 lanes, 1 block = 256 lanes) price 2381 to 20 557 paths, three to ten trips per
lane, across the 2^32-unit seam too; every test first holds its own call to `grid * group * 2 <= n` of its last launch
(Engine.last_launch), so that a changed grid rule fails it instead of turning it back into a one-trip test.

Three assertions:
 a. test_*_same_bits_on_every_grid: the small engine's values are the default engine's (one trip), bit for bit: every date or step
    count of the family's list on range A, three counts on B and C.  This compares the kernel with itself: it counts only together
    with (b) and with the one-trip reference tests of the families' own modules, which hold the default engine's values to the model.
 b. test_*_every_path_and_the_sums_of_many_trips: every path of the many-trip call against the family's float64 model, by the
    family's own rule and tolerance (imported, not copied: TOL[X]["pay"] per unit of the model's scale; a path near a barrier must
    match one of the values it can take; kink and near paths under the families' caps, which tests/test_*_ref.py hold as
    conditions on these shapes).  No path is left out.  The model's normals, uniforms and words are drawn with the DEFAULT engine,
    in chunks: one-trip launches, off the path under test.
 c. in the same tests: {sum, sum2, n} of the run form on the same small engine against that call's own dump
    (greeks_ref.check_sums).  These six products hand walk_enqueue the unit 1, so the closing scale * s is exact and the bound is
    the additions' alone.

The wave-uniform choices (barrier and lookback kinds) are spread over the cases, each at least once per family, not multiplied.

Wall time on the MI355X: the module's 240 tests take 3.6 s together; a same-bits case 0.01 s, a per-path case 0.01 to 0.03 s on
range C and 0.07 to 0.21 s on range A (the slowest: lookback), where the numpy models and the exact sums dominate.  Worst err/bound
on the later trips, as printed (fp32, fp64): Asian 0.016, 0.0091; barrier 0.020, 0.014; lookback 0.0092, 0.0065; Merton 0.011,
0.0061; Heston 0.013, 0.0078; Heston path 0.010, 0.0081.
"""
import contextlib
import itertools
from types import SimpleNamespace as V

import numpy as np
import pytest

import asian_ref as ar
import barrier_ref as br
import greeks_ref as gr
import heston_path_ref as hp
import heston_ref as hr
import lookback_ref as lr
import merton_ref as mr
from greeks_ref import TRIP_RANGES, check_sums
from test_gpu_asian import dates_list
from test_gpu_barrier import check_paths as barrier_check_paths
from test_gpu_heston import check as heston_check
from test_gpu_heston_path import barrier_kinds, finite
from test_gpu_lookback import check_paths as lookback_check_paths
from test_gpu_merton import draws as merton_draws, paths as merton_paths, run as merton_run
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

CHUNK = 8192   # paths per draw of the model's inputs on the default engine
PRECISIONS = ["f32", "f64"]
MODEL_RANGES = ["A", "C"]


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def engines(mc):
    """{blocks: engine}: 0 is the default engine (one trip on these ranges), 16 and 1 are the small ones of greeks_ref.TRIP_RANGES."""
    engs = {b: mc.Engine(0, blocks=b) for b in (0, 16, 1)}
    assert {r.blocks for r in TRIP_RANGES.values()} == {16, 1} and engs[16].blocks == 16 and engs[1].blocks == 1
    assert max(r.n for r in TRIP_RANGES.values()) <= gr.trip_lanes(engs[0].blocks)   # one trip on the default engine
    yield engs
    for e in engs.values():
        e.close()


@contextlib.contextmanager
def estimator(engs, anti, control=False):
    for e in engs:
        e.set_antithetic(anti), e.set_control_variate(control)
    try:
        yield
    finally:
        for e in engs:
            e.set_antithetic(False), e.set_control_variate(False)


def guard(e, name):
    """After a call on range `name`: greeks_ref.trip_guard on its last launch.  Returns the number of full trips."""
    r = TRIP_RANGES[name]
    return gr.trip_guard(e, r.blocks, gr.trip_last_segment(r))


def normals_of(e, X):
    return lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X)


def chunked(draw, first, n):
    """draw(first, count) -> an array, or a tuple of arrays, of one row per path: the rows of first ... first + n - 1, CHUNK paths a call."""
    parts = [draw(first + i, min(CHUNK, n - i)) for i in range(0, n, CHUNK)]
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate(c) for c in zip(*parts))
    return np.concatenate(parts)


def same_bits(engines, names, variants):
    """(a): on every range of `names`, every variant's values on the range's small engine are the default engine's, bit for bit."""
    variants = list(variants)
    assert variants
    for name in names:
        r = TRIP_RANGES[name]
        eng, small = engines[0], engines[r.blocks]
        for v in variants:
            with estimator((eng, small), v.anti, getattr(v, "control", False)):
                got = v.paths(small, r.first, r.n)
                trips = guard(small, name)
                want = v.paths(eng, r.first, r.n)
            assert got.shape == (r.n,) and np.array_equal(got, want), (name, v.tag, trips, np.flatnonzero(got != want)[:8])
        print(f"walk trips same bits range {name}: {trips} full trips a lane, {len(variants)} calls, first {variants[0].tag}")


def many_trips(small, name, v):
    """The per-path dump and the run form's estimate of one variant on the small engine of range `name`, each held to its guard."""
    r = TRIP_RANGES[name]
    with estimator((small,), v.anti, getattr(v, "control", False)):
        got = v.paths(small, r.first, r.n)
        trips = guard(small, name)
        est = v.run(small, r.first, r.n)
        assert guard(small, name) == trips
    assert got.shape == (r.n,)
    return got, est, trips


def report(family, X, name, trips, worst, extra=""):
    print(f"walk trips {family} {X} range {name}: {trips} full trips a lane, worst err/bound {worst:.3g}{extra}")


# ---- Asian: control variate off or on ---------------------------------------------------------------------------------------
def asian_variants(X, m, o):
    for anti, control in itertools.product((False, True), repeat=2):
        yield V(tag=(X, m, anti, control), anti=anti, control=control, paths=lambda e, f, n: e.asian_paths(o, m, n, SEED, f, X),
                run=lambda e, f, n: e.asian(o, m, n, SEED, f, X))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("mi", range(16))
def test_asian_same_bits_on_every_grid(mc, engines, X, mi):
    m = dates_list(mc)[mi]
    assert set(ar.TRIP_BITS_DATES) < set(dates_list(mc))
    same_bits(engines, ["A"] + (["B", "C"] if m in ar.TRIP_BITS_DATES else []), asian_variants(X, m, ar.CASES[mi % len(ar.CASES)]))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_asian_every_path_and_the_sums_of_many_trips(engines, X, name):
    r, tol, worst = TRIP_RANGES[name], TOL[X]["pay"], 0.0
    eng, small = engines[0], engines[r.blocks]
    for i, m in enumerate(ar.TRIP_DATES):
        o = gr.trip_pick(ar.CASES, i, name)
        z = chunked(lambda f, c: ar.asian_normals(normals_of(eng, X), f, c, m, gr.NPB[X]), r.first, r.n)
        for v in asian_variants(X, m, o):
            got, est, trips = many_trips(small, name, v)
            p = ar.asian(o, m, z, v.control, v.anti)
            b, err = gr.bound(p, tol)[0], np.abs(got.astype(np.float64) - p.value[0])
            assert np.all(np.isfinite(got)) and np.all(err <= b), (v.tag, o, int(np.argmax(err / b)), float((err / b).max()))
            worst = max(worst, float((err / b).max()))
            check_sums(est, got, r.n, v.tag)
    report("asian", X, name, trips, worst)


# ---- barrier: discrete or continuous ----------------------------------------------------------------------------------------
def barrier_variants(X, m, o, B):
    """Both monitorings x plain and antithetic; the market's two types (knock-out, knock-in) alternate over them."""
    for (mi, monitoring), (ai, anti) in itertools.product(enumerate(br.MONITORINGS), enumerate((False, True))):
        kind = br.kinds_of(o, B)[(mi + ai) % 2]
        yield V(tag=(X, m, B, kind, monitoring, anti), anti=anti, kind=kind, monitoring=monitoring,
                paths=lambda e, f, n, kind=kind, monitoring=monitoring: e.barrier_paths(o, B, m, n, SEED, f, X, kind, monitoring),
                run=lambda e, f, n, kind=kind, monitoring=monitoring: e.barrier(o, B, m, n, SEED, f, X, kind, monitoring))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("mi", range(len(br.DATES)))
def test_barrier_same_bits_on_every_grid(engines, X, mi):
    m = br.DATES[mi]
    assert set(br.TRIP_BITS_DATES) < set(br.DATES)
    same_bits(engines, ["A"] + (["B", "C"] if m in br.TRIP_BITS_DATES else []), barrier_variants(X, m, *br.CASES[mi % len(br.CASES)]))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_barrier_every_path_and_the_sums_of_many_trips(engines, X, name):
    r, tol, worst, nears, kinds = TRIP_RANGES[name], TOL[X]["pay"], 0.0, 0, set()
    eng, small = engines[0], engines[r.blocks]
    for i, m in enumerate(br.TRIP_DATES):
        o, B = gr.trip_pick(br.CASES, i, name)
        z = chunked(lambda f, c: br.barrier_normals(normals_of(eng, X), f, c, m, gr.NPB[X]), r.first, r.n)
        for v in barrier_variants(X, m, o, B):
            got, est, trips = many_trips(small, name, v)
            sides = br.walk(o, B, m, z, B > o["s"], v.monitoring, v.anti)
            w, near = barrier_check_paths(got.astype(np.float64), sides, v.kind.endswith("in"), v.monitoring, tol)
            worst, nears = max(worst, w), nears + near
            kinds.add(v.kind)
            check_sums(est, got, r.n, v.tag)
    assert kinds == set(br.KINDS)
    report("barrier", X, name, trips, worst, f", {nears} near paths")


# ---- lookback: discrete or continuous ---------------------------------------------------------------------------------------
LOOKBACK_PAIRS = (("floating-put", "fixed-put"), ("fixed-call", "floating-call"))   # each: one type on the maximum, one on the minimum


def lookback_variants(X, m, o, i):
    """Both monitorings x plain and antithetic; the four types alternate over them and over the counts, two at a time."""
    for (mi, monitoring), (ai, anti) in itertools.product(enumerate(lr.MONITORINGS), enumerate((False, True))):
        for kind in LOOKBACK_PAIRS[(mi + ai + i) % 2]:
            yield V(tag=(X, m, kind, monitoring, anti), anti=anti, kind=kind, monitoring=monitoring,
                    paths=lambda e, f, n, kind=kind, monitoring=monitoring: e.lookback_paths(o, m, n, SEED, f, X, kind, monitoring),
                    run=lambda e, f, n, kind=kind, monitoring=monitoring: e.lookback(o, m, n, SEED, f, X, kind, monitoring))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("mi", range(len(lr.DATES)))
def test_lookback_same_bits_on_every_grid(engines, X, mi):
    m = lr.DATES[mi]
    assert set(lr.TRIP_BITS_DATES) < set(lr.DATES)
    same_bits(engines, ["A"] + (["B", "C"] if m in lr.TRIP_BITS_DATES else []), lookback_variants(X, m, lr.CASES[mi % len(lr.CASES)], mi))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_lookback_every_path_and_the_sums_of_many_trips(engines, X, name):
    r, tol, worst, kinds = TRIP_RANGES[name], TOL[X]["pay"], 0.0, set()
    assert tol == lr.EPS[X]
    eng, small = engines[0], engines[r.blocks]
    words_of = lambda domain, u0, c, b0, nb: eng.words(SEED, domain, u0, c, b0, nb)
    for i, m in enumerate(lr.TRIP_DATES):
        o = gr.trip_pick(lr.CASES, i, name)
        z, u = chunked(lambda f, c: lr.lookback_draws(normals_of(eng, X), words_of, f, c, m, X), r.first, r.n)
        walks = {}
        for v in lookback_variants(X, m, o, i):
            got, est, trips = many_trips(small, name, v)
            key = (lr.ON_MAX[v.kind], v.monitoring, v.anti)
            if key not in walks:
                walks[key] = lr.walk(o, m, z, u, lr.ON_MAX[v.kind], v.monitoring, v.anti, tol)
            worst = max(worst, lookback_check_paths(got.astype(np.float64), lr.value(walks[key], v.kind, o["k"]), tol))
            kinds.add(v.kind)
            check_sums(est, got, r.n, v.tag)
    assert kinds == set(lr.KINDS)
    report("lookback", X, name, trips, worst)


# ---- Merton: european, asian or barrier -------------------------------------------------------------------------------------
def merton_variants(X, m, o, B, jp):
    """The three payoffs x plain and antithetic; the market's knock-out type runs plain, its knock-in type antithetic."""
    for ai, anti in enumerate((False, True)):
        for payoff, kind in (("european", None), ("asian", None), ("barrier", mr.kinds_of(o, B)[ai])):
            yield V(tag=(X, m, B, payoff, kind, anti), anti=anti, payoff=payoff, kind=kind,
                    paths=lambda e, f, n, payoff=payoff, kind=kind: merton_paths(e, o, jp, B, m, n, f, X, payoff, kind),
                    run=lambda e, f, n, payoff=payoff, kind=kind: merton_run(e, o, jp, B, m, n, f, X, payoff, kind))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("mi", range(len(mr.DATES)))
def test_merton_same_bits_on_every_grid(engines, X, mi):
    m = mr.DATES[mi]
    assert set(mr.TRIP_BITS_DATES) < set(mr.DATES)
    cases = [mr.CASES[mi % len(mr.CASES)]] + ([mr.HEAVY] if m in mr.HEAVY_DATES else [])
    for case in cases:
        same_bits(engines, ["A"] + (["B", "C"] if m in mr.TRIP_BITS_DATES else []), merton_variants(X, m, *case))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_merton_every_path_and_the_sums_of_many_trips(mc, engines, X, name):
    r, tol, worst, nears, kinds = TRIP_RANGES[name], TOL[X]["pay"], 0.0, 0, set()
    eng, small = engines[0], engines[r.blocks]
    assert mr.TRIP_HEAVY_DATES in mr.HEAVY_DATES
    cases = [(m, gr.trip_pick(mr.CASES, i, name)) for i, m in enumerate(mr.TRIP_DATES)] + [(mr.TRIP_HEAVY_DATES, mr.HEAVY)]
    for m, (o, B, jp) in cases:
        z, N = chunked(lambda f, c: merton_draws(mc, eng, X, o, jp, f, c, m), r.first, r.n)
        walks = {anti: mr.walk(o, jp, m, z, N, B, B > o["s"], anti) for anti in (False, True)}
        for v in merton_variants(X, m, o, B, jp):
            got, est, trips = many_trips(small, name, v)
            c, sides = walks[v.anti]
            w, near = mr.check_paths(got, c, sides, v.payoff, bool(v.kind) and v.kind.endswith("in"), tol)
            worst, nears = max(worst, w), nears + near
            kinds.add(v.kind)
            check_sums(est, got, r.n, v.tag)
    assert kinds == set(mr.KINDS) | {None}
    report("merton", X, name, trips, worst, f", {nears} near paths")


# ---- Heston: no switch ------------------------------------------------------------------------------------------------------
def heston_variants(X, m, mkt, model):
    for anti in (False, True):
        yield V(tag=(X, m, anti), anti=anti, paths=lambda e, f, n: e.heston_paths(mkt, model, m, n, SEED, f, X),
                run=lambda e, f, n: e.heston(mkt, model, m, n, SEED, f, X))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("mi", range(len(hr.STEPS)))
def test_heston_same_bits_on_every_grid(engines, X, mi):
    m = hr.STEPS[mi]
    assert set(hr.TRIP_BITS_STEPS) < set(hr.STEPS)
    _, mkt, model = hr.CASES[mi % len(hr.CASES)]
    same_bits(engines, ["A"] + (["B", "C"] if m in hr.TRIP_BITS_STEPS else []), heston_variants(X, m, mkt, model))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_heston_every_path_and_the_sums_of_many_trips(engines, X, name):
    r, tol, worst, kinks = TRIP_RANGES[name], TOL[X]["pay"], 0.0, 0
    eng, small = engines[0], engines[r.blocks]
    for i, m in enumerate(hr.TRIP_STEPS):
        case, mkt, model = gr.trip_pick(hr.CASES, i, name)
        assert hr.runs(case, X, m)
        z1, z2 = chunked(lambda f, c: hr.heston_normals(normals_of(eng, X), f, c, m, hr.NPB[X]), r.first, r.n)
        both = hr.walk(mkt, model, m, z1, z2, anti=True)
        for v in heston_variants(X, m, mkt, model):
            got, est, trips = many_trips(small, name, v)
            w, k = heston_check(got, both if v.anti else hr.plain_of(both), tol, (case,) + v.tag)
            assert k <= hr.KINK_CAP * r.n, (case, v.tag, k)
            worst, kinks = max(worst, w), kinks + k
            check_sums(est, got, r.n, v.tag)
    report("heston", X, name, trips, worst, f", {kinks} kink paths")


# ---- Heston path: asian or barrier ------------------------------------------------------------------------------------------
def heston_path_variants(X, shape, mkt, model):
    """Both payoffs x plain and antithetic; the shape's barrier types (four at heston_path_ref.FOUR_KIND_SHAPES, two elsewhere) are
    split between plain (knock-out) and antithetic (knock-in)."""
    nd, spd = shape
    for ai, anti in enumerate((False, True)):
        yield V(tag=(X, shape, "asian", anti), anti=anti, payoff="asian",
                paths=lambda e, f, n: e.heston_asian_paths(mkt, model, nd, spd, n, SEED, f, X),
                run=lambda e, f, n: e.heston_asian(mkt, model, nd, spd, n, SEED, f, X))
        for B, kind in barrier_kinds(shape)[ai::2]:
            yield V(tag=(X, shape, kind, anti), anti=anti, payoff="barrier", B=B, kind=kind,
                    paths=lambda e, f, n, B=B, kind=kind: e.heston_barrier_paths(mkt, model, B, nd, spd, n, SEED, f, X, kind),
                    run=lambda e, f, n, B=B, kind=kind: e.heston_barrier(mkt, model, B, nd, spd, n, SEED, f, X, kind))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("si", range(len(hp.SHAPES)))
def test_heston_path_same_bits_on_every_grid(engines, X, si):
    shape = hp.SHAPES[si]
    assert set(hp.TRIP_BITS_SHAPES) < set(hp.SHAPES)
    _, mkt, model = hr.CASES[si % len(hr.CASES)]
    same_bits(engines, ["A"] + (["B", "C"] if shape in hp.TRIP_BITS_SHAPES else []), heston_path_variants(X, shape, mkt, model))


@pytest.mark.parametrize("X", PRECISIONS)
@pytest.mark.parametrize("name", MODEL_RANGES)
def test_heston_path_every_path_and_the_sums_of_many_trips(engines, X, name):
    r, tol, worst, nears, kinks, kinds = TRIP_RANGES[name], TOL[X]["pay"], 0.0, 0, 0, set()
    eng, small = engines[0], engines[r.blocks]
    assert set(hp.TRIP_SHAPES) < set(hp.SHAPES) and set(hp.TRIP_SHAPES) & set(hp.FOUR_KIND_SHAPES)
    for i, shape in enumerate(hp.TRIP_SHAPES):
        nd, spd = shape
        m = nd * spd
        case, mkt, model = gr.trip_pick(hr.CASES, i, name)
        assert hr.runs(case, X, m) and hp.barrier_runs(case, X, nd, spd)
        z1, z2 = chunked(lambda f, c: hp.heston_path_normals(normals_of(eng, X), f, c, m, hp.NPB[X]), r.first, r.n)
        both = hp.walk(mkt, model, nd, spd, z1, z2, anti=True)
        for v in heston_path_variants(X, shape, mkt, model):
            got, est, trips = many_trips(small, name, v)
            sides, what = both if v.anti else both[:1], (case,) + v.tag
            val = finite(got, what)
            if v.payoff == "asian":
                b, kink = hp.asian_bound(sides, tol)
                ratio, near = np.abs(val - hp.asian(sides)) / b, np.zeros(r.n, dtype=bool)
            else:
                ratio, near, kink = hp.barrier_errors(val, sides, v.B, v.kind, tol)
                kinds.add(v.kind)
            assert np.all(ratio <= 1.0), (what, int(np.argmax(ratio)), float(ratio.max()))
            assert near.sum() <= hp.NEAR_CAP * r.n and kink.sum() <= hr.KINK_CAP * r.n, (what, int(near.sum()), int(kink.sum()))
            worst, nears, kinks = max(worst, float(ratio.max())), nears + int(near.sum()), kinks + int(kink.sum())
            check_sums(est, got, r.n, v.tag)
    assert kinds == set(hp.KINDS)
    report("heston path", X, name, trips, worst, f", {nears} near and {kinks} kink paths")
