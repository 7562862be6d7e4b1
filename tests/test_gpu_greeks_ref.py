"""The six Greeks kernels (vanilla_greeks_kernel, basket_greeks_kernel, cva_greeks_kernel; pathwise and likelihood ratio)
against the independent float64 reference greeks_ref.py on the kernels' own normals (Engine.normals), on random asymmetric
markets, one path at a time, through many trips, workgroups and the 2^32-unit seam, and -- with no statistics involved --
against central differences of the pricing kernels on the same paths.

Tolerances are the per-path bounds of greeks_ref (TOL[X]["pay"] per unit of its scale, plus the step of an indicator on a
path within that bound of it); the bound on a sum is the sum of the per-path bounds."""

import numpy as np
import pytest

import greeks_ref as gr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

U32 = 1 << 32
BASKET_SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33, 63, 64]


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


def draw(eng, X):
    return lambda domain, u0, n, block: eng.normals(SEED, domain, u0, n, block, X)


def planes(kind, got):
    return list(got) if kind != "basket" else [got[0]] + list(got[1]) + list(got[2])


def run(e, kind, market, n, first, X, lr):
    if kind == "vanilla":
        return planes(kind, (e.vanilla_greeks_lr if lr else e.vanilla_greeks)(market, n, SEED, first, X))
    f = e.basket_greeks if kind == "basket" else e.cva_greeks
    return planes(kind, f(market, n, SEED, first, X, lr=lr))


def reference(e, kind, market, n, first, X, lr, chunk=50_000):
    """greeks_ref on the kernels' normals for paths first .. first + n - 1, in chunks of paths (bounded host memory)."""
    npb = gr.NPB[X]
    parts = []
    for f in range(first, first + n, chunk):
        m = min(chunk, first + n - f)
        if kind == "vanilla":
            parts.append(gr.vanilla(market, gr.vanilla_normals(draw(e, X), f, m, npb), lr))
        elif kind == "basket":
            parts.append(gr.basket(market, gr.basket_normals(draw(e, X), f, m, len(market["s"]), npb), lr))
        else:
            parts.append(gr.cva(market, gr.cva_normals(draw(e, X), f, m, gr.cva_dates(market, X)[1].size, npb), X, lr))
    return gr.Paths(*(np.concatenate([getattr(p, k) for p in parts], axis=-1) for k in gr.Paths._fields))


def check(got, p, X, what=""):
    """Every plane's (n, sum, sum2) against the reference's per-path values, within the sums of the per-path bounds."""
    b = gr.bound(p, TOL[X]["pay"])
    assert len(got) == len(p.value)
    for q, g in enumerate(got):
        v = p.value[q]
        assert g.n == v.size
        tol, tol2 = b[q].sum(), (2 * np.abs(v) * b[q] + b[q] * b[q]).sum()
        assert abs(g.sum - v.sum()) <= tol, (what, q, g.sum, v.sum(), tol)
        assert abs(g.sum2 - (v * v).sum()) <= tol2, (what, q, g.sum2, (v * v).sum(), tol2)


# ---- a. random asymmetric markets ----------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_vanilla_random_markets(eng, X, lr):
    rng = np.random.default_rng(31 + lr)
    n = 20011
    for i in range(8):
        o = gr.random_vanilla(rng)
        first = int(rng.integers(0, 1 << 36))
        check(run(eng, "vanilla", o, n, first, X, lr), reference(eng, "vanilla", o, n, first, X, lr), X, o)
    # a strike at or below 0: every path is in the money, the pathwise delta of a path is S_T / S exactly
    for k in (0.0, -25.0):
        o = dict(s=73.0, k=k, r=0.03, v=0.4, t=1.3)
        got, p = run(eng, "vanilla", o, n, 5, X, lr), reference(eng, "vanilla", o, n, 5, X, lr)
        check(got, p, X, o)
        assert np.all(p.value[0] > 0)
    # deep out of the money: no path pays, all three sums are exactly 0
    o = dict(s=50.0, k=5000.0, r=0.01, v=0.1, t=0.5)
    assert all(g.sum == 0 and g.sum2 == 0 for g in run(eng, "vanilla", o, n, 9, X, lr))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
@pytest.mark.parametrize("n_assets", BASKET_SIZES)
def test_basket_random_markets(mc, eng, X, lr, n_assets):
    rng = np.random.default_rng(1000 + n_assets)
    b = gr.random_basket(rng, n_assets, lambda c: mc.chol(c, X))
    n, first = 6007, int(rng.integers(0, 1 << 34))
    check(run(eng, "basket", b, n, first, X, lr), reference(eng, "basket", b, n, first, X, lr), X, (n_assets, b["k"]))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_cva_random_markets(eng, X, lr):
    rng = np.random.default_rng(41 + lr)
    cases = [gr.random_cva(rng) for _ in range(5)]
    cases += [dict(gr.random_cva(rng, n_grid=64), t=1.0), dict(gr.random_cva(rng, n_grid=300), t=3.0),   # last date at maturity: intrinsic
              dict(s=100.0, k=30.0, r=0.03, v=0.02, t=2.0, defint=0.05, lgd=0.6, n_grid=50),         # deep ITM, small v
              dict(s=100.0, k=400.0, r=0.03, v=0.03, t=2.0, defint=0.05, lgd=0.6, n_grid=32),        # deep OTM, small v: A underflows
              dict(s=100.0, k=100.0, r=0.01, v=0.05, t=1.0, defint=0.05, lgd=0.6, n_grid=1)]
    intrinsic = 0
    n = 3001
    for c in cases:
        intrinsic += gr.cva_dates(c, X)[2][-1] == 0
        first = int(rng.integers(0, 1 << 34))
        check(run(eng, "cva", c, n, first, X, lr), reference(eng, "cva", c, n, first, X, lr), X, c)
    assert intrinsic >= 1


# ---- b. one path per call: per-path parity through the sums -------------------------------------------------------------
def single_paths(eng, kind, market, firsts, X, lr):
    for first in firsts:
        got = run(eng, kind, market, 1, first, X, lr)
        p = reference(eng, kind, market, 1, first, X, lr)
        b = gr.bound(p, TOL[X]["pay"])[:, 0]
        for q, g in enumerate(got):
            v = p.value[q, 0]
            assert g.n == 1 and abs(g.sum - v) <= b[q], (kind, first, q, g.sum, v, b[q])
            assert abs(g.sum2 - v * v) <= 2 * abs(v) * b[q] + b[q] * b[q], (kind, first, q)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_single_paths(mc, eng, X, lr):
    npb = gr.NPB[X]
    units = [0, 1, 5, 77777, U32 // 2, U32 - 3, U32 - 2, U32 - 1, U32, U32 + 1, U32 + 2, 2 * U32 - 1, 2 * U32, 3 * U32 + 7, 1 << 40, 12345]
    # every position inside a unit, units on both sides of 2^32
    single_paths(eng, "vanilla", dict(s=90.0, k=85.0, r=0.02, v=0.35, t=1.5), [u * npb + j for u in units for j in range(npb)], X, lr)
    firsts = [u + j for u in (0, 1000, U32 - 16, U32, 5 * U32 - 8) for j in range(13)][:64]   # path = unit: 2^32 - 16 .. 2^32 + 12
    rng = np.random.default_rng(51)
    b = gr.random_basket(rng, 9, lambda c: mc.chol(c, X))
    b["k"] = 0.9 * float(np.dot(b["w"], b["s"]))
    single_paths(eng, "basket", b, firsts, X, lr)
    single_paths(eng, "cva", dict(s=95.0, k=100.0, r=0.03, v=0.3, t=2.0, defint=0.04, lgd=0.6, n_grid=19), firsts, X, lr)


# ---- c. the pathwise Greeks are the slopes of the pricing kernels on the same paths (f64) -----------------------------------
def bumped(market, key, index, factor):
    m = dict(market)
    if index is None:
        m[key] = market[key] * factor
    else:
        m[key] = list(market[key])
        m[key][index] = market[key][index] * factor
    return m


def test_pathwise_greeks_are_slopes_of_the_pricing_kernels(mc, eng):
    h, n, first = 1e-7, 100_003, 4321
    rng = np.random.default_rng(61)
    X = "f64"
    b = gr.random_basket(rng, 5, lambda c: mc.chol(c, X))
    b["k"] = float(np.dot(b["w"], b["s"]))
    products = [("vanilla", dict(s=87.0, k=92.0, r=0.035, v=0.28, t=1.4), eng.vanilla, [(1, "s", None), (2, "v", None)]),
                ("basket", b, eng.basket, [(1 + a, "s", a) for a in range(5)] + [(6 + a, "v", a) for a in range(5)])]
    checked = 0
    for kind, market, price, steps in products:
        got = run(eng, kind, market, n, first, X, False)
        p = reference(eng, kind, market, n, first, X, False)
        for q, key, index in steps:
            up, dn = bumped(market, key, index, 1 + h), bumped(market, key, index, 1 - h)
            pu, pd = reference(eng, kind, up, n, first, X, False), reference(eng, kind, dn, n, first, X, False)
            if np.any((pu.value[0] > 0) != (pd.value[0] > 0)):
                continue          # a path the step moves across the strike: that difference quotient is not a slope
            x = market[key] if index is None else market[key][index]
            fd = (price(up, n, SEED, first, X).sum - price(dn, n, SEED, first, X).sum) / (2 * h * x)
            assert abs(fd - got[q].sum) <= 1e-7 * np.abs(p.value[q]).sum(), (kind, key, index, fd, got[q].sum)
            checked += 1
    assert checked >= 10
    c = dict(s=96.0, k=104.0, r=0.03, v=0.27, t=1.5, defint=0.045, lgd=0.55, n_grid=24)
    got = run(eng, "cva", c, n, first, X, False)
    z = gr.cva_normals(draw(eng, X), first, n, gr.cva_dates(c, X)[1].size, gr.NPB[X])
    p = gr.cva(c, z, X)
    gaps = gr.cva_hastings_gap(c, z, X)
    for q, key in ((1, "s"), (2, "v")):
        up, dn = bumped(c, key, None, 1 + h), bumped(c, key, None, 1 - h)
        assert np.all(gr.cva_sides(up, z, X) == gr.cva_sides(dn, z, X))
        fd = (eng.cva(up, n, SEED, first, X).sum - eng.cva(dn, n, SEED, first, X).sum) / (2 * h * c[key])
        assert abs(fd - got[q].sum) <= gaps[q - 1].sum() + 1e-7 * np.abs(p.value[q]).sum(), (key, fd, got[q].sum, gaps[q - 1].sum())


# ---- d. many trips, many workgroups, the 2^32-unit seam -----------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_many_trips_and_workgroups(mc, X, lr, blocks):
    n = 300_007
    rng = np.random.default_rng(71)
    with mc.Engine(0, blocks=blocks) as e:
        for n_assets, first in ((4, 0), (9, 12345), (16, U32 - n // 2), (40, 3)):   # the third straddles 2^32 units: two launches
            b = gr.random_basket(rng, n_assets, lambda c: mc.chol(c, X))
            check(run(e, "basket", b, n, first, X, lr), reference(e, "basket", b, n, first, X, lr), X, (blocks, n_assets, first))
        for n_grid, first in ((25, U32 - 100_001), (75, 7)):
            c = gr.random_cva(rng, n_grid=n_grid)
            check(run(e, "cva", c, n, first, X, lr), reference(e, "cva", c, n, first, X, lr), X, (blocks, n_grid, first))
        npb = gr.NPB[X]
        o = dict(s=110.0, k=100.0, r=0.02, v=0.3, t=0.7)
        for first in (0, 7, U32 * npb - 150_001):   # vanilla units are npb paths: the seam is at path 2^32 npb
            check(run(e, "vanilla", o, n, first, X, lr), reference(e, "vanilla", o, n, first, X, lr), X, (blocks, first))
