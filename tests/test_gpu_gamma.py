"""The second-order Greeks kernels (vanilla_greeks_kernel's SECOND_ORDER form, basket_gamma_kernel) against the independent float64 reference
gamma_ref.py on the kernels' own normals (Engine.normals), one path at a time and through many trips, workgroups, tiles and the
2^32-unit seam; against the first-order kernels' bits; against Black-Scholes; and their refusals.

Per-path tolerances are greeks_ref.bound of gamma_ref's Paths (TOL[X]["pay"] per unit of scale, plus the step of the indicator
on a path within that bound of the strike); the bound on a sum is the sum of the per-path bounds."""
import math

import numpy as np
import pytest

import gamma_ref as gm
import greeks_ref as gr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

U32 = 1 << 32
BASKET_SIZES = [1, 2, 4, 7, 8, 9, 16, 17, 33, 64]   # 4 x 4 tiles: edges at 4, 8, 16; 64 = 2080 entries, 136 tiles


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
    if kind == "vanilla":
        return list(got)
    price, G = got
    n = len(G)
    return [price] + [G[a][b] for a, b in gm.upper_index(n)]


def run(e, kind, market, n, first, X):
    if kind == "vanilla":
        return planes(kind, e.vanilla_greeks2(market, n, SEED, first, X))
    return planes(kind, e.basket_gamma(market, n, SEED, first, X))


def reference(e, kind, market, n, first, X, chunk=20_000):
    npb = gr.NPB[X]
    parts = []
    for f in range(first, first + n, chunk):
        m = min(chunk, first + n - f)
        if kind == "vanilla":
            parts.append(gm.vanilla_greeks2(market, gr.vanilla_normals(draw(e, X), f, m, npb)))
        else:
            parts.append(gm.basket_gamma(market, gr.basket_normals(draw(e, X), f, m, len(market["s"]), npb)))
    return gr.Paths(*(np.concatenate([getattr(p, k) for p in parts], axis=-1) for k in gr.Paths._fields))


def check(got, p, X, what=""):
    b = gr.bound(p, TOL[X]["pay"])
    assert len(got) == len(p.value)
    for q, g in enumerate(got):
        v = p.value[q]
        assert g.n == v.size
        tol, tol2 = b[q].sum(), (2 * np.abs(v) * b[q] + b[q] * b[q]).sum()
        assert abs(g.sum - v.sum()) <= tol, (what, q, g.sum, v.sum(), tol)
        assert abs(g.sum2 - (v * v).sum()) <= tol2, (what, q, g.sum2, (v * v).sum(), tol2)


# ---- 1. per-path parity on random asymmetric markets ------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_vanilla_random_markets(eng, X):
    rng = np.random.default_rng(131)
    n = 20011
    for _ in range(8):
        o = gr.random_vanilla(rng)
        first = int(rng.integers(0, 1 << 36))
        check(run(eng, "vanilla", o, n, first, X), reference(eng, "vanilla", o, n, first, X), X, o)
    o = dict(s=50.0, k=5000.0, r=0.01, v=0.1, t=0.5)   # deep out of the money: every sum is exactly 0
    assert all(g.sum == 0 and g.sum2 == 0 for g in run(eng, "vanilla", o, n, 9, X))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", BASKET_SIZES)
def test_basket_random_markets(mc, eng, X, n_assets):
    rng = np.random.default_rng(2000 + n_assets)
    b = gr.random_basket(rng, n_assets, lambda c: mc.chol(c, X))
    n, first = (1009 if n_assets > 32 else 3001), int(rng.integers(0, 1 << 34))
    check(run(eng, "basket", b, n, first, X), reference(eng, "basket", b, n, first, X), X, (n_assets, b["k"]))


def single_paths(eng, kind, market, firsts, X):
    for first in firsts:
        got = run(eng, kind, market, 1, first, X)
        p = reference(eng, kind, market, 1, first, X)
        b = gr.bound(p, TOL[X]["pay"])[:, 0]
        for q, g in enumerate(got):
            v = p.value[q, 0]
            assert g.n == 1 and abs(g.sum - v) <= b[q], (kind, first, q, g.sum, v, b[q])
            assert abs(g.sum2 - v * v) <= 2 * abs(v) * b[q] + b[q] * b[q], (kind, first, q)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_single_paths_across_the_seam(mc, eng, X):
    npb = gr.NPB[X]
    units = [0, 1, 77777, U32 - 2, U32 - 1, U32, U32 + 1, 2 * U32 - 1, 2 * U32, 1 << 40]
    single_paths(eng, "vanilla", dict(s=90.0, k=85.0, r=0.02, v=0.35, t=1.5), [u * npb + j for u in units for j in range(npb)], X)
    rng = np.random.default_rng(151)
    b = gr.random_basket(rng, 9, lambda c: mc.chol(c, X))
    b["k"] = 0.9 * float(np.dot(b["w"], b["s"]))
    single_paths(eng, "basket", b, [u + j for u in (0, U32 - 8, U32, 5 * U32 - 4) for j in range(8)], X)


@pytest.mark.parametrize("blocks", [1, 7])
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_many_trips_and_workgroups(mc, X, blocks):
    rng = np.random.default_rng(171)
    with mc.Engine(0, blocks=blocks) as e:
        for n_assets, first, n in ((5, 0, 100_003), (17, U32 - 40_000, 80_001)):   # the second straddles 2^32 units: two launches
            b = gr.random_basket(rng, n_assets, lambda c: mc.chol(c, X))
            check(run(e, "basket", b, n, first, X), reference(e, "basket", b, n, first, X), X, (blocks, n_assets, first))
        o = dict(s=110.0, k=100.0, r=0.02, v=0.3, t=0.7)
        n = 300_007
        for first in (7, U32 * gr.NPB[X] - 150_001):
            check(run(e, "vanilla", o, n, first, X), reference(e, "vanilla", o, n, first, X), X, (blocks, first))


# ---- 2, 5. the first-order kernels' bits, an exactly symmetric matrix --------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_same_bits_as_the_first_order_kernels(mc, eng, X):
    o = dict(s=87.0, k=92.0, r=0.035, v=0.28, t=1.4)
    for n, first in ((1_000_003, 0), (200_001, 13)):
        two = eng.vanilla_greeks2(o, n, SEED, first, X)
        one = eng.vanilla_greeks(o, n, SEED, first, X)
        assert [(g.sum, g.sum2, g.n) for g in two[:3]] == [(g.sum, g.sum2, g.n) for g in one]
        assert [(g.expected, g.confidence) for g in two[:3]] == [(g.expected, g.confidence) for g in one]
    rng = np.random.default_rng(181)
    for n_assets in (3, 6, 13):
        b = gr.random_basket(rng, n_assets, lambda c: mc.chol(c, X))
        price, G = eng.basket_gamma(b, 100_003, SEED, 5, X)
        pw = eng.basket_greeks(b, 100_003, SEED, 5, X)
        assert (price.sum, price.sum2, price.expected) == (pw[0].sum, pw[0].sum2, pw[0].expected)
        assert len(G) == n_assets and all(len(row) == n_assets for row in G)
        for a in range(n_assets):
            for c in range(n_assets):
                assert G[a][c] == G[c][a]


# ---- 3, 4. Black-Scholes ----------------------------------------------------------------------------------------------------
def test_vanilla_gamma_vanna_meet_black_scholes(eng):
    n = 5 * 10 ** 7
    for o in (dict(s=100.0, k=100.0, r=0.048790, v=0.2, t=1.0), dict(s=37.0, k=41.5, r=-0.01, v=0.55, t=0.4),
              dict(s=210.0, k=160.0, r=0.07, v=0.12, t=1.8)):
        got = eng.vanilla_greeks2(o, n, SEED, 0, "f64")
        bs = gm.black_scholes(o)
        for q in range(5):
            assert abs(got[q].expected - bs[q]) <= 4 * got[q].confidence, (o, q, got[q].expected, bs[q], got[q].confidence)


def test_basket_gamma_of_a_single_asset_payoff(mc, eng):
    C = np.array([[1.0, 0.5, 0.3, -0.2], [0.5, 1.0, 0.4, 0.1], [0.3, 0.4, 1.0, 0.25], [-0.2, 0.1, 0.25, 1.0]])
    L, bad = mc.chol(C, "f64")
    assert bad == 0
    b = dict(s=[90.0, 120.0, 45.0, 200.0], v=[0.3, 0.2, 0.5, 0.15], p=np.asarray(L).tolist(), d=[0.0] * 4, w=[1.0, 0.0, 0.0, 0.0],
             k=95.0, t=1.2, r=0.03)
    price, G = eng.basket_gamma(b, 10 ** 7, SEED, 0, "f64")
    want = gm.black_scholes(dict(s=90.0, k=95.0, r=0.03, v=0.3, t=1.2))
    assert abs(price.expected - want[0]) <= 4 * price.confidence
    assert abs(G[0][0].expected - want[3]) <= 4 * G[0][0].confidence, (G[0][0].expected, want[3], G[0][0].confidence)
    for a in range(1, 4):
        assert abs(G[0][a].expected) <= 4 * G[0][a].confidence, (a, G[0][a].expected, G[0][a].confidence)
        for c in range(1, 4):
            assert G[a][c].sum == 0 and G[a][c].sum2 == 0


# ---- 6. fused and unfused finish ----------------------------------------------------------------------------------------
def test_fused_and_unfused_finish_give_the_same_bits(mc):
    rng = np.random.default_rng(191)
    b = gr.random_basket(rng, 11, lambda c: mc.chol(c, "f64"))
    o = dict(s=96.0, k=104.0, r=0.03, v=0.27, t=1.5)
    with mc.Engine(0, blocks=3) as fused, mc.Engine(0, blocks=3) as two:
        two.set_finish(False)
        for X in ("f32", "f64"):
            a, c = fused.vanilla_greeks2(o, 200_001, SEED, 1, X), two.vanilla_greeks2(o, 200_001, SEED, 1, X)
            assert [(g.sum, g.sum2) for g in a] == [(g.sum, g.sum2) for g in c]
            a, c = planes("basket", fused.basket_gamma(b, 50_001, SEED, 1, X)), planes("basket", two.basket_gamma(b, 50_001, SEED, 1, X))
            assert [(g.sum, g.sum2) for g in a] == [(g.sum, g.sum2) for g in c]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(mc):
    import ctypes as C
    from montecarlocuda_amd import _lib
    o = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
    b = dict(s=[100.0, 90.0], v=[0.3, 0.2], p=[[1.0, 0.0], [0.5, math.sqrt(0.75)]], d=[0.0, 0.0], w=[0.5, 0.5], k=95.0, t=1.0, r=0.05)
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            e.set_antithetic(True)
            for f in (lambda: e.vanilla_greeks2(o, 1000, SEED, 0, X), lambda: e.basket_gamma(b, 1000, SEED, 0, X)):
                with pytest.raises(mc.McError, match="mc error 4:.*plain estimator"):
                    f()
            e.set_antithetic(False)
            e.set_generator("xorwow")
            for f in (lambda: e.vanilla_greeks2(o, 1000, SEED, 0, X), lambda: e.basket_gamma(b, 1000, SEED, 0, X)):
                with pytest.raises(mc.McError, match="mc error 4:.*Philox"):
                    f()
            e.set_generator("philox")
            with pytest.raises(mc.McError, match="mc error 1:.*non-singular"):
                e.basket_gamma(dict(b, p=[[1.0, 0.0], [1.0, 0.0]]), 1000, SEED, 0, X)
            with pytest.raises(mc.McError, match="mc error 1:.*non-singular"):
                e.basket_gamma(dict(b, v=[0.3, 0.0]), 1000, SEED, 0, X)
            with pytest.raises(mc.McError, match="mc error 1:.*t>0"):
                e.basket_gamma(dict(b, t=0.0), 1000, SEED, 0, X)
            for bad in (dict(o, v=0.0), dict(o, t=0.0)):
                with pytest.raises(mc.McError, match="mc error 1:.*v>0 and t>0"):
                    e.vanilla_greeks2(bad, 1000, SEED, 0, X)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match="mc error 4:.*native normals"):
            e.vanilla_greeks2(o, 1000, SEED, 0, "f64")
        with pytest.raises(mc.McError, match="mc error 4:.*native normals"):
            e.basket_gamma(b, 1000, SEED, 0, "f64")
        e.vanilla_greeks2(o, 1000, SEED, 0, "f32")   # no effect on the _f32 entry points
        e.set_normals("native")
        L = _lib.lib()
        opt = _lib.OPTION["f64"](100.0, 100.0, 0.05, 0.2, 1.0)
        assert L.mc_vanilla_greeks2_run_f64(e._ctx, C.byref(opt), SEED, 0, 1000, None) == 1
        h = mc.engine._BasketHolder("f64", b)
        price, gamma = _lib.Result(), (_lib.Result * 4)()
        assert L.mc_basket_gamma_run_f64(e._ctx, C.byref(h.struct), SEED, 0, 1000, None, gamma) == 1
        assert L.mc_basket_gamma_run_f64(e._ctx, C.byref(h.struct), SEED, 0, 1000, C.byref(price), None) == 1
        assert L.mc_basket_gamma_run_f64(e._ctx, C.byref(h.struct), SEED, 0, 1000, C.byref(price), gamma) == 0
        assert gamma[1].sum == gamma[2].sum and price.n == 1000
