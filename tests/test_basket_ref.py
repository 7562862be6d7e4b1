"""The float64 basket model (basket_ref.py) on the CPU: that it is right -- against greeks_ref.basket, the fp64 oracle twin of the
four estimators, the oracle's closed form and a Monte-Carlo check of it -- and that its bound has power: the index errors of
basket_ref.MUTATIONS are invisible on the suite's symmetric market (test_gpu_parity.basket_inputs) and rejected on almost every
path of every market test_gpu_basket_ref.py prices, while an honest fp32 evaluation uses a small part of the bound."""
import math

import numpy as np
import pytest

import basket_ref as br
import greeks_ref as gr
import test_gpu_basket_ref as gpu
from test_gpu_parity import SEED, TOL, basket_inputs


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def cpu_market(mc, seed, n_assets, positive=True):
    return br.random_market(np.random.default_rng(seed), n_assets, lambda c: mc.chol(c, "f64"), positive_weights=positive)


def test_plain_value_is_greeks_ref_row_0(mc):
    rng = np.random.default_rng(1)
    for n_assets in (1, 2, 5, 16, 40):
        b = cpu_market(mc, 100 + n_assets, n_assets, positive=False)
        g = rng.standard_normal((500, n_assets))
        p, q = br.value(b, g), gr.basket(b, g)
        assert p.value.shape == (1, 500)
        assert np.array_equal(p.value[0], q.value[0]) and np.array_equal(p.scale[0], q.scale[0])
        assert not p.jump.any() and np.isinf(p.edge).all() and gr.kink_free(p, 1.0)


@pytest.mark.parametrize("n_assets", [1, 3, 8, 16, 33, 64])
def test_model_matches_the_fp64_oracle(mc, po, n_assets):
    """All four estimators against po.dev_basket on the oracle's own normals, within the fp64 bound per path."""
    n, first = 301, 11
    g = gr.basket_normals(lambda dom, u0, c, blk: np.array([po.dev_normals("f64", SEED, dom, u0 + u, blk) for u in range(c)]),
                          first, n, n_assets, gr.NPB["f64"])
    b = cpu_market(mc, 200 + n_assets, n_assets)
    for m in (b, br.in_the_money(b)):
        for anti, cv in br.ESTIMATORS:
            want, o = po.dev_basket("f64", m, SEED, first, n, antithetic=anti, control=cv)
            p = br.value(m, g, anti, cv)
            bnd = gr.bound(p, TOL["f64"]["pay"])[0]
            assert np.all(np.abs(want - p.value[0]) <= bnd), (n_assets, anti, cv, float((np.abs(want - p.value[0]) / bnd).max()))
            assert abs(o["sum"] - p.value[0].sum()) <= bnd.sum()


def test_control_mean_is_the_oracles_closed_form(mc, po):
    for n_assets in (1, 2, 3, 7, 16, 33, 64):
        b = cpu_market(mc, 300 + n_assets, n_assets)
        for m in (b, br.in_the_money(b)):
            assert br.control_mean(m) == pytest.approx(po.basket_control_mean("f64", m), rel=1e-13)
    one = dict(s=[100.0], v=[0.0], p=[[1.0]], d=[0.0], w=[1.0], k=90.0, t=1.0, r=0.05)      # no variance: intrinsic of the forward
    assert br.control_mean(one) == pytest.approx(100.0 * math.exp(0.05) - 90.0, rel=1e-14)


def test_control_mean_is_the_mean_of_the_models_geometric_payoff(mc):
    rng = np.random.default_rng(7)
    for n_assets in (1, 6, 19):
        b = cpu_market(mc, 400 + n_assets, n_assets)
        b["k"] = 0.95 * float(np.dot(b["w"], b["s"]))
        G, _ = br.geometric(b, rng.standard_normal((200_000, n_assets)))
        pay = np.maximum(G - b["k"], 0.0)
        assert abs(pay.mean() - br.control_mean(b)) <= 4 * pay.std() / math.sqrt(pay.size), n_assets
        # and the control variate is what its name says: the model's values are payoff - that payoff
    g = rng.standard_normal((100, n_assets))
    G, _ = br.geometric(b, g)
    assert np.array_equal(br.value(b, g, control=True).value[0], br.value(b, g).value[0] - np.maximum(G - b["k"], 0.0))
    assert np.array_equal(br.value(b, g, anti=True).value[0], 0.5 * (br.value(b, g).value[0] + br.value(b, -g).value[0]))


def test_folded_form_is_the_model(mc):
    rng = np.random.default_rng(8)
    for n_assets in (1, 5, 16, 37):
        b = cpu_market(mc, 500 + n_assets, n_assets, positive=False)
        g = rng.standard_normal((400, n_assets))
        p = br.value(b, g)
        assert np.all(np.abs(br.value_folded(b, g) - p.value[0]) <= gr.bound(p, 1e-14)[0])


# ---- the blindness of the suite's market, the power on the new ones ------------------------------------------------------
@pytest.mark.parametrize("n_assets", [16, 24, 40])
def test_symmetric_market_cannot_see_an_index_error(mc, n_assets):
    """On basket_inputs' market every mutation that applies leaves every path value BIT-identical."""
    b = basket_inputs(mc, n_assets, "f64")
    g = np.random.default_rng(n_assets).standard_normal((4000, n_assets))
    clean = br.value_folded(b, g)
    assert (clean > 0).mean() > 0.3
    muts = br.mutations(n_assets)
    assert len(muts) == 5
    npad = len(br.folded(b)[1])
    distinct = (np.arange(npad * npad, dtype=np.float64).reshape(npad, npad), np.arange(npad) + 0.5, np.arange(npad) + 0.25, np.arange(npad) + 0.125)
    for name, f in muts.items():
        assert not all(np.array_equal(x, y) for x, y in zip(f(n_assets, *distinct), distinct)), name    # it does move constants
        assert np.array_equal(br.value_folded(b, g, f), clean), name


def test_mutations_apply_from_their_sizes():
    assert [len(br.mutations(n)) for n in (1, 3, 4, 15, 16, 64)] == [0, 0, 2, 2, 5, 5]


@pytest.mark.parametrize("test,n_assets", gpu.power_cases())
def test_every_gpu_market_rejects_every_index_error(mc, test, n_assets):
    """The condition the GPU test's markets are chosen under: struck in the money (as test_gpu_basket_ref.py prices each of them),
    every index error that applies moves at least 90 % of 4000 paths beyond the fp32 per-path bound.  (A seed that fails this is
    replaced in test_gpu_basket_ref.seed_of; the 90 % stays.)"""
    b = br.in_the_money(gpu.market(mc, test, n_assets)[0])
    g = np.random.default_rng(gpu.seed_of(test, n_assets)).standard_normal((4000, n_assets))
    bnd = gr.bound(br.value(b, g), TOL["f32"]["pay"])[0]
    clean = br.value_folded(b, g)
    for name, f in br.mutations(n_assets).items():
        moved = np.abs(br.value_folded(b, g, f) - clean) > bnd
        assert moved.mean() >= 0.9, (test, n_assets, name, int(moved.sum()))


# ---- the reference alone leaves the kernel room -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_assets", [1, 6, 12, 16, 28, 32, 47, 64])
def test_an_honest_fp32_evaluation_uses_at_most_half_the_bound(mc, n_assets):
    """basket_ref.value_folded_f32 (constants rounded once, fma chains, exp2, all in float32) against the model on the same float
    normals, |z| < 6.7 as the fp32 generator's: at most 0.5 of the fp32 bound per path, on six markets, each at its drawn strike and struck in the money.  Measured worst: 0.12, at 64 assets."""
    rng = np.random.default_rng(900 + n_assets)
    worst = 0.0
    for i in range(6):
        b = cpu_market(mc, 600 + 10 * n_assets + i, n_assets, positive=bool(i % 2))
        g = np.clip(rng.standard_normal((2000, n_assets)), -6.69, 6.69)
        g[:8] = rng.choice([-6.69, 6.69], size=(8, n_assets))         # the generator's extremes, every asset at once
        g = g.astype(np.float32).astype(np.float64)
        for m in (b, br.in_the_money(b)):
            p = br.value(m, g)
            ratio = np.abs(br.value_folded_f32(m, g) - p.value[0]) / gr.bound(p, TOL["f32"]["pay"])[0]
            worst = max(worst, float(ratio.max()))
    print(f"fp32 emulation, n_assets={n_assets}: worst err/bound {worst:.3f}")
    assert worst <= 0.5
