"""The float64 second-order Greeks reference (gamma_ref.py) on the CPU: its gamma and vanna against Black-Scholes on numpy
normals, its basket gamma matrix against its vanilla gamma at one asset and against Black-Scholes for a single-asset payoff
inside a correlated basket, and its first-order rows against greeks_ref.  What the GPU tests (test_gpu_gamma.py) then hold
the kernels to."""
import math

import numpy as np

import gamma_ref as gm
import greeks_ref as gr

MARKETS = [dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0),
           dict(s=37.0, k=41.5, r=-0.01, v=0.55, t=0.4),
           dict(s=210.0, k=160.0, r=0.07, v=0.12, t=1.8),
           dict(s=64.0, k=80.0, r=0.02, v=0.35, t=2.0)]


def mean_hw(x, disc):
    """Discounted mean and its 95 % half-width."""
    return disc * x.mean(), disc * 1.96 * x.std(ddof=1) / math.sqrt(x.size)


def test_vanilla_gamma_vanna_meet_black_scholes():
    z = np.random.default_rng(3).standard_normal(1_000_000)
    for o in MARKETS:
        p = gm.vanilla_greeks2(o, z)
        bs = gm.black_scholes(o)
        disc = math.exp(-o["r"] * o["t"])
        for q in range(5):
            m, hw = mean_hw(p.value[q], disc)
            assert abs(m - bs[q]) <= 4 * hw, (o, q, m, bs[q], hw)


def test_first_order_rows_equal_greeks_ref():
    z = np.random.default_rng(4).standard_normal(20_000)
    for o in MARKETS:
        p, q = gm.vanilla_greeks2(o, z), gr.vanilla(o, z)
        assert np.array_equal(p.value[:3], q.value)
        assert np.array_equal(p.edge, q.edge)


def test_one_asset_basket_gamma_is_the_vanilla_gamma():
    z = np.random.default_rng(5).standard_normal(20_000)
    for o in MARKETS:
        b = dict(s=[o["s"]], v=[o["v"]], p=[[1.0]], d=[0.0], w=[1.0], k=o["k"], t=o["t"], r=o["r"])
        pb, pv = gm.basket_gamma(b, z[:, None]), gm.vanilla_greeks2(o, z)
        assert pb.value.shape == (2, z.size)
        np.testing.assert_array_equal(pb.value[0], pv.value[0])
        np.testing.assert_allclose(pb.value[1], pv.value[3], rtol=1e-12, atol=1e-15 * np.abs(pv.value[3]).max())
        assert np.all(gr.bound(pb, 1e-14)[1] > 0)


def test_basket_gamma_of_a_single_asset_payoff():
    """Weights (1, 0, 0, 0) in a correlated basket: gamma[0][0] is asset 0's Black-Scholes gamma, every entry outside row and
    column 0 is exactly 0, the cross-gammas gamma[0][b] are 0 within their half-widths."""
    rng = np.random.default_rng(6)
    A = rng.normal(size=(4, 6))
    C = A @ A.T
    C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
    L = np.linalg.cholesky(C)
    b = dict(s=[90.0, 120.0, 45.0, 200.0], v=[0.3, 0.2, 0.5, 0.15], p=L.tolist(), d=[0.0] * 4, w=[1.0, 0.0, 0.0, 0.0],
             k=95.0, t=1.2, r=0.03)
    g = rng.standard_normal((1_000_000, 4))
    p = gm.basket_gamma(b, g)
    G = gm.gamma_matrix(p)
    assert np.array_equal(G, np.transpose(G, (0, 2, 1)))
    disc = math.exp(-b["r"] * b["t"])
    o = dict(s=90.0, k=95.0, r=0.03, v=0.3, t=1.2)
    m, hw = mean_hw(G[:, 0, 0], disc)
    assert abs(m - gm.black_scholes(o)[3]) <= 4 * hw, (m, gm.black_scholes(o)[3], hw)
    assert np.all(G[:, 1:, 1:] == 0)
    for c in range(1, 4):
        m, hw = mean_hw(G[:, 0, c], disc)
        assert abs(m) <= 4 * hw, (c, m, hw)


def test_upper_index_is_the_kernels_plane_order():
    for n in (1, 2, 5, 64):
        ent = gm.upper_index(n)
        assert len(ent) == n * (n + 1) // 2
        for u, (a, b) in enumerate(ent):
            assert u == a * n - a * (a - 1) // 2 + b - a
