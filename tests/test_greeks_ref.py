"""The float64 Greeks reference (greeks_ref.py) on the CPU: against the oracle twins of the six estimators on the same
Philox normals, and against its own prices by central differences.  Two derivations by different hands that agree here
are what the GPU tests (test_gpu_greeks_ref.py) then hold the kernels to."""
import numpy as np
import pytest

import greeks_ref as gr

SEED = 0x4D435F4D49333535
TOL = {"f32": 2e-6, "f64": 1e-14}   # per-path bounds per unit of greeks_ref scale (test_gpu_parity.TOL[X]["pay"])


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def cpu_draw(po, X):
    def draw(domain, u0, n, block):
        return np.array([po.dev_normals(X, SEED, domain, u0 + u, block) for u in range(n)])
    return draw


def check_sums(p, orc, X):
    """Sums of the reference's per-path values against the oracle's sums (rows of p.value against orc dicts)."""
    for q, o in enumerate(orc):
        v = p.value[q]
        if X == "f64":   # the same formulas in the same precision: 1e-12 of the sum of magnitudes (relative unless it cancels)
            tol, tol2 = 1e-12 * np.abs(v).sum(), 1e-12 * (v * v).sum()
        else:            # the oracle's fp32 arithmetic: the per-path bounds
            b = gr.bound(p, TOL[X])[q]
            tol, tol2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
        assert abs(o["sum"] - v.sum()) <= tol, (q, o["sum"], v.sum(), tol)
        assert abs(o["sum2"] - (v * v).sum()) <= tol2, (q, o["sum2"], (v * v).sum(), tol2)


@pytest.mark.parametrize("X", ["f64", "f32"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_vanilla_reference_matches_oracle_twin(po, X, lr):
    rng = np.random.default_rng(11)
    n, first = 2003, 13
    z = gr.vanilla_normals(cpu_draw(po, X), first, n, gr.NPB[X])
    twin = po.dev_vanilla_greeks_lr if lr else po.dev_vanilla_greeks
    for _ in range(6):
        o = gr.random_vanilla(rng)
        check_sums(gr.vanilla(o, z, lr), twin(X, o, SEED, first, n), X)


@pytest.mark.parametrize("X", ["f64", "f32"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_basket_reference_matches_oracle_twin(mc, po, X, lr):
    rng = np.random.default_rng(12 + lr)
    n, first = 1501, 7
    g = gr.basket_normals(cpu_draw(po, X), first, n, 17, gr.NPB[X])
    for na in (1, 2, 7, 8, 9, 17):   # one side and the other of the kernel's 8-asset chunks
        b = gr.random_basket(rng, na, lambda c: mc.chol(c, X))
        op, od, ov = po.dev_basket_greeks(X, b, SEED, first, n, lr=lr)
        check_sums(gr.basket(b, g[:, :na], lr), [op] + od + ov, X)


@pytest.mark.parametrize("X", ["f64", "f32"])
@pytest.mark.parametrize("lr", [False, True], ids=["pathwise", "lr"])
def test_cva_reference_matches_oracle_twin(po, X, lr):
    rng = np.random.default_rng(14 + lr)
    n, first = 1001, 3
    z = gr.cva_normals(cpu_draw(po, X), first, n, 300, gr.NPB[X])
    cases = [gr.random_cva(rng) for _ in range(5)] + [dict(gr.random_cva(rng, n_grid=64), t=1.0),   # last date at maturity: intrinsic
                                                      dict(gr.random_cva(rng, n_grid=40), v=0.05, k=0.5 * 100, s=100.0)]   # deep ITM, small v
    intrinsic = 0
    for c in cases:
        intrinsic += gr.cva_dates(c, X)[2][-1] == 0
        check_sums(gr.cva(c, z, X, lr), po.dev_cva_greeks(X, c, SEED, first, n, lr=lr), X)
    assert intrinsic >= 1


def test_hastings_slope_gap():
    """The stated sup |cnd' - phi| of the reference's Hastings cnd, and cnd_prime as its slope away from the step at 0."""
    d = np.linspace(-40, 40, 800001)
    gap = np.abs(gr.cnd_prime(d) - gr.INV_SQRT_2PI * np.exp(-0.5 * d * d))
    assert gap.max() <= gr.HASTINGS_SLOPE_GAP and gap.max() > 0.9 * gr.HASTINGS_SLOPE_GAP
    x = d[np.abs(d) > 1e-3]
    h = 1e-6
    assert np.abs((gr.cnd(x + h) - gr.cnd(x - h)) / (2 * h) - gr.cnd_prime(x)).max() < 1e-8
    assert abs(1 - 2 * float(gr.cnd(0.0))) < 2e-9


def difference(f, market, key, index=None, h=1e-7):
    """Central difference of f(market) in market[key] (or market[key][index]) with relative step h; f returns Paths."""
    def bumped(sign):
        m = dict(market)
        if index is None:
            m[key] = market[key] * (1 + sign * h)
        else:
            m[key] = list(market[key])
            m[key][index] = market[key][index] * (1 + sign * h)
        return f(m)
    x = market[key] if index is None else market[key][index]
    up, dn = bumped(1), bumped(-1)
    return (up.value[0] - dn.value[0]) / (2 * h * x), up, dn


def test_pathwise_vanilla_and_basket_are_slopes_of_the_reference_price():
    rng = np.random.default_rng(21)
    z = rng.standard_normal(200_000)
    for _ in range(4):
        o = gr.random_vanilla(rng)
        p = gr.vanilla(o, z)
        for q, key in ((1, "s"), (2, "v")):
            fd, up, dn = difference(lambda m: gr.vanilla(m, z), o, key)
            keep = (up.value[0] > 0) == (dn.value[0] > 0)      # a path the step moves across the strike has no slope there
            assert keep.mean() > 0.999
            assert abs(fd[keep].sum() - p.value[q][keep].sum()) <= 1e-7 * np.abs(p.value[q][keep]).sum() + 1e-9, (o, key)
    g = rng.standard_normal((200_000, 4))
    for _ in range(2):
        b = gr.random_basket(rng, 4, lambda c: (np.linalg.cholesky(c), 0))
        b["k"] = float(np.dot(b["w"], b["s"]))
        p = gr.basket(b, g)
        for a in range(4):
            for q, key in ((1 + a, "s"), (5 + a, "v")):
                fd, up, dn = difference(lambda m: gr.basket(m, g), b, key, a)
                keep = (up.value[0] > 0) == (dn.value[0] > 0)
                assert keep.mean() > 0.999
                err = abs(fd[keep].sum() - p.value[q][keep].sum())
                assert err <= 1e-7 * np.abs(p.value[q][keep]).sum() + 1e-9, (a, key, err)


def test_pathwise_cva_is_the_slope_of_the_reference_price_up_to_the_hastings_gap():
    rng = np.random.default_rng(22)
    for c in (dict(gr.random_cva(rng, n_grid=12), k=None), dict(gr.random_cva(rng, n_grid=64), t=1.0, k=None)):
        c["k"] = c["s"] * 1.05
        z = rng.standard_normal((20_000, c["n_grid"]))
        p = gr.cva(c, z)
        gaps = gr.cva_hastings_gap(c, z)
        for q, key in ((1, "s"), (2, "v")):
            fd, up, dn = difference(lambda m: gr.cva(m, z), c, key)
            keep = np.ones(len(z), bool)   # no date's d1, d2 or intrinsic indicator may change side between the two steps
            for m in (dict(c, **{key: c[key] * (1 + 1e-7)}), dict(c, **{key: c[key] * (1 - 1e-7)})):
                keep &= (gr.cva_sides(m, z) == gr.cva_sides(c, z)).all(axis=1)
            assert keep.mean() > 0.99
            err = np.abs(fd[keep] - p.value[q][keep])
            assert np.all(err <= gaps[q - 1][keep] + 1e-6 * np.abs(p.value[q][keep]) + 1e-9), (key, (err / gaps[q - 1][keep]).max())
            # the Hastings gap is real: the bound is not vacuous and the difference is not zero
            assert err.max() > 0 and gaps[q - 1].sum() < 1e-3 * np.abs(p.value[q]).sum()

