"""Launch-geometry (compatibility) mode, every path against the float64 models on asymmetric markets: grid_vanilla_f32_kernel,
grid_vanilla_f64_kernel, grid_basket_kernel<Real, 4 | 8 | 16>, grid_cva_kernel and xorwow_grid_init_kernel (csrc/mc_grid.hpp, the
fused form), grid_normals_kernel feeding the simulation kernels (the staged form), and the host side that cuts a thread's stream
into pieces (csrc/mc_api.hip: grid_run_fused, grid_run_staged; csrc/mc_launch_shape.hpp: grid_pieces).

Why: tests/test_gpu_grid.py compares this mode with the oracle's device formulas -- the same formulas in the same precision by the
same hand -- on symmetric markets (one spot, no dividends, equal weights, one correlation, t = 1) under absolute constants, with the
arrangement taken from the oracle's own grid_path_normals: an exchanged asset row, a zero-padded row that is not exactly neutral or a
date table off by one row is invisible there, baskets never met more than 256 threads or 8 pieces, the CVA 32 threads and 2 pieces,
and the piece counts were never asserted.

Here the sample is grid_ref.py's, written from the header's paragraph (include/mc_mi355x.h, "compatibility mode"): the streams are
Engine.grid_normals -- the one-piece layout, pinned bit for bit to rocRAND's device engine by test_gpu_grid.py and here tied to
Engine.xorwow_words (seed b + G, subsequence t; pinned to rocRAND on the host) through a float64 Box-Muller -- the arrangement is
grid_ref.arrange, and the values are greeks_ref.vanilla, basket_ref.value and cva_ref.price on the inputs as the entry point of the
precision reads them.  Every path of both forms stays within greeks_ref.bound(p, TOL[X]["pay"]); no path is left out.
tests/test_grid_ref.py shows on the CPU that this bound rejects every wrong sample of grid_ref.MUTATIONS on at least 90 % of the
paths it reaches.

Geometries (grid_ref.GEOMS): T = 1, 3, 5, 7, 64, 100, 512 and 1024, several blocks, paths_per_block below T and (seven of nine) no multiple of it,
and 32, 32, 16, 8, 4, 2, 1, 1, 1 pieces per thread -- READ from every fused launch (Engine.last_launch()[0] // G) and asserted, so
that a changed piece rule fails the test instead of thinning it; the first five leave a thread's last pieces empty.  Every basket
size and CVA grid runs every geometry (the 257-date cut schedule: the 16-piece one only), so each family meets 1024 threads, 16 and
32 pieces, and odd draws per path in several pieces.

Sums: {sum, sum2, n} of run_grid in each form against the same form's own dump.
  fp64, every product; fp32 CVA; fp32 basket fused: the kernel adds (double) p and fma((double) p, (double) p, acc) in fp64 and the
      dump is p itself (basket: times an exact power of two): greeks_ref.check_sums, n 2^-53 of sum |p| and (n + 1) 2^-53 of sum p^2.
  Float partial sums: a kernel that adds m non-negative payoffs in float, in some order, before it flushes to fp64 is within
      gamma_(m-1) = (m - 1) u / (1 - (m - 1) u), u = 2^-24, of the partial sum; its squares -- fma(p, p, .), or a rounded p p that
      starts a partial sum -- within gamma_m; the call's scale is applied to the fp64 total (one more fp64 rounding).
      fp32 vanilla, both forms (grid_vanilla_f32_kernel; vanilla_f32_kernel and the masked kernel): m <= 32 (8 trips of 4), and the
          dump is fl32(p x scale), 2^-24 of every dumped value: 32 x 2^-24 = 1.9e-6 of sum p and 34 x 2^-24 = 2.0e-6 of sum p^2.
      fp32 basket staged (basket_f32_kernel, up to 16 assets; the larger families add in fp64): m <= 16 (8 trips of 2), the dump
          exact: 15 x 2^-24 = 8.9e-7 and 16 x 2^-24 = 9.5e-7.
      Each plus n 2^-53, and below the 3e-6 test_gpu_grid.py allows.
Same bits: the fused and the staged dump are the same bits on every one of these markets and geometries.

Wall time on the MI355X: the module's 59 tests take 5.9 s together, the slowest (the 65-date CVA grid: 72 calls on nine geometries
and the model on 30 000 paths) 0.49 s.  Worst err/bound as printed (fp32, fp64): vanilla 0.105, 0.032; basket 0.088, 0.035 (33 assets,
in the money; fused sizes at most 0.063, 0.029); CVA 0.032, 0.028; the streams within 1.8e-6 of the float64 Box-Muller of their words.
"""
import math

import numpy as np
import pytest

import grid_ref as gf
from greeks_ref import check_sums

pytestmark = pytest.mark.gpu

STREAM_TOL = 4e-6      # test_gpu_grid.py's: the device's float log, sqrt, sin and cos against the float64 ones
STREAM_COUNT = 512


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.set_grid_form("auto")
    e.close()


_STREAMS = {}


def streams(eng, geom, count):
    """Engine.grid_normals of the geometry's threads, (G, T, >= count): drawn once per geometry and grown when a product needs more
    (a thread's stream is sequential: the first `count` normals do not depend on how many are asked for)."""
    G, T, _ = geom
    have = _STREAMS.get((G, T))
    if have is None or have.shape[2] < count:
        have = eng.grid_normals(G, T, max(count, 2 * have.shape[2] if have is not None else 0))
        assert np.isfinite(have).all()
        _STREAMS[(G, T)] = have
    return have


def model_normals(eng, c):
    return gf.arrange(streams(eng, (c.G, c.T, c.per_block), gf.count_needed(c)), c).astype(np.float64)


def pieces_of_last_launch(eng, geom):
    """The pieces per thread of the fused call just made, from the launch itself: one workgroup per (block, piece), threads rounded up
    to whole waves."""
    G, T, _ = geom
    grid, group = eng.last_launch()
    assert group == -(-T // 64) * 64 and grid % G == 0, (geom, grid, group)
    return grid // G


def check_sums_of_float_partials(est, got, n, what, m, dump_rounded):
    """The module docstring's bound for a kernel that adds its payoffs in float partial sums of at most m terms, term by term:
    gamma_(m-1) on the sum, gamma_m on the sum of squares, 2^-24 of every dumped value where the dump is rounded, and the fp64 part."""
    u, r = 2.0 ** -53, 2.0 ** -24
    g1, g2, d = (m - 1) * r / (1 - (m - 1) * r), m * r / (1 - m * r), r if dump_rounded else 0.0
    p = [float(x) for x in got]
    assert est.n == n and min(p) >= 0.0, what
    s, q = math.fsum(p), math.fsum(x * x for x in p)
    tol1 = ((1 + g1) * (1 + (n + 1) * u) - 1 + d) / (1 - d)
    tol2 = ((1 + g2) * (1 + (n + 2) * u) - 1 + 2 * d + d * d) / (1 - d) ** 2
    assert tol1 <= 3e-6 and tol2 <= 3e-6      # none looser than test_gpu_grid.py's SUMS
    assert abs(est.sum - s) <= tol1 * s, (what, est.sum, s, abs(est.sum - s) / (tol1 * s))
    assert abs(est.sum2 - q) <= tol2 * q, (what, est.sum2, q, abs(est.sum2 - q) / (tol2 * q))


def sums_check_of(prod, X, form):
    if (prod, X) == ("vanilla", "f32"):
        return lambda est, got, n, what: check_sums_of_float_partials(est, got, n, what, 32, True)
    if (prod, X, form) == ("basket", "f32", "staged"):
        return lambda est, got, n, what: check_sums_of_float_partials(est, got, n, what, 16, False)
    return check_sums


def both_forms(mc, eng, prod, market, geom, X, fused_exists=True):
    """{form: (per-path dump, estimate)} of one call in the staged and the fused form; the fused launches' piece count asserted."""
    G, T, per_block = geom
    out = {}
    try:
        for form in ("staged", "fused"):
            eng.set_grid_form(form)
            if form == "fused" and not fused_exists:
                with pytest.raises(mc.McError, match="no fused kernel"):
                    eng.paths_grid(prod, market, G, T, per_block, X)
                with pytest.raises(mc.McError, match="no fused kernel"):
                    eng.run_grid(prod, market, G, T, per_block, X)
                continue
            vals = eng.paths_grid(prod, market, G, T, per_block, X)
            if form == "fused":
                assert pieces_of_last_launch(eng, geom) == gf.GEOMS[geom], (geom, eng.last_launch())
            est = eng.run_grid(prod, market, G, T, per_block, X)
            if form == "fused":
                assert pieces_of_last_launch(eng, geom) == gf.GEOMS[geom], (geom, eng.last_launch())
            assert vals.shape == (G, per_block) and vals.dtype == gf.NP[X]
            out[form] = (vals.reshape(-1), est)
    finally:
        eng.set_grid_form("auto")
    return out


def check_call(mc, eng, prod, market, geom, X, z, what, fused_exists=True):
    """One market on one geometry: both forms per path against the model, their sums against their own dumps, the two dumps the same
    bits.  Returns the worst err / bound."""
    c = gf.call(prod, geom, market, X)
    p = gf.value(c, market, z, X)
    v, bnd = p.value[0], gf.bound(p, X)
    n, worst = c.G * c.per_block, 0.0
    forms = both_forms(mc, eng, prod, market, geom, X, fused_exists)
    assert set(forms) == ({"staged", "fused"} if fused_exists else {"staged"})
    for form, (got, est) in forms.items():
        g = got.astype(np.float64)
        assert g.shape == v.shape and np.all(np.isfinite(g)), (what, form)
        err = np.abs(g - v)
        r = gf.ratio(err, bnd)
        i = int(np.argmax(r))
        assert np.all(err <= bnd), (what, form, i, g[i], v[i], err[i], bnd[i], int((err > bnd).sum()), float(r[i]))
        worst = max(worst, float(r[i]))
        sums_check_of(prod, X, form)(est, got, n, (what, form))
    if fused_exists:
        U = np.uint32 if X == "f32" else np.uint64
        st, fu = forms["staged"][0].view(U), forms["fused"][0].view(U)
        assert np.array_equal(st, fu), (what, int((st != fu).sum()))
    return worst


# ---- the streams ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(gf.GEOMS))
def test_streams_are_box_muller_of_the_words_of_seed_block_plus_blocks(eng, geom):
    """Thread (b, t) owns (seed b + G, subsequence t, offset 0): Engine.grid_normals against a float64 Box-Muller of
    Engine.xorwow_words(b + G, 0, T, count), words that test_rocrand_xcheck.py pins to rocRAND."""
    G, T, _ = geom
    got = eng.grid_normals(G, T, STREAM_COUNT).astype(np.float64)
    worst = 0.0
    for b in range(G):
        want = gf.box_muller(eng.xorwow_words(b + G, 0, T, STREAM_COUNT))
        worst = max(worst, float(np.abs(got[b] - want).max()))
    print(f"grid_ref streams {geom}: max |normal - float64 Box-Muller| = {worst:.3g}")
    assert worst <= STREAM_TOL, (geom, worst)
    # an odd count ends inside a pair: the same stream
    assert np.array_equal(eng.grid_normals(G, T, 7).view(np.uint32), got[:, :, :7].astype(np.float32).view(np.uint32))


# ---- per path, both forms, sums, same bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", gf.PRECISIONS)
def test_vanilla_every_path_both_forms(mc, eng, X):
    worst = {}
    for geom in gf.GEOMS:
        z = model_normals(eng, gf.call("vanilla", geom, None, X))
        for i in range(gf.N_VANILLA_MARKETS):
            for tag, m in gf.vanilla_markets(i):
                worst[tag] = max(worst.get(tag, 0.0), check_call(mc, eng, "vanilla", m, geom, X, z, (X, geom, i, tag)))
    print(f"grid_ref vanilla {X}: worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("X", gf.PRECISIONS)
@pytest.mark.parametrize("n_assets", gf.BASKET_FUSED + gf.BASKET_STAGED_ONLY)
def test_basket_every_path_both_forms(mc, eng, X, n_assets):
    """n = 1 ... 16: grid_basket_kernel<Real, 4 | 8 | 16>, every n that is no compiled size zero-padded inside the next one; 17 and 33:
    the staged form only, "fused" refused."""
    worst = {}
    markets = gf.basket_markets(mc, n_assets)
    for geom in gf.GEOMS:
        z = model_normals(eng, gf.call("basket", geom, markets[0][1], X))
        assert z.shape == (geom[0] * geom[2], n_assets)
        for tag, m in markets:
            worst[tag] = max(worst.get(tag, 0.0), check_call(mc, eng, "basket", m, geom, X, z, (X, n_assets, geom, tag), n_assets <= 16))
    print(f"grid_ref basket {X} n_assets={n_assets}: worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("X", gf.PRECISIONS)
@pytest.mark.parametrize("n_dates", gf.CVA_DATES + ["long"])
def test_cva_every_path_both_forms(mc, eng, X, n_dates):
    """Full, cut and intrinsic endings (xorwow_ref.cva_schedules), one date, odd and even draws; "long": cva_ref.CUT_LONG, 257 of 258
    dates draw, on the 16-piece geometry."""
    worst = {}
    markets = gf.cva_markets(X, n_dates)
    for geom in gf.cva_geoms(n_dates):
        c = gf.call("cva", geom, markets[0][1], X)
        assert c.draws == (257 if n_dates == "long" else n_dates)
        z = model_normals(eng, c)
        for tag, m in markets:
            worst[tag] = max(worst.get(tag, 0.0), check_call(mc, eng, "cva", m, geom, X, z, (X, n_dates, geom, tag)))
    print(f"grid_ref cva {X} n_dates={n_dates}: worst err/bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
