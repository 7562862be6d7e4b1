"""The worst-of / best-of options without a GPU: the closed form (mc_rainbow_closed_form_*, plain C in mc_hostmath_impl.h) against
rainbow_ref.py's first-principles Stulz, a 30-digit mpmath evaluation and (where installed) scipy's bivariate normal; the float64
reference model rainbow_ref.py against the exact prices on numpy's own normals; identities of the model on every path; a float32
evaluation of the walk inside the per-path bound on every shape of tests/test_gpu_rainbow.py; five wrong walks that the bound must
reject; how many paths of those shapes carry a jump term; the refusals that need no device; the structs' layout.

The Monte Carlo checks use ONE fixed seed and 3 half-widths (1.96 sigma / sqrt(n) each, so 5.9 sigma): the margin is for nothing
but sampling noise."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import barrier_ref as br
import greeks_ref as gr
import rainbow_ref as rr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CLOSED_FORM_BOUND = 1e-10   # include/mc_mi355x.h: the closed form is within 1e-10 max(S_1, S_2)


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def two_assets(S, v, rho, k, r, t):
    n = 2
    return dict(s=np.array(S, dtype=np.float64), v=np.array(v, dtype=np.float64), p=np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]])),
                d=np.zeros(n), w=np.ones(n), k=k, t=t, r=r)


# r < 0; rho < 0; |rho| >= 0.95 (twice, the second with rho_1, rho_2 near -1 and +1 as well); very unequal levels
ACCURACY_MARKETS = [((1.0, 1.1), (0.2, 0.3), 0.5, -0.02, 1.0, (0.8, 1.0, 1.25)),
                    ((100.0, 95.0), (0.25, 0.18), -0.6, 0.03, 2.0, (80.0, 100.0, 120.0)),
                    ((1.0, 1.0), (0.2, 0.3), 0.95, 0.02, 1.0, (0.8, 1.0, 1.25)),
                    ((1.0, 1.05), (0.15, 0.35), -0.999, 0.04, 0.5, (0.8, 1.0, 1.25)),
                    ((1.0, 40.0), (0.3, 0.2), 0.3, 0.01, 1.5, (0.9, 5.0, 45.0))]


def rounded(b, X):
    """The basket as the precision's struct holds it."""
    if X == "f64":
        return b
    f = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    return dict(b, **{c: f(b[c]) for c in "svpdw"}, **{c: float(np.float32(b[c])) for c in "ktr"})


def test_closed_form_matches_the_first_principles_stulz(mc):
    for S, v, rho, r, t, strikes in ACCURACY_MARKETS:
        for k in strikes:
            for X in ("f64", "f32"):
                b = rounded(two_assets(S, v, rho, k, r, t), X)
                for kind in rr.KINDS:
                    got, want = mc.rainbow_closed_form(b, kind, precision=X), rr.stulz(b, kind)
                    assert abs(got - want) <= CLOSED_FORM_BOUND * max(S), (S, v, rho, k, kind, X, got, want)


def test_closed_form_against_30_digits(mc):
    """The worst difference of the four prices from a 30-digit evaluation of the same formulas, per unit of max(S_1, S_2); the
    header's bound is at least ten times the figure printed here."""
    import mpmath as mp
    mp.mp.dps = 30

    def M2(a, b, rho):
        a, b, rho = mp.mpf(a), mp.mpf(b), mp.mpf(rho)
        den = mp.sqrt(1 - rho * rho)
        f = lambda x: mp.npdf(x) * mp.ncdf((b - rho * x) / den)
        knee = b / rho if rho != 0 else a
        pts = sorted({mp.mpf(-40), min(max(knee, mp.mpf(-40)), a), a})
        return mp.quad(f, pts) if len(pts) > 1 else mp.mpf(0)

    def exact(S, v, rho, k, r, t, kind):
        S, v = [mp.mpf(x) for x in S], [mp.mpf(x) for x in v]
        rho, k, r, t = mp.mpf(rho), mp.mpf(k), mp.mpf(r), mp.mpf(t)
        st, kd = mp.sqrt(t), k * mp.exp(-r * t)
        sg = mp.sqrt(v[0] ** 2 + v[1] ** 2 - 2 * rho * v[0] * v[1])
        y = [(mp.log(S[i] / k) + (r + v[i] ** 2 / 2) * t) / (v[i] * st) for i in range(2)]
        d = (mp.log(S[0] / S[1]) + sg * sg * t / 2) / (sg * st)
        cmin = S[0] * M2(y[0], -d, -(v[0] - rho * v[1]) / sg) + S[1] * M2(y[1], d - sg * st, -(v[1] - rho * v[0]) / sg) - \
            kd * M2(y[0] - v[0] * st, y[1] - v[1] * st, rho)
        ex = S[0] * mp.ncdf(d) - S[1] * mp.ncdf(d - sg * st)
        bs = [S[i] * mp.ncdf(y[i]) - kd * mp.ncdf(y[i] - v[i] * st) for i in range(2)]
        c, pv = (bs[0] + bs[1] - cmin, S[1] + ex) if kind.endswith("max") else (cmin, S[0] - ex)
        return c if kind.startswith("call") else c - pv + kd

    worst = 0.0
    for S, v, rho, r, t, strikes in ACCURACY_MARKETS:
        L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
        rho_held = L[1, 0] / math.hypot(L[1, 0], L[1, 1])   # the correlation the factor holds
        for k in strikes:
            b = two_assets(S, v, rho, k, r, t)
            for kind in rr.KINDS:
                err = abs(mp.mpf(mc.rainbow_closed_form(b, kind)) - exact(S, v, rho_held, k, r, t, kind)) / max(S)
                worst = max(worst, float(err))
    print(f"worst |closed form - 30 digits| / max(S): {worst:.3g}")
    assert worst <= CLOSED_FORM_BOUND


def test_closed_form_against_scipy(mc):
    st = pytest.importorskip("scipy.stats")
    M2 = lambda a, b, rho: float(st.multivariate_normal.cdf([a, b], mean=[0.0, 0.0], cov=[[1.0, rho], [rho, 1.0]]))
    S, v, rho, r, t, strikes = ACCURACY_MARKETS[0]
    for k in strikes:
        b = two_assets(S, v, rho, k, r, t)
        for kind in rr.KINDS:
            assert mc.rainbow_closed_form(b, kind) == pytest.approx(rr.stulz(b, kind, M2), abs=1e-6)


def test_one_asset_is_black_scholes_and_parity_holds(mc):
    for X in ("f64", "f32"):
        b = rounded(dict(rr.market(1), k=1.1, r=-0.01), X)
        S, v, k, r, t, _ = rr.levels(b)
        for kind in rr.KINDS:   # on one asset the minimum is the maximum
            want = rr.black_scholes(S[0], k, r, v[0], t, kind.startswith("call"))
            assert mc.rainbow_closed_form(b, kind, precision=X) == pytest.approx(want, abs=1e-14)
    for S, v, rho, r, t, strikes in ACCURACY_MARKETS:
        b = two_assets(S, v, rho, strikes[1], r, t)
        f = lambda kind: mc.rainbow_closed_form(b, kind)
        kd, ex = strikes[1] * math.exp(-r * t), rr.margrabe(S[0], S[1], v[0], v[1], rho, t)
        tol = 4 * CLOSED_FORM_BOUND * max(S)
        assert f("call-on-min") - f("put-on-min") == pytest.approx(S[0] - ex - kd, abs=tol)
        assert f("call-on-max") - f("put-on-max") == pytest.approx(S[1] + ex - kd, abs=tol)
        # min + max = the two assets: the calls add up to the two Black-Scholes calls
        assert f("call-on-min") + f("call-on-max") == pytest.approx(sum(rr.black_scholes(S[i], strikes[1], r, v[i], t) for i in range(2)), abs=tol)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_refusals(mc, X):
    ok = rr.market(2)
    assert mc.rainbow_closed_form(ok, "put-on-min", precision=X) > 0
    bad = [dict(ok, s=np.array([0.0, 1.0])), dict(ok, w=np.array([1.0, -1.0])), dict(ok, v=np.array([0.2, -0.1])), dict(ok, v=np.array([0.0, 0.2])),
           dict(ok, t=0.0), dict(ok, r=float("nan")), dict(ok, k=float("inf")), dict(ok, k=0.0), dict(ok, d=np.array([0.0, 0.1])),
           dict(ok, v=np.array([0.2, 0.2]), p=np.array([[1.0, 0.0], [1.0, 0.0]])), rr.market(3),
           dict(ok, p=np.array([[1.0, 0.0], [0.5, 0.5]])), dict(ok, p=np.array([[1.1, 0.0], [0.6, 0.8]])),   # rows not of unit length
           dict(rr.market(1), p=np.array([[0.9]]))]
    for b in bad:
        with pytest.raises(mc.McError, match="mc error 1"):   # MC_ERR_INVALID
            mc.rainbow_closed_form(b, "put-on-min", precision=X)
    for kind in (4, -1):
        with pytest.raises(mc.McError, match="mc error 1"):
            mc.rainbow_closed_form(ok, kind, precision=X)
    with pytest.raises(mc.McError, match="none with a barrier"):
        mc.rainbow_closed_form(ok, "put-on-min", 0.7, "down-and-in", precision=X)
    # n_dates is ignored
    L = mc._lib
    from montecarlocuda_amd.engine import _RainbowHolder
    h, price = _RainbowHolder(X, ok, 1, "put-on-min"), C.c_double()
    f = getattr(L.lib(), f"mc_rainbow_closed_form_{X}")
    assert f(C.byref(h.struct), C.byref(price)) == 0
    a = price.value
    h.struct.n_dates = -5
    assert f(C.byref(h.struct), C.byref(price)) == 0 and price.value == a
    assert f(None, C.byref(price)) == 1
    assert mc.rainbow_closed_form(ok, "put-on-min", precision=X) == pytest.approx(a)   # and the next call is served


def test_one_factor_quadrature_matches_stulz():
    for b in (rr.market(2), dict(rr.market(2), k=1.2, r=-0.01, t=2.0)):
        for kind in rr.KINDS:
            assert rr.one_factor(b, rr.betas(2), kind) == pytest.approx(rr.stulz(b, kind), abs=1e-7)


MC_PATHS, MC_CHUNK = 1 << 20, 1 << 16


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("m", [1, 16])
def test_reference_model_prices_the_exact_european_at_any_date_count(n, m):
    """2^20 numpy paths of the model: the walk's law and the layout-independent maths."""
    b = rr.market(n)
    rng = np.random.default_rng(20261019 + 100 * n + m)
    acc = {kind: [0.0, 0.0] for kind in rr.KINDS}
    for _ in range(MC_PATHS // MC_CHUNK):
        z = rng.standard_normal((MC_CHUNK, m, n))
        for kind in rr.KINDS:
            v = rr.rainbow(b, m, z, kind).value[0]
            acc[kind][0] += v.sum()
            acc[kind][1] += (v * v).sum()
    disc = math.exp(-b["r"] * b["t"])
    for kind, (s1, s2) in acc.items():
        mean = s1 / MC_PATHS
        price, half = disc * mean, 1.96 * disc * math.sqrt(max(s2 / MC_PATHS - mean * mean, 0.0) / (MC_PATHS - 1))
        exact = rr.one_factor(b, rr.betas(n), kind)
        print(f"n={n} m={m} {kind}: {price:.6f} +- {half:.2g}, exact {exact:.6f}: {abs(price - exact) / half:.2f} half-widths")
        assert abs(price - exact) <= 3 * half, (n, m, kind, price, exact, half)


@pytest.fixture(scope="module")
def shape_normals():
    """numpy normals for the shapes of the GPU test: N_PATHS paths of the largest table, shared and left unchanged."""
    z = np.random.default_rng(14).standard_normal((rr.N_PATHS, rr.MAX_TABLE))
    z.setflags(write=False)
    return z


def normals_of(shape_normals, n, m):
    return shape_normals[:, :n * m].reshape(rr.N_PATHS, m, n)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_model_identities_on_every_path(shape_normals, n):
    for m in (1, 5, 64):
        z = normals_of(shape_normals, n, m)
        for b, kind, B, up in rr.cases(n):
            for anti in (False, True):
                sides = rr.walk(b, m, z, kind, B, up, anti)
                k_out, k_in = rr.kinds_of(up)
                free = rr.value(sides).value[0]
                assert np.array_equal(rr.value(sides, k_out).value[0] + rr.value(sides, k_in).value[0], free)
        # min <= every asset <= max, on the terminal levels: the put on the minimum pays at least the put on any single asset
        b = rr.market(n)
        lo, hi = rr.rainbow(b, m, z, "put-on-min").value[0], rr.rainbow(b, m, z, "put-on-max").value[0]
        for i in range(n):
            one = dict(s=b["s"][i:i + 1], v=b["v"][i:i + 1], w=b["w"][i:i + 1], p=np.ones((1, 1)), d=np.zeros(1), k=b["k"], t=b["t"], r=b["r"])
            L = np.asarray(b["p"])
            zi = (z @ L[i])[:, :, None]   # asset i's own normals: the factor's row has unit length
            single = rr.rainbow(one, m, zi, "put-on-min").value[0]
            assert np.all(lo >= single - 1e-12) and np.all(hi <= single + 1e-12)


def test_one_asset_is_the_barrier_call_on_the_same_normals(shape_normals):
    for m in (1, 7, 64):
        z = normals_of(shape_normals, 1, m)
        for o, B in br.CASES:
            b = dict(s=np.array([o["s"]]), v=np.array([o["v"]]), w=np.ones(1), p=np.ones((1, 1)), d=np.zeros(1), k=o["k"], t=o["t"], r=o["r"])
            for kind in br.kinds_of(o, B):
                for anti in (False, True):
                    got, want = rr.rainbow(b, m, z, "call-on-max", B, kind, anti), br.barrier(o, B, m, z[:, :, 0], kind, "discrete", anti)
                    assert np.allclose(got.value[0], want.value[0], rtol=0, atol=1e-11 * o["s"])
                    assert np.array_equal(got.value[0] > 0, want.value[0] > 0)


def test_a_barrier_at_one_date_is_the_terminal_condition(shape_normals):
    n = 3
    z = normals_of(shape_normals, n, 1)
    for b, kind, B, up in rr.cases(n):
        free = rr.rainbow(b, 1, z, kind).value[0]
        ln_s, a, M = rr.fold(b, 1)
        y = ln_s + a + z[:, 0, :] @ M.T
        X = np.exp(y.max(axis=1) if kind.endswith("max") else y.min(axis=1))
        live = X < B if up else X > B
        assert np.array_equal(rr.rainbow(b, 1, z, kind, B, rr.kinds_of(up)[0]).value[0], np.where(live, free, 0.0))


def walk_f32(b, m, z, kind, B, up, knock_in, anti):
    """The walk in float32 arithmetic, in the order the header states it (constants folded in fp64 and rounded once)."""
    f = np.float32
    ln_s, a, M = rr.fold(b, m)
    e, q = (1.0 if kind.endswith("max") else -1.0), (1.0 if kind.startswith("call") else -1.0)
    j = np.arange(1, m + 1, dtype=np.float64)
    tab = (e * (ln_s[None, :] + j[:, None] * a[None, :])).astype(f)
    Me = (e * M).astype(f)
    W = np.cumsum(z.astype(f), axis=1, dtype=f)
    sgn = 1.0 if up else -1.0
    out = np.zeros(z.shape[0])
    for sign in ((1.0, -1.0) if anti else (1.0,)):
        cs = np.zeros(W.shape, dtype=f)
        for k in range(M.shape[0]):
            cs += Me[None, None, :, k] * W[:, :, k:k + 1]
        Y = (tab[None] + f(sign) * cs).max(axis=2)
        d = f(-sgn * e) * Y + f(sgn * math.log(B))
        P = (d.min(axis=1) > 0).astype(f)
        X = np.exp2(f(e * 1.4426950408889634) * Y[:, -1]).astype(f)
        pay = np.maximum(f(q) * (X - f(b["k"])), f(0))
        out += ((f(1) - P) if knock_in else P) * pay / (2.0 if anti else 1.0)
    return out


@pytest.mark.parametrize("n", rr.ASSETS)
def test_a_float32_walk_stays_inside_the_bound_on_every_shape(shape_normals, n):
    tol = TOL["f32"]["pay"]
    for m in rr.DATES(n):
        z = normals_of(shape_normals, n, m).astype(np.float32).astype(np.float64)
        for b, kind, B, up in rr.cases(n) + ([rr.ABSOLUTE] if n == 3 else []):
            for anti in (False, True):
                sides = rr.walk(b, m, z, kind, B, up, anti)
                for bk in rr.kinds_of(up):
                    p = rr.value(sides, bk)
                    got = walk_f32(b, m, z, kind, B, up, bk.endswith("in"), anti)
                    assert np.all(np.abs(got - p.value[0]) <= gr.bound(p, tol)[0]), (n, m, kind, bk, anti)


def test_the_bound_rejects_five_wrong_walks(shape_normals):
    """Each outside the fp32 bound on more than 0.40 of the paths of a case where most paths are in the money: the worst-of-5
    knock-in put struck at 1 with the barrier at 0.95, at three dates (one date for the late barrier, whose other dates agree)."""
    n, tol = 5, TOL["f32"]["pay"]
    b, kind, B, bk = rr.market(n), "put-on-min", 0.95, "down-and-in"

    def share(m, z_wrong=None, kind_wrong=kind, mutate=None):
        z = normals_of(shape_normals, n, m)
        p = rr.rainbow(b, m, z, kind, B, bk)
        assert (p.value[0] > 0).mean() > 0.5
        wrong = rr.rainbow(b, m, z if z_wrong is None else z_wrong, kind_wrong, B, bk, mutate=mutate)
        return float((np.abs(wrong.value[0] - p.value[0]) > gr.bound(p, tol)[0]).mean())

    date_minor = shape_normals[:, :n * 3].reshape(rr.N_PATHS, n, 3).transpose(0, 2, 1)
    shares = {"min read as max": share(3, kind_wrong="put-on-max"), "M transposed": share(3, mutate="transpose"),
              "normals read date-minor": share(3, z_wrong=date_minor), "barrier one date late": share(1, mutate="late"),
              "j a_i with j zero-based": share(3, mutate="zero-based")}
    print(shares)
    for what, s in shares.items():
        assert s > 0.40, (what, s)


@pytest.mark.parametrize("n", rr.ASSETS)
def test_few_paths_carry_a_jump_term(shape_normals, n):
    """Per path direction: none at the fp64 tolerance; at the fp32 tolerance at most 0.05 of a shape up to 64 dates and at most
    0.5 above, where the GPU test's check of the two possible values is what keeps those paths tested."""
    for m in rr.DATES(n):
        z = normals_of(shape_normals, n, m)
        cap = 0.05 if m <= 64 else 0.5
        for b, kind, B, up in rr.cases(n) + ([rr.ABSOLUTE] if n == 3 else []):
            for zz in (z, -z):
                p = rr.rainbow(b, m, zz, kind, B, rr.kinds_of(up)[0])
                share32, share64 = float((p.edge <= TOL["f32"]["pay"]).mean()), float((p.edge <= TOL["f64"]["pay"]).mean())
                print(f"n={n} m={m} {kind} B={B}: share of paths with a jump term {share32:.3g} (fp32), {share64:.3g} (fp64)")
                assert share32 <= cap, (n, m, kind, share32)
                assert share64 == 0.0, (n, m, kind, share64)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, basket), offsetof(T, barrier), offsetof(T, n_dates), offsetof(T, type), offsetof(T, barrier_type)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %u %d %d %d %d %d\n", ROW(mc_rainbow_f32), ROW(mc_rainbow_f64),
         MC_MAX_RAINBOW_ASSETS, MC_MAX_RAINBOW_TABLE, MC_DOMAIN_RAINBOW, MC_RAINBOW_CALL_ON_MIN, MC_RAINBOW_CALL_ON_MAX,
         MC_RAINBOW_PUT_ON_MIN, MC_RAINBOW_PUT_ON_MAX, MC_RAINBOW_NO_BARRIER);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.basket.offset, T.barrier.offset, T.n_dates.offset, T.type.offset, T.barrier_type.offset]
    assert got == row(L.RainbowF32) + row(L.RainbowF64) + [L.MAX_RAINBOW_ASSETS, L.MAX_RAINBOW_TABLE, L.DOMAIN_RAINBOW] + \
        [L.RAINBOW_TYPES[k] for k in rr.KINDS] + [L.RAINBOW_NO_BARRIER]
    assert L.MAX_RAINBOW_TABLE == rr.MAX_TABLE and L.DOMAIN_RAINBOW == rr.DOMAIN_RAINBOW and max(rr.ASSETS) == L.MAX_RAINBOW_ASSETS
    assert "rainbow_closed_form" in mc.__all__
