"""The lookback options without a GPU: the closed forms (mc_lookback_closed_form_*, plain C in mc_hostmath_impl.h) against a numerical
quadrature of the running extremum's law (lookback_ref.quadrature_price); the float64 reference model lookback_ref.py on numpy's
own normals and uniforms -- its identities per path, and the continuous form against the closed forms at 1 and 16 dates, which
is the guard on the bridge formula itself; the soundness of the model's forward-error scale (a float32 evaluation of the same
formulas stays inside the bound on every path of every shape of tests/test_gpu_lookback.py) and its power (three mutations fall
outside it); the uniforms' arithmetic; the refusals that need no device; the structs' layout.

The Monte Carlo check uses ONE fixed seed and 3 half-widths (1.96 sigma / sqrt(n) each, so 5.9 sigma): the margin is for nothing
but sampling noise."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import lookback_ref as lr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

NEG_R = dict(s=237.5, k=213.75, r=-0.015, v=0.17, t=1.3)
MARKETS = lr.CASES + [NEG_R]
MC_PATHS, MC_CHUNK = 1 << 20, 1 << 17


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def rounded(o, X):
    """The market as the precision's struct holds it."""
    f = (lambda x: float(np.float32(x))) if X == "f32" else float
    return {c: f(x) for c, x in o.items()}


# ---- the closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_matches_the_quadrature_of_the_extremums_law(mc, X):
    """1e-7 relative: the quadrature's own accuracy."""
    strikes = set()
    for o in MARKETS + [dict(lr.ATM, k=120.0), dict(lr.ATM, k=80.0)]:
        q = rounded(o, X)
        strikes.add((o["k"] > o["s"]) - (o["k"] < o["s"]))
        for kind in lr.KINDS:
            got, want = mc.lookback_closed_form(q, kind, X), lr.quadrature_price(q, kind)
            print(f"{X} {o} {kind}: closed form {got:.9f} quadrature {want:.9f}")
            assert abs(got - want) <= 1e-7 * abs(want), (o, kind, got, want)
    assert strikes == {-1, 0, 1}   # both branches of the fixed-strike formulas, and their common point


def test_closed_form_orders_and_parities(mc):
    f = lambda kind, o=lr.ATM: mc.lookback_closed_form(o, kind)
    s, k, r, t = (lr.ATM[c] for c in "skrt")
    D = math.exp(-r * t)
    # at the money the fixed types are the floating ones plus the forward's leg (the formulas' first branches)
    assert f("fixed-call") == pytest.approx(f("floating-put") + s - D * k, rel=1e-14)
    assert f("fixed-put") == pytest.approx(f("floating-call") - s + D * k, rel=1e-14)
    # the issue's digits, to the five decimals it prints
    assert [round(f(kind), 5) for kind in lr.KINDS] == [17.21680, 14.29057, 19.16763, 12.33974]
    # a lookback is worth more than the vanilla option it dominates path by path
    sd = 0.2
    d1 = (r + 0.5 * 0.04) / sd
    call = s * 0.5 * math.erfc(-d1 / math.sqrt(2)) - k * D * 0.5 * math.erfc(-(d1 - sd) / math.sqrt(2))
    assert f("fixed-call") > call and f("floating-call") > call


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_refusals(mc, X):
    ok = lr.ATM
    for kind in lr.KINDS:
        assert mc.lookback_closed_form(ok, kind, X) > 0
    INVALID = "mc error 1"
    for bad in (dict(ok, s=0.0), dict(ok, t=0.0), dict(ok, v=-0.1), dict(ok, v=0.0), dict(ok, r=float("nan")), dict(ok, r=0.0),
                dict(ok, s=float("inf"))):
        for kind in lr.KINDS:
            with pytest.raises(mc.McError, match=INVALID):
                mc.lookback_closed_form(bad, kind, X)
    with pytest.raises(mc.McError, match="r -> 0"):
        mc.lookback_closed_form(dict(ok, r=0.0), "floating-put", X)
    for bad_k in (0.0, -1.0, float("inf"), float("nan")):
        for kind in ("fixed-call", "fixed-put"):
            with pytest.raises(mc.McError, match="finite k > 0"):
                mc.lookback_closed_form(dict(ok, k=bad_k), kind, X)
        for kind in ("floating-call", "floating-put"):   # k is ignored by the floating types
            assert mc.lookback_closed_form(dict(ok, k=bad_k), kind, X) == mc.lookback_closed_form(ok, kind, X)
    for kind in (4, -1):
        with pytest.raises(mc.McError, match=INVALID):
            mc.lookback_closed_form(ok, kind, X)
    # n_dates and monitoring are ignored by the formula
    L = mc._lib
    price = C.c_double()
    f = getattr(L.lib(), f"mc_lookback_closed_form_{X}")
    opt = L.OPTION[X](100.0, 100.0, 0.05, 0.2, 1.0)
    assert f(C.byref(L.LOOKBACK[X](opt, 1, 2, 0)), C.byref(price)) == 0
    a = price.value
    for n_dates, mon in ((4096, 1), (0, 0), (-7, 5)):
        assert f(C.byref(L.LOOKBACK[X](opt, n_dates, 2, mon)), C.byref(price)) == 0 and price.value == a
    assert f(None, C.byref(price)) == 1
    assert f(C.byref(L.LOOKBACK[X](opt, 1, 2, 0)), None) == 1
    assert mc.lookback_closed_form(ok, "fixed-call", X) == pytest.approx(a)   # and the next call is served


# ---- the model on numpy draws -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_draws():
    """numpy normals and uniforms for the shapes of the GPU test: N_PATHS paths of the largest date count, shared and left unchanged.
    The uniforms are float32 values in (0, 1], some of them next to 1 and exactly 1: where E_j is next to 0."""
    rng = np.random.default_rng(11)
    z = rng.standard_normal((lr.N_PATHS, max(lr.DATES))).astype(np.float32)
    u = lr.u01_f32(rng.integers(0, 1 << 32, size=z.shape, dtype=np.uint64).astype(np.uint32))
    u[::7, ::5] = np.float32(1.0) - np.float32(2.0 ** -24) * rng.integers(0, 4, size=u[::7, ::5].shape).astype(np.float32)
    z.setflags(write=False)
    u.setflags(write=False)
    return z, u


def test_one_date_discrete(shape_draws):
    z, u = shape_draws
    for o, anti in ((o, anti) for o in lr.CASES for anti in (False, True)):
        for kind in ("floating-call", "floating-put"):
            assert np.all(lr.lookback(o, 1, z, None, kind, "discrete", anti).value[0] == 0.0)   # the extremum IS the terminal spot
        s0, k, r, v, t = (o[c] for c in "skrvt")
        ST = s0 * np.exp((r - 0.5 * v * v) * t + v * math.sqrt(t) * z[:, 0].astype(np.float64))
        assert np.allclose(lr.lookback(o, 1, z, None, "fixed-call", "discrete").value[0], np.maximum(ST - k, 0.0), rtol=1e-13, atol=1e-12)
        assert np.allclose(lr.lookback(o, 1, z, None, "fixed-put", "discrete").value[0], np.maximum(k - ST, 0.0), rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("m", [1, 2, 7, 64, 257])
def test_identities_per_path(shape_draws, m):
    z, u = shape_draws
    for o in lr.CASES:
        s0, k = o["s"], o["k"]
        up = {mon: lr.walk(o, m, z, u, True, mon) for mon in lr.MONITORINGS}
        dn = {mon: lr.walk(o, m, z, u, False, mon) for mon in lr.MONITORINGS}
        for mon in lr.MONITORINGS:
            mx, mn, ST = up[mon][0]["ext"], dn[mon][0]["ext"], up[mon][0]["ST"]
            assert np.array_equal(ST, dn[mon][0]["ST"]) or np.allclose(ST, dn[mon][0]["ST"], rtol=1e-15)
            # the same bridge draws feed both extremes here: the maximum and the minimum are each marginally exact, and the sum of the
            # two floating values is max S - min S in either monitoring
            put, call = lr.value(up[mon], "floating-put", k).value[0], lr.value(dn[mon], "floating-call", k).value[0]
            assert np.allclose(put + call, mx - mn, rtol=1e-13, atol=1e-12)
            assert np.all(mx >= ST * (1 - 1e-15)) and np.all(mn <= ST * (1 + 1e-15))
            assert np.allclose(lr.value(up[mon], "fixed-call", k).value[0], np.maximum(mx - k, 0.0), rtol=0, atol=0)
            assert np.allclose(lr.value(dn[mon], "fixed-put", k).value[0], np.maximum(k - mn, 0.0), rtol=0, atol=0)
            if mon == "continuous":
                assert np.all(mx >= s0) and np.all(mn <= s0)   # t_0 is included
        # continuous >= discrete on every path, every type
        for kind, w in (("floating-put", up), ("fixed-call", up), ("floating-call", dn), ("fixed-put", dn)):
            assert np.all(lr.value(w["continuous"], kind, k).value[0] >= lr.value(w["discrete"], kind, k).value[0])
        # the antithetic value is the mean of the two directions
        both = lr.lookback(o, m, z, u, "fixed-call", "continuous", True).value[0]
        one, other = (lr.lookback(o, m, zz, u, "fixed-call", "continuous").value[0] for zz in (z, -z.astype(np.float64)))
        assert np.allclose(both, 0.5 * (one + other), rtol=1e-15, atol=0)


@pytest.mark.parametrize("m", [1, 16])
def test_reference_model_prices_the_continuous_lookbacks_at_any_date_count(mc, m):
    """2^20 numpy paths, one seed: each type within 3 half-widths of the closed form; the discrete form at 16 dates lies below."""
    rng = np.random.default_rng(20241019 + m)
    o = lr.ATM
    acc = {(kind, mon): [0.0, 0.0] for kind in lr.KINDS for mon in lr.MONITORINGS}
    for _ in range(MC_PATHS // MC_CHUNK):
        z, u = rng.standard_normal((MC_CHUNK, m)), 1.0 - rng.random((MC_CHUNK, m))
        for mon in lr.MONITORINGS:
            walks = {True: lr.walk(o, m, z, u, True, mon), False: lr.walk(o, m, z, u, False, mon)}
            for kind in lr.KINDS:
                v = lr.value(walks[lr.ON_MAX[kind]], kind, o["k"]).value[0]
                acc[kind, mon][0] += v.sum()
                acc[kind, mon][1] += (v * v).sum()
    disc, n = math.exp(-o["r"] * o["t"]), MC_PATHS
    for kind in lr.KINDS:
        est = {}
        for mon in lr.MONITORINGS:
            mean = acc[kind, mon][0] / n
            est[mon] = (disc * mean, 1.96 * disc * math.sqrt(max(acc[kind, mon][1] / n - mean * mean, 0.0) / (n - 1)))
        exact = mc.lookback_closed_form(o, kind)
        price, half = est["continuous"]
        print(f"m={m} {kind}: continuous {price:.5f} +- {half:.2g}, exact {exact:.5f} ({abs(price - exact) / half:.2f} half-widths); discrete {est['discrete'][0]:.5f}")
        assert abs(price - exact) <= 3 * half, (kind, price, exact, half)
        assert est["discrete"][0] < exact - 3 * est["discrete"][1]   # the monitoring bias that the bridge removes


# ---- the scale: sound and sharp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", lr.DATES)
def test_a_float32_evaluation_stays_inside_the_bound(shape_draws, m):
    tol = TOL["f32"]["pay"]
    assert tol == lr.EPS["f32"] and TOL["f64"]["pay"] == lr.EPS["f64"]
    worst = 0.0
    shapes = [(o, shape_draws) for o in lr.CASES]
    if m in lr.TRIP_DATES:   # the shapes of tests/test_gpu_walk_trips.py: the path counts of its ranges, each on the market it rotates to
        rng = np.random.default_rng(70 + m)
        for name in ("A", "C"):
            n = gr.TRIP_RANGES[name].n
            draws = rng.standard_normal((n, m)).astype(np.float32), lr.u01_f32(rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64).astype(np.uint32))
            shapes.append((gr.trip_pick(lr.CASES, lr.TRIP_DATES.index(m), name), draws))
    for o, (z, u) in shapes:
        q = rounded(o, "f32")
        for mon in lr.MONITORINGS:
            for anti in (False, True):
                walks = {side: lr.walk(q, m, z, u, side, mon, anti, tol) for side in (True, False)}
                for kind in lr.KINDS:
                    p = lr.value(walks[lr.ON_MAX[kind]], kind, q["k"])
                    got = lr.lookback_f32(q, m, z, u, kind, mon, anti).astype(np.float64)
                    b = gr.bound(p, tol)[0]
                    assert gr.kink_free(p, 1.0) and np.all(p.jump == 0)
                    err = np.abs(got - p.value[0])
                    assert np.all(np.isfinite(got)) and np.all(err <= b), (o, m, kind, mon, anti, int(np.argmax(err - b)), float((err / b).max()))
                    worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    print(f"m={m}: worst float32 error / bound {worst:.3g}")


@pytest.mark.parametrize("m", [2, 16, 257])
def test_the_bound_rejects_three_mutations(shape_draws, m):
    """At the weaker (fp32) tolerance, on more than 0.40 of the paths of a continuous shape (the share of tests/test_heston_ref.py)."""
    z, u = shape_draws
    tol = TOL["f32"]["pay"]
    for o in lr.CASES:
        for kind in ("floating-put", "floating-call"):   # one on the maximum, one on the minimum
            p = lr.lookback(o, m, z, u, kind, "continuous", False, tol)
            b = gr.bound(p, tol)[0]
            for mutation in ("half_e", "next_bridge", "min_for_max"):
                mutant = lr.lookback(o, m, z, u, kind, "continuous", False, tol, mutation).value[0]
                share = float((np.abs(mutant - p.value[0]) > b).mean())
                print(f"m={m} {kind} {mutation}: outside the bound on {share:.3f} of the paths")
                assert share > 0.40, (o, m, kind, mutation, share)


# ---- the uniforms -----------------------------------------------------------------------------------------------------------
def test_uniforms_restate_the_devices_arithmetic():
    ends = np.array([0, 1, (1 << 32) - 1, (1 << 32) - 2, 0x7FFFFFFF, 0x80000000, 0x00FFFFFF, 0x01000001], dtype=np.uint32)
    u = lr.u01_f32(ends)
    assert u.dtype == np.float32
    assert float(u[0]) == 2.0 ** -33 and float(u[2]) == 1.0   # (2^32 - 1) rounds to 2^32 as a float: u = 1 exactly, E = 0
    assert float(u[1]) == 1.5 * 2.0 ** -32
    rng = np.random.default_rng(3)
    w = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    u = lr.u01_f32(np.concatenate([ends, w]))
    assert np.all(u > 0) and np.all(u <= 1)
    # the fma form against exact rational arithmetic on a sample
    for x in [int(v) for v in np.concatenate([ends, w[:2000]])]:
        xf = float(np.float32(x))
        assert float(lr.u01_f32(np.uint32(x))) == float(np.float32(xf * 2.0 ** -32 + 2.0 ** -33))
    lo = np.concatenate([np.array([0, 0xFFFFFFFF, 0, 0xFFFFFFFF], dtype=np.uint32), w[: 1 << 19]])
    hi = np.concatenate([np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0], dtype=np.uint32), w[1 << 19:]])
    d = lr.u01_f64(lo, hi)
    assert d[0] == 2.0 ** -53 and d[1] == 1.0 - 2.0 ** -53
    assert np.all(d > 0) and np.all(d < 1)
    assert lr.u01_f64(np.uint32(0xFFF), np.uint32(0)) == 2.0 ** -53   # the low 12 bits are dropped
    assert lr.u01_f64(np.uint32(0x1000), np.uint32(0)) == 1.5 * 2.0 ** -52
    # the stream rule: which words make which date's uniform
    words = np.arange(2 * 3 * 4, dtype=np.uint32).reshape(2, 3, 4) * np.uint32(0x01010101)
    u32 = lr.bridge_uniforms(words, 9, "f32")
    assert u32.shape == (2, 9) and u32[1, 5] == float(lr.u01_f32(words[1, 1, 1]))
    u64 = lr.bridge_uniforms(words, 5, "f64")
    assert u64.shape == (2, 5) and u64[1, 3] == lr.u01_f64(words[1, 1, 2], words[1, 1, 3]) and u64[0, 4] == lr.u01_f64(words[0, 2, 0], words[0, 2, 1])
    assert [lr.bridge_blocks(m, "f32") for m in (1, 4, 5)] == [1, 1, 2] and [lr.bridge_blocks(m, "f64") for m in (1, 2, 3)] == [1, 1, 2]


# ---- the header -------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, n_dates), offsetof(T, type), offsetof(T, monitoring)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %u %u %d %d %d %d %d\n", ROW(mc_lookback_f32), ROW(mc_lookback_f64),
         MC_MAX_LOOKBACK_DATES, MC_DOMAIN_LOOKBACK, MC_DOMAIN_LOOKBACK_BRIDGE, MC_LOOKBACK_FLOAT_CALL, MC_LOOKBACK_FLOAT_PUT,
         MC_LOOKBACK_FIXED_CALL, MC_LOOKBACK_FIXED_PUT, MC_STREAM_VERSION);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.n_dates.offset, T.type.offset, T.monitoring.offset]
    assert got == row(L.LookbackF32) + row(L.LookbackF64) + [L.MAX_LOOKBACK_DATES, L.DOMAIN_LOOKBACK, L.DOMAIN_LOOKBACK_BRIDGE] + \
        [L.LOOKBACK_TYPES[k] for k in lr.KINDS] + [2]
    assert L.MAX_LOOKBACK_DATES == max(lr.DATES) and (L.DOMAIN_LOOKBACK, L.DOMAIN_LOOKBACK_BRIDGE) == (lr.DOMAIN_LOOKBACK, lr.DOMAIN_LOOKBACK_BRIDGE)
    assert "lookback_closed_form" in mc.__all__
