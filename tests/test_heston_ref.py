"""The Heston call without a GPU: the closed form (mc_heston_closed_form_*, plain C in mc_hostmath.c) against the second, independent
quadrature of heston_ref.py, its limits and bounds; the float64 reference model heston_ref.py itself -- how many paths of the shapes
of tests/test_gpu_heston.py are kink paths (the cap is a condition: at most KINK_CAP of any parametrisation), that the truncation
branch is really taken, that a float32 evaluation of the same formulas stays within the per-path bound and that four mutations of
the step break it; the refusals that need no device; the structs' layout."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import heston_ref as hr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CLOSED_FORM_ACCURACY = 1e-11   # absolute, at S = 100: what include/mc_mi355x.h states for mc_heston_closed_form_*
STRIKES = (70.0, 90.0, 100.0, 110.0, 140.0)
BROADIE_KAYA = (dict(s=100.0, k=100.0, r=0.0319, t=1.0), dict(v0=0.010201, kappa=6.21, theta=0.019, xi=0.61, rho=-0.7), 6.8061)


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def rounded(d, X):
    """Inputs as the precision's struct holds them."""
    return {c: float(np.float32(x)) if X == "f32" else float(x) for c, x in d.items()}


def numpy_normals(m, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, m)), rng.standard_normal((n, m))


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", hr.STEPS)
def test_kink_paths_stay_under_the_cap_on_the_shapes_of_the_gpu_test(m):
    """The cap is a condition on the test's shapes, not a measurement: exactly the (case, m, precision) set of the GPU test, on
    numpy normals, both path directions."""
    n = (4 if m < 1024 else 2) * hr.n_paths_for(m)
    shapes = [(case, n) for case in hr.cases_for(m)]
    if m in hr.TRIP_STEPS:   # the shapes of tests/test_gpu_walk_trips.py: the path counts of its ranges, each on the case it rotates to
        shapes += [(gr.trip_pick(hr.CASES, hr.TRIP_STEPS.index(m), name), gr.TRIP_RANGES[name].n) for name in ("A", "C")]
    for (name, mkt, model), n in shapes:
        z1, z2 = numpy_normals(m, n, 1000 + m)
        p = hr.walk(mkt, model, m, z1, z2, anti=True)
        for X in ("f32", "f64"):
            if not hr.runs(name, X, m):
                continue
            b, kink = hr.bound(p, TOL[X]["pay"])
            assert np.all(np.isfinite(b[~kink])) and np.all(b > 0)
            print(f"{name} m={m} {X}: {kink.mean():.2%} kink paths, {hr.truncated(p).mean():.2%} truncated")
            assert kink.mean() <= hr.KINK_CAP, (name, m, X, kink.mean())
            if X == "f64":
                assert not kink.any(), (name, m)
        if name == "STRONG" and m >= 16:   # far from zero once the step is short: a clean case in both precisions
            assert not hr.bound(p, TOL["f32"]["pay"])[1].any()


def test_the_excluded_shapes_are_excluded_for_a_reason():
    """VIOLATED in fp32 beyond VIOLATED_F32_MAX_STEPS is over the cap (so it is left out, the cap is not raised)."""
    m = 256
    z1, z2 = numpy_normals(m, 4000, 5)
    _, kink = hr.bound(hr.walk(hr.OTM, hr.VIOLATED, m, z1, z2, anti=True), TOL["f32"]["pay"])
    assert kink.mean() > hr.KINK_CAP
    assert [m for m in hr.STEPS if not hr.runs("VIOLATED", "f32", m)] == [m for m in hr.STEPS if m > 64]
    assert all(hr.runs(name, X, m) for name in ("STRONG", "FELLER", "POSRHO") for X in ("f32", "f64") for m in hr.STEPS)
    assert all(hr.runs("VIOLATED", "f64", m) for m in hr.STEPS)


@pytest.mark.parametrize("m", [16, 64, 257])
def test_the_truncation_branch_is_taken(m):
    z1, z2 = numpy_normals(m, 20_000, 11)
    share = {name: hr.truncated(hr.walk(hr.ATM, model, m, z1, z2)).mean() for name, model in hr.MODELS.items()}
    print(m, share)
    assert share["VIOLATED"] >= 0.5
    assert share["STRONG"] == 0.0
    assert 0.0 < share["FELLER"] < share["VIOLATED"]


@pytest.mark.parametrize("m", [1, 2, 16, 64, 257])
def test_a_float32_evaluation_stays_within_the_bound(m):
    """The same formulas in numpy float32 (its own association: running sums by cumsum) on float32 normals: every path of every
    case, kink paths included, within bound(., TOL f32)."""
    n = 4000
    z1, z2 = (z.astype(np.float32).astype(np.float64) for z in numpy_normals(m, n, 21))
    for name, mkt, model in hr.CASES:
        for anti in (False, True):
            p = hr.walk(mkt, model, m, z1, z2, anti)
            q = hr.walk(mkt, model, m, z1, z2, anti, dtype=np.float32)
            b, kink = hr.bound(p, TOL["f32"]["pay"])
            r = np.abs(q.value[0] - p.value[0]) / b
            print(f"{name} m={m} anti={anti}: worst err/bound {r.max():.3g}, {int(kink.sum())} kink paths")
            assert np.all(r <= 1.0), (name, m, anti, float(r.max()))


@pytest.mark.parametrize("mutation", hr.MUTATIONS)
@pytest.mark.parametrize("m", [16, 64])
def test_the_bound_rejects_a_mutated_step(mutation, m):
    """Each mutation, evaluated in float64 on VIOLATED at the money (about 70 % of the paths end in the money, nearly all are
    truncated somewhere), changes the formula by O(1) on every path it touches: it must leave the fp32 bound on more than 40 %
    of the paths -- more than half of those in the money."""
    z1, z2 = numpy_normals(m, 4000, 31)
    p = hr.walk(hr.ATM, hr.VIOLATED, m, z1, z2)
    b, _ = hr.bound(p, TOL["f32"]["pay"])
    q = hr.walk(hr.ATM, hr.VIOLATED, m, z1, z2, mutation=mutation)
    share = (np.abs(q.value[0] - p.value[0]) > b).mean()
    print(mutation, m, share)
    assert share > 0.40, (mutation, m, share)


def test_one_step_is_the_vanilla_payoff_at_the_starting_volatility():
    z1, z2 = numpy_normals(1, 1000, 41)
    for name, mkt, model in hr.CASES:
        got = hr.walk(mkt, model, 1, z1, z2).value[0]
        v = math.sqrt(model["v0"])
        want = np.maximum(mkt["s"] * np.exp((mkt["r"] - 0.5 * v * v) * mkt["t"] + v * math.sqrt(mkt["t"]) * z1[:, 0]) - mkt["k"], 0.0)
        assert np.allclose(got, want, rtol=1e-13, atol=1e-12)


def test_euler_variance_path():
    V, var = hr.euler_variance_path(dict(hr.FELLER, v0=0.09, xi=0.0), 4, 1.0)
    assert V.tolist() == pytest.approx([0.09, 0.09 + 2.0 * (0.04 - 0.09) * 0.25, 0.065 + 2.0 * (0.04 - 0.065) * 0.25, 0.0525 + 2.0 * (0.04 - 0.0525) * 0.25])
    assert var == pytest.approx(V.sum() * 0.25)


# ---- the closed form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_matches_the_independent_quadrature(mc, X):
    worst = 0.0
    for name, mkt, model in hr.CASES:
        for k in STRIKES:
            o, md = rounded(dict(mkt, k=k), X), rounded(model, X)
            got, want = mc.heston_closed_form(o, md, X), hr.closed_form(o, md)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= CLOSED_FORM_ACCURACY, (name, k, got, want)
    print(f"{X}: worst |C - Python| {worst:.3g}")


def test_closed_form_limits(mc):
    for name, mkt, model in hr.CASES:
        kt = model["kappa"] * mkt["t"]
        w = model["theta"] + (model["v0"] - model["theta"]) * (1.0 - math.exp(-kt)) / kt
        assert mc.heston_closed_form(mkt, dict(model, xi=0.0)) == pytest.approx(hr.black_scholes_call(dict(mkt, v=math.sqrt(w))), rel=1e-13)
        assert mc.heston_closed_form(mkt, dict(model, xi=0.0, kappa=0.0)) == pytest.approx(
            hr.black_scholes_call(dict(mkt, v=math.sqrt(model["v0"]))), rel=1e-13)
        # a small xi is next to the xi = 0 limit (the price moves with xi^2 and rho xi), from the quadrature's side
        assert mc.heston_closed_form(mkt, dict(model, xi=1e-3)) == pytest.approx(mc.heston_closed_form(mkt, dict(model, xi=0.0)), abs=2e-3)
        assert mc.heston_closed_form(mkt, dict(model, xi=1e-3)) == pytest.approx(hr.closed_form(mkt, dict(model, xi=1e-3)), abs=1e-9)
        # kappa = 0 with xi > 0, |rho| = 1: valid inputs
        edge = [dict(model, kappa=0.0)] + ([dict(model, rho=-1.0), dict(model, rho=1.0)] if name == "FELLER" else [])
        for md in edge:
            assert mc.heston_closed_form(mkt, md) == pytest.approx(hr.closed_form(mkt, md), abs=CLOSED_FORM_ACCURACY)


def test_closed_form_is_monotone_in_strike_and_within_the_no_arbitrage_bounds(mc):
    for name, mkt, model in hr.CASES:
        ks = np.linspace(40.0, 250.0, 43)
        c = np.array([mc.heston_closed_form(dict(mkt, k=float(k)), model) for k in ks])
        assert np.all(np.diff(c) < 0), name
        lower = np.maximum(mkt["s"] - ks * math.exp(-mkt["r"] * mkt["t"]), 0.0)
        assert np.all(c >= lower - 1e-10) and np.all(c <= mkt["s"]), name


def test_broadie_kaya_case(mc):
    """The case quoted from Broadie and Kaya (2006) at 6.8061.  Both quadratures land on it, so it is asserted."""
    o, md, quoted = BROADIE_KAYA
    got, want = mc.heston_closed_form(o, md), hr.closed_form(o, md)
    print(f"Broadie-Kaya: C {got:.10f}  Python {want:.10f}  quoted {quoted}")
    assert abs(got - want) <= CLOSED_FORM_ACCURACY
    assert abs(got - quoted) <= 5e-5 and abs(want - quoted) <= 5e-5   # the quoted value has four decimals


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_refusals(mc, X):
    o, md = hr.ATM, hr.FELLER
    a = mc.heston_closed_form(o, md, X)
    assert a > 0
    nan, inf = float("nan"), float("inf")
    bad = [(dict(o, s=0.0), md), (dict(o, s=-1.0), md), (dict(o, t=0.0), md), (dict(o, k=0.0), md), (dict(o, r=inf), md), (dict(o, k=nan), md),
           (dict(o, s=inf), md), (dict(o, t=nan), md)]
    bad += [(o, dict(md, **{f: v})) for f in ("v0", "kappa", "theta", "xi") for v in (-0.01, nan, inf)]
    bad += [(o, dict(md, rho=v)) for v in (1.0001, -1.5, nan, inf)]
    for oo, mm in bad:
        with pytest.raises(mc.McError, match="mc error 1"):   # MC_ERR_INVALID
            mc.heston_closed_form(oo, mm, X)
    # |rho| = 1 with a tiny variance: the integrands outlast the quadrature's panels, which is reported, not returned
    with pytest.raises(mc.McError, match="does not decay"):
        mc.heston_closed_form(o, dict(md, v0=1e-6, theta=1e-6, xi=0.5, rho=1.0), X)
    # a variance that never leaves 0: the discounted intrinsic value
    assert mc.heston_closed_form(dict(o, k=90.0), dict(md, v0=0.0, theta=0.0), X) == pytest.approx(100.0 - 90.0 * math.exp(-o["r"] * o["t"]), rel=1e-6)
    L = mc._lib
    price = C.c_double()
    f = getattr(L.lib(), f"mc_heston_closed_form_{X}")
    opt = L.OPTION[X](100.0, 100.0, 0.05, 123.0, 1.0)   # option.v is ignored
    row = [md[k] for k in hr.MODEL_FIELDS]
    assert f(C.byref(L.HESTON[X](opt, *row, 1)), C.byref(price)) == 0 and price.value == a
    assert f(C.byref(L.HESTON[X](opt, *row, -7)), C.byref(price)) == 0 and price.value == a   # n_steps is ignored
    assert f(None, C.byref(price)) == 1 and f(C.byref(L.HESTON[X](opt, *row, 1)), None) == 1
    assert mc.heston_closed_form(o, md, X) == a   # and the next call is served


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, option), offsetof(T, v0), offsetof(T, kappa), offsetof(T, theta), offsetof(T, xi), offsetof(T, rho), offsetof(T, n_steps)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %u\n", ROW(mc_heston_f32), ROW(mc_heston_f64),
         MC_MAX_HESTON_STEPS, MC_DOMAIN_HESTON);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.option.offset, T.v0.offset, T.kappa.offset, T.theta.offset, T.xi.offset, T.rho.offset, T.n_steps.offset]
    assert got == row(L.HestonF32) + row(L.HestonF64) + [L.MAX_HESTON_STEPS, L.DOMAIN_HESTON]
    assert L.MAX_HESTON_STEPS == max(hr.STEPS) and L.DOMAIN_HESTON == hr.DOMAIN_HESTON
    for X in ("f32", "f64"):
        for sym in ("run", "launch", "paths", "closed_form"):
            assert f"mc_heston_{sym}_{X}" in L.EXPORTS


def test_recorded_bias_is_the_models_own(mc):
    """BIAS was measured with this module's walk against its own closed form; a short rerun of the same command's code agrees with
    the record within the two half-widths."""
    assert set(hr.BIAS) == {"STRONG", "FELLER"}
    rng = np.random.default_rng(99)
    n = 1 << 17
    for name in hr.BIAS:
        z1, z2 = rng.standard_normal((n, hr.BIAS_STEPS)), rng.standard_normal((n, hr.BIAS_STEPS))
        v = hr._fast_values(hr.ATM, hr.MODELS[name], hr.BIAS_STEPS, z1, z2)
        disc = math.exp(-hr.ATM["r"] * hr.ATM["t"])
        mean, half = disc * v.mean(), 1.96 * disc * v.std(ddof=1) / math.sqrt(n)
        b, h = hr.BIAS[name]
        assert abs(mean - mc.heston_closed_form(hr.ATM, hr.MODELS[name]) - b) <= 3 * (half + h), (name, mean, b)
        # _fast_values is walk's antithetic value
        assert np.allclose(v[:500], hr.walk(hr.ATM, hr.MODELS[name], hr.BIAS_STEPS, z1[:500], z2[:500], anti=True).value[0], rtol=1e-12, atol=1e-12)
