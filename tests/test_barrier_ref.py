"""The barrier call without a GPU: the closed form (mc_barrier_closed_form_*, plain C in mc_hostmath_impl.h) against the
first-principles derivation in barrier_ref.py; the float64 reference model barrier_ref.py against the exact prices on numpy's
own normals (the Brownian-bridge estimator is unbiased for the continuously monitored price at any number of dates, the
one-date discrete form has its own closed form); two mutations of the model that the per-path bound must reject; how many
paths of the shapes of tests/test_gpu_barrier.py carry a jump term; the refusals that need no device; the structs' layout.

The Monte Carlo checks use ONE fixed seed and 3 half-widths (1.96 sigma / sqrt(n) each, so 5.9 sigma): the margin is for nothing
but sampling noise.  With 2e6 numpy paths every valid case lay within 1.6 half-widths; a model with the exponent's 2 replaced by
1 was 14 to 900 half-widths away."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import barrier_ref as br
import greeks_ref as gr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

# (option, barrier): K on both sides of B, both directions
MARKETS = br.CASES + [(br.ATM, 90.0), (dict(s=100.0, k=90.0, r=0.02, v=0.25, t=2.0), 130.0), (dict(s=100.0, k=125.0, r=0.03, v=0.3, t=1.5), 115.0),
                      (dict(s=237.5, k=213.75, r=-0.015, v=0.17, t=1.3), 190.0)]
MC_MARKETS = [(br.ATM, 120.0), (br.ATM, 90.0), (dict(s=100.0, k=90.0, r=0.02, v=0.25, t=2.0), 130.0)]
MC_PATHS, MC_CHUNK = 2_000_000, 250_000


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def rounded(o, B, X):
    """The market as the precision's struct holds it."""
    f = (lambda x: float(np.float32(x))) if X == "f32" else float
    return {c: f(x) for c, x in o.items()}, f(B)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_matches_the_first_principles_model(mc, X):
    sides = set()
    for o, B in MARKETS:
        q, b = rounded(o, B, X)
        sides.add((B > o["s"], o["k"] > B))
        for kind in br.kinds_of(o, B):
            got, want = mc.barrier_closed_form(q, b, kind, X), br.reiner_rubinstein(q, b, kind)
            assert abs(got - want) <= 1e-12 * abs(want), (o, B, kind, got, want)
    assert len(sides) == 4   # up and down, K below and above B
    # in + out = the vanilla call
    assert mc.barrier_closed_form(br.ATM, 120.0, "up-and-out") + mc.barrier_closed_form(br.ATM, 120.0, "up-and-in") == \
        pytest.approx(br.black_scholes_call(br.ATM), rel=1e-13)
    assert mc.barrier_closed_form(dict(br.ATM, k=125.0), 120.0, "up-and-out") == 0.0   # K above an up barrier: nothing is left


def _mc_estimates(m, monitoring):
    """sum and sum of squares of the reference model's per-path values for MC_MARKETS x their two kinds, on seeded numpy normals."""
    rng = np.random.default_rng(20241017 + m)
    acc = {(i, kind): [0.0, 0.0] for i, (o, B) in enumerate(MC_MARKETS) for kind in br.kinds_of(o, B)}
    for _ in range(MC_PATHS // MC_CHUNK):
        z = rng.standard_normal((MC_CHUNK, m))
        for i, (o, B) in enumerate(MC_MARKETS):
            sides = br.walk(o, B, m, z, B > o["s"], monitoring)
            for kind in br.kinds_of(o, B):
                v = br.value(sides, kind.endswith("in")).value[0]
                acc[(i, kind)][0] += v.sum()
                acc[(i, kind)][1] += (v * v).sum()
    out = {}
    for (i, kind), (s1, s2) in acc.items():
        o = MC_MARKETS[i][0]
        disc, n = math.exp(-o["r"] * o["t"]), MC_PATHS
        mean = s1 / n
        out[(i, kind)] = (disc * mean, 1.96 * disc * math.sqrt(max(s2 / n - mean * mean, 0.0) / (n - 1)))
    return out


@pytest.mark.parametrize("m", [1, 16])
def test_reference_model_prices_the_continuous_barrier_at_any_date_count(m):
    seen = set()
    for (i, kind), (price, half) in _mc_estimates(m, "continuous").items():
        o, B = MC_MARKETS[i]
        exact = br.reiner_rubinstein(o, B, kind)
        print(f"m={m} {kind} B={B}: {price:.5f} +- {half:.2g}, exact {exact:.5f}: {abs(price - exact) / half:.2f} half-widths")
        assert abs(price - exact) <= 3 * half, (o, B, kind, price, exact, half)
        seen.add(kind)
    assert seen == set(br.KINDS)


def test_reference_model_one_date_discrete():
    for (i, kind), (price, half) in _mc_estimates(1, "discrete").items():
        o, B = MC_MARKETS[i]
        exact = br.one_date_discrete(o, B, kind)
        print(f"m=1 discrete {kind} B={B}: {price:.5f} +- {half:.2g}, exact {exact:.5f}")   # down-and-in with K above B is exactly 0 at one date
        assert abs(price - exact) <= 3 * half, (o, B, kind, price, exact, half)
        assert exact >= br.reiner_rubinstein(o, B, kind) if kind.endswith("out") else exact <= br.reiner_rubinstein(o, B, kind)


@pytest.fixture(scope="module")
def shape_normals():
    """numpy normals for the shapes of the GPU test: N_PATHS paths of the largest date count, shared and left unchanged."""
    z = np.random.default_rng(5).standard_normal((br.N_PATHS, max(br.DATES)))
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("m", [m for m in br.DATES if m >= 2])
def test_the_continuous_bound_rejects_two_mutations(shape_normals, m):
    """At the weaker (fp32) tolerance, on at least one live path of every shape: the bridge exponent's 2 replaced by 1, and
    d_{j-1} replaced by d_j."""
    z = shape_normals[:, :m]
    for o, B in br.CASES:
        kind = br.kinds_of(o, B)[0]   # knock-out
        p = br.barrier(o, B, m, z, kind, "continuous")
        b = gr.bound(p, TOL["f32"]["pay"])[0]
        live = p.value[0] > 0
        for what, mutant in (("exponent", br.barrier(o, B, m, z, kind, "continuous", exponent=1.0)),
                             ("lag", br.barrier(o, B, m, z, kind, "continuous", lagged=False))):
            caught = (np.abs(mutant.value[0] - p.value[0]) > b) & live
            assert caught.any(), (o, B, m, what)


@pytest.mark.parametrize("m", br.DATES)
def test_few_paths_carry_a_jump_term(shape_normals, m):
    """Discrete form, per path direction (an antithetic pair carries the jump of either of its two paths): none at the fp64
    tolerance; at the fp32 tolerance at most 5 % up to 257 dates and at most 50 % at 1000 and 4096 dates, where the running sum
    W_j is charged its worst case and the GPU test's check of the two possible values is what keeps those paths tested.
    Measured on these shapes: 0 at 1, 1e-3 at 16, 0.03 at 257, 0.16 at 1000, 0.39 at 4096."""
    cap = 0.05 if m <= 257 else 0.5
    shapes = [(o, B, shape_normals[:, :m]) for o, B in br.CASES]
    if m in br.TRIP_DATES:   # the shapes of tests/test_gpu_walk_trips.py: the path counts of its ranges, each on the market it rotates to
        for name in ("A", "C"):
            o, B = gr.trip_pick(br.CASES, br.TRIP_DATES.index(m), name)
            shapes.append((o, B, np.random.default_rng(50 + m).standard_normal((gr.TRIP_RANGES[name].n, m))))
    for o, B, z in shapes:
        for zz in (z, -z):
            p = br.barrier(o, B, m, zz, br.kinds_of(o, B)[0], "discrete")
            share32, share64 = float((p.edge <= TOL["f32"]["pay"]).mean()), float((p.edge <= TOL["f64"]["pay"]).mean())
            print(f"m={m} B={B} {len(z)} paths: share of paths with a jump term {share32:.3g} (fp32), {share64:.3g} (fp64)")
            assert share32 <= cap, (o, B, m, share32)
            assert share64 == 0.0, (o, B, m, share64)
            assert not gr.kink_free(p, 1.0)   # the edge is finite: the discrete form does have a step


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_closed_form_refusals(mc, X):
    ok = br.ATM
    assert mc.barrier_closed_form(ok, 120.0, "up-and-out", X) > 0
    bad = [(dict(ok, s=0.0), 120.0, "up-and-out"), (dict(ok, t=0.0), 120.0, "up-and-out"), (dict(ok, v=-0.1), 120.0, "up-and-out"),
           (dict(ok, v=0.0), 120.0, "up-and-out"), (dict(ok, r=float("nan")), 120.0, "up-and-out"), (dict(ok, k=float("inf")), 120.0, "up-and-out"),
           (ok, 0.0, "down-and-out"), (ok, -5.0, "down-and-in"), (ok, float("inf"), "up-and-out"), (ok, 120.0, 7), (ok, 120.0, -1)]
    for o, B, kind in bad:
        with pytest.raises(mc.McError, match="mc error 1"):   # MC_ERR_INVALID
            mc.barrier_closed_form(o, B, kind, X)
    # the spot on or beyond the barrier: the product is the vanilla call or nothing (the formula gives nonsense: 100/105 down is negative)
    for B, kind in ((100.0, "up-and-out"), (95.0, "up-and-in"), (100.0, "down-and-out"), (105.0, "down-and-in"), (105.0, "down-and-out")):
        with pytest.raises(mc.McError, match="vanilla call or nothing"):
            mc.barrier_closed_form(ok, B, kind, X)
    with pytest.raises(mc.McError, match="v != 0"):
        mc.barrier_closed_form(dict(ok, v=0.0), 120.0, "up-and-out", X)
    # n_dates and monitoring are ignored by the formula but checked like every other field
    L = mc._lib
    price = C.c_double()
    f = getattr(L.lib(), f"mc_barrier_closed_form_{X}")
    opt = L.OPTION[X](100.0, 100.0, 0.05, 0.2, 1.0)
    assert f(C.byref(L.BARRIER[X](opt, 120.0, 1, 0, 0)), C.byref(price)) == 0
    a = price.value
    assert f(C.byref(L.BARRIER[X](opt, 120.0, 4096, 0, 1)), C.byref(price)) == 0 and price.value == a
    for n_dates, mon in ((0, 0), (L.MAX_BARRIER_DATES + 1, 0), (12, 2), (12, -1)):
        assert f(C.byref(L.BARRIER[X](opt, 120.0, n_dates, 0, mon)), C.byref(price)) == 1
    assert f(None, C.byref(price)) == 1
    assert mc.barrier_closed_form(ok, 120.0, "up-and-out", X) == pytest.approx(a)   # and the next call is served


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, barrier), offsetof(T, n_dates), offsetof(T, type), offsetof(T, monitoring)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %u %d %d %d %d %d %d\n", ROW(mc_barrier_f32), ROW(mc_barrier_f64),
         MC_MAX_BARRIER_DATES, MC_DOMAIN_BARRIER, MC_BARRIER_UP_OUT, MC_BARRIER_UP_IN, MC_BARRIER_DOWN_OUT, MC_BARRIER_DOWN_IN,
         MC_MONITOR_DISCRETE, MC_MONITOR_CONTINUOUS);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.barrier.offset, T.n_dates.offset, T.type.offset, T.monitoring.offset]
    assert got == row(L.BarrierF32) + row(L.BarrierF64) + [L.MAX_BARRIER_DATES, L.DOMAIN_BARRIER] + \
        [L.BARRIER_TYPES[k] for k in br.KINDS] + [L.MONITORING[k] for k in br.MONITORINGS]
    assert L.MAX_BARRIER_DATES == max(br.DATES) and L.DOMAIN_BARRIER == br.DOMAIN_BARRIER
