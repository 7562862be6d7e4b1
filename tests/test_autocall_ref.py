"""The float64 model of the worst-of autocallable notes (tests/autocall_ref.py) checked on its own, without a GPU: the exact
single-asset price by density propagation against closed forms and against itself; the model's prices against that exact price;
identities on every path; a float32 walk in the header's order against the bound; six wrong walks the bound must reject; how many
paths of the GPU test's shapes lie near a decision; the structs' layout against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import autocall_ref as ar
import rainbow_ref as rr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
EXACT = 1e-7   # of the notional: a thousand times below the half-width of a 1e7-path price


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def shape_normals():
    """numpy normals for the shapes of the GPU test: N_PATHS paths of the largest table, shared and left unchanged."""
    z = np.random.default_rng(15).standard_normal((ar.N_PATHS, ar.MAX_TABLE))
    z.setflags(write=False)
    return z


def normals_of(shape_normals, n, m):
    return shape_normals[:, :n * m].reshape(ar.N_PATHS, m, n)


def cases(n, n_obs):
    """(basket, contract) of the shapes: contract A on performance levels; at n = 3 contract B on absolute levels as well."""
    out = [(rr.market(n), ar.contract_a(n_obs))]
    if n == 3:
        out.append((rr.ABSOLUTE[0], ar.contract_b(n_obs)))
    return out


# ---- the exact single-asset price -------------------------------------------------------------------------------------
def test_exact_price_at_one_observation_is_black_scholes():
    b = rr.market(1)
    for ki, B in (("dates", 0.6), ("maturity", 0.9), (None, None)):
        for A, Cb in ((1.0, 0.8), (math.inf, 0.0), (0.7, 0.9)):
            con = ar.contract([A], [Cb], 0.02, barrier=B, ki=ki, gearing=1.0)
            assert abs(ar.exact_single(b, 1, con) - ar.single_one_obs(b, con)) <= EXACT, (ki, A, Cb)


def test_exact_price_at_two_observations_is_the_bivariate_formula():
    b = rr.market(1)
    for memory in (False, True):
        for A, Cb in (([1.0, 0.95], [0.8, 0.8]), ([math.inf, 1.0], [0.9, 0.0]), ([0.9, 0.9], [0.95, 0.85])):
            con = ar.contract(A, Cb, 0.03, barrier=None, ki=None, gearing=1.0, memory=memory)
            assert abs(ar.exact_single(b, 2, con) - ar.single_two_obs(b, con)) <= EXACT, (memory, A, Cb)


@pytest.mark.parametrize("m,n_obs", [(4, 4), (16, 4)])
def test_exact_price_is_stable_under_doubled_resolution(m, n_obs):
    b, con = rr.market(1), ar.contract_a(n_obs)
    assert abs(ar.exact_single(b, m, con) - ar.exact_single(b, m, con, panels_per_sd=4.0)) <= EXACT


@pytest.mark.parametrize("m,n_obs", [(4, 4), (16, 4)])
def test_model_prices_the_exact_value(m, n_obs):
    b, con = rr.market(1), ar.contract_a(n_obs)
    exact = ar.exact_single(b, m, con)
    z = np.random.default_rng(4).standard_normal((200_000, m, 1))
    for anti in (False, True):
        v = ar.autocall(b, m, z, con, anti).value[0]
        half = 1.96 * v.std(ddof=1) / math.sqrt(v.size)
        print(f"m={m} anti={anti}: model {v.mean():.6f} +- {half:.2g}, exact {exact:.6f}")
        assert abs(v.mean() - exact) <= 3 * half


# ---- identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 8])
def test_model_identities_on_every_path(shape_normals, n):
    b = rr.market(n)
    for m, n_obs in ((4, 4), (16, 4), (63, 3)):
        z = normals_of(shape_normals, n, m)
        for anti in (False, True):
            # no trigger, no coupon: the notional minus the knock-in put of the rainbow model on the same normals
            con = ar.contract(math.inf, 0.8, 0.0, barrier=0.7, ki="dates", gearing=0.9, n_obs=n_obs)
            D = math.exp(-b["r"] * b["t"])
            put = rr.rainbow(b, m, z, "put-on-min", 0.7, "down-and-in", anti).value[0]
            assert np.allclose(ar.autocall(b, m, z, con, anti).value[0], D - 0.9 * D * put, rtol=0, atol=1e-12)
            # memory pays at least as much
            a = ar.contract_a(n_obs)
            with_memory, without = ar.autocall(b, m, z, a, anti).value[0], ar.autocall(b, m, z, dict(a, memory=False), anti).value[0]
            assert np.all(with_memory >= without) and np.any(with_memory > without)
        # lowering a trigger never keeps a path alive longer
        (y, _), = ar.walk(b, m, z)

        def life(con):
            rows = ar._schedule(b, m, con, None)
            called = np.stack([y[:, j] >= LA for j, LA, _, _ in rows[:-1]] + [np.ones(y.shape[0], dtype=bool)], axis=1)
            return called.argmax(axis=1)

        a = ar.contract_a(n_obs)
        lower = dict(a, autocall=a["autocall"] - 0.03)
        assert np.all(life(lower) <= life(a)) and np.any(life(lower) < life(a))


def test_the_enumeration_contains_the_models_own_value(shape_normals):
    """With every decision taken as near, the scalar re-walk of a path reaches the vectorised walk's (value, scale) among others."""
    n, m, n_obs = 3, 8, 4
    b, con = rr.market(n), ar.contract_a(n_obs)
    z = normals_of(shape_normals, n, m)[:200]
    p, cands = ar.autocall(b, m, z, con, anti=True, tol=1.0, full=True)
    assert len(cands) == 200
    for i, sides in cands.items():
        both = [(0.5 * (v0 + v1), 0.5 * (s0 + s1)) for v0, s0 in sides[0] for v1, s1 in sides[1]]
        assert any(abs(v - p.value[0][i]) <= 1e-15 and abs(s - p.scale[0][i]) <= 1e-12 * s for v, s in both)
        assert len(sides[0]) > 1


# ---- the fp32 walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ar.ASSETS)
def test_a_float32_walk_stays_inside_the_bound_on_every_shape(shape_normals, n):
    tol = TOL["f32"]["pay"]
    worst = 0.0
    for m, n_obs in ar.SHAPES(n):
        z = normals_of(shape_normals, n, m).astype(np.float32).astype(np.float64)
        for b, con in cases(n, n_obs):
            for anti in (False, True):
                p, cands = ar.autocall(b, m, z, con, anti, tol, full=True)
                w, near = ar.check(ar.walk_f32(b, m, z, con, anti), p, cands, tol)
                worst = max(worst, w)
    print(f"n={n}: worst err/bound of the float32 walk {worst:.3g}")


# ---- mutants ----------------------------------------------------------------------------------------------------------
# per wrong walk: (n_dates, n_obs, triggers, coupon level, knock-in level, strike) of a note on which it shows on many paths
MUTANT_SHAPES = {"late": (16, 4, 1.0, 0.95, 0.75, 1.0), "no-reset": (8, 8, math.inf, 1.0, 0.75, 1.0), "dead-coupon": (8, 8, 1.0, 0.95, 0.75, 1.0),
                 "discount-maturity": (8, 8, 1.0, 0.95, 0.75, 1.0), "ki-obs": (64, 2, math.inf, 0.8, 0.95, 1.3),
                 "paid-not-forced": (8, 8, 0.9, 0.95, 0.75, 1.0)}


@pytest.mark.parametrize("mutate", ar.MUTANTS)
def test_the_bound_rejects_six_wrong_walks(shape_normals, mutate):
    """On a shape where the wrong walk's fp64 value differs from the true one by more than 1e-3 on at least 10 % of the paths, the
    per-path rule (at the weaker, fp32 tolerance) refuses at least 90 % of those paths."""
    n, tol = 3, TOL["f32"]["pay"]
    m, n_obs, A, Cb, B, k = MUTANT_SHAPES[mutate]
    b = dict(rr.market(n), r=0.08, t=4.0, k=k)
    con = ar.contract(A, Cb, 0.05, barrier=B, ki="dates", gearing=1.0, n_obs=n_obs)
    z = normals_of(shape_normals, n, m)
    p, cands = ar.autocall(b, m, z, con, tol=tol, full=True)
    wrong = ar.autocall(b, m, z, con, mutate=mutate).value[0]
    differs = np.abs(wrong - p.value[0]) > 1e-3
    print(f"{mutate}: differs on {differs.mean():.3f} of the paths")
    assert differs.mean() >= 0.10
    refused = ar.rejects(wrong, p, cands, tol)
    assert refused[differs].mean() >= 0.90


# ---- how many paths lie near a decision ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ar.ASSETS)
def test_few_paths_lie_near_a_decision(shape_normals, n):
    """Per path direction: none at the fp64 tolerance; at the fp32 tolerance at most 0.05 of a shape up to 64 dates and at most 0.5
    above (the rainbow's caps).  Contract A exercises every branch: paths are called, and paths are knocked in."""
    called_any = knocked_any = False
    for m, n_obs in ar.SHAPES(n):
        z = normals_of(shape_normals, n, m)
        cap = 0.05 if m <= 64 else 0.5
        for b, con in cases(n, n_obs):
            for zz in (z, -z):
                p = ar.autocall(b, m, zz, con)
                share32, share64 = float((p.edge <= TOL["f32"]["pay"]).mean()), float((p.edge <= TOL["f64"]["pay"]).mean())
                called, knocked = ar.shares(b, m, zz, con)
                print(f"n={n} ({m},{n_obs}): near a decision {share32:.3g} (fp32), {share64:.3g} (fp64); called {called:.2f}, knocked in {knocked:.2f}")
                assert share32 <= cap, (n, m, n_obs, share32)
                assert share64 == 0.0, (n, m, n_obs, share64)
                called_any |= 0.1 <= called <= 0.9
                knocked_any |= knocked >= 0.02
    assert called_any and knocked_any


# ---- layout -----------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, basket), offsetof(T, autocall), offsetof(T, coupon_barrier), offsetof(T, coupon), offsetof(T, barrier), \
               offsetof(T, gearing), offsetof(T, n_dates), offsetof(T, n_obs), offsetof(T, memory), offsetof(T, ki_monitoring)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %u %d %d %d\n", ROW(mc_autocall_f32), ROW(mc_autocall_f64),
         MC_MAX_AUTOCALL_TABLE, MC_DOMAIN_AUTOCALL, MC_AUTOCALL_KI_NONE, MC_AUTOCALL_KI_DATES, MC_AUTOCALL_KI_MATURITY);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T)] + [getattr(T, f).offset for f in ("basket", "autocall", "coupon_barrier", "coupon", "barrier", "gearing", "n_dates",
                                                                   "n_obs", "memory", "ki_monitoring")]
    assert got == row(L.AutocallF32) + row(L.AutocallF64) + [L.MAX_AUTOCALL_TABLE, L.DOMAIN_AUTOCALL, L.AUTOCALL_KI[None], L.AUTOCALL_KI["dates"],
                                                              L.AUTOCALL_KI["maturity"]]
    assert L.MAX_AUTOCALL_TABLE == ar.MAX_TABLE and L.DOMAIN_AUTOCALL == ar.DOMAIN_AUTOCALL
