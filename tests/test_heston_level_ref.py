"""The multilevel correction on the Heston walk without a GPU: the float64 model heston_level_ref.py -- its soundness (a float32
evaluation of both legs stays within bound(., 2^-24) of it on every path of the GPU test's shapes), its power (four mutations of the
coarse leg leave the bound on a clear majority of paths), exactness at constant variance, the cap on kink paths on every shape of
tests/test_gpu_heston_level.py, the variance decay the GPU test asserts -- and the host side of the feature: mc_mlmc_plan against its
restatement, the driver's algorithm on the model, the layout of the new structs and the new symbols.

Shares of paths that leave the fp32 bound (TOL["f32"]["pay"]) under a mutation, numpy normals, 4000 paths, FELLER in the money /
VIOLATED at the money (printed by test_the_bound_rejects_a_mutated_coarse_leg): first_only 0.93 / 0.81 at 4 x 16 and 0.92 / 0.77 at
3 x 2; dt_once 0.83 / 0.75 and 0.82 / 0.66; date_late 0.82 / 0.67 and 0.78 / 0.52; half_twice 0.88 / 0.72 and 0.87 / 0.66.  The paths
that stay are those that end out of the money on both legs, where Y = 0 whatever the coarse leg does.  (date_late moves nothing at
one date: the last date is never late.)

Kink paths (either leg, both directions, TOL["f32"]["pay"]): none in fp64; in fp32 none outside VIOLATED, whose share is at most
0.3 % up to 20 fine steps, 2 - 5 % at 64 (too close to the cap to be a condition on the device's normals) and 17 - 34 % at 256: VIOLATED
runs in fp32 up to heston_level_ref.VIOLATED_F32_MAX_STEPS = 32 fine steps."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import heston_level_ref as hl
import heston_path_ref as hp
import heston_ref as hr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")


def numpy_normals(m, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, m)), rng.standard_normal((n, m))


# ---- ties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2), (3, 2), (2, 10)], **IDS)
def test_the_two_forms_of_the_model_agree_and_the_fine_leg_is_the_asian_call(shape):
    nd, spd = shape
    z1, z2 = numpy_normals(nd * spd, 1000, 3)
    for name, mkt, model in hr.CASES:
        lv = hl.walk(mkt, model, nd, spd, z1, z2, anti=True)
        assert np.array_equal(hp.asian(lv.fine), hp.asian(hp.walk(mkt, model, nd, spd, z1, z2, anti=True)))
        y = 0.0
        for sign in (1.0, -1.0):
            pf, pc = hl.fast_values(mkt, model, nd, spd, sign * z1, sign * z2)
            y = y + 0.5 * (pf - pc)
        assert np.allclose(hl.value(lv), y, rtol=0, atol=1e-11), (name, shape)
        assert np.array_equal(hl.value(hl.plain_of(lv)), hl.value(hl.walk(mkt, model, nd, spd, z1, z2)))


def test_the_coarse_leg_is_the_fine_walk_of_half_the_steps_on_the_summed_normals():
    """sqrt(2 dt) z_c = sdt W: heston_path_ref on m / 2 steps and z_c = (z_a + z_b) / sqrt 2 is the same real number."""
    nd, spd = 3, 8
    z1, z2 = numpy_normals(nd * spd, 1000, 4)
    c1, c2 = ((z[:, 0::2] + z[:, 1::2]) * math.sqrt(0.5) for z in (z1, z2))
    for name, mkt, model in hr.CASES:
        lv = hl.walk(mkt, model, nd, spd, z1, z2, anti=True)
        assert np.allclose(hp.asian(lv.coarse), hp.asian(hp.walk(mkt, model, nd, spd // 2, c1, c2, anti=True)), rtol=0, atol=1e-10), name


# ---- soundness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hl.SHAPES, **IDS)
def test_a_float32_evaluation_stays_within_the_bound(shape):
    """Both legs in numpy float32 on float32 normals against the float64 model at one float32 roundoff, every path, kink paths
    included, every case (VIOLATED beyond its fp32 limit too: the bound holds there, only its kink share is too large)."""
    nd, spd = shape
    z1, z2 = (z.astype(np.float32).astype(np.float64) for z in numpy_normals(nd * spd, hr.N_PATHS, 21))
    for name, mkt, model in hr.CASES:
        for anti in (False, True):
            p = hl.walk(mkt, model, nd, spd, z1, z2, anti, prec=np.float32)
            q = hl.walk(mkt, model, nd, spd, z1, z2, anti, dtype=np.float32)
            b, _ = hl.bound(p, 2.0 ** -24)
            worst = float((np.abs(hl.value(q) - hl.value(p)) / b).max())
            print(f"{name} {shape} anti={anti}: worst err/bound {worst:.3g}")
            assert worst <= 1.0, (name, shape, anti)
            assert np.count_nonzero(hl.value(p)) > 0


# ---- power ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", hl.MUTATIONS)
@pytest.mark.parametrize("shape", [(3, 2), (4, 16)], **IDS)
def test_the_bound_rejects_a_mutated_coarse_leg(mutation, shape):
    nd, spd = shape
    z1, z2 = numpy_normals(nd * spd, 4000, 31)
    for name, mkt, model in (("FELLER", hr.ITM, hr.FELLER), ("VIOLATED", hr.ATM, hr.VIOLATED)):
        p = hl.walk(mkt, model, nd, spd, z1, z2)
        b, _ = hl.bound(p, TOL["f32"]["pay"])
        share = (np.abs(hl.value(hl.walk(mkt, model, nd, spd, z1, z2, mutation=mutation)) - hl.value(p)) > b).mean()
        print(mutation, shape, name, share)
        assert share > 0.50, (mutation, shape, name, share)


# ---- exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hl.SHAPES + [(5, 4), (7, 6)], **IDS)
def test_at_constant_variance_the_two_walks_are_the_same_real_number(shape):
    nd, spd = shape
    z1, z2 = numpy_normals(nd * spd, 2000, 5)
    for name, mkt, model in hr.CASES:
        flat = dict(model, xi=0.0, kappa=0.0)
        for anti in (False, True):
            lv = hl.walk(mkt, flat, nd, spd, z1, z2, anti)
            b, kink = hl.bound(lv, TOL["f64"]["pay"])
            assert not kink.any() and np.all(np.abs(hl.value(lv)) <= b), (name, shape, anti)
            assert np.count_nonzero(hp.asian(lv.fine)) > 0


# ---- caps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hl.SHAPES, **IDS)
def test_kink_paths_stay_under_the_cap_on_every_shape_of_the_gpu_test(shape):
    nd, spd = shape
    m = nd * spd
    z1, z2 = numpy_normals(m, 4 * hr.N_PATHS, 2000 + m + spd)
    for name, mkt, model in hr.CASES:
        lv = hl.walk(mkt, model, nd, spd, z1, z2, anti=True)
        for X in ("f32", "f64"):
            b, kink = hl.bound(lv, TOL[X]["pay"])
            print(f"{name} {shape} {X}: {kink.mean():.2%} kink paths, runs: {hl.runs(name, X, m)}")
            assert np.all(b > 0)
            if hl.runs(name, X, m):
                assert np.all(np.isfinite(b[~kink])) and kink.mean() <= hr.KINK_CAP, (name, shape, X, kink.mean())
            if X == "f64":
                assert not kink.any()
    assert all(hl.runs(name, X, m) for name in ("STRONG", "FELLER", "POSRHO") for X in ("f32", "f64")) and hl.runs("VIOLATED", "f64", m)


def test_the_excluded_shapes_are_excluded_for_a_reason():
    z1, z2 = numpy_normals(256, 4 * hr.N_PATHS, 6)
    _, kink = hl.bound(hl.walk(hr.OTM, hr.VIOLATED, 1, 256, z1, z2, anti=True), TOL["f32"]["pay"])
    assert kink.mean() > hr.KINK_CAP and not hl.runs("VIOLATED", "f32", 256)
    assert [s for s in hl.SHAPES if hl.runs("VIOLATED", "f32", s[0] * s[1])] == [(1, 2), (1, 6), (3, 2), (2, 10)]


# ---- variance decay -------------------------------------------------------------------------------------------------------
def level_variance(mkt, model, m, rng, n=1 << 16):
    z1, z2 = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    pf, pc = hl.fast_values(mkt, model, 1, m, z1, z2)
    return float((pf - pc).var())


@pytest.mark.parametrize("name", ["STRONG", "VIOLATED"])
def test_the_models_correction_variance_decays(name):
    """The assertion of the GPU test on the model: Var[Y] at 128 fine steps at most half of Var[Y] at 16 (the ratios are about 10 and 3.7)."""
    _, mkt, model = next(c for c in hr.CASES if c[0] == name)
    rng = np.random.default_rng(11)
    v16, v128 = level_variance(mkt, model, 16, rng), level_variance(mkt, model, 128, rng)
    print(f"{name}: Var[Y] {v16:.4g} at 16 steps, {v128:.4g} at 128, ratio {v16 / v128:.3g}")
    assert v128 <= 0.5 * v16


# ---- mc_mlmc_plan ---------------------------------------------------------------------------------------------------------
def test_the_plan_is_its_restatement():
    import montecarlocuda_amd as mc
    rng = np.random.default_rng(8)
    for levels in (1, 2, 3, 7, 13):
        for _ in range(20):
            var, cost = rng.uniform(0.0, 50.0, levels), rng.uniform(0.5, 5000.0, levels)
            eps = float(10.0 ** rng.uniform(-3, 0))
            got, want = mc.mlmc_plan(var, cost, eps), hl.mlmc_plan(var, cost, eps)
            assert all(abs(g - w) <= 1 + 1e-12 * w for g, w in zip(got, want)), (var, cost, eps)   # ceil of two roundings of one real number
    assert mc.mlmc_plan([52.0, 25.0, 0.0, 10.0], [4, 12, 24, 48], 0.05) == hl.mlmc_plan([52.0, 25.0, 0.0, 10.0], [4, 12, 24, 48], 0.05)
    assert mc.mlmc_plan([52.0, 25.0, 0.0, 10.0], [4, 12, 24, 48], 0.05)[2] == 0          # a level of zero variance needs no path
    assert mc.mlmc_plan([0.0, 0.0], [1, 2], 0.1) == [0, 0]
    assert mc.mlmc_plan([1.0], [1.0], 1.0) == [2]                                         # 2 eps^-2 V
    for var, cost, eps in (([1.0], [1.0], 0.0), ([1.0], [1.0], -0.1), ([1.0], [1.0], math.nan), ([1.0], [1.0], math.inf), ([-1e-9, 1.0], [1.0, 2.0], 0.1),
                           ([math.nan], [1.0], 0.1), ([math.inf], [1.0], 0.1), ([1.0, 1.0], [1.0, 0.0], 0.1), ([1.0], [-2.0], 0.1), ([1.0], [math.nan], 0.1),
                           ([1e300], [1e-300], 1e-9)):
        with pytest.raises(mc.McError, match="mc error 1"):
            mc.mlmc_plan(var, cost, eps)
        if max(var) < 1e300:
            with pytest.raises(ValueError):
                hl.mlmc_plan(var, cost, eps)
    L = mc._lib.lib()
    n = (C.c_uint64 * 1)()
    one = (C.c_double * 1)(1.0)
    assert L.mc_mlmc_plan(0, one, one, 0.1, n) == 1 and L.mc_mlmc_plan(1, None, one, 0.1, n) == 1 and L.mc_mlmc_plan(1, one, one, 0.1, None) == 1


# ---- the driver's algorithm -----------------------------------------------------------------------------------------------
def model_sampler(case, seed):
    """sample(l, first, n) of heston_level_ref.mlmc on the float64 model and numpy normals: level l draws from its own generator, in
    order (the driver asks for consecutive ranges)."""
    mkt, model, nd, spd0 = case["mkt"], case["model"], case["n_dates"], case["steps_per_date"]
    disc = math.exp(-mkt["r"] * mkt["t"])
    rngs, at = {}, {}

    def sample(l, first, n):
        rng = rngs.setdefault(l, np.random.default_rng([seed, l]))
        assert at.get(l, 0) == first
        at[l] = first + n
        spd, s, s2, done = spd0 * 2 ** l, 0.0, 0.0, 0
        while done < n:
            k = min(n - done, max(1, (1 << 22) // (nd * spd)))
            z1, z2 = rng.standard_normal((k, nd * spd)), rng.standard_normal((k, nd * spd))
            pf, pc = hl.fast_values(mkt, model, nd, spd, z1, z2, coarse=l > 0)
            y = disc * (pf - pc if l > 0 else pf)
            s, s2, done = s + float(y.sum()), s2 + float((y * y).sum()), done + k
        return s, s2
    return sample


def test_the_drivers_algorithm_converges_on_the_model():
    """VIOLATED out of the money, the European call, level 0 at 4 steps, eps = 0.05: converged, within 3 eps of the closed form."""
    c = hl.MLMC_CASE
    r = hl.mlmc(model_sampler(c, hl.MLMC_SEED), c["n_dates"] * c["steps_per_date"], c["eps"], c["min_levels"], c["max_levels"], c["n_pilot"])
    exact = hr.closed_form(c["mkt"], c["model"])
    print(f"price {r['price']:.4f} +- {r['stderr']:.4f} (closed form {exact:.4f}), bias {r['bias']:.4f}, levels {len(r['levels'])}: "
          + ", ".join(f"{e['n']} x {e['mean']:.4f} (var {e['var']:.3g})" for e in r["levels"]))
    assert r["converged"] and r["bias"] <= c["eps"] / math.sqrt(2.0)
    assert abs(r["price"] - exact) <= 3 * c["eps"]
    assert r["stderr"] <= c["eps"] / math.sqrt(2.0) * 1.001
    assert 3 <= len(r["levels"]) <= c["max_levels"] + 1
    assert all(a["n"] > b["n"] for a, b in zip(r["levels"], r["levels"][1:]))   # the expensive levels need few paths
    # an eps out of reach of max_levels: not converged, and says so
    r = hl.mlmc(model_sampler(c, hl.MLMC_SEED), c["n_dates"] * c["steps_per_date"], 0.02, 2, 2, 2000)
    assert not r["converged"] and len(r["levels"]) == 3


# ---- the ABI --------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu ", sizeof(mc_mlmc_spec), offsetof(mc_mlmc_spec, eps), offsetof(mc_mlmc_spec, min_levels), offsetof(mc_mlmc_spec, max_levels),
         offsetof(mc_mlmc_spec, n_pilot));
  printf("%zu %zu %zu %zu ", sizeof(mc_mlmc_level), offsetof(mc_mlmc_level, result), offsetof(mc_mlmc_level, n_paths), offsetof(mc_mlmc_level, first_path));
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(mc_mlmc_result), offsetof(mc_mlmc_result, price), offsetof(mc_mlmc_result, stderr_), offsetof(mc_mlmc_result, bias),
         offsetof(mc_mlmc_result, converged), offsetof(mc_mlmc_result, levels), offsetof(mc_mlmc_result, level));
  printf("%u %d %d\n", MC_DOMAIN_HESTON_LEVEL, MC_MLMC_MAX_LEVELS, MC_MAX_HESTON_STEPS);
  return 0;
}
"""


def test_struct_layout_matches_the_header_and_the_symbols_are_there(tmp_path):
    import montecarlocuda_amd as mc
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    S, V, R = L.MlmcSpec, L.MlmcLevel, L.MlmcResult
    assert got == [C.sizeof(S), S.eps.offset, S.min_levels.offset, S.max_levels.offset, S.n_pilot.offset,
                   C.sizeof(V), V.result.offset, V.n_paths.offset, V.first_path.offset,
                   C.sizeof(R), R.price.offset, R.stderr_.offset, R.bias.offset, R.converged.offset, R.levels.offset, R.level.offset,
                   hl.DOMAIN_HESTON_LEVEL, L.MLMC_MAX_LEVELS, L.MAX_HESTON_STEPS]
    assert L.DOMAIN_HESTON_LEVEL == hl.DOMAIN_HESTON_LEVEL and L.PRODUCTS["heston_level"] is L.HESTON_PATH
    lib = L.lib()
    for X in ("f32", "f64"):
        for sym in [f"mc_heston_level_{f}_{X}" for f in ("run", "launch", "paths")] + [f"mc_heston_mlmc_run_{X}"]:
            assert sym in L.EXPORTS and hasattr(lib, sym), sym
    assert "mc_mlmc_plan" in L.EXPORTS and hasattr(lib, "mc_mlmc_plan")
    assert {"heston_level", "heston_level_paths", "heston_mlmc"} <= set(dir(mc.Engine)) and callable(mc.mlmc_plan)
    assert all(nd * spd <= L.MAX_HESTON_STEPS and spd % 2 == 0 for nd, spd in hl.SHAPES)
