"""The Heston Asian and barrier calls without a GPU: the float64 model heston_path_ref.py against the models it extends (heston_ref at
one date, asian_ref and barrier_ref at constant variance), the soundness of its per-date forward bound (a float32 evaluation stays
inside it on every path and date), its power (heston_ref's four step mutations and three mutations of the payoff leave it), the caps
on kink paths and near-barrier paths on every shape of tests/test_gpu_heston_path.py, and the structs' layout.

Shares of near-barrier paths under this bound (numpy normals, S0 = 100, B = 125 / B = 80, both directions of a path, printed by
test_caps_hold_on_every_shape_of_the_gpu_test): fp64 0 at every shape up to 4096 steps; fp32 at most 0.3 % up to 17 dates x 1, at most
2.0 % at 63 / 64 dates x 1, at most 2.5 % at 16 x 16 and 1.9 % at 12 x 21 (STRONG, FELLER, POSRHO), 15 - 28 % at 255 - 257 dates x 1, 13 - 20 %
at 1 x 4096 and 50 - 94 % at 256 x 16 and 4096 x 1.  So the fp32 barrier runs per path up to 64 total steps plus 16 x 16 without VIOLATED
(heston_path_ref.barrier_runs); the Asian payoff runs wherever heston_ref.runs admits the total step count."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import asian_ref
import barrier_ref
import greeks_ref as gr
import heston_path_ref as hp
import heston_ref as hr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def numpy_normals(m, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, m)), rng.standard_normal((n, m))


# ---- ties to the existing models ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 7, 64])
def test_one_date_asian_is_the_european_value(m):
    z1, z2 = numpy_normals(m, 1000, 3)
    for name, mkt, model in hr.CASES:
        for anti in (False, True):
            sides = hp.walk(mkt, model, 1, m, z1, z2, anti)
            want = hr.walk(mkt, model, m, z1, z2, anti).value[0]
            assert np.allclose(hp.asian(sides), want, rtol=1e-12, atol=1e-12), (name, m, anti)
            assert np.array_equal(hp.european(sides), want)


@pytest.mark.parametrize("n_dates", [1, 5, 16, 64])
def test_constant_variance_is_the_constant_volatility_model(n_dates):
    """xi = kappa = 0 and one step per date: the walk on z1 is asian_ref's and barrier_ref's at v = sqrt(v0)."""
    z1, z2 = numpy_normals(n_dates, 1000, 4)
    for name, mkt, model in hr.CASES:
        flat, o = dict(model, xi=0.0, kappa=0.0), dict(mkt, v=math.sqrt(model["v0"]))
        for anti in (False, True):
            sides = hp.walk(mkt, flat, n_dates, 1, z1, z2, anti)
            assert np.allclose(hp.asian(sides), asian_ref.asian(o, n_dates, z1, anti=anti).value[0], rtol=1e-12, atol=1e-12), (name, anti)
            for B, kinds in ((hp.UP, hp.KINDS[:2]), (hp.DOWN, hp.KINDS[2:])):
                for kind in kinds:
                    want = barrier_ref.barrier(o, B, n_dates, z1, kind, anti=anti).value[0]
                    assert np.allclose(hp.barrier(sides, B, kind), want, rtol=1e-12, atol=1e-12), (name, kind, anti)


def test_knock_in_plus_knock_out_is_the_european_value():
    z1, z2 = numpy_normals(21, 1000, 5)
    for name, mkt, model in hr.CASES:
        sides = hp.walk(mkt, model, 7, 3, z1, z2, anti=True)
        for B, (out, inn) in ((hp.UP, hp.KINDS[:2]), (hp.DOWN, hp.KINDS[2:])):
            assert np.allclose(hp.barrier(sides, B, out) + hp.barrier(sides, B, inn), hp.european(sides), rtol=1e-14, atol=1e-14)
            assert 0.0 < (hp.barrier(sides, B, inn) > 0).mean() < 1.0   # the barrier matters
        assert np.array_equal(hp.barrier(sides, 1e30, "up-and-out"), hp.european(sides))


# ---- soundness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (16, 1), (16, 16), (256, 1)])
def test_a_float32_evaluation_stays_within_the_bound(shape):
    """The same formulas in numpy float32 on float32 normals: x at every date of every path within bx, the Asian value within
    asian_bound, and the barrier value an admissible one within its bound -- every path, kink and near paths included."""
    nd, spd = shape
    m, tol = nd * spd, TOL["f32"]["pay"]
    z1, z2 = (z.astype(np.float32).astype(np.float64) for z in numpy_normals(m, 2000, 21))
    for name, mkt, model in hr.CASES:
        if not hr.runs(name, "f32", m):
            continue
        for anti in (False, True):
            p = hp.walk(mkt, model, nd, spd, z1, z2, anti)
            q = hp.walk(mkt, model, nd, spd, z1, z2, anti, dtype=np.float32)
            worst_x = max(float((np.abs(b["x"] - a["x"]) / hp.x_bounds(a, tol)[1]).max()) for a, b in zip(p, q))
            b, _ = hp.asian_bound(p, tol)
            worst_a = float((np.abs(hp.asian(q) - hp.asian(p)) / b).max())
            worst_b = 0.0
            for B, kind in ((hp.UP, "up-and-out"), (hp.DOWN, "down-and-in")):
                r, _, _ = hp.barrier_errors(hp.barrier(q, B, kind), p, B, kind, tol)
                worst_b = max(worst_b, float(r.max()))
            print(f"{name} {shape} anti={anti}: worst err/bound x {worst_x:.3g} asian {worst_a:.3g} barrier {worst_b:.3g}")
            assert worst_x <= 1.0 and worst_a <= 1.0 and worst_b <= 1.0, (name, shape, anti)


# ---- power ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", hr.MUTATIONS)
@pytest.mark.parametrize("shape", [(16, 1), (16, 4)])
def test_the_bound_rejects_a_mutated_step(mutation, shape):
    """heston_ref's four step mutations on VIOLATED at the money, tests/test_heston_ref.py's threshold, on the Asian value."""
    nd, spd = shape
    z1, z2 = numpy_normals(nd * spd, 4000, 31)
    p = hp.walk(hr.ATM, hr.VIOLATED, nd, spd, z1, z2)
    b, _ = hp.asian_bound(p, TOL["f32"]["pay"])
    q = hp.walk(hr.ATM, hr.VIOLATED, nd, spd, z1, z2, mutation=mutation)
    share = (np.abs(hp.asian(q) - hp.asian(p)) > b).mean()
    print(mutation, shape, share)
    assert share > 0.40, (mutation, shape, share)


@pytest.mark.parametrize("mutation", hp.PAYOFF_MUTATIONS)
@pytest.mark.parametrize("shape", [(16, 1), (16, 4)])
def test_the_bound_rejects_a_mutated_payoff(mutation, shape):
    """A date read one step late, the average over n_dates + 1, an up barrier read as a down barrier: FELLER in the money (K = 90;
    about two thirds of the paths end in the money and few reach B = 125), more than 40 % of the paths must leave the fp32 bound."""
    nd, spd = shape
    tol = TOL["f32"]["pay"]
    z1, z2 = numpy_normals(nd * spd, 4000, 32)
    p = hp.walk(hr.ITM, hr.FELLER, nd, spd, z1, z2)
    if mutation == "up_as_down":
        r, _, _ = hp.barrier_errors(hp.barrier(p, hp.UP, "up-and-out", up_as_down=True), p, hp.UP, "up-and-out", tol)
        share = (r > 1.0).mean()
    else:
        q = hp.walk(hr.ITM, hr.FELLER, nd, spd, z1, z2, late=True) if mutation == "late" else p
        b, _ = hp.asian_bound(p, tol)
        share = (np.abs(hp.asian(q, one_more=mutation == "one_more") - hp.asian(p)) > b).mean()
    print(mutation, shape, share)
    assert share > 0.40, (mutation, shape, share)


# ---- caps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hp.SHAPES)
def test_caps_hold_on_every_shape_of_the_gpu_test(shape):
    """Conditions on the GPU test's shapes, not measurements: kink paths <= KINK_CAP wherever a payoff runs, near-barrier paths
    <= NEAR_CAP wherever the barrier runs; fp64 has neither."""
    nd, spd = shape
    m = nd * spd
    n = (4 if m < 1024 else 2) * hr.n_paths_for(m)
    shapes = [(case, n) for case in hr.cases_for(m)]
    if shape in hp.TRIP_SHAPES:   # the shapes of tests/test_gpu_walk_trips.py: the path counts of its ranges, each on the case it rotates to
        shapes += [(gr.trip_pick(hr.CASES, hp.TRIP_SHAPES.index(shape), name), gr.TRIP_RANGES[name].n) for name in ("A", "C")]
        assert all(hp.barrier_runs(case[0], X, nd, spd) for case, _ in shapes for X in ("f32", "f64"))
    for (name, mkt, model), n in shapes:
        z1, z2 = numpy_normals(m, n, 2000 + m + spd)
        sides = hp.walk(mkt, model, nd, spd, z1, z2, anti=True)
        for X in ("f32", "f64"):
            if not hr.runs(name, X, m):
                continue
            tol = TOL[X]["pay"]
            b, kink = hp.asian_bound(sides, tol)
            assert np.all(np.isfinite(b[~kink])) and np.all(b > 0)
            assert kink.mean() <= hr.KINK_CAP, (name, shape, X, kink.mean())
            nears = []
            for B, kind in ((hp.UP, "up-and-out"), (hp.DOWN, "down-and-in")):
                r, near, kink_b = hp.barrier_errors(hp.barrier(sides, B, kind), sides, B, kind, tol)
                assert np.all(r == 0.0)
                nears.append(float(near.mean()))
                if hp.barrier_runs(name, X, nd, spd):
                    assert near.mean() <= hp.NEAR_CAP and kink_b.mean() <= hr.KINK_CAP, (name, shape, X, near.mean(), kink_b.mean())
            print(f"{name} {shape} {X}: {kink.mean():.2%} kink paths, near-barrier {nears[0]:.2%} up / {nears[1]:.2%} down, "
                  f"barrier runs: {hp.barrier_runs(name, X, nd, spd)}")
            if X == "f64":
                assert not kink.any() and max(nears) == 0.0, (name, shape)


def test_the_excluded_barrier_shapes_are_excluded_for_a_reason():
    z1, z2 = numpy_normals(256, 2000, 6)
    sides = hp.walk(hr.ATM, hr.STRONG, 256, 1, z1, z2, anti=True)
    _, near, _ = hp.barrier_errors(hp.barrier(sides, hp.UP, "up-and-out"), sides, hp.UP, "up-and-out", TOL["f32"]["pay"])
    assert near.mean() > hp.NEAR_CAP
    assert not hp.barrier_runs("STRONG", "f32", 256, 1) and hp.barrier_runs("STRONG", "f64", 256, 1)
    assert hp.barrier_runs("STRONG", "f32", 16, 16) and not hp.barrier_runs("VIOLATED", "f32", 16, 16)
    assert all(hp.barrier_runs(name, "f64", nd, spd) for name, _, _ in hr.CASES for nd, spd in hp.SHAPES)
    assert all(hp.barrier_runs(name, "f32", nd, spd) for name, _, _ in hr.CASES for nd, spd in hp.SHAPES if nd * spd <= 64)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, heston), offsetof(T, steps_per_date), offsetof(T, payoff), offsetof(T, barrier_type), offsetof(T, barrier)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d %d\n", ROW(mc_heston_path_f32), ROW(mc_heston_path_f64),
         MC_DOMAIN_HESTON_PATH, MC_HESTON_PATH_ASIAN, MC_HESTON_PATH_BARRIER);
  return 0;
}
"""


def test_struct_layout_matches_the_header(tmp_path):
    import montecarlocuda_amd as mc
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.heston.offset, T.steps_per_date.offset, T.payoff.offset, T.barrier_type.offset, T.barrier.offset]
    assert got == row(L.HestonPathF32) + row(L.HestonPathF64) + [hp.DOMAIN_HESTON_PATH, L.HESTON_PATH_PAYOFFS["asian"], L.HESTON_PATH_PAYOFFS["barrier"]]
    for X in ("f32", "f64"):
        for sym in ("run", "launch", "paths"):
            assert f"mc_heston_path_{sym}_{X}" in L.EXPORTS
    assert max(nd * spd for nd, spd in hp.SHAPES) == L.MAX_HESTON_STEPS
