"""Multilevel Monte Carlo on the Heston walk on the GPU (heston_level_kernel, mc_heston_level_*, mc_heston_mlmc_run_*): every path of
one level against the independent float64 model heston_level_ref.py on the kernels' own normals (Engine.normals, domain 17), both
precisions, antithetic off and on, on the smallest shapes (n_dates, steps_per_date) that reach every branch of the two walks (fp32:
one Philox block = two fine steps = one coarse step; fp64: four pairs = two coarse steps per trip, a remainder of one coarse step where
m = 2 (mod 4)) and on path ranges across the 2^32-unit seam; a lane's later grid-stride trips; the bit rules of the stream; exactness at
constant variance; the decay of the correction's variance; the telescoping sum; the multilevel driver; refusals; the C driver.

Tolerances: heston_level_ref's per-path bound at TOL[X]["pay"] (TOL: tests/test_gpu_parity.py).  tests/test_heston_level_ref.py holds
the kink paths of these shapes under their cap, shows the bound's power, and runs the driver's algorithm on the model."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import heston_level_ref as hl
import heston_ref as hr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODD = (dict(s=87.0, k=91.0, r=0.02, t=0.75), dict(v0=0.05, kappa=1.2, theta=0.07, xi=0.45, rho=-0.3))
PREC = {"f32": np.float32, "f64": np.float64}
IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def few(mc):
    """An engine of 16 blocks: a dated product then runs at most 24 workgroups (6144 lanes), so that a lane of a 20 000-path call
    takes three full grid-stride trips and part of a fourth; on the default engine it takes one."""
    e = mc.Engine(0, blocks=16)
    yield e
    e.close()


def normals(e, X, first, n, m):
    return hl.level_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, hl.NPB[X])


def discounted_variance(g, mkt, X):
    r, t = (float(np.float32(mkt[c])) if X == "f32" else mkt[c] for c in "rt")
    n = float(g.n)
    return math.exp(-2.0 * r * t) * (n * g.sum2 - g.sum * g.sum) / (n * (n - 1.0))


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", hl.SHAPES, **IDS)
def test_every_path_against_the_reference(eng, X, shape):
    nd, spd = shape
    m, n, tol = nd * spd, hr.N_PATHS, TOL[X]["pay"]
    ran, firsts_met = set(), set()
    try:
        for name, mkt, model in hr.CASES:
            if not hl.runs(name, X, m):
                continue
            for first in hr.FIRSTS:
                z1, z2 = normals(eng, X, first, n, m)
                both = hl.walk(mkt, model, nd, spd, z1, z2, anti=True, prec=PREC[X])
                for anti, lv in ((False, hl.plain_of(both)), (True, both)):
                    eng.set_antithetic(anti)
                    got = eng.heston_level_paths(mkt, model, nd, spd, n, SEED, first, X)
                    worst, kinks = hl.check(got, lv, tol, (name, shape, first, anti))
                    assert np.count_nonzero(got) > 0
                    print(f"{X} {shape} {name} first={first} anti={anti}: worst err/bound {worst:.3g}, {kinks} kink paths of {n}")
                    ran.add((name, anti))
                firsts_met.add(first)
    finally:
        eng.set_antithetic(False)
    names = {name for name, _ in ran}
    assert {"STRONG", "FELLER", "POSRHO"} <= names and ("VIOLATED" in names) == hl.runs("VIOLATED", X, m)
    assert {(name, anti) for name in names for anti in (False, True)} == ran and firsts_met == set(hr.FIRSTS)
    assert hr.FIRSTS[-1] < (1 << 32) < hr.FIRSTS[-1] + n


# ---- 2. later grid-stride trips ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_later_grid_stride_trips_per_path_and_in_the_sums(eng, few, X):
    """2 dates x 10 steps (m = 2 mod 4, a date in the fp64 remainder) on 20 000 paths: the engine of 16 blocks takes three full trips a
    lane and part of a fourth; per path against the model, the sums within the summed bounds, and the same bits as the default engine."""
    nd, spd, n, first, tol = 2, 10, 20_000, 777, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, nd * spd)
    try:
        for name, mkt, model in hr.CASES[:3]:
            both = hl.walk(mkt, model, nd, spd, z1, z2, anti=True, prec=PREC[X])
            for anti, lv in ((False, hl.plain_of(both)), (True, both)):
                eng.set_antithetic(anti), few.set_antithetic(anti)
                got = few.heston_level_paths(mkt, model, nd, spd, n, SEED, first, X)
                assert trip_guard(few, 16, n) == 3
                worst, kinks = hl.check(got, lv, tol, (name, anti))
                assert np.array_equal(got, eng.heston_level_paths(mkt, model, nd, spd, n, SEED, first, X))
                v, (b, _) = hl.value(lv), hl.bound(lv, tol)
                t1, t2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                g = few.heston_level(mkt, model, nd, spd, n, SEED, first, X)
                assert trip_guard(few, 16, n) == 3 and g.n == n
                print(f"{X} {name} anti={anti}: worst err/bound {worst:.3g}, {kinks} kink paths; sum err {abs(g.sum - v.sum()):.3g} (tol {t1:.3g}), "
                      f"sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {t2:.3g})")
                assert abs(g.sum - v.sum()) <= t1 and abs(g.sum2 - (v * v).sum()) <= t2, (name, anti)
                r, t = (float(np.float32(mkt[c])) if X == "f32" else mkt[c] for c in "rt")   # as the precision's struct holds them
                assert g.expected == pytest.approx(math.exp(-r * t) * g.sum / n, rel=1e-14)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 3. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    import torch
    (o, md), nd, spd, f, n = ODD, 3, 6, 3001, 2500
    other = mc.Engine(0, blocks=96)
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            paths = lambda e, n, f: e.heston_level_paths(o, md, nd, spd, n, SEED, f, X)
            run = lambda n, f: eng.heston_level(o, md, nd, spd, n, SEED, f, X)
            whole, lo, part = paths(eng, f + n, 0), paths(eng, f, 0), paths(eng, n, f)
            assert np.array_equal(np.concatenate([lo, part]), whole)            # [0, n) = [0, k) u [k, n), bitwise per path
            assert np.count_nonzero(whole) > 0
            assert np.array_equal(paths(other, n, f), part)                      # not on the engine's block count
            fused = run(123_457, f)
            eng.set_finish(False)
            two = run(123_457, f)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)   # nor on the finish form
            struct, keep = eng.prepared("heston_level", X, dict(o, **md, n_dates=nd, steps_per_date=spd))
            eng.launch("heston_level", X, struct, SEED, f, 123_457, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (fused.sum, fused.sum2, float(fused.n))   # the launch form's triple is the run form's
            a, b = run(50_001, f), run(123_457 - 50_001, f + 50_001)             # ranges add up
            assert a.n + b.n == fused.n
            assert a.sum + b.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"], abs=TOL[X]["rel"] * math.sqrt(fused.sum2 * fused.n))
            assert a.sum2 + b.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
            # its own domain: not the values of mc_heston_path_* minus anything on the same indices
            assert not np.array_equal(part != 0, eng.heston_asian_paths(o, md, nd, spd, n, SEED, f, X) != 0)
    finally:
        eng.set_finish(True)
        eng.set_antithetic(False)
        other.close()


# ---- 4. constant variance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 2), (3, 2), (2, 10), (4, 16)], **IDS)
def test_at_constant_variance_the_correction_is_zero_within_the_bound(eng, X, shape):
    nd, spd = shape
    n, first, tol = hr.N_PATHS, 99, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, nd * spd)
    try:
        for name, mkt, model in hr.CASES:
            flat = dict(model, xi=0.0, kappa=0.0)
            both = hl.walk(mkt, flat, nd, spd, z1, z2, anti=True, prec=PREC[X])
            for anti, lv in ((False, hl.plain_of(both)), (True, both)):
                eng.set_antithetic(anti)
                got = eng.heston_level_paths(mkt, flat, nd, spd, n, SEED, first, X).astype(np.float64)
                b, kink = hl.bound(lv, tol)
                assert not kink.any() and np.all(np.abs(got) <= b), (name, shape, anti, float((np.abs(got) / b).max()))
    finally:
        eng.set_antithetic(False)


# ---- 5. variance decay, telescoping -----------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("name", ["STRONG", "VIOLATED"])
def test_the_corrections_variance_decays(eng, X, name):
    """Var[Y] at 128 fine steps is at most half of Var[Y] at 16, on 2^16 paths, plain (the float64 model: ratios of about 10 and 3.7)."""
    _, mkt, model = next(c for c in hr.CASES if c[0] == name)
    v16, v128 = (discounted_variance(eng.heston_level(mkt, model, 1, m, 1 << 16, SEED, 0, X), mkt, X) for m in (16, 128))
    print(f"{X} {name}: Var[Y] {v16:.4g} at 16 steps, {v128:.4g} at 128, ratio {v16 / v128:.3g}")
    assert 0.0 < v128 <= 0.5 * v16


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_levels_telescope_to_the_fine_walk(eng, X):
    """mc_heston_path_run at 64 steps against level 0 at 4 steps plus the levels at 8, 16, 32 and 64 fine steps, 2^18 paths each, fixed
    seeds, disjoint ranges: within 5 combined standard errors."""
    mkt, model, n = hr.OTM, hr.VIOLATED, 1 << 18
    fine = eng.heston_asian(mkt, model, 1, 64, n, SEED, 1 << 36, X)
    parts = [eng.heston_asian(mkt, model, 1, 4, n, SEED, 0, X)] + [eng.heston_level(mkt, model, 1, 4 << l, n, SEED, l << 40, X) for l in (1, 2, 3, 4)]
    total = sum(p.expected for p in parts)
    se = math.sqrt(sum(discounted_variance(p, mkt, X) / n for p in parts + [fine]))
    print(f"{X}: 64 steps {fine.expected:.5f}, levels {[round(p.expected, 5) for p in parts]} sum {total:.5f}, combined standard error {se:.3g}")
    assert abs(total - fine.expected) <= 5 * se
    assert all(p.expected < 0 for p in parts[1:3])   # the Euler bias of this case: the first corrections are clearly negative


# ---- 6. the driver ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_multilevel_run(mc, eng, X):
    c = hl.MLMC_CASE
    mkt, model, nd, spd, eps = c["mkt"], c["model"], c["n_dates"], c["steps_per_date"], c["eps"]
    kw = dict(seed=hl.MLMC_SEED, precision=X, min_levels=c["min_levels"], max_levels=c["max_levels"], n_pilot=c["n_pilot"])
    r = eng.heston_mlmc(mkt, model, nd, spd, eps, **kw)
    exact = hr.closed_form(mkt, model)
    print(f"{X}: price {r.price:.4f} +- {r.stderr:.4f} (closed form {exact:.4f}), bias {r.bias:.4f}, converged {r.converged}, levels: "
          + ", ".join(f"{v.n_paths} x {v.estimate.expected:.4f}" for v in r.levels))
    assert r.converged and r.bias <= eps / math.sqrt(2.0)
    assert abs(r.price - exact) <= 3 * eps
    assert 3 <= len(r.levels) <= c["max_levels"] + 1
    assert r.price == pytest.approx(sum(v.estimate.expected for v in r.levels), rel=1e-14)
    assert r.stderr == pytest.approx(math.sqrt(sum(discounted_variance(v.estimate, mkt, X) / v.n_paths for v in r.levels)), rel=1e-12)
    assert r.stderr <= eps / math.sqrt(2.0) * 1.001
    assert r.bias == max(abs(r.levels[-1].estimate.expected), 0.5 * abs(r.levels[-2].estimate.expected))
    # each level's sums are those of one call over the reported range
    for l, v in enumerate(r.levels):
        assert v.first_path == l << 40 and v.estimate.n == v.n_paths >= c["n_pilot"]
        one = (eng.heston_asian if l == 0 else eng.heston_level)(mkt, model, nd, spd << l, v.n_paths, hl.MLMC_SEED, v.first_path, X)
        assert v.estimate.sum == pytest.approx(one.sum, rel=1e-12) and v.estimate.sum2 == pytest.approx(one.sum2, rel=1e-12), l
        assert v.estimate.expected == pytest.approx(one.expected, rel=1e-12)
    # a pure function of (inputs, seed)
    again = eng.heston_mlmc(mkt, model, nd, spd, eps, **kw)
    assert (again.price, again.stderr, again.bias, again.converged) == (r.price, r.stderr, r.bias, r.converged)
    assert [(v.n_paths, v.first_path, v.estimate.sum, v.estimate.sum2) for v in again.levels] == [(v.n_paths, v.first_path, v.estimate.sum, v.estimate.sum2) for v in r.levels]
    # an eps out of reach of max_levels: reported, not an error
    short = eng.heston_mlmc(mkt, model, nd, spd, 0.005, seed=hl.MLMC_SEED, precision=X, min_levels=0, max_levels=3, n_pilot=c["n_pilot"])
    assert not short.converged and len(short.levels) == 4 and short.bias > 0.005 / math.sqrt(2.0) and math.isfinite(short.price)
    # antithetic levels price the same thing
    try:
        eng.set_antithetic(True)
        anti = eng.heston_mlmc(mkt, model, nd, spd, eps, **kw)
    finally:
        eng.set_antithetic(False)
    assert anti.converged and abs(anti.price - exact) <= 3 * eps


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc):
    o, md, nd, spd, n = hr.ATM, hr.FELLER, 4, 6, 50_000
    with mc.Engine(0) as fresh:
        want = {X: (fresh.heston_level(o, md, nd, spd, n, SEED, 0, X), fresh.heston_asian(o, md, nd, spd, n, SEED, 0, X)) for X in ("f32", "f64")}

    def still_fine(e):
        for X, (w0, w1) in want.items():
            g0, g1 = e.heston_level(o, md, nd, spd, n, SEED, 0, X), e.heston_asian(o, md, nd, spd, n, SEED, 0, X)
            assert (g0.sum, g0.sum2, g0.n, g1.sum, g1.sum2, g1.n) == (w0.sum, w0.sum2, w0.n, w1.sum, w1.sum2, w1.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    nan, inf = float("nan"), float("inf")
    L = mc._lib
    from montecarlocuda_amd.engine import _as_heston, check

    def struct(X, opt=o, model=md, nd=nd, spd=spd, payoff="asian", n_steps=None):
        return L.HESTON_PATH[X](_as_heston(X, opt, model, nd * spd if n_steps is None else n_steps), spd,
                                L.HESTON_PATH_PAYOFFS[payoff] if isinstance(payoff, str) else payoff, 0, 125.0)

    def run(e, X, n=n, **kw):
        r = L.Result()
        check(getattr(L.lib(), f"mc_heston_level_run_{X}")(e._ctx, C.byref(struct(X, **kw)), SEED, 0, n, C.byref(r)))
        return r

    def mlmc(e, X, eps=0.05, min_levels=2, max_levels=5, n_pilot=1000, **kw):
        spec, r = L.MlmcSpec(eps, min_levels, max_levels, n_pilot), L.MlmcResult()
        check(getattr(L.lib(), f"mc_heston_mlmc_run_{X}")(e._ctx, C.byref(struct(X, **kw)), C.byref(spec), SEED, C.byref(r)))
        return r

    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            # everything mc_heston_path_run_* refuses
            for bad_steps in (0, -2, L.MAX_HESTON_STEPS + 2):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, spd=2, n_steps=bad_steps)
            for bad in (dict(o, s=0.0), dict(o, s=-3.0), dict(o, t=0.0), dict(o, t=-1.0), dict(o, r=inf), dict(o, k=nan), dict(o, s=inf), dict(o, t=nan)):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, opt=bad)
            for f in ("v0", "kappa", "theta", "xi"):
                for v in (-0.01, nan, inf):
                    with pytest.raises(mc.McError, match=INVALID):
                        run(e, X, model=dict(md, **{f: v}))
            for v in (1.001, -1.001, nan, inf):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, model=dict(md, rho=v))
            with pytest.raises(mc.McError, match=INVALID):
                run(e, X, n=0)
            with pytest.raises(mc.McError, match="outside the range of a double"):
                run(e, X, model=dict(md, xi=3e4), nd=L.MAX_HESTON_STEPS // 2, spd=2)
            for bad_spd in (0, -2, 10, 14):                                   # even, but no divisor of 24
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, spd=bad_spd, n_steps=24)
            for bad_payoff in (-1, 2, 7):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, payoff=bad_payoff)
            still_fine(e)
            # what the level adds: an odd steps_per_date, the barrier payoff
            for odd in (1, 3):
                with pytest.raises(mc.McError, match="is odd"):
                    run(e, X, spd=odd, n_steps=24)
            with pytest.raises(mc.McError, match="discontinuous"):
                run(e, X, payoff="barrier")
            # the multilevel run: its own arguments, and what its levels refuse
            for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=nan), dict(eps=inf), dict(min_levels=-1), dict(max_levels=1), dict(min_levels=4, max_levels=3),
                       dict(max_levels=L.MLMC_MAX_LEVELS + 1), dict(n_pilot=1), dict(n_pilot=0), dict(max_levels=9), dict(payoff="barrier"),
                       dict(opt=dict(o, s=-1.0)), dict(model=dict(md, rho=2.0))):
                with pytest.raises(mc.McError, match=INVALID):
                    mlmc(e, X, **kw)                                           # max_levels = 9: 24 * 2^9 steps, beyond MC_MAX_HESTON_STEPS
            assert mlmc(e, X, nd=1, spd=3).levels >= 3                         # an odd steps_per_date at level 0 is even from level 1 on
            still_fine(e)
            # valid corners
            for okm in (dict(md, xi=0.0), dict(md, kappa=0.0), dict(md, rho=1.0), dict(md, rho=-1.0), hr.VIOLATED, dict(md, v0=0.0)):
                assert np.isfinite(e.heston_level(o, okm, nd, spd, n, SEED, 0, X).expected)
            assert np.isfinite(e.heston_level(o, md, 1, 2, n, SEED, 0, X).expected)
            assert np.isfinite(e.heston_level(o, md, 1, L.MAX_HESTON_STEPS, 2000, SEED, 0, X).expected)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, X)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                mlmc(e, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, X)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                mlmc(e, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            run(e, "f64")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            mlmc(e, "f64")
        e.set_normals("native")
        still_fine(e)
        # external normals and the launch geometry: a context is in those forms only inside the from-normals and grid entry points, and
        # a level has neither
        for X in ("f32", "f64"):
            for form in ("run_grid", "paths_grid", "from_normals"):
                assert not hasattr(L.lib(), f"mc_heston_level_{form}_{X}")


# ---- 8. the C driver --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prints_both_estimates_next_to_the_closed_form(X):
    exe = os.path.join(ROOT, "drivers", f"hestonMlmcOpt_{X}")
    assert os.path.exists(exe), f"drivers/hestonMlmcOpt_{X} not built (build())"
    out = subprocess.run([exe, "0.05", "10000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(s), float(steps), float(err)) for k, p, s, steps, err in
           re.findall(r"^(\w+) price=(\S+) stderr=(\S+) kernel_ms=\S+ path_steps=(\S+) err_in_eps=(\S+)", out.stdout, re.M)}
    assert set(row) == {"mlmc", "single", "closed_form"}, out.stdout
    exact = hr.closed_form(hr.OTM, hr.VIOLATED)
    assert row["closed_form"][0] == pytest.approx(exact, rel=1e-6)
    for k, slack in (("mlmc", 1.001), ("single", 1.15)):         # the single level's N comes from a pilot variance of 10 000 paths
        assert abs(row[k][0] - exact) <= 3 * 0.05 and 0 < row[k][1] <= 0.05 / math.sqrt(2.0) * slack, out.stdout
        assert row[k][2] > 0, out.stdout
    assert "converged=1" in out.stdout and len(re.findall(r"^level \d+ steps=\d+ paths=\d+", out.stdout, re.M)) >= 3, out.stdout
