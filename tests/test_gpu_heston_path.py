"""The Asian and the discretely monitored barrier call on the Heston walk on the GPU (heston_path_kernel, mc_heston_path_*): every
path against the independent float64 model heston_path_ref.py on the kernels' own normals (Engine.normals, domain 7), both payoffs,
both precisions, antithetic off and on, shapes (n_dates, steps_per_date) whose date boundaries meet every loop boundary (the fp32 loop
takes two steps per Philox block -- an odd steps_per_date splits a block; the fp64 loop four pairs per trip, then one) and path
ranges across the 2^32-unit seam; identities per path; the sums of a call of many grid-stride trips; the bit rules of the stream; the
launch form; prices end to end; refusals; the C driver.

Tolerances: heston_path_ref's per-path bounds at TOL[X]["pay"] (TOL: tests/test_gpu_parity.py).  A barrier path whose distance to the
barrier is within its bound at some date may take either of its two values; no path is left out.  tests/test_heston_path_ref.py holds
the kink and near-barrier paths of these shapes under their caps and shows the bounds' power."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import asian_ref
import barrier_ref
import heston_path_ref as hp
import heston_ref as hr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODD = (dict(s=87.0, k=91.0, r=0.02, t=0.75), dict(v0=0.05, kappa=1.2, theta=0.07, xi=0.45, rho=-0.3))


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
    """An engine of 16 blocks: a dated product then runs at most 24 workgroups (6144 lanes), so that a lane of a 300 000-path call
    takes 48 full grid-stride trips and part of a 49th; on the default engine (3072 workgroups) it takes one below 786 432 paths."""
    e = mc.Engine(0, blocks=16)
    yield e
    e.close()


def normals(e, X, first, n, m):
    return hp.heston_path_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, hp.NPB[X])


def finite(got, what):
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    return got


def barrier_kinds(shape):
    if shape in hp.FOUR_KIND_SHAPES:
        return [(hp.UP, k) for k in hp.KINDS[:2]] + [(hp.DOWN, k) for k in hp.KINDS[2:]]
    return [(hp.UP, "up-and-out"), (hp.DOWN, "down-and-in")]


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", hp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_path_against_the_reference(mc, eng, X, shape):
    nd, spd = shape
    m = nd * spd
    assert max(a * b for a, b in hp.SHAPES) == mc._lib.MAX_HESTON_STEPS
    n, tol = hr.n_paths_for(m), TOL[X]["pay"]
    ran, firsts_met = set(), set()
    try:
        for name, mkt, model in hr.cases_for(m):
            if not hr.runs(name, X, m):
                continue
            for first in hr.FIRSTS:
                z1, z2 = normals(eng, X, first, n, m)
                both = hp.walk(mkt, model, nd, spd, z1, z2, anti=True)
                for anti, sides in ((False, both[:1]), (True, both)):
                    eng.set_antithetic(anti)
                    what = (name, shape, first, anti)
                    worst, kinks = hp.check_asian(eng.heston_asian_paths(mkt, model, nd, spd, n, SEED, first, X), sides, tol, what)
                    print(f"{X} {shape} {name} first={first} anti={anti}: asian worst err/bound {worst:.3g}, {kinks} kink paths of {n}")
                    ran.add((name, "asian", anti))
                    if not hp.barrier_runs(name, X, nd, spd):
                        continue
                    for B, kind in barrier_kinds(shape):
                        worst, nears, kinks = hp.check_barrier(eng.heston_barrier_paths(mkt, model, B, nd, spd, n, SEED, first, X, kind), sides, B, kind, tol, what)
                        print(f"{X} {shape} {name} first={first} anti={anti} {kind} B={B}: worst err/bound {worst:.3g}, {nears} near, {kinks} kink paths of {n}")
                        ran.add((name, kind, anti))
                firsts_met.add(first)
    finally:
        eng.set_antithetic(False)
    names = {name for name, _, _ in ran}
    assert {"STRONG", "FELLER"} <= names and ("VIOLATED" in names) == hr.runs("VIOLATED", X, m)
    assert {(name, "asian", anti) for name in names for anti in (False, True)} <= ran
    assert firsts_met == set(hr.FIRSTS)
    if X == "f64" or m <= hp.F32_BARRIER_MAX_STEPS:
        assert {(name, kind, anti) for name in names for _, kind in barrier_kinds(shape) for anti in (False, True)} <= ran
    assert hr.FIRSTS[-1] < (1 << 32) < hr.FIRSTS[-1] + n


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (7, 3), (16, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_knock_in_plus_knock_out_and_a_far_barrier_are_the_european_value(eng, X, shape):
    """... which is the one-date Asian value on the same total steps, within the two bounds."""
    nd, spd = shape
    m, n, first, tol = nd * spd, hr.N_PATHS, 4242, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, m)
    try:
        for name, mkt, model in hr.CASES:
            for anti in (False, True):
                eng.set_antithetic(anti)
                one = hp.walk(mkt, model, 1, m, z1, z2, anti)
                euro = eng.heston_asian_paths(mkt, model, 1, m, n, SEED, first, X).astype(np.float64)
                b = hp.european_bound(one, tol)[0] + hp.asian_bound(one, tol)[0]
                assert np.all(np.abs(euro - hp.european(one)) <= hp.asian_bound(one, tol)[0]), (name, anti)
                for B, (out, inn) in ((hp.UP, hp.KINDS[:2]), (hp.DOWN, hp.KINDS[2:])):
                    ko, ki = (eng.heston_barrier_paths(mkt, model, B, nd, spd, n, SEED, first, X, k).astype(np.float64) for k in (out, inn))
                    assert np.all(np.abs(ko + ki - euro) <= b), (name, anti, B)
                    assert np.count_nonzero(ko + ki) > 0
                far = eng.heston_barrier_paths(mkt, model, 1e30, nd, spd, n, SEED, first, X, "up-and-out").astype(np.float64)
                assert np.all(np.abs(far - euro) <= b), (name, anti)
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("nd", [2, 7, 64])
def test_constant_variance_and_antithetic_identities(eng, X, nd):
    n, first, tol = hr.N_PATHS, 99, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, nd)
    try:
        for name, mkt, model in hr.CASES:
            # xi = kappa = 0, one step per date: asian_ref's and barrier_ref's constant-volatility models on z1
            flat, o = dict(model, xi=0.0, kappa=0.0), dict(mkt, v=math.sqrt(model["v0"]))
            sides = hp.walk(mkt, flat, nd, 1, z1, z2)
            eng.set_antithetic(False)
            got = eng.heston_asian_paths(mkt, flat, nd, 1, n, SEED, first, X).astype(np.float64)
            b, kink = hp.asian_bound(sides, tol)
            assert not kink.any() and np.all(np.abs(got - asian_ref.asian(o, nd, z1).value[0]) <= b), name
            for B, kind in ((hp.UP, "up-and-out"), (hp.DOWN, "down-and-in")):
                want = barrier_ref.barrier(o, B, nd, z1, kind).value[0]
                assert np.allclose(hp.barrier(sides, B, kind), want, rtol=1e-12, atol=1e-12)
                got = eng.heston_barrier_paths(mkt, flat, B, nd, 1, n, SEED, first, X, kind)
                r, near, _ = hp.barrier_errors(got, sides, B, kind, tol)
                assert np.all(r <= 1.0) and near.sum() <= hp.NEAR_CAP * n, (name, kind)
            # antithetic = the mean of the two one-sided values of the model
            if hr.runs(name, X, nd):
                up, down = hp.walk(mkt, model, nd, 1, z1, z2), hp.walk(mkt, model, nd, 1, -z1, -z2)
                eng.set_antithetic(True)
                got = eng.heston_asian_paths(mkt, model, nd, 1, n, SEED, first, X).astype(np.float64)
                b = 0.5 * (hp.asian_bound(up, tol)[0] + hp.asian_bound(down, tol)[0])
                assert np.all(np.abs(got - 0.5 * (hp.asian(up) + hp.asian(down))) <= b), name
                got = eng.heston_barrier_paths(mkt, model, hp.UP, nd, 1, n, SEED, first, X, "up-and-in")
                r, _, _ = hp.barrier_errors(got, up + down, hp.UP, "up-and-in", tol)
                assert np.all(r <= 1.0), name
    finally:
        eng.set_antithetic(False)


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    nd, spd, n, first, chunk = 4, 4, 300_000, 777, 50_000
    tol = TOL[X]["pay"]
    zs = [normals(eng, X, f, min(chunk, first + n - f), nd * spd) for f in range(first, first + n, chunk)]
    try:
        for name, mkt, model in hr.CASES[:2]:
            walks = [hp.walk(mkt, model, nd, spd, z1, z2, anti=True) for z1, z2 in zs]
            for anti in (False, True):
                eng.set_antithetic(anti), few.set_antithetic(anti)
                parts = walks if anti else [w[:1] for w in walks]
                for payoff in ("asian", "barrier"):
                    if payoff == "asian":
                        v = np.concatenate([hp.asian(p) for p in parts])
                        b = np.concatenate([hp.asian_bound(p, tol)[0] for p in parts])
                        run = lambda e: e.heston_asian(mkt, model, nd, spd, n, SEED, first, X)
                    else:
                        v = np.concatenate([hp.barrier(p, hp.UP, "up-and-out") for p in parts])
                        b = np.concatenate([hp.barrier_bound(p, hp.UP, "up-and-out", tol)[0] for p in parts])
                        run = lambda e: e.heston_barrier(mkt, model, hp.UP, nd, spd, n, SEED, first, X, "up-and-out")
                    t1, t2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                    for e in (eng, few):
                        g = run(e)
                        if e is few:
                            assert trip_guard(e, 16, n) == 48   # full trips a lane
                        assert g.n == v.size == n
                        print(f"{X} {name} {payoff} anti={anti} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {t1:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {t2:.3g})")
                        assert abs(g.sum - v.sum()) <= t1 and abs(g.sum2 - (v * v).sum()) <= t2, (name, payoff, anti, e.blocks)
                        r, t = (float(np.float32(mkt[c])) if X == "f32" else mkt[c] for c in "rt")   # as the precision's struct holds them
                        assert g.expected == pytest.approx(math.exp(-r * t) * g.sum / n, rel=1e-14)
                        dev = math.sqrt((n * g.sum2 - g.sum * g.sum) / (n * (n - 1.0)))
                        assert g.confidence == pytest.approx(1.96 * dev / math.sqrt(n), rel=1e-12)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 4. bit rules -----------------------------------------------------------------------------------------------------
def calls(e, o, md, nd, spd, X, payoff):
    """(paths(n, first), run(n, first), the inputs of `prepared`) of one payoff."""
    if payoff == "asian":
        return (lambda n, f: e.heston_asian_paths(o, md, nd, spd, n, SEED, f, X), lambda n, f: e.heston_asian(o, md, nd, spd, n, SEED, f, X),
                dict(o, **md, n_dates=nd, steps_per_date=spd, payoff="asian"))
    return (lambda n, f: e.heston_barrier_paths(o, md, 70.0, nd, spd, n, SEED, f, X, "down-and-out"),
            lambda n, f: e.heston_barrier(o, md, 70.0, nd, spd, n, SEED, f, X, "down-and-out"),
            dict(o, **md, n_dates=nd, steps_per_date=spd, payoff="barrier", barrier=70.0, kind="down-and-out"))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("payoff", ["asian", "barrier"])
def test_bit_rules(mc, eng, X, payoff):
    import torch
    (o, md), nd, spd, f, n = ODD, 5, 3, 3001, 2500
    other = mc.Engine(0, blocks=96)
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            paths, run, inputs = calls(eng, o, md, nd, spd, X, payoff)
            whole, lo, part = paths(f + n, 0), paths(f, 0), paths(n, f)
            assert np.array_equal(np.concatenate([lo, part]), whole)                       # [0, n) = [0, k) u [k, n), bitwise per path
            assert np.count_nonzero(whole) > 0
            assert np.array_equal(calls(other, o, md, nd, spd, X, payoff)[0](n, f), part)    # not on the launch geometry
            fused = run(123_457, f)
            eng.set_finish(False)
            two = run(123_457, f)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)            # nor on the finish form
            # the launch form's triple is the run form's
            struct, keep = eng.prepared("heston_path", X, inputs)
            eng.launch("heston_path", X, struct, SEED, f, 123_457, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (fused.sum, fused.sum2, float(fused.n))
            # ranges add up
            a, b = run(50_001, f), run(123_457 - 50_001, f + 50_001)
            assert a.n + b.n == fused.n
            assert a.sum + b.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"]) and a.sum2 + b.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
    finally:
        eng.set_finish(True)
        eng.set_antithetic(False)
        other.close()


# ---- 5. prices --------------------------------------------------------------------------------------------------------
N_PRICE = 10_000_000


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("spd", [1, 4])
def test_constant_variance_prices_agree_with_the_constant_volatility_products(eng, X, spd):
    """xi = kappa = 0: the log-Euler walk is exact at constant variance whatever steps_per_date is, so the Asian call prices what
    Engine.asian (control variate on) prices and the up-and-out call what Engine.barrier (discrete) prices.  Independent samples
    (other domains), one seed, 3 x the sum of the two half-widths."""
    nd, mkt = 16, hr.ATM
    flat, o = dict(hr.FELLER, xi=0.0, kappa=0.0), dict(hr.ATM, v=math.sqrt(hr.FELLER["v0"]))
    a = eng.heston_asian(mkt, flat, nd, spd, N_PRICE, SEED, 0, X)
    b = eng.heston_barrier(mkt, flat, hp.UP, nd, spd, N_PRICE, SEED, 0, X, "up-and-out")
    try:
        eng.set_control_variate(True)
        a0 = eng.asian(o, nd, N_PRICE, SEED, 0, X)
    finally:
        eng.set_control_variate(False)
    b0 = eng.barrier(o, hp.UP, nd, N_PRICE, SEED, 0, X, "up-and-out", "discrete")
    print(f"{X} 16x{spd}: asian {a.expected:.6f} +- {a.confidence:.2g} vs {a0.expected:.6f} +- {a0.confidence:.2g}; "
          f"up-and-out {b.expected:.6f} +- {b.confidence:.2g} vs {b0.expected:.6f} +- {b0.confidence:.2g}")
    assert abs(a.expected - a0.expected) <= 3 * (a.confidence + a0.confidence)
    assert abs(b.expected - b0.expected) <= 3 * (b.confidence + b0.confidence)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("name", ["STRONG", "FELLER"])
def test_one_date_price_against_the_closed_form_within_the_schemes_bias(mc, eng, X, name):
    """n_dates = 1 is the European call: |GPU price - closed form| <= 3 GPU half-widths + |b| + 3 h of heston_ref.BIAS, the bias of the
    scheme at 64 steps measured on the model, never on the kernel."""
    mkt, model = hr.ATM, hr.MODELS[name]
    exact = mc.heston_closed_form(mkt, model)
    bias, h = hr.BIAS[name]
    try:
        eng.set_antithetic(True)
        e = eng.heston_asian(mkt, model, 1, hr.BIAS_STEPS, N_PRICE, SEED, 0, X)
    finally:
        eng.set_antithetic(False)
    print(f"{X} {name}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
    assert abs(e.expected - exact) <= 3 * e.confidence + abs(bias) + 3 * h


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_average_is_worth_less_than_the_final_value(eng, X):
    """12 dates x 21 steps, FELLER at the money: the Asian price lies below the European price of the same walk (n_dates = 1 on the
    same 252 steps) by more than 3 summed half-widths."""
    mkt, model = hr.ATM, hr.FELLER
    a = eng.heston_asian(mkt, model, 12, 21, N_PRICE, SEED, 0, X)
    e = eng.heston_asian(mkt, model, 1, 252, N_PRICE, SEED, 0, X)
    print(f"{X}: asian {a.expected:.6f} +- {a.confidence:.2g}, european {e.expected:.6f} +- {e.confidence:.2g}")
    assert a.expected < e.expected - 3 * (a.confidence + e.confidence)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc):
    o, md, nd, spd, n = hr.ATM, hr.FELLER, 4, 3, 50_000
    with mc.Engine(0) as fresh:
        want = {X: (fresh.heston(o, md, 12, n, SEED, 0, X), fresh.heston_asian(o, md, nd, spd, n, SEED, 0, X)) for X in ("f32", "f64")}

    def still_fine(e):
        for X, (w0, w1) in want.items():
            g0, g1 = e.heston(o, md, 12, n, SEED, 0, X), e.heston_asian(o, md, nd, spd, n, SEED, 0, X)
            assert (g0.sum, g0.sum2, g0.n, g1.sum, g1.sum2, g1.n) == (w0.sum, w0.sum2, w0.n, w1.sum, w1.sum2, w1.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    nan, inf = float("nan"), float("inf")
    L = mc._lib

    def run(e, X, opt=o, model=md, nd=nd, spd=spd, payoff="asian", barrier=hp.UP, kind="up-and-out", n=n, n_steps=None):
        """mc_heston_path_run_* on a struct built field by field, so that n_steps need not be n_dates * steps_per_date."""
        from montecarlocuda_amd.engine import _as_heston, check
        s = L.HESTON_PATH[X](_as_heston(X, opt, model, nd * spd if n_steps is None else n_steps), spd,
                             L.HESTON_PATH_PAYOFFS[payoff] if isinstance(payoff, str) else payoff,
                             L.BARRIER_TYPES[kind] if isinstance(kind, str) else kind, barrier)
        r = L.Result()
        check(getattr(L.lib(), f"mc_heston_path_run_{X}")(e._ctx, C.byref(s), SEED, 0, n, C.byref(r)))
        return r

    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for payoff in ("asian", "barrier"):
                # everything mc_heston_check_* refuses
                for bad_steps in (0, -3, L.MAX_HESTON_STEPS + 1):
                    with pytest.raises(mc.McError, match=INVALID):
                        run(e, X, payoff=payoff, spd=1, n_steps=bad_steps)
                for bad in (dict(o, s=0.0), dict(o, s=-3.0), dict(o, t=0.0), dict(o, t=-1.0), dict(o, r=inf), dict(o, k=nan), dict(o, s=inf), dict(o, t=nan)):
                    with pytest.raises(mc.McError, match=INVALID):
                        run(e, X, opt=bad, payoff=payoff)
                for f in ("v0", "kappa", "theta", "xi"):
                    for v in (-0.01, nan, inf):
                        with pytest.raises(mc.McError, match=INVALID):
                            run(e, X, model=dict(md, **{f: v}), payoff=payoff)
                for v in (1.001, -1.001, nan, inf):
                    with pytest.raises(mc.McError, match=INVALID):
                        run(e, X, model=dict(md, rho=v), payoff=payoff)
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, payoff=payoff, n=0)                                   # the range errors of the other products
                with pytest.raises(mc.McError, match="outside the range of a double"):
                    run(e, X, model=dict(md, xi=3e4), nd=L.MAX_HESTON_STEPS, spd=1, payoff=payoff)   # the exponent-range guard
                # the dates
                for bad_spd in (0, -1, 5, 7, 13):
                    with pytest.raises(mc.McError, match=INVALID):
                        run(e, X, spd=bad_spd, n_steps=12, payoff=payoff)
            still_fine(e)
            for bad_payoff in (-1, 2, 7):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, payoff=bad_payoff)
            # the barrier
            for bad_kind in (-1, 4):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, payoff="barrier", kind=bad_kind)
            for bad_b in (0.0, -5.0, nan, inf):
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, payoff="barrier", barrier=bad_b)
            for bad_b, kind in ((100.0, "up-and-out"), (90.0, "up-and-in"), (100.0, "down-and-out"), (110.0, "down-and-in")):
                with pytest.raises(mc.McError, match="on or beyond"):
                    run(e, X, payoff="barrier", barrier=bad_b, kind=kind)
            still_fine(e)
            # the Asian payoff ignores barrier and barrier_type
            w = want[X][1]
            for bad_b, kind in ((nan, 0), (-1.0, 99), (100.0, "up-and-out")):
                assert run(e, X, barrier=bad_b, kind=kind).sum == w.sum
            # valid corners
            for okm in (dict(md, xi=0.0), dict(md, kappa=0.0), dict(md, rho=1.0), dict(md, rho=-1.0), hr.VIOLATED, dict(md, v0=0.0)):
                assert np.isfinite(e.heston_asian(o, okm, nd, spd, n, SEED, 0, X).expected)
                assert np.isfinite(e.heston_barrier(o, okm, hp.UP, nd, spd, n, SEED, 0, X).expected)
            assert np.isfinite(e.heston_asian(o, md, 1, 12, n, SEED, 0, X).expected)       # steps_per_date = n_steps
            assert np.isfinite(e.heston_barrier(o, md, hp.DOWN, 1, 12, n, SEED, 0, X, "down-and-in").expected)
            e.set_control_variate(True)
            for payoff in ("asian", "barrier"):
                with pytest.raises(mc.McError, match=UNSUPPORTED):
                    run(e, X, payoff=payoff)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            run(e, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 7. driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prints_the_heston_prices_next_to_their_constant_volatility_neighbours(X):
    exe = os.path.join(ROOT, "drivers", f"hestonPathOpt_{X}")
    assert os.path.exists(exe), f"drivers/hestonPathOpt_{X} not built (build())"
    out = subprocess.run([exe, "12", "21", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(\w+) price=(\S+) ci=(\S+) kernel_ms=\S+ diff_in_ci=\S+", out.stdout, re.M)}
    heston = ["asian_plain", "asian_antithetic", "up_out_plain", "up_out_antithetic"]
    assert set(row) == set(heston) | {"flat_asian", "mc_asian", "flat_up_out", "mc_barrier"}, out.stdout
    for k in row:
        assert all(math.isfinite(v) for v in row[k]) and row[k][0] > 0 and row[k][1] > 0, out.stdout
    assert row["asian_antithetic"][1] < row["asian_plain"][1] and row["up_out_antithetic"][1] < row["up_out_plain"][1], out.stdout
    for a, b in (("flat_asian", "mc_asian"), ("flat_up_out", "mc_barrier")):
        assert abs(row[a][0] - row[b][0]) <= 3 * (row[a][1] + row[b][1]), out.stdout
