"""The Heston call on the GPU (heston_kernel, mc_heston_*): every path against the independent float64 model heston_ref.py on the
kernels' own normals (Engine.normals, domain 6), for both precisions, antithetic off and on, step counts around every loop
boundary (the fp32 loop takes 2 steps per Philox block, the fp64 loop 4 pairs per trip, then 1) and path ranges across the
2^32-unit seam; exact identities per path; the sums of a call of many grid-stride trips; the bit rules of the stream; the launch
form; prices end to end, exact where the scheme has no bias (xi = 0) and within the model's own measured bias where it has;
refusals; the C driver.

Tolerances: heston_ref.bound(paths, TOL[X]["pay"]) (TOL: tests/test_gpu_parity.py) per path -- the model's first-order forward error
with the square root's min(e / sqrt V+, sqrt e) at the truncation; no path is left out; the bound on a sum is the sum of the per-path
bounds.  tests/test_heston_ref.py holds the kink paths of these shapes under heston_ref.KINK_CAP and shows the bound's power."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

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
    return hr.heston_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, hr.NPB[X])


def check(got, p, tol, what):
    """Every value finite, >= 0 and within its bound.  Returns (worst error / bound, number of kink paths)."""
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    b, kink = hr.bound(p, tol)
    r = np.abs(got - p.value[0]) / b
    assert np.all(r <= 1.0), (what, int(np.argmax(r)), float(r.max()))
    return float(r.max()), int(kink.sum())


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", hr.STEPS)
def test_every_path_against_the_reference(mc, eng, X, m):
    assert hr.STEPS[-1] == mc._lib.MAX_HESTON_STEPS
    n, tol = hr.n_paths_for(m), TOL[X]["pay"]
    ran = set()
    try:
        for name, mkt, model in hr.cases_for(m):
            if not hr.runs(name, X, m):
                continue
            for first in hr.FIRSTS:
                z1, z2 = normals(eng, X, first, n, m)
                both = hr.walk(mkt, model, m, z1, z2, anti=True)
                for anti, p in ((False, hr.plain_of(both)), (True, both)):
                    eng.set_antithetic(anti)
                    got = eng.heston_paths(mkt, model, m, n, SEED, first, X)
                    worst, kinks = check(got, p, tol, (name, m, first, anti))
                    print(f"{X} m={m} {name} first={first} anti={anti}: worst err/bound {worst:.3g}, {kinks} kink paths of {n}")
                    assert kinks <= hr.KINK_CAP * n, (name, m, kinks)
                    ran.add((name, first, anti))
    finally:
        eng.set_antithetic(False)
    names = {name for name, _, _ in ran}
    assert {"STRONG", "FELLER"} <= names and ("VIOLATED" in names) == hr.runs("VIOLATED", X, m)
    # every case that ran met all three ranges, the one across the 2^32-unit seam included, with antithetic off and on
    assert ran == {(name, first, anti) for name in names for first in hr.FIRSTS for anti in (False, True)}
    assert hr.FIRSTS[-1] < (1 << 32) < hr.FIRSTS[-1] + n


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_one_step_is_the_vanilla_payoff_at_the_starting_volatility(eng, X):
    """V is used only at step 0: whatever kappa, theta, xi and rho are, m = 1 is the vanilla payoff at volatility sqrt(v0) on z1."""
    n, first, tol = hr.N_PATHS, 4242, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, 1)
    for name, mkt, model in hr.CASES + [("ODD",) + ODD]:
        v = math.sqrt(model["v0"])
        want = np.maximum(mkt["s"] * np.exp((mkt["r"] - 0.5 * v * v) * mkt["t"] + v * math.sqrt(mkt["t"]) * z1[:, 0]) - mkt["k"], 0.0)
        b, _ = hr.bound(hr.walk(mkt, model, 1, z1, z2), tol)
        for other in (model, dict(model, kappa=9.0, theta=0.5, xi=2.0, rho=0.9)):
            got = eng.heston_paths(mkt, other, 1, n, SEED, first, X).astype(np.float64)
            assert np.all(np.abs(got - want) <= b), name


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [2, 7, 64, 257])
def test_constant_variance_and_antithetic_identities(eng, X, m):
    n, first, tol = hr.N_PATHS, 99, TOL[X]["pay"]
    z1, z2 = normals(eng, X, first, n, m)
    try:
        for name, mkt, model in hr.CASES:
            # xi = 0, kappa = 0: the constant-volatility walk, x_m = ln S0 + (r - v0/2) T + sqrt(v0 dt) sum z1
            flat = dict(model, xi=0.0, kappa=0.0)
            v0, dt = model["v0"], mkt["t"] / m
            want = np.maximum(mkt["s"] * np.exp((mkt["r"] - 0.5 * v0) * mkt["t"] + math.sqrt(v0 * dt) * z1.sum(axis=1)) - mkt["k"], 0.0)
            eng.set_antithetic(False)
            got = eng.heston_paths(mkt, flat, m, n, SEED, first, X).astype(np.float64)
            b, kink = hr.bound(hr.walk(mkt, flat, m, z1, z2), tol)
            assert not kink.any() and np.all(np.abs(got - want) <= b), name
            # antithetic = the mean of the two one-sided values of the model
            if hr.runs(name, X, m):
                up, down = hr.walk(mkt, model, m, z1, z2), hr.walk(mkt, model, m, -z1, -z2)
                eng.set_antithetic(True)
                got = eng.heston_paths(mkt, model, m, n, SEED, first, X).astype(np.float64)
                b = 0.5 * (hr.bound(up, tol)[0] + hr.bound(down, tol)[0])
                assert np.all(np.abs(got - 0.5 * (up.value[0] + down.value[0])) <= b), name
    finally:
        eng.set_antithetic(False)


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    m, n, first, chunk = 16, 300_000, 777, 50_000
    tol = TOL[X]["pay"]
    zs = [normals(eng, X, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for name, mkt, model in hr.CASES[:2]:
            walks = [hr.walk(mkt, model, m, z1, z2, anti=True) for z1, z2 in zs]
            for anti in (False, True):
                eng.set_antithetic(anti), few.set_antithetic(anti)
                parts = walks if anti else [hr.plain_of(w) for w in walks]
                v = np.concatenate([p.value[0] for p in parts])
                b = np.concatenate([hr.bound(p, tol)[0] for p in parts])
                t1, t2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                for e in (eng, few):
                    g = e.heston(mkt, model, m, n, SEED, first, X)
                    if e is few:
                        assert trip_guard(e, 16, n) == 48   # full trips a lane
                    assert g.n == v.size == n
                    print(f"{X} {name} anti={anti} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {t1:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {t2:.3g})")
                    assert abs(g.sum - v.sum()) <= t1 and abs(g.sum2 - (v * v).sum()) <= t2, (name, anti, e.blocks)
                    r, t = (float(np.float32(mkt[c])) if X == "f32" else mkt[c] for c in "rt")   # as the precision's struct holds them
                    assert g.expected == pytest.approx(math.exp(-r * t) * g.sum / n, rel=1e-14)
                    dev = math.sqrt((n * g.sum2 - g.sum * g.sum) / (n * (n - 1.0)))
                    assert g.confidence == pytest.approx(1.96 * dev / math.sqrt(n), rel=1e-12)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 4. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    import torch
    (o, md), m, f, n = ODD, 13, 3001, 2500
    other = mc.Engine(0, blocks=96)
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            whole = eng.heston_paths(o, md, m, f + n, SEED, 0, X)
            lo, part = eng.heston_paths(o, md, m, f, SEED, 0, X), eng.heston_paths(o, md, m, n, SEED, f, X)
            assert np.array_equal(np.concatenate([lo, part]), whole)                       # [0, n) = [0, k) u [k, n), bitwise per path
            assert np.array_equal(other.heston_paths(o, md, m, n, SEED, f, X), part)         # not on the launch geometry
            fused = eng.heston(o, md, m, 123_457, SEED, f, X)
            eng.set_finish(False)
            two = eng.heston(o, md, m, 123_457, SEED, f, X)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)            # nor on the finish form
            # the launch form's triple is the run form's
            struct, keep = eng.prepared("heston", X, dict(o, **md, n_steps=m))
            eng.launch("heston", X, struct, SEED, f, 123_457, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (fused.sum, fused.sum2, float(fused.n))
            # ranges add up
            a, b = eng.heston(o, md, m, 50_001, SEED, f, X), eng.heston(o, md, m, 123_457 - 50_001, SEED, f + 50_001, X)
            assert a.n + b.n == fused.n
            assert a.sum + b.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"]) and a.sum2 + b.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
    finally:
        eng.set_finish(True)
        eng.set_antithetic(False)
        other.close()


# ---- 5. exact prices, no discretisation bias ------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16, 257])
def test_deterministic_variance_prices_black_scholes(eng, X, m):
    """xi = 0 with v0 != theta: the Euler log-price is Gaussian with variance sum_j V+_{j-1} dt (heston_ref.euler_variance_path), so the
    scheme's price is Black-Scholes at that variance exactly.  One fixed seed, 1e7 paths, 3 half-widths (5.9 sigma: the margin is
    for sampling noise alone, as in tests/test_gpu_barrier.py)."""
    mkt, model = hr.ATM, dict(v0=0.09, kappa=2.0, theta=0.03, xi=0.0, rho=-0.7)
    _, var = hr.euler_variance_path(model, m, mkt["t"])
    exact = hr.black_scholes_call(dict(mkt, v=math.sqrt(var / mkt["t"])))
    e = eng.heston(mkt, model, m, 10_000_000, SEED, 0, X)
    print(f"{X} m={m}: expected {e.expected:.6f} Black-Scholes at the Euler variance {exact:.6f} confidence {e.confidence:.2g}")
    assert abs(e.expected - exact) <= 3 * e.confidence


# ---- 6. the closed form, xi > 0 -------------------------------------------------------------------------------------------
def bias_margin(name):
    b, h = hr.BIAS[name]
    return abs(b) + 3 * h


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("name", ["STRONG", "FELLER"])
def test_price_against_the_closed_form_within_the_schemes_bias(mc, eng, X, name):
    """Full-truncation Euler is biased; the bias at 64 steps was measured on the reference model, never on the kernel
    (heston_ref.BIAS: b and its half-width h).  |GPU price - closed form| <= 3 GPU half-widths + |b| + 3 h."""
    mkt, model = hr.ATM, hr.MODELS[name]
    exact = mc.heston_closed_form(mkt, model)
    assert abs(exact - hr.closed_form(mkt, model)) <= 1e-11
    try:
        eng.set_antithetic(True)
        e = eng.heston(mkt, model, hr.BIAS_STEPS, 10_000_000, SEED, 0, X)
    finally:
        eng.set_antithetic(False)
    print(f"{X} {name}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g} bias margin {bias_margin(name):.3g}")
    assert abs(e.expected - exact) <= 3 * e.confidence + bias_margin(name)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    o, md, m, n = hr.ATM, hr.FELLER, 12, 50_000
    with mc.Engine(0) as fresh:
        want = {X: fresh.heston(o, md, m, n, SEED, 0, X) for X in ("f32", "f64")}

    def still_fine(e):
        for X, w in want.items():
            got = e.heston(o, md, m, n, SEED, 0, X)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    nan, inf = float("nan"), float("inf")
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, -1, mc._lib.MAX_HESTON_STEPS + 1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.heston(o, md, bad_m, n, SEED, 0, X)
            still_fine(e)
            for bad in (dict(o, s=0.0), dict(o, s=-3.0), dict(o, t=0.0), dict(o, t=-1.0), dict(o, r=inf), dict(o, k=nan), dict(o, s=inf), dict(o, t=nan)):
                with pytest.raises(mc.McError, match=INVALID):
                    e.heston(bad, md, m, n, SEED, 0, X)
            for f in ("v0", "kappa", "theta", "xi"):
                for v in (-0.01, nan, inf):
                    with pytest.raises(mc.McError, match=INVALID):
                        e.heston(o, dict(md, **{f: v}), m, n, SEED, 0, X)
            for v in (1.001, -1.001, nan, inf):
                with pytest.raises(mc.McError, match=INVALID):
                    e.heston(o, dict(md, rho=v), m, n, SEED, 0, X)
            with pytest.raises(mc.McError, match=INVALID):
                e.heston(o, md, m, 0, SEED, 0, X)                      # the range errors of the other products
            with pytest.raises(mc.McError, match="outside the range of a double"):
                e.heston(o, dict(md, xi=3e4), mc._lib.MAX_HESTON_STEPS, n, SEED, 0, X)   # the heuristic guard of the device's exp
            still_fine(e)
            # valid corners: xi = 0, kappa = 0, |rho| = 1, a violated Feller condition, option.v anything
            for okm in (dict(md, xi=0.0), dict(md, kappa=0.0), dict(md, rho=1.0), dict(md, rho=-1.0), hr.VIOLATED, dict(md, v0=0.0)):
                assert np.isfinite(e.heston(o, okm, m, n, SEED, 0, X).expected)
            assert e.heston(dict(o, v=55.0), md, m, n, SEED, 0, X).sum == want[X].sum
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.heston(o, md, m, n, SEED, 0, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.heston(o, md, m, n, SEED, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.heston(o, md, m, n, SEED, 0, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 8. driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prints_estimates_next_to_the_closed_form(mc, X):
    exe = os.path.join(ROOT, "drivers", f"hestonOpt_{X}")
    assert os.path.exists(exe), f"drivers/hestonOpt_{X} not built (build())"
    out = subprocess.run([exe, str(hr.BIAS_STEPS), "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c), float(d)) for k, p, c, d in
           re.findall(r"^(plain|antithetic|closed_form) price=(\S+) ci=(\S+) kernel_ms=\S+ diff_in_ci=(\S+)", out.stdout, re.M)}
    assert set(row) == {"plain", "antithetic", "closed_form"}, out.stdout
    exact = row["closed_form"][0]
    assert exact == pytest.approx(mc.heston_closed_form(hr.ATM, hr.FELLER, X), rel=1e-12)   # the driver prices FELLER at the money
    for form in ("plain", "antithetic"):
        price, ci, diff = row[form]
        assert abs(price - exact) <= 3 * ci + bias_margin("FELLER"), out.stdout
        assert diff == pytest.approx((price - exact) / ci, abs=2e-3)
    assert row["antithetic"][1] < row["plain"][1]
