"""Calls and puts under a local-volatility surface on the GPU (localvol_kernel, mc_localvol_*): every path against the independent
float64 model localvol_ref.py on the kernels' own normals (Engine.normals, domain 16), the three payoffs, both rights, the four barrier
types, both precisions, antithetic off and on, over shapes (n_steps, n_times, steps_per_date, n_nodes) whose slice and date boundaries
meet every loop boundary (fp32: four steps per Philox block; fp64: eight per trip, then two), the table cap, a grid so narrow that both
clamps run, path ranges across the 2^32-unit seam and a lane's later grid-stride trips (engines of 16 and 1 blocks, with the sums); the flat surface against the constant-volatility
products; identities per path; sums; the bit rules of the stream; the launch form; prices end to end; refusals; the C driver.

Tolerances: localvol_ref's per-path bounds at TOL[X]["pay"] (TOL: tests/test_gpu_parity.py).  A barrier path whose distance to the
barrier is within its bound at some date may take either of its two values; no path is left out.  tests/test_localvol_ref.py holds the
near-barrier paths of these shapes under their cap and shows the bounds' power."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import localvol_ref as lv
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPX = {"f32": np.float32, "f64": np.float64}
BARRIERS = [(lv.UP, "up-and-out"), (lv.UP, "up-and-in"), (lv.DOWN, "down-and-out"), (lv.DOWN, "down-and-in")]


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


def normals(e, X, first, n, m):
    return lv.localvol_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, lv.NPB[X])


def every_payoff(e, X, o, surf, shape, first, n, z, barriers=True, what=(), sums=False):
    """All payoffs of one (shape, surface, range) per path against the model, plain and antithetic; sums: also {sum, sum2, n} of the run
    form on the same engine against that call's own dump (greeks_ref.check_sums).  Returns what ran."""
    m, nt, spd, nn = shape
    nd, tol = m // spd, TOL[X]["pay"]
    both = lv.walk(o, surf, nd, spd, z, anti=True, tol=tol, table=NPX[X])
    one = lv.walk(o, surf, 1, m, z, anti=True, tol=tol, table=NPX[X]) if nd > 1 else both
    ran = set()
    for anti, sides, last in ((False, both[:1], one[:1]), (True, both, one)):
        e.set_antithetic(anti)
        for right in ("call", "put"):
            w = what + (shape, first, anti, right)
            got = e.localvol_paths(o, surf, m, n, right, SEED, first, X)
            worst = lv.check(got, lv.european(last, right), lv.european_bound(last, right), w)
            print(f"{X} {w}: european worst err/bound {worst:.3g}")
            if sums:
                gr.check_sums(e.localvol(o, surf, m, n, right, SEED, first, X), got, n, w)
            got = e.localvol_asian_paths(o, surf, nd, spd, n, right, SEED, first, X)
            worst = lv.check(got, lv.asian(sides, right), lv.asian_bound(sides, right), w)
            print(f"{X} {w}: asian worst err/bound {worst:.3g}")
            if sums:
                gr.check_sums(e.localvol_asian(o, surf, nd, spd, n, right, SEED, first, X), got, n, w)
            ran |= {("european", right, anti), ("asian", right, anti)}
            if not barriers:
                continue
            for B, kind in BARRIERS:
                got = e.localvol_barrier_paths(o, surf, B, nd, spd, n, right, SEED, first, X, kind)
                worst, nears = lv.check_barrier(got, sides, B, kind, right, w)
                print(f"{X} {w} {kind}: worst err/bound {worst:.3g}, {nears} near paths of {n}")
                if sums:
                    gr.check_sums(e.localvol_barrier(o, surf, B, nd, spd, n, right, SEED, first, X, kind), got, n, w + (kind,))
                ran.add((kind, right, anti))
    return ran


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", lv.SHAPES, ids=str)
def test_every_path_against_the_reference(mc, eng, X, shape):
    """The wide grid on the first range, the narrow grid (both clamps) on the range across 2^32 units."""
    assert {s[0] for s in lv.SHAPES} == {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 64} and lv.BIG_SHAPE[0] == mc._lib.MAX_LOCALVOL_STEPS
    assert max(s[1] * s[3] for s in lv.SHAPES) == mc._lib.MAX_LOCALVOL_NODES
    m, n = shape[0], lv.N_PATHS
    ran = set()
    try:
        for grid, first in zip((lv.WIDE, lv.NARROW), lv.FIRSTS):
            ran |= every_payoff(eng, X, lv.MKT, lv.surface_for(shape, grid), shape, first, n, normals(eng, X, first, n, m), what=(grid,))
    finally:
        eng.set_antithetic(False)
    assert len(ran) == 2 * 2 * 6
    assert lv.FIRSTS[-1] < (1 << 32) < lv.FIRSTS[-1] + n


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_every_path_at_the_step_cap(mc, eng, X):
    shape = lv.BIG_SHAPE
    m, n, first = shape[0], lv.N_PATHS, lv.FIRSTS[0]
    try:
        ran = every_payoff(eng, X, lv.MKT, lv.surface_for(shape, lv.WIDE), shape, first, n, normals(eng, X, first, n, m),
                           barriers=X == "f64" or m <= lv.F32_BARRIER_MAX_STEPS)
    finally:
        eng.set_antithetic(False)
    assert ("asian", "put", True) in ran and (("up-and-in", "put", True) in ran) == (X == "f64")


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_every_path_of_a_lanes_later_trips(mc, eng, X, name):
    """On an engine of few blocks a lane takes several grid-stride trips (greeks_ref.TRIP_RANGES; B crosses 2^32 units, so its second
    launch writes behind the first): the LDS copy is made once, before the loop, and every later trip reads it.  All three payoffs, both
    rights, the four barrier types, plain and antithetic, per path, and the run form's sums on the same small engine.  The model's
    normals are drawn on the default engine: one-trip launches, off the path under test."""
    r = gr.TRIP_RANGES[name]
    shape = (9, 3, 3, 65)
    z = normals(eng, X, r.first, r.n, shape[0])
    with mc.Engine(0, blocks=r.blocks) as e:
        ran = every_payoff(e, X, lv.MKT, lv.surface_for(shape, lv.WIDE), shape, r.first, r.n, z, what=(name,), sums=True)
        trips = gr.trip_guard(e, r.blocks, gr.trip_last_segment(r))
        print(f"{X} {name}: {trips} full trips")
    assert trips >= 2 and len(ran) == 2 * 2 * 6


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("nd", [1, 5, 16])
def test_a_flat_surface_is_the_constant_volatility_products(eng, X, nd):
    """... per path: asian_paths, barrier_paths and the vanilla payoff draw other domains, so the comparison is through the models, which
    tests/test_localvol_ref.py ties to asian_ref and barrier_ref at 1e-12; here the kernel on a flat surface against them directly."""
    import asian_ref
    import barrier_ref
    n, first, tol = lv.N_PATHS, 99, TOL[X]["pay"]
    o = dict(lv.MKT, v=0.23)
    z = normals(eng, X, first, n, nd)
    for nt, nn in ((1, 2), (nd, 3)):
        surf = lv.make_surface(np.full((nt, nn), o["v"]), -0.2, 0.3)
        sides = lv.walk(o, surf, nd, 1, z, tol=tol, table=NPX[X])
        ro = lv.rounded(o, NPX[X])
        got = eng.localvol_asian_paths(o, surf, nd, 1, n, "call", SEED, first, X).astype(np.float64)
        assert np.all(np.abs(got - asian_ref.asian(ro, nd, z).value[0]) <= lv.asian_bound(sides)), (nt, nn)
        for B, kind in BARRIERS:
            want = barrier_ref.barrier(ro, B, nd, z, kind).value[0]
            assert np.allclose(lv.barrier(sides, B, kind), want, rtol=1e-12, atol=1e-12)
            lv.check_barrier(eng.localvol_barrier_paths(o, surf, B, nd, 1, n, "call", SEED, first, X, kind), sides, B, kind, "call", (nt, nn))
        one = lv.walk(o, surf, 1, nd, z, tol=tol, table=NPX[X])
        S = ro["s"] * np.exp((ro["r"] - 0.5 * float(NPX[X](o["v"])) ** 2) * ro["t"] + float(NPX[X](o["v"])) * math.sqrt(ro["t"] / nd) * z.sum(axis=1))
        for right, sgn in (("call", 1.0), ("put", -1.0)):
            got = eng.localvol_paths(o, surf, nd, n, right, SEED, first, X).astype(np.float64)
            assert np.all(np.abs(got - np.maximum(sgn * (S - ro["k"]), 0.0)) <= lv.european_bound(one, right) + 1e-12 * S), (nt, nn, right)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (7, 1, 1, 65), (9, 3, 3, 65), (16, 2, 2, 3)], ids=str)
def test_knock_in_plus_knock_out_is_the_european_value(eng, X, shape):
    m, nt, spd, nn = shape
    n, first, tol = lv.N_PATHS, 4242, TOL[X]["pay"]
    surf = lv.surface_for(shape, lv.WIDE)
    z = normals(eng, X, first, n, m)
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            one = lv.walk(lv.MKT, surf, 1, m, z, anti, tol=tol, table=NPX[X])
            for right in ("call", "put"):
                euro = eng.localvol_paths(lv.MKT, surf, m, n, right, SEED, first, X).astype(np.float64)
                b = 2.0 * lv.european_bound(one, right)
                for B, (out, inn) in ((lv.UP, lv.KINDS[:2]), (lv.DOWN, lv.KINDS[2:])):
                    ko, ki = (eng.localvol_barrier_paths(lv.MKT, surf, B, m // spd, spd, n, right, SEED, first, X, k).astype(np.float64) for k in (out, inn))
                    assert np.all(np.abs(ko + ki - euro) <= b), (anti, right, B)
                    assert np.count_nonzero(ko + ki) > 0
                far = eng.localvol_barrier_paths(lv.MKT, surf, 1e30, m // spd, spd, n, right, SEED, first, X, "up-and-out").astype(np.float64)
                assert np.all(np.abs(far - euro) <= b), (anti, right)
    finally:
        eng.set_antithetic(False)


# ---- 3. sums, bit rules, launch form ----------------------------------------------------------------------------------
def calls(e, surf, nd, spd, X, payoff, right):
    o = lv.MKT
    if payoff == "european":
        return (lambda n, f: e.localvol_paths(o, surf, nd * spd, n, right, SEED, f, X), lambda n, f: e.localvol(o, surf, nd * spd, n, right, SEED, f, X),
                dict(o, **surf, n_dates=1, steps_per_date=nd * spd, payoff="european", right=right))
    if payoff == "asian":
        return (lambda n, f: e.localvol_asian_paths(o, surf, nd, spd, n, right, SEED, f, X), lambda n, f: e.localvol_asian(o, surf, nd, spd, n, right, SEED, f, X),
                dict(o, **surf, n_dates=nd, steps_per_date=spd, payoff="asian", right=right))
    return (lambda n, f: e.localvol_barrier_paths(o, surf, lv.DOWN, nd, spd, n, right, SEED, f, X, "down-and-out"),
            lambda n, f: e.localvol_barrier(o, surf, lv.DOWN, nd, spd, n, right, SEED, f, X, "down-and-out"),
            dict(o, **surf, n_dates=nd, steps_per_date=spd, payoff="barrier", right=right, barrier=lv.DOWN, kind="down-and-out"))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("payoff,right", [("european", "put"), ("asian", "call"), ("barrier", "call")])
def test_sums_and_bit_rules(mc, eng, X, payoff, right):
    import torch
    nd, spd, f, n = 5, 3, 3001, 2500
    surf = lv.wavy_surface(3, 65, *lv.WIDE)
    other = mc.Engine(0, blocks=96)
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            paths, run, inputs = calls(eng, surf, nd, spd, X, payoff, right)
            whole, lo, part = paths(f + n, 0), paths(f, 0), paths(n, f)
            assert np.array_equal(np.concatenate([lo, part]), whole)                       # a range split in two, bitwise per path
            assert np.array_equal(paths(n, f), part)                                       # the same call twice
            assert np.count_nonzero(whole) > 0
            assert np.array_equal(calls(other, surf, nd, spd, X, payoff, right)[0](n, f), part)   # not on the launch geometry
            gr.check_sums(run(n, f), part, n, (payoff, anti))                              # the sums of _paths against _run
            big = 123_457
            fused = run(big, f)
            again = run(big, f)
            assert (fused.sum, fused.sum2, fused.n) == (again.sum, again.sum2, again.n)      # the same call twice
            eng.set_finish(False)
            two = run(big, f)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)            # nor on the finish form
            # the launch form's triple is the run form's, and mc_closing closes it
            struct, keep = eng.prepared("localvol", X, inputs)
            eng.launch("localvol", X, struct, SEED, f, big, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (fused.sum, fused.sum2, float(fused.n))
            r, t = (float(NPX[X](lv.MKT[c])) for c in "rt")
            expected, confidence = mc.closing(fused.sum, fused.sum2, fused.n, math.exp(-r * t))
            assert (expected, confidence) == (fused.expected, fused.confidence)
            a, b = run(50_001, f), run(big - 50_001, f + 50_001)
            assert a.n + b.n == fused.n
            assert a.sum + b.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"]) and a.sum2 + b.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
    finally:
        eng.set_finish(True)
        eng.set_antithetic(False)
        other.close()


def test_the_surface_is_copied_during_the_call_and_cached_by_content(mc, eng):
    """Two surfaces alternate on one context, and another product's table in between: each call prices its own surface."""
    o, n = lv.MKT, 5000
    s1, s2 = lv.wavy_surface(2, 65, *lv.WIDE), lv.wavy_surface(3, 3, *lv.NARROW)
    w1, w2 = eng.localvol_paths(o, s1, 6, n, "call", SEED, 0, "f64"), eng.localvol_paths(o, s2, 6, n, "call", SEED, 0, "f64")
    assert not np.array_equal(w1, w2)
    eng.asian(dict(o, v=0.2), 4096, 1000, SEED, 0, "f64")
    assert np.array_equal(eng.localvol_paths(o, s1, 6, n, "call", SEED, 0, "f64"), w1)
    assert np.array_equal(eng.localvol_paths(o, s2, 6, n, "call", SEED, 0, "f64"), w2)
    assert np.array_equal(eng.localvol_paths(o, lv.wavy_surface(32, 64, *lv.WIDE), 64, n, "call", SEED, 0, "f64"),
                          eng.localvol_paths(o, lv.wavy_surface(32, 64, *lv.WIDE), 64, n, "call", SEED, 0, "f64"))
    assert np.array_equal(eng.localvol_paths(o, s1, 6, n, "call", SEED, 0, "f64"), w1)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_no_pointer_to_the_surface_is_retained(mc, eng, X):
    """The caller's array is overwritten in place after a call, then freed: a replay through the launch form with the SAME struct prices
    the new content, and a fresh array with the first content prices what the first call did -- neither reads memory of an earlier call."""
    import torch
    o, n, f = lv.MKT, 123_457, 3001
    s1, s2 = lv.wavy_surface(2, 65, *lv.WIDE), lv.wavy_surface(2, 65, *lv.NARROW)
    inputs = lambda s: dict(o, **dict(s, sigma=s["sigma"].copy()), n_dates=3, steps_per_date=2, payoff="asian", right="put")   # an array of the call's own
    want1, want2 = (eng.localvol_asian(o, s, 3, 2, n, "put", SEED, f, X) for s in (s1, s2))
    assert want1.sum != want2.sum
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")

    def launch(struct):
        eng.launch("localvol", X, struct, SEED, f, n, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return tuple(triple.tolist())

    struct, keep = eng.prepared("localvol", X, inputs(s1))
    assert launch(struct) == (want1.sum, want1.sum2, float(n))
    keep.sigma[:] = s2["sigma"]                                   # the caller's array, overwritten in place; y_lo and y_hi follow
    struct.y_lo, struct.y_hi = s2["y_lo"], s2["y_hi"]
    assert launch(struct) == (want2.sum, want2.sum2, float(n))    # the replay reads the array again: the new content
    keep.sigma[:] = np.nan                                        # ... and then it is poisoned and dropped
    del struct, keep
    fresh, keep2 = eng.prepared("localvol", X, inputs(s1))
    assert launch(fresh) == (want1.sum, want1.sum2, float(n))
    assert launch(fresh) == (want1.sum, want1.sum2, float(n))    # a cache hit: nothing of the poisoned array is read


# ---- 4. prices --------------------------------------------------------------------------------------------------------
N_PRICE = 10_000_000


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_a_time_only_surface_prices_black_scholes_at_the_rms_volatility(eng, X):
    o, rows = dict(s=100.0, k=100.0, r=0.03, t=1.0), np.array([0.15, 0.3, 0.22, 0.4])
    surf = lv.make_surface(np.stack([rows, rows], axis=1), -0.1, 0.1)
    rms = math.sqrt((rows.astype(NPX[X]).astype(np.float64) ** 2).mean())
    exact = lv.black_scholes_call(dict(o, v=rms))
    for right, want in (("call", exact), ("put", exact - o["s"] + o["k"] * math.exp(-o["r"] * o["t"]))):
        e = eng.localvol(o, surf, 64, N_PRICE, right, SEED, 0, X)
        print(f"{X} {right}: {e.expected:.6f} +- {e.confidence:.2g} vs {want:.6f}")
        assert abs(e.expected - want) <= 3 * e.confidence


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_displaced_surface_prices_the_displaced_diffusion_within_the_schemes_bias(eng, X):
    """|GPU price - exact| <= 3 GPU half-widths + |b| + h of localvol_ref.BIAS, the scheme's and the sampled surface's bias at 64 steps on
    the 8 x 65 surface, measured on the model, never on the kernel; call and put at the three strikes."""
    c = lv.BIAS_CASE
    surf = lv.bias_surface()
    try:
        eng.set_antithetic(True)
        for k, (bias, h) in lv.BIAS.items():
            for right in ("call", "put"):
                exact = lv.displaced_price(c["s"], k, c["r"], c["t"], c["sd"], c["a"], right)
                e = eng.localvol(dict(s=c["s"], k=k, r=c["r"], t=c["t"]), surf, c["n_steps"], N_PRICE, right, SEED, 0, X)
                print(f"{X} k={k} {right}: {e.expected:.6f} +- {e.confidence:.2g} vs {exact:.6f} (bias {bias:+.4f} +- {h:.4f})")
                assert abs(e.expected - exact) <= 3 * e.confidence + abs(bias) + h, (k, right)
    finally:
        eng.set_antithetic(False)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_every_refusal_enqueues_nothing_and_leaves_the_context_usable(mc):
    from montecarlocuda_amd.engine import _LocalVolHolder, check
    o, n = dict(s=100.0, k=100.0, r=0.03, t=1.0), 50_000
    good = lv.wavy_surface(2, 5, -0.5, 0.5)
    with mc.Engine(0) as fresh:
        want = {X: (fresh.localvol_asian(o, good, 4, 3, n, "put", SEED, 0, X), fresh.asian(dict(o, v=0.2), 7, n, SEED, 0, X)) for X in ("f32", "f64")}
    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    nan, inf = float("nan"), float("inf")
    L = mc._lib

    def run(e, X, opt=o, surface=good, nd=4, spd=3, payoff="asian", right="put", barrier=130.0, kind="up-and-out", n=n, **fields):
        h = _LocalVolHolder(X, opt, surface, nd, spd, payoff, right, barrier, kind)
        for k, v in fields.items():
            setattr(h.struct, k, C.POINTER(L.CT[X])() if k == "sigma" else v)
        r = L.Result()
        check(getattr(L.lib(), f"mc_localvol_run_{X}")(e._ctx, C.byref(h.struct), SEED, 0, n, C.byref(r)))
        return r

    def still_fine(e):
        """Nothing was enqueued and nothing uploaded: the same bits as a fresh context, and the other product's table still its own."""
        for X, (w0, w1) in want.items():
            g0, g1 = run(e, X), e.asian(dict(o, v=0.2), 7, n, SEED, 0, X)
            assert (g0.sum, g0.sum2, g0.n, g1.sum, g1.sum2, g1.n) == (w0.sum, w0.sum2, w0.n, w1.sum, w1.sum2, w1.n)
            assert e.last_launch()[0] > 0

    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            bad_surface = good["sigma"].copy()
            bad_surface[1, 2] = -0.1
            refused = [dict(n_steps=0), dict(n_steps=L.MAX_LOCALVOL_STEPS + 1), dict(n_times=0), dict(n_nodes=1), dict(n_times=5),
                       dict(n_times=1025, n_nodes=2, n_steps=2050), dict(steps_per_date=0), dict(steps_per_date=5), dict(sigma=None),
                       dict(surface=dict(good, sigma=bad_surface)), dict(surface=dict(good, sigma=np.full((2, 5), nan))),
                       dict(surface=dict(good, y_lo=0.5)), dict(surface=dict(good, y_hi=inf)), dict(payoff=3), dict(payoff=-1), dict(right=2),
                       dict(payoff="barrier", kind=4), dict(payoff="barrier", barrier=0.0), dict(payoff="barrier", barrier=nan),
                       dict(payoff="barrier", barrier=100.0), dict(payoff="barrier", barrier=110.0, kind="down-and-in"),
                       dict(opt=dict(o, s=0.0)), dict(opt=dict(o, t=-1.0)), dict(opt=dict(o, r=inf)), dict(opt=dict(o, k=nan)), dict(n=0),
                       dict(surface=dict(good, sigma=np.full((2, 5), 3e4)), nd=4096, spd=1)]
            for bad in refused:
                e.asian(dict(o, v=0.2), 7, n, SEED, 0, X)
                before = e.last_launch()
                with pytest.raises(mc.McError, match=INVALID):
                    run(e, X, **bad)
                assert e.last_launch() == before, bad
            still_fine(e)
            assert np.isfinite(run(e, X, barrier=nan, barrier_type=99).expected)          # ignored by the Asian payoff
            assert np.isfinite(run(e, X, opt=dict(o, v=nan)).expected)                    # option.v is ignored
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, X)
        e.set_generator("philox")
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            run(e, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 6. driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prints_the_prices_next_to_the_exact_ones(X):
    exe = os.path.join(ROOT, "drivers", f"localvolOpt_{X}")
    assert os.path.exists(exe), f"drivers/localvolOpt_{X} not built (build())"
    out = subprocess.run([exe, "16", "4", "2000000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(\w+) price=(\S+) ci=(\S+) kernel_ms=\S+", out.stdout, re.M)}
    exact = {k: float(p) for k, p in re.findall(r"^(\w+) price=\S+ ci=\S+ kernel_ms=\S+ exact=(\S+)", out.stdout, re.M)}
    products = ["asian_plain", "asian_antithetic", "up_out_plain", "up_out_antithetic"]
    assert set(row) == set(products) | {"european_call", "european_put", "flat_call"} and set(exact) == {"european_call", "european_put", "flat_call"}, out.stdout
    for k in row:
        assert all(math.isfinite(v) for v in row[k]) and row[k][0] > 0 and row[k][1] > 0, out.stdout
    assert row["asian_antithetic"][1] < row["asian_plain"][1] and row["up_out_antithetic"][1] < row["up_out_plain"][1], out.stdout
    c = lv.BIAS_CASE
    for right in ("call", "put"):
        assert exact[f"european_{right}"] == pytest.approx(lv.displaced_price(c["s"], 100.0, c["r"], c["t"], c["sd"], c["a"], right), rel=1e-9)
        b, h = lv.BIAS[100.0]
        assert abs(row[f"european_{right}"][0] - exact[f"european_{right}"]) <= 3 * row[f"european_{right}"][1] + abs(b) + h, out.stdout
    assert abs(row["flat_call"][0] - exact["flat_call"]) <= 3 * row["flat_call"][1], out.stdout
    assert row["asian_plain"][0] < row["european_call"][0] and row["up_out_plain"][0] < row["european_call"][0]
