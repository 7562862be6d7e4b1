"""The worst-of / best-of options on the GPU (rainbow_kernel, mc_rainbow_*): every path against the independent float64 model
rainbow_ref.py on the kernels' own normals (Engine.normals, domain 14), for both precisions, every basket size class of the flat
(date, factor) layout, antithetic off and on, date counts around every loop boundary and up to the table's cap, and path ranges
across the 2^32-unit seam; the four types and five barrier choices; the sums of a call; a call of many grid-stride trips;
identities per path; the bit rules of the stream; the launch form; the exact prices; orderings; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of rainbow_ref's forward-error scale, per path.  The barrier is a
step: a path farther from it than the tolerance (in units of the error of its distance) must match the model's value; a nearer
one must match one of the two values it can take, knocked or not -- no path is left out.  tests/test_rainbow_ref.py caps how
many paths are that near."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import rainbow_ref as rr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
WORST = {"f32": 0.0, "f64": 0.0}


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


def normals(e, X, first, n, n_assets, m):
    return rr.rainbow_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, n_assets, m, gr.NPB[X])


def ratio(err, b):
    """err / b per path, with 0 / 0 = 0: a knocked-out path has value 0 and bound 0, and the kernel must return exactly 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / b)


def check_paths(got, sides, barrier_kind, tol):
    """The per-path rule of the module docstring.  Returns (worst error / bound, number of near paths)."""
    p, cands = rr.value(sides, barrier_kind, full=True)
    assert np.all(np.isfinite(got))
    r = ratio(np.abs(got - p.value[0]), tol * p.scale[0])
    near = p.edge <= tol
    worst = float(r[~near].max()) if (~near).any() else 0.0
    assert worst <= 1.0, (int(np.argmax(np.where(near, 0.0, r))), worst)
    if near.any():
        w = 1.0 / len(cands)
        best = np.full(int(near.sum()), np.inf)
        for pick in itertools.product((0, 1), repeat=len(cands)):
            v = w * sum(c[0][i][near] for c, i in zip(cands, pick))
            s = w * sum(c[1][i][near] for c, i in zip(cands, pick))
            best = np.minimum(best, ratio(np.abs(got[near] - v), tol * s))
        assert np.all(best <= 1.0), float(best.max())
        worst = max(worst, float(best.max()))
    return worst, int(near.sum())


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets,m", [(a, m) for a in rr.ASSETS for m in rr.DATES(a)])
def test_every_path_against_the_reference(eng, X, n_assets, m):
    n, tol = rr.N_PATHS, TOL[X]["pay"]
    cases = rr.cases(n_assets) + ([rr.ABSOLUTE] if n_assets == 3 else [])
    try:
        for first, (b, kind, B, up) in zip((U32 - 1000, 12345, 0), cases):   # the first range straddles the 2^32-unit seam
            z = normals(eng, X, first, n, n_assets, m)
            both = rr.walk(b, m, z, kind, B, up, anti=True)
            for anti in (False, True):
                eng.set_antithetic(anti)
                sides = both if anti else both[:1]
                for bk in rr.kinds_of(up):
                    got = eng.rainbow_paths(b, m, n, kind, B, bk, SEED, first, X).astype(np.float64)
                    worst, near = check_paths(got, sides, bk, tol)
                    WORST[X] = max(WORST[X], worst)
                    print(f"{X} n={n_assets} m={m} first={first} {kind} {bk} anti={anti}: worst err/bound {worst:.3g}, {near} near paths; "
                          f"worst so far {WORST[X]:.3g}")
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [5, 17])
def test_all_four_types_and_five_barrier_choices(eng, X, m):
    n_assets, n, first, tol = 3, rr.N_PATHS, 777, TOL[X]["pay"]
    b = rr.market(n_assets)
    z = normals(eng, X, first, n, n_assets, m)
    try:
        for kind, anti in itertools.product(rr.KINDS, (False, True)):
            eng.set_antithetic(anti)
            for bk in [None] + rr.BARRIER_KINDS:
                up = None if bk is None else bk.startswith("up")
                B = None if bk is None else 1.3 if up else 0.75
                sides = rr.walk(b, m, z, kind, B, up, anti)
                got = eng.rainbow_paths(b, m, n, kind, B, bk, SEED, first, X).astype(np.float64)
                check_paths(got, sides, bk, tol)
    finally:
        eng.set_antithetic(False)


# ---- 2. sums, many trips ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_match_the_dumped_paths(mc, eng, X):
    """(sum x, sum x^2) of mc_rainbow_run_* against the fp64 sums of the dumped paths; again on an engine of 16 blocks, where a
    lane walks several paths: bit for bit the same paths, and every one of them against the model."""
    small = mc.Engine(0, blocks=16)
    n, first = 16 * 256 * 5 + 77, 4242
    try:
        for (n_assets, m), anti in itertools.product(((3, 16), (8, 5), (2, 7)), (False, True)):
            b, kind, B, up = rr.cases(n_assets)[0]
            for e in (eng, small):
                e.set_antithetic(anti)
            v = eng.rainbow_paths(b, m, n, kind, B, "down-and-in", SEED, first, X)
            v_small = small.rainbow_paths(b, m, n, kind, B, "down-and-in", SEED, first, X)
            assert np.array_equal(v_small, v)
            v = v.astype(np.float64)
            # every path of the many-trip call against the model itself, not only against the default engine
            z = np.concatenate([normals(small, X, f, min(4096, first + n - f), n_assets, m) for f in range(first, first + n, 4096)])
            worst, near = check_paths(v_small.astype(np.float64), rr.walk(b, m, z, kind, B, up, anti), "down-and-in", TOL[X]["pay"])
            print(f"{X} n={n_assets} m={m} anti={anti} on 16 blocks: worst err/bound {worst:.3g}, {near} near paths")
            for e in (eng, small):
                g = e.rainbow(b, m, n, kind, B, "down-and-in", SEED, first, X)
                assert g.n == n
                assert g.sum == pytest.approx(v.sum(), rel=TOL[X]["rel"]) and g.sum2 == pytest.approx((v * v).sum(), rel=TOL[X]["rel"])
                assert g.expected == pytest.approx(math.exp(-b["r"] * b["t"]) * v.mean(), rel=TOL[X]["rel"])
    finally:
        eng.set_antithetic(False)
        small.close()


# ---- 3. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_identities_on_the_device(eng, X):
    n, first = rr.N_PATHS, 99
    try:
        for n_assets, m, anti in itertools.product((2, 5), (1, 9), (False, True)):
            eng.set_antithetic(anti)
            for b, kind, B, up in rr.cases(n_assets):
                k_out, k_in = rr.kinds_of(up)
                run = lambda barrier, bk: eng.rainbow_paths(b, m, n, kind, barrier, bk, SEED, first, X)
                free = run(None, None)
                assert np.array_equal(run(B, k_out) + run(B, k_in), free)   # P is 0 or 1: one of the two is 0, the other the payoff
                assert np.all(run(B, k_out) >= 0)
                h = eng.prepared("rainbow", X, dict(b, n_dates=m, kind=kind))   # no barrier: the barrier field is not read
                h[0].barrier = 123.0
                assert np.array_equal(eng._paths("rainbow", X, h[0], SEED, first, n), free)
    finally:
        eng.set_antithetic(False)
    # one asset, one date: the vanilla call's payoff on the same normal
    o = dict(s=100.0, k=95.0, r=0.03, v=0.25, t=1.5)
    b = dict(s=np.array([o["s"]]), v=np.array([o["v"]]), w=np.ones(1), p=np.ones((1, 1)), k=o["k"], t=o["t"], r=o["r"])
    z = normals(eng, X, first, n, 1, 1)
    got = eng.rainbow_paths(b, 1, n, "call-on-min", None, None, SEED, first, X).astype(np.float64)
    ST = o["s"] * np.exp((o["r"] - 0.5 * o["v"] ** 2) * o["t"] + o["v"] * math.sqrt(o["t"]) * z[:, 0, 0])
    p = rr.rainbow(dict(b, d=np.zeros(1)), 1, z, "call-on-min")
    assert np.all(np.abs(got - np.maximum(ST - o["k"], 0.0)) <= gr.bound(p, TOL[X]["pay"])[0])


# ---- 4. the frame's rules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    n_assets, m, f, n = 3, 13, 3001, 2500
    b, kind, B, up = rr.cases(n_assets)[0]
    other = mc.Engine(0, blocks=96)
    args = (kind, B, "down-and-out", SEED)
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            whole = eng.rainbow_paths(b, m, f + n, *args, 0, X)
            part = eng.rainbow_paths(b, m, n, *args, f, X)
            assert np.array_equal(part, whole[f:])                                   # a path's value depends on its global index only
            assert np.array_equal(other.rainbow_paths(b, m, n, *args, f, X), part)   # not on the grid
            fused = eng.rainbow(b, m, 123_457, *args, f, X)
            eng.set_finish(False)
            two = eng.rainbow(b, m, 123_457, *args, f, X)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)
            eng.set_timing(False)
            quiet = eng.rainbow(b, m, 123_457, *args, f, X)
            eng.set_timing(True)
            assert (quiet.sum, quiet.sum2, quiet.n, quiet.kernel_ms) == (fused.sum, fused.sum2, fused.n, 0.0)
            lo, hi = eng.rainbow(b, m, 50_001, *args, f, X), eng.rainbow(b, m, 123_457 - 50_001, *args, f + 50_001, X)
            assert lo.sum + hi.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"]) and lo.sum2 + hi.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
            seam = eng.rainbow(b, m, 5000, *args, U32 - 2500, X)   # a range across 2^32: two segments
            a, c = eng.rainbow(b, m, 2500, *args, U32 - 2500, X), eng.rainbow(b, m, 2500, *args, U32, X)
            assert a.sum + c.sum == pytest.approx(seam.sum, rel=TOL[X]["rel"]) and seam.n == 5000
    finally:
        eng.set_finish(True)
        eng.set_timing(True)
        eng.set_antithetic(False)
        other.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_and_armed_slot(mc, eng, X):
    import torch
    n_assets, m, n = 4, 12, 200_000
    b, kind, B, up = rr.cases(n_assets)[1]
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    struct, keep = eng.prepared("rainbow", X, dict(b, n_dates=m, kind=kind, barrier=B, barrier_kind="up-and-out"))
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            want = eng.rainbow(b, m, n, kind, B, "up-and-out", SEED, 5, X)
            eng.launch("rainbow", X, struct, SEED, 5, n, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
            held = (lambda x: float(np.float32(x))) if X == "f32" else float   # the rate and maturity as the struct holds them
            price, half = mc.closing(want.sum, want.sum2, n, math.exp(-held(b["r"]) * held(b["t"])))
            assert (price, half) == (want.expected, want.confidence)
            slot = eng.arm_direct()
            assert slot[2] == -1.0
            eng.launch("rainbow", X, struct, SEED, 5, n, triple.data_ptr(), eng.stream)
            assert eng.wait_slot(slot) == (want.sum, want.sum2, float(n))
            torch.cuda.synchronize()
    finally:
        eng.set_antithetic(False)


def test_the_table_is_cached_by_content_and_survives_another_product(eng):
    b, kind, B, up = rr.cases(3)[0]
    m, n = 16, 10_000
    first = eng.rainbow(b, m, n, kind, B, "down-and-in", SEED, 0, "f64")
    again = eng.rainbow(b, m, n, "call-on-min", B, "down-and-out", SEED, 0, "f64")   # same table: e, the dates and the levels are the same
    assert eng.last_call_stats()["table_upload_ms"] == 0.0
    eng.asian(dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0), m, n, SEED, 0, "f64")   # a second product takes the table
    third = eng.rainbow(b, m, n, kind, B, "down-and-in", SEED, 0, "f64")
    assert eng.last_call_stats()["table_upload_ms"] > 0.0
    assert (first.sum, first.sum2) == (third.sum, third.sum2) and again.n == n
    eng.rainbow(dict(b, r=0.031), m, n, kind, B, "down-and-in", SEED, 0, "f64")
    assert eng.last_call_stats()["table_upload_ms"] > 0.0


# ---- 5. prices --------------------------------------------------------------------------------------------------------
PRICE_PATHS = 10_000_000


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16])
def test_two_assets_price_stulz(mc, eng, X, m):
    """One fixed seed, 1e7 paths, 3 half-widths (5.9 sigma: the margin is for sampling noise alone)."""
    b = rr.market(2)
    try:
        for kind, anti in itertools.product(rr.KINDS, (False, True)):
            eng.set_antithetic(anti)
            e = eng.rainbow(b, m, PRICE_PATHS, kind, None, None, SEED, 0, X)
            exact = mc.rainbow_closed_form(b, kind)
            print(f"{X} m={m} {kind} anti={anti}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence
            assert abs(exact - rr.stulz(b, kind)) <= 1e-10
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", [5, 8])
def test_many_assets_price_the_one_factor_quadrature(eng, X, n_assets):
    b = rr.market(n_assets)
    try:
        for kind in ("put-on-min", "call-on-max"):
            exact = rr.one_factor(b, rr.betas(n_assets), kind)
            for m, anti in itertools.product((1, 8), (False, True)):
                eng.set_antithetic(anti)
                e = eng.rainbow(b, m, PRICE_PATHS, kind, None, None, SEED, 0, X)
                print(f"{X} n={n_assets} m={m} {kind} anti={anti}: expected {e.expected:.6f} exact {exact:.6f} confidence {e.confidence:.2g}")
                assert abs(e.expected - exact) <= 3 * e.confidence
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_one_asset_prices_the_barrier_call(eng, X):
    """The same contract from two domains of the stream: within 3 combined half-widths."""
    o, B, m = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0), 120.0, 16
    b = dict(s=np.array([o["s"]]), v=np.array([o["v"]]), w=np.ones(1), p=np.ones((1, 1)), k=o["k"], t=o["t"], r=o["r"])
    for bk in ("up-and-out", "up-and-in"):
        e, ref = eng.rainbow(b, m, PRICE_PATHS, "call-on-max", B, bk, SEED, 0, X), eng.barrier(o, B, m, PRICE_PATHS, SEED, 0, X, bk, "discrete")
        print(f"{X} {bk}: rainbow {e.expected:.6f} +- {e.confidence:.2g}, barrier {ref.expected:.6f} +- {ref.confidence:.2g}")
        assert abs(e.expected - ref.expected) <= 3 * (e.confidence + ref.confidence)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_orderings(eng, X):
    b, m, n = rr.market(3), 8, 2_000_000
    call, out = eng.rainbow(b, m, n, "call-on-min", None, None, SEED, 0, X), eng.rainbow(b, m, n, "call-on-min", 0.9, "down-and-out", SEED, 0, X)
    assert out.expected < call.expected - 3 * (out.confidence + call.confidence)
    one = dict(s=b["s"][:1], v=b["v"][:1], w=b["w"][:1], p=np.ones((1, 1)), k=b["k"], t=b["t"], r=b["r"])
    worst, single = eng.rainbow(b, m, n, "put-on-min", None, None, SEED, 0, X), eng.rainbow(one, m, n, "put-on-min", None, None, SEED, 0, X)
    assert worst.expected > single.expected + 3 * (worst.confidence + single.confidence)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    b, kind, B, up = rr.cases(3)[0]
    m, n = 12, 50_000
    with mc.Engine(0) as fresh:
        want = {X: fresh.rainbow(b, m, n, kind, B, "down-and-in", SEED, 0, X) for X in ("f32", "f64")}

    def still_fine(e):
        for X, w in want.items():
            got = e.rainbow(b, m, n, kind, B, "down-and-in", SEED, 0, X)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    L = mc._lib
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            empty = dict(s=np.zeros(0), v=np.zeros(0), p=np.zeros(0), d=np.zeros(0), w=np.zeros(0), k=1.0, t=1.0, r=0.03)
            bad_calls = [lambda: e.rainbow(rr.market(9), m, n, kind, precision=X), lambda: e.rainbow(empty, m, n, kind, precision=X),   # n outside 1..8
                         lambda: e.rainbow(b, 0, n, kind, precision=X), lambda: e.rainbow(b, -1, n, kind, precision=X),
                         lambda: e.rainbow(b, L.MAX_RAINBOW_TABLE // 3 + 1, n, kind, precision=X),                    # n * n_dates > the cap
                         lambda: e.rainbow(b, m, n, 4, precision=X), lambda: e.rainbow(b, m, n, -1, precision=X),
                         lambda: e.rainbow(b, m, n, kind, B, 4, precision=X), lambda: e.rainbow(b, m, n, kind, B, -2, precision=X),
                         lambda: e.rainbow(dict(b, s=b["s"] * np.array([1.0, 0.0, 1.0])), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, w=-b["w"]), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, v=b["v"] * np.array([1.0, -1.0, 1.0])), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, t=0.0), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, r=float("inf")), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, k=float("nan")), m, n, kind, precision=X),
                         lambda: e.rainbow(dict(b, d=np.array([0.0, 0.0, 0.5])), m, n, kind, precision=X),
                         lambda: e.rainbow(b, m, n, kind, 0.0, "down-and-in", precision=X),
                         lambda: e.rainbow(b, m, n, kind, float("inf"), "up-and-out", precision=X),
                         lambda: e.rainbow(b, m, n, kind, 1.01, "down-and-in", precision=X),    # the initial worst performance is 1: beyond the barrier
                         lambda: e.rainbow(b, m, n, kind, 0.99, "up-and-out", precision=X),
                         lambda: e.rainbow(dict(b, w=np.ones(3)), m, n, kind, 100.0, "down-and-in", precision=X),   # the worst level 100: on it
                         lambda: e.rainbow(b, m, n, "call-on-max", 0.9, "up-and-in", precision=X),
                         lambda: e.rainbow(b, m, 0, kind, precision=X)]
            for i, call in enumerate(bad_calls):
                with pytest.raises(mc.McError, match=INVALID):
                    call()
                    print(f"bad call {i} ({X}) was served")
            assert e.rainbow(b, L.MAX_RAINBOW_TABLE // 3, 1000, kind, precision=X).n == 1000   # the cap itself is served
            assert e.rainbow(dict(b, v=np.zeros(3)), m, 1000, kind, precision=X).sum2 >= 0       # v = 0 is valid
            still_fine(e)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=INVALID):   # as mc_american_run_* refuses it
                e.rainbow(b, m, n, kind, precision=X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.rainbow(b, m, n, kind, precision=X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.rainbow(b, m, n, kind, precision="f64")
        e.set_normals("native")
        still_fine(e)


# ---- 7. driver --------------------------------------------------------------------------------------------------------
def test_driver_prints_prices_consistent_with_its_closed_form(mc):
    exe = os.path.join(ROOT, "drivers", "rainbowOpt_f64")
    assert os.path.exists(exe), "drivers/rainbowOpt_f64 not built (build())"
    out = subprocess.run([exe, "16", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(\w+) price=(\S+) ci=(\S+)", out.stdout, re.M)}
    assert set(row) == {"min2_1_date", "min2_1_date_antithetic", "min2_16_dates", "min2_16_dates_antithetic", "closed_form", "worst3_put",
                        "worst3_knock_in", "worst3_knock_out"}, out.stdout
    exact = row["closed_form"][0]
    for k in ("min2_1_date", "min2_1_date_antithetic", "min2_16_dates", "min2_16_dates_antithetic"):
        assert abs(row[k][0] - exact) <= 3 * row[k][1], out.stdout
    two = dict(s=np.array([100.0, 50.0]), v=np.array([0.2, 0.3]), w=np.array([0.01, 0.02]), p=np.linalg.cholesky(np.array([[1.0, 0.5], [0.5, 1.0]])),
               d=np.zeros(2), k=1.0, t=1.0, r=0.03)
    assert exact == pytest.approx(rr.stulz(two, "call-on-min"), abs=1e-10)
    assert row["worst3_knock_in"][0] + row["worst3_knock_out"][0] == pytest.approx(row["worst3_put"][0], rel=1e-12)   # the same paths
    assert 0 < row["worst3_knock_in"][0] < row["worst3_put"][0]
