"""The barrier call on the GPU (barrier_kernel, mc_barrier_*): every path against the independent float64 model barrier_ref.py on the
kernels' own normals (Engine.normals, domain 5), for both precisions, the four types, both monitorings, antithetic off and on, date
counts around every loop boundary (the fp32 loop takes 4 dates per trip, the fp64 loop 8 then 2) and path ranges across the
2^32-unit seam; identities per path; the sums of a call of many grid-stride trips; the bit rules of the stream; the launch form;
the exact prices; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of barrier_ref's forward-error scale, per path; the bound on a sum
is the sum of the per-path bounds.  The discrete form has a step at the barrier: a path farther from it than the tolerance (in
units of the error of its distance) must match the model's value; a nearer one must match one of the two values it can take,
knocked or not -- no path is left out.  tests/test_barrier_ref.py caps how many paths are that near."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import barrier_ref as br
import greeks_ref as gr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
ATM = br.ATM


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
    return br.barrier_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, gr.NPB[X])


def ratio(err, b):
    """err / b per path, with 0 / 0 = 0: a knocked-out path has value 0 and bound 0, and the kernel must return exactly 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / b)


def check_paths(got, sides, knock_in, monitoring, tol):
    """The per-path rule of the module docstring.  Returns (worst error / bound, number of near paths)."""
    p, cands = br.value(sides, knock_in, full=True)
    assert np.all(np.isfinite(got))
    r = ratio(np.abs(got - p.value[0]), tol * p.scale[0])
    if monitoring == "continuous":
        assert np.all(r <= 1.0), (int(np.argmax(r)), float(r.max()))
        return float(r.max()), 0
    near = p.edge <= tol
    worst = float(r[~near].max()) if (~near).any() else 0.0
    assert worst <= 1.0, (int(np.argmax(np.where(near, 0.0, r))), worst)
    if near.any():
        # one of the two values of each path direction: the mean over the directions of every combination
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
@pytest.mark.parametrize("m", br.DATES)
def test_every_path_against_the_reference(mc, eng, X, m):
    assert br.DATES[-1] == mc._lib.MAX_BARRIER_DATES
    n, tol = br.N_PATHS, TOL[X]["pay"]
    kinds = set()
    try:
        for first, (o, B) in zip((0, 12345, U32 - 100), br.CASES):
            z = normals(eng, X, first, n, m)
            for monitoring in br.MONITORINGS:
                for anti in (False, True):
                    eng.set_antithetic(anti)
                    sides = br.walk(o, B, m, z, B > o["s"], monitoring, anti)
                    for kind in br.kinds_of(o, B):
                        got = eng.barrier_paths(o, B, m, n, SEED, first, X, kind, monitoring).astype(np.float64)
                        worst, near = check_paths(got, sides, kind.endswith("in"), monitoring, tol)
                        print(f"{X} m={m} first={first} {kind} {monitoring} anti={anti}: worst err/bound {worst:.3g}, {near} near paths")
                        kinds.add(kind)
    finally:
        eng.set_antithetic(False)
    assert kinds == set(br.KINDS)


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 7, 64, 257])
def test_identities_per_path(eng, X, m):
    n, first, tol = br.N_PATHS, 4242, TOL[X]["pay"]
    try:
        for (o, B), anti in itertools.product(br.CASES, (False, True)):
            eng.set_antithetic(anti)
            z = normals(eng, X, first, n, m)
            k_out, k_in = br.kinds_of(o, B)
            vals, bounds = {}, {}
            for monitoring in br.MONITORINGS:
                sides = br.walk(o, B, m, z, B > o["s"], monitoring, anti)
                for kind in (k_out, k_in):
                    vals[kind, monitoring] = eng.barrier_paths(o, B, m, n, SEED, first, X, kind, monitoring).astype(np.float64)
                    bounds[kind, monitoring] = tol * br.value(sides, kind.endswith("in")).scale[0]
                # knock-in + knock-out = the vanilla payoff (the model's own): the knocked weight cancels exactly
                pay = sum(s["pay"] for s in sides) / len(sides)
                b = bounds[k_out, monitoring] + bounds[k_in, monitoring]
                assert np.all(np.abs(vals[k_out, monitoring] + vals[k_in, monitoring] - pay) <= b), (o, B, monitoring, anti)
                assert np.all(vals[k_out, monitoring] >= 0.0)
            # the bridge can only take value away from the discretely monitored knock-out call
            assert np.all(vals[k_out, "continuous"] <= vals[k_out, "discrete"] + bounds[k_out, "continuous"] + bounds[k_out, "discrete"])
    finally:
        eng.set_antithetic(False)


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    m, n, first, chunk = 16, 300_000, 777, 50_000
    o, B = br.CASES[0]
    zs = [normals(eng, X, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for monitoring, anti in itertools.product(br.MONITORINGS, (False, True)):
            eng.set_antithetic(anti), few.set_antithetic(anti)
            walks = [br.walk(o, B, m, z, True, monitoring, anti) for z in zs]
            for kind in br.kinds_of(o, B):
                parts = [br.value(w, kind.endswith("in")) for w in walks]
                p = gr.Paths(*(np.concatenate([getattr(q, k) for q in parts], axis=-1) for k in gr.Paths._fields))
                b, v = gr.bound(p, TOL[X]["pay"])[0], p.value[0]
                tol, tol2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                for e in (eng, few):
                    g = e.barrier(o, B, m, n, SEED, first, X, kind, monitoring)
                    if e is few:
                        assert trip_guard(e, 16, n) == 48   # full trips a lane
                    assert g.n == v.size == n
                    print(f"{X} {kind} {monitoring} anti={anti} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {tol:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {tol2:.3g})")
                    assert abs(g.sum - v.sum()) <= tol, (kind, monitoring, anti, e.blocks, g.sum, v.sum(), tol)
                    assert abs(g.sum2 - (v * v).sum()) <= tol2, (kind, monitoring, anti, e.blocks, g.sum2, (v * v).sum(), tol2)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 4. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    o, B, m, f, n = dict(s=87.0, k=91.0, r=0.02, v=0.45, t=0.75), 110.0, 13, 3001, 2500
    other = mc.Engine(0, blocks=96)
    try:
        for anti, monitoring, kind in itertools.product((False, True), br.MONITORINGS, ("up-and-out", "up-and-in")):
            for e in (eng, other):
                e.set_antithetic(anti)
            args = (X, kind, monitoring)
            whole = eng.barrier_paths(o, B, m, f + n, SEED, 0, *args)
            part = eng.barrier_paths(o, B, m, n, SEED, f, *args)
            assert np.array_equal(part, whole[f:])                                       # a path's value depends on its global index only
            assert np.array_equal(other.barrier_paths(o, B, m, n, SEED, f, *args), part)   # not on the grid
            fused = eng.barrier(o, B, m, 123_457, SEED, f, *args)
            eng.set_finish(False)
            two = eng.barrier(o, B, m, 123_457, SEED, f, *args)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)
    finally:
        eng.set_finish(True)
        eng.set_antithetic(False)
        other.close()


# ---- 5. splitting -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_ranges_add_up(eng, X):
    o, B, m, n, a = dict(s=120.0, k=100.0, r=0.01, v=0.3, t=1.5), 95.0, 24, 400_000, 150_001
    try:
        for anti, monitoring, kind in itertools.product((False, True), br.MONITORINGS, ("down-and-out", "down-and-in")):
            eng.set_antithetic(anti)
            run = lambda cnt, first: eng.barrier(o, B, m, cnt, SEED, first, X, kind, monitoring)
            whole, lo, hi = run(n, 0), run(a, 0), run(n - a, a)
            assert lo.n + hi.n == whole.n == n
            rel = TOL[X]["rel"]   # the same per-path values either way (bit rules): only the order of the fp64 additions differs
            assert lo.sum + hi.sum == pytest.approx(whole.sum, rel=rel)
            assert lo.sum2 + hi.sum2 == pytest.approx(whole.sum2, rel=rel)
    finally:
        eng.set_antithetic(False)


# ---- 6. launch form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_returns_the_run_forms_triple(eng, X):
    import torch
    o, B, m, n = dict(s=95.0, k=100.0, r=0.03, v=0.25, t=1.0), 125.0, 12, 200_000
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti, monitoring, kind in itertools.product((False, True), br.MONITORINGS, ("up-and-out", "up-and-in")):
            eng.set_antithetic(anti)
            struct, keep = eng.prepared("barrier", X, dict(o, barrier=B, n_dates=m, kind=kind, monitoring=monitoring))
            want = eng.barrier(o, B, m, n, SEED, 5, X, kind, monitoring)
            stream = torch.cuda.current_stream().cuda_stream
            eng.launch("barrier", X, struct, SEED, 5, n, triple.data_ptr(), stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
    finally:
        eng.set_antithetic(False)


# ---- 7. exact prices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16])
def test_continuous_monitoring_prices_the_closed_form(mc, eng, X, m):
    """One fixed seed, 1e7 paths, 3 half-widths (5.9 sigma: the margin is for sampling noise alone).  The bridge estimator is
    unbiased for the continuously monitored price at any number of dates, even one."""
    for (o, B), kinds in (((ATM, 120.0), ("up-and-out", "up-and-in")), ((ATM, 90.0), ("down-and-out", "down-and-in"))):
        for kind in kinds:
            e = eng.barrier(o, B, m, 10_000_000, SEED, 0, X, kind, "continuous")
            exact = mc.barrier_closed_form(o, B, kind)
            print(f"{X} m={m} {kind}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence
            assert abs(exact - br.reiner_rubinstein(o, B, kind)) <= 1e-12 * exact


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_one_date_discrete_prices_its_closed_form(eng, X):
    for (o, B), kinds in (((ATM, 120.0), ("up-and-out", "up-and-in")), ((ATM, 90.0), ("down-and-out", "down-and-in"))):
        for kind in kinds:
            e = eng.barrier(o, B, 1, 10_000_000, SEED, 0, X, kind, "discrete")
            exact = br.one_date_discrete(o, B, kind)
            print(f"{X} {kind}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    o, B, m, n = ATM, 120.0, 12, 50_000
    with mc.Engine(0) as fresh:
        want = {(X, mon): fresh.barrier(o, B, m, n, SEED, 0, X, "up-and-out", mon) for X in ("f32", "f64") for mon in br.MONITORINGS}

    def still_fine(e):
        for (X, mon), w in want.items():
            got = e.barrier(o, B, m, n, SEED, 0, X, "up-and-out", mon)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, -1, mc._lib.MAX_BARRIER_DATES + 1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.barrier(o, B, bad_m, n, SEED, 0, X)
            for kind, mon in ((4, 0), (-1, 0), (0, 2), (0, -1)):
                with pytest.raises(mc.McError, match=INVALID):
                    e.barrier(o, B, m, n, SEED, 0, X, kind, mon)
            still_fine(e)
            for bad in (dict(o, s=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf")), dict(o, k=float("nan"))):
                with pytest.raises(mc.McError, match=INVALID):
                    e.barrier(bad, B, m, n, SEED, 0, X)
            for bad_b in (0.0, -1.0, float("inf"), float("nan")):
                with pytest.raises(mc.McError, match=INVALID):
                    e.barrier(o, bad_b, m, n, SEED, 0, X, "down-and-out" if bad_b <= 0 else "up-and-out")
            for bad_b, kind in ((100.0, "up-and-out"), (90.0, "up-and-in"), (100.0, "down-and-out"), (110.0, "down-and-in")):
                with pytest.raises(mc.McError, match="vanilla call or nothing"):
                    e.barrier(o, bad_b, m, n, SEED, 0, X, kind)
            with pytest.raises(mc.McError, match="v != 0"):
                e.barrier(dict(o, v=0.0), B, m, n, SEED, 0, X, "up-and-out", "continuous")
            assert e.barrier(dict(o, v=0.0), B, m, n, SEED, 0, X, "up-and-out", "discrete").sum2 > 0   # a (deterministic) discrete call
            with pytest.raises(mc.McError, match=INVALID):
                e.barrier(o, B, m, 0, SEED, 0, X)
            still_fine(e)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.barrier(o, B, m, n, SEED, 0, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.barrier(o, B, m, n, SEED, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.barrier(o, B, m, n, SEED, 0, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 9. driver --------------------------------------------------------------------------------------------------------
def test_driver_prints_discrete_continuous_and_closed_form():
    exe = os.path.join(ROOT, "drivers", "barrierOpt_f64")
    assert os.path.exists(exe), "drivers/barrierOpt_f64 not built (build())"
    out = subprocess.run([exe, "64", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(discrete|continuous|closed_form) price=(\S+) ci=(\S+)", out.stdout, re.M)}
    assert set(row) == {"discrete", "continuous", "closed_form"}, out.stdout
    assert abs(row["continuous"][0] - row["closed_form"][0]) <= row["continuous"][1] + row["closed_form"][1], out.stdout
    assert row["discrete"][0] >= row["continuous"][0]
    assert row["closed_form"][0] == pytest.approx(br.reiner_rubinstein(ATM, 120.0, "up-and-out"), rel=1e-12)
