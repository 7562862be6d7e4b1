"""The lookback options on the GPU (lookback_kernel, mc_lookback_*): the raw-words hook against the oracle's Philox; every path against
the independent float64 model lookback_ref.py on the kernels' own normals (Engine.normals, domain 8) and bridge uniforms (rebuilt
from Engine.words, domain 9, with the device's exact arithmetic), for both precisions, the four types, both monitorings,
antithetic off and on, date counts around every loop boundary (the fp32 loop takes 4 dates per trip, the fp64 loop 8 then 2, the
fp64 uniforms come two dates per block) and path ranges across the 2^32-unit seam; identities per path; the sums of a call of
many grid-stride trips; the bit rules of the stream; the launch form, timing off and an armed slot; the exact prices; refusals;
the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of lookback_ref's forward-error scale, per path; the bound on a sum
is the sum of the per-path bounds.  The values are continuous in every intermediate quantity: no path is left out and none has
two admissible values."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import lookback_ref as lr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
ATM = lr.ATM


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


def draws(e, X, first, n, m):
    """The device's own normals and bridge uniforms of paths first ... first + n - 1, (n, m) each."""
    return lr.lookback_draws(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X),
                             lambda domain, u0, c, b0, nb: e.words(SEED, domain, u0, c, b0, nb), first, n, m, X)


def check_paths(got, p, tol):
    """|got - value| <= tol * scale on every path, finite everywhere.  Returns the worst error / bound."""
    assert np.all(np.isfinite(got))
    err, b = np.abs(got - p.value[0]), gr.bound(p, tol)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    assert np.all(r <= 1.0), (int(np.argmax(r)), float(r.max()), float(got[np.argmax(r)]), float(p.value[0][np.argmax(r)]))
    return float(r.max())


# ---- 0. the words hook --------------------------------------------------------------------------------------------------
def test_words_are_the_oracles_philox_blocks(eng, po):
    key = [SEED & 0xFFFFFFFF, SEED >> 32]
    for domain, first, n, b0, nb in ((lr.DOMAIN_LOOKBACK_BRIDGE, 0, 70, 0, 3), (lr.DOMAIN_LOOKBACK_BRIDGE, U32 - 2, 5, 1023, 2),
                                     (lr.DOMAIN_LOOKBACK, 5 * U32 + 17, 3, 7, 1), (1, 123456789, 2, 0, 1)):
        w = eng.words(SEED, domain, first, n, b0, nb)
        assert w.shape == (n, nb, 4) and w.dtype == np.uint32
        for i, b in itertools.product((0, n - 1, n // 2), range(nb)):
            assert [int(x) for x in w[i, b]] == po.philox(po.counter(first + i, b0 + b, domain), key), (domain, first + i, b0 + b)


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", lr.DATES)
def test_every_path_against_the_reference(mc, eng, X, m):
    assert lr.DATES[-1] == mc._lib.MAX_LOOKBACK_DATES and TOL[X]["pay"] == lr.EPS[X]
    n, tol = lr.N_PATHS, TOL[X]["pay"]
    try:
        for first, o in zip((0, 12345, U32 - 100), lr.CASES):
            z, u = draws(eng, X, first, n, m)
            for monitoring in lr.MONITORINGS:
                # the antithetic walk's first direction is the plain walk
                both = {side: lr.walk(o, m, z, u, side, monitoring, True, tol) for side in (True, False)}
                for anti in (False, True):
                    eng.set_antithetic(anti)
                    for kind in lr.KINDS:
                        sides = both[lr.ON_MAX[kind]]
                        p = lr.value(sides if anti else sides[:1], kind, o["k"])
                        got = eng.lookback_paths(o, m, n, SEED, first, X, kind, monitoring).astype(np.float64)
                        worst = check_paths(got, p, tol)
                        print(f"{X} m={m} first={first} {kind} {monitoring} anti={anti}: worst err/bound {worst:.3g}")
    finally:
        eng.set_antithetic(False)


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 7, 64, 257])
def test_identities_per_path(eng, X, m):
    """Within the summed bounds.  floating put + floating call = max S - min S holds in BOTH monitorings: the model (and the header)
    feed the same bridge draws E_j to the maximum's and to the minimum's walk, so the two extremes of the identity are the two
    walks' own."""
    n, first, tol = lr.N_PATHS, 4242, TOL[X]["pay"]
    try:
        for o, anti in itertools.product(lr.CASES, (False, True)):
            eng.set_antithetic(anti)
            z, u = draws(eng, X, first, n, m)
            vals, bounds = {}, {}
            for monitoring in lr.MONITORINGS:
                walks = {side: lr.walk(o, m, z, u, side, monitoring, anti, tol) for side in (True, False)}
                for kind in lr.KINDS:
                    vals[kind, monitoring] = eng.lookback_paths(o, m, n, SEED, first, X, kind, monitoring).astype(np.float64)
                    bounds[kind, monitoring] = tol * lr.value(walks[lr.ON_MAX[kind]], kind, o["k"]).scale[0]
                    assert np.all(vals[kind, monitoring] >= 0.0)
                spread = sum(s["ext"] for s in walks[True]) / len(walks[True]) - sum(s["ext"] for s in walks[False]) / len(walks[False])
                b = bounds["floating-put", monitoring] + bounds["floating-call", monitoring]
                assert np.all(np.abs(vals["floating-put", monitoring] + vals["floating-call", monitoring] - spread) <= b), (o, monitoring, anti)
            for kind in lr.KINDS:
                assert np.all(vals[kind, "continuous"] >= vals[kind, "discrete"] - bounds[kind, "continuous"] - bounds[kind, "discrete"]), (o, kind, anti)
                if m == 1 and kind.startswith("floating"):
                    assert np.all(vals[kind, "discrete"] == 0.0)   # the extremum over one date IS the terminal spot
    finally:
        eng.set_antithetic(False)


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    m, n, first, chunk = 16, 300_000, 777, 50_000
    o, tol = lr.CASES[1], TOL[X]["pay"]
    zs = [draws(eng, X, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for monitoring in lr.MONITORINGS:
            both = [{side: lr.walk(o, m, z, u, side, monitoring, True, tol) for side in (True, False)} for z, u in zs]
            for anti in (False, True):
                eng.set_antithetic(anti), few.set_antithetic(anti)
                for kind in lr.KINDS:
                    parts = [lr.value(w[lr.ON_MAX[kind]] if anti else w[lr.ON_MAX[kind]][:1], kind, o["k"]) for w in both]
                    p = gr.Paths(*(np.concatenate([getattr(q, k) for q in parts], axis=-1) for k in gr.Paths._fields))
                    b, v = gr.bound(p, tol)[0], p.value[0]
                    t1, t2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                    for e in (eng, few):
                        g = e.lookback(o, m, n, SEED, first, X, kind, monitoring)
                        if e is few:
                            assert trip_guard(e, 16, n) == 48   # full trips a lane
                        assert g.n == v.size == n
                        print(f"{X} {kind} {monitoring} anti={anti} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {t1:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {t2:.3g})")
                        assert abs(g.sum - v.sum()) <= t1, (kind, monitoring, anti, e.blocks, g.sum, v.sum(), t1)
                        assert abs(g.sum2 - (v * v).sum()) <= t2, (kind, monitoring, anti, e.blocks, g.sum2, (v * v).sum(), t2)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 4. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    o, m, f, n = dict(s=87.0, k=91.0, r=0.02, v=0.45, t=0.75), 13, 3001, 2500
    other = mc.Engine(0, blocks=96)
    try:
        for anti, monitoring, kind in itertools.product((False, True), lr.MONITORINGS, ("floating-call", "fixed-call")):
            for e in (eng, other):
                e.set_antithetic(anti)
            args = (X, kind, monitoring)
            whole = eng.lookback_paths(o, m, f + n, SEED, 0, *args)
            part = eng.lookback_paths(o, m, n, SEED, f, *args)
            assert np.array_equal(part, whole[f:])                                        # a path's value depends on its global index only
            assert np.array_equal(other.lookback_paths(o, m, n, SEED, f, *args), part)   # not on the grid
            fused = eng.lookback(o, m, 123_457, SEED, f, *args)
            eng.set_finish(False)
            two = eng.lookback(o, m, 123_457, SEED, f, *args)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)
            eng.set_timing(False)
            quiet = eng.lookback(o, m, 123_457, SEED, f, *args)
            eng.set_timing(True)
            assert (quiet.sum, quiet.sum2, quiet.n, quiet.kernel_ms) == (fused.sum, fused.sum2, fused.n, 0.0)
    finally:
        eng.set_finish(True)
        eng.set_timing(True)
        eng.set_antithetic(False)
        other.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_ranges_add_up(eng, X):
    o, m, n, a = dict(s=120.0, k=100.0, r=0.01, v=0.3, t=1.5), 24, 400_000, 150_001
    try:
        for anti, monitoring, kind in itertools.product((False, True), lr.MONITORINGS, ("floating-put", "fixed-put")):
            eng.set_antithetic(anti)
            run = lambda cnt, first: eng.lookback(o, m, cnt, SEED, first, X, kind, monitoring)
            whole, lo, hi = run(n, 0), run(a, 0), run(n - a, a)
            assert lo.n + hi.n == whole.n == n
            rel = TOL[X]["rel"]   # the same per-path values either way (bit rules): only the order of the fp64 additions differs
            assert lo.sum + hi.sum == pytest.approx(whole.sum, rel=rel)
            assert lo.sum2 + hi.sum2 == pytest.approx(whole.sum2, rel=rel)
    finally:
        eng.set_antithetic(False)


# ---- 5. launch form, armed slot -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_returns_the_run_forms_triple(eng, X):
    import torch
    o, m, n = dict(s=95.0, k=100.0, r=0.03, v=0.25, t=1.0), 12, 200_000
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti, monitoring, kind in itertools.product((False, True), lr.MONITORINGS, lr.KINDS):
            eng.set_antithetic(anti)
            struct, keep = eng.prepared("lookback", X, dict(o, n_dates=m, kind=kind, monitoring=monitoring))
            want = eng.lookback(o, m, n, SEED, 5, X, kind, monitoring)
            stream = torch.cuda.current_stream().cuda_stream
            eng.launch("lookback", X, struct, SEED, 5, n, triple.data_ptr(), stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
        # an armed direct slot receives the same triple
        slot = eng.arm_direct()
        assert slot[2] == -1.0
        eng.launch("lookback", X, struct, SEED, 5, n, triple.data_ptr(), eng.stream)
        assert eng.wait_slot(slot) == (want.sum, want.sum2, float(n))
        torch.cuda.synchronize()
    finally:
        eng.set_antithetic(False)


# ---- 6. exact prices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16])
def test_continuous_monitoring_prices_the_closed_form(mc, eng, X, m):
    """One fixed seed, 1e7 paths, 3 half-widths (5.9 sigma: the margin is for sampling noise alone).  The bridge estimator is
    unbiased for the continuously monitored price at any number of dates, even one; the discrete form at 16 dates lies below it
    by more than 3 half-widths: the monitoring bias that the bridge removes."""
    for kind in lr.KINDS:
        e = eng.lookback(ATM, m, 10_000_000, SEED, 0, X, kind, "continuous")
        exact = mc.lookback_closed_form(ATM, kind)
        print(f"{X} m={m} {kind}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
        assert abs(e.expected - exact) <= 3 * e.confidence
        assert abs(exact - lr.quadrature_price(ATM, kind)) <= 1e-7 * exact
        if m == 16:
            d = eng.lookback(ATM, m, 10_000_000, SEED, 0, X, kind, "discrete")
            print(f"{X} m={m} {kind}: discrete {d.expected:.6f} confidence {d.confidence:.2g}")
            assert d.expected < exact - 3 * d.confidence


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    o, m, n = ATM, 12, 50_000
    with mc.Engine(0) as fresh:
        want = fresh.vanilla(o, n, SEED, 0, "f64")
        want_lb = {(X, mon): fresh.lookback(o, m, n, SEED, 0, X, "fixed-call", mon) for X in ("f32", "f64") for mon in lr.MONITORINGS}

    def still_fine(e):
        got = e.vanilla(o, n, SEED, 0, "f64")
        assert (got.sum, got.sum2, got.n) == (want.sum, want.sum2, want.n)
        for (X, mon), w in want_lb.items():
            got = e.lookback(o, m, n, SEED, 0, X, "fixed-call", mon)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, -1, mc._lib.MAX_LOOKBACK_DATES + 1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.lookback(o, bad_m, n, SEED, 0, X)
            for kind, mon in ((4, 0), (-1, 0), (0, 2), (0, -1)):
                with pytest.raises(mc.McError, match=INVALID):
                    e.lookback(o, m, n, SEED, 0, X, kind, mon)
            still_fine(e)
            for bad in (dict(o, s=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf")), dict(o, v=float("nan")), dict(o, s=float("inf"))):
                for kind in lr.KINDS:
                    with pytest.raises(mc.McError, match=INVALID):
                        e.lookback(bad, m, n, SEED, 0, X, kind)
            for bad_k in (0.0, -1.0, float("inf"), float("nan")):
                for kind in ("fixed-call", "fixed-put"):
                    with pytest.raises(mc.McError, match="finite k > 0"):
                        e.lookback(dict(o, k=bad_k), m, n, SEED, 0, X, kind)
                got = e.lookback(dict(o, k=bad_k), m, n, SEED, 0, X, "floating-put")   # k is ignored by the floating types
                ref = e.lookback(o, m, n, SEED, 0, X, "floating-put")
                assert (got.sum, got.sum2) == (ref.sum, ref.sum2)
            with pytest.raises(mc.McError, match="v != 0"):
                e.lookback(dict(o, v=0.0), m, n, SEED, 0, X, "fixed-call", "continuous")
            assert e.lookback(dict(o, v=0.0), m, n, SEED, 0, X, "fixed-call", "discrete").sum > 0   # a (deterministic) discrete lookback
            with pytest.raises(mc.McError, match="outside the range of a double"):
                e.lookback(dict(o, r=1.0e6, t=10.0), m, n, SEED, 0, X)   # beyond the device exponential's argument range
            with pytest.raises(mc.McError, match=INVALID):
                e.lookback(o, m, 0, SEED, 0, X)
            still_fine(e)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.lookback(o, m, n, SEED, 0, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.lookback(o, m, n, SEED, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.lookback(o, m, n, SEED, 0, "f64")
        e.set_normals("native")
        still_fine(e)
        assert f"lookback_dates_max={mc._lib.MAX_LOOKBACK_DATES}" in e.describe()


# ---- 8. driver --------------------------------------------------------------------------------------------------------
def test_driver_prints_the_four_types_next_to_the_closed_form(mc):
    exe = os.path.join(ROOT, "drivers", "lookbackOpt_f64")
    assert os.path.exists(exe), "drivers/lookbackOpt_f64 not built (build())"
    out = subprocess.run([exe, "64", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^(\S+) (discrete|continuous|antithetic_discrete|antithetic_continuous|closed_form) price=(\S+) ci=(\S+)", out.stdout, re.M)
    got = {(kind, form): (float(p), float(c)) for kind, form, p, c in rows}
    assert set(got) == {(kind, form) for kind in lr.KINDS for form in ("discrete", "continuous", "antithetic_discrete", "antithetic_continuous", "closed_form")}, out.stdout
    for kind in lr.KINDS:
        exact = got[kind, "closed_form"][0]
        assert exact == pytest.approx(mc.lookback_closed_form(ATM, kind), rel=1e-12)
        for form in ("continuous", "antithetic_continuous"):
            assert abs(got[kind, form][0] - exact) <= 3 * got[kind, form][1], out.stdout
        assert got[kind, "discrete"][0] < got[kind, "continuous"][0]
