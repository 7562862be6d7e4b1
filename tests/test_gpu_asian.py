"""The Asian call on the GPU (asian_kernel, mc_asian_*): every path against the independent float64 model asian_ref.py on the
kernels' own normals (Engine.normals, domain 4), for both precisions, the four estimators, date counts around every loop
boundary (the fp32 loop takes 4 dates per trip, the fp64 loop 8 then 2) and path ranges across the 2^32-unit seam; the sums of a
call of many grid-stride trips; the bit rules of the stream; the launch form; closed forms; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of asian_ref's forward-error scale, per path; the bound on a sum
is the sum of the per-path bounds."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import asian_ref as ar
import greeks_ref as gr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
ESTIMATORS = [(False, False), (True, False), (False, True), (True, True)]   # (antithetic, control)
ATM = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)


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


def dates_list(mc):
    return [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 255, 256, 257, 1000, mc._lib.MAX_ASIAN_DATES]


def estimator(e, anti, control):
    e.set_antithetic(anti)
    e.set_control_variate(control)


def normals(e, X, first, n, m):
    return ar.asian_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, gr.NPB[X])


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("mi", range(16))
def test_every_path_against_the_reference(mc, eng, X, mi):
    m = dates_list(mc)[mi]
    rng = np.random.default_rng(7000 + m)
    n = 2121   # eight workgroups and a partial wave
    try:
        for first in (0, 12345, U32 - 100):
            o = gr.random_vanilla(rng)
            z = normals(eng, X, first, n, m)
            for anti, control in ESTIMATORS:
                estimator(eng, anti, control)
                got = eng.asian_paths(o, m, n, SEED, first, X).astype(np.float64)
                p = ar.asian(o, m, z, control, anti)
                b = gr.bound(p, TOL[X]["pay"])[0]
                err = np.abs(got - p.value[0])
                worst = int(np.argmax(err / b))
                print(f"{X} m={m} first={first} anti={anti} cv={control}: worst err/bound {err[worst] / b[worst]:.3g} (path {worst})")
                assert np.all(err <= b), (o, first, anti, control, worst, got[worst], p.value[0][worst], b[worst])
    finally:
        estimator(eng, False, False)


# ---- 2. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    m, n, first, chunk = 16, 300_000, 777, 50_000
    o = gr.random_vanilla(np.random.default_rng(99))
    zs = [normals(eng, X, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for anti, control in ESTIMATORS:
            parts = [ar.asian(o, m, z, control, anti) for z in zs]
            p = gr.Paths(*(np.concatenate([getattr(q, k) for q in parts], axis=-1) for k in gr.Paths._fields))
            b, v = gr.bound(p, TOL[X]["pay"])[0], p.value[0]
            tol, tol2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
            for e in (eng, few):
                estimator(e, anti, control)
                g = e.asian(o, m, n, SEED, first, X)
                if e is few:
                    assert trip_guard(e, 16, n) == 48   # full trips a lane
                assert g.n == v.size == n
                print(f"{X} anti={anti} cv={control} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {tol:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {tol2:.3g})")
                assert abs(g.sum - v.sum()) <= tol, (anti, control, e.blocks, g.sum, v.sum(), tol)
                assert abs(g.sum2 - (v * v).sum()) <= tol2, (anti, control, e.blocks, g.sum2, (v * v).sum(), tol2)
    finally:
        estimator(eng, False, False)
        estimator(few, False, False)


# ---- 3. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    o, m, f, n = dict(s=87.0, k=91.0, r=0.02, v=0.45, t=0.75), 13, 3001, 2500
    other = mc.Engine(0, blocks=96)
    try:
        for anti, control in ESTIMATORS:
            for e in (eng, other):
                estimator(e, anti, control)
            whole = eng.asian_paths(o, m, f + n, SEED, 0, X)
            part = eng.asian_paths(o, m, n, SEED, f, X)
            assert np.array_equal(part, whole[f:])                                   # a path's value depends on its global index only
            assert np.array_equal(other.asian_paths(o, m, n, SEED, f, X), part)      # not on the grid
            fused = eng.asian(o, m, 123_457, SEED, f, X)
            eng.set_finish(False)
            two = eng.asian(o, m, 123_457, SEED, f, X)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)
    finally:
        eng.set_finish(True)
        estimator(eng, False, False)
        other.close()


# ---- 4. splitting -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_ranges_add_up(eng, X):
    o, m, n, a = dict(s=120.0, k=100.0, r=0.01, v=0.3, t=1.5), 24, 400_000, 150_001
    try:
        for anti, control in ESTIMATORS:
            estimator(eng, anti, control)
            whole, lo, hi = eng.asian(o, m, n, SEED, 0, X), eng.asian(o, m, a, SEED, 0, X), eng.asian(o, m, n - a, SEED, a, X)
            assert lo.n + hi.n == whole.n == n
            rel = TOL[X]["rel"]   # the same per-path values either way (bit rules): only the order of the fp64 additions differs
            assert lo.sum + hi.sum == pytest.approx(whole.sum, rel=rel)
            assert lo.sum2 + hi.sum2 == pytest.approx(whole.sum2, rel=rel)
    finally:
        estimator(eng, False, False)


# ---- 5. launch form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_returns_the_run_forms_triple(eng, X):
    import torch
    o, m, n = dict(s=95.0, k=100.0, r=0.03, v=0.25, t=1.0), 12, 200_000
    struct, keep = eng.prepared("asian", X, dict(o, n_dates=m))
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti, control in ESTIMATORS:
            estimator(eng, anti, control)
            want = eng.asian(o, m, n, SEED, 5, X)
            stream = torch.cuda.current_stream().cuda_stream
            eng.launch("asian", X, struct, SEED, 5, n, triple.data_ptr(), stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
    finally:
        estimator(eng, False, False)


# ---- 6. closed forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_one_date_prices_the_black_scholes_call(eng, X):
    """One fixed seed, 1e7 paths: an Asian call with one date is the vanilla call."""
    e = eng.asian(ATM, 1, 10_000_000, SEED, 0, X)
    bs = ar.black_scholes_call(ATM)
    print(f"{X}: expected {e.expected:.6f} BS {bs:.6f} confidence {e.confidence:.2g}")
    assert abs(e.expected - bs) <= 2 * e.confidence


def test_control_variate_against_the_plain_estimator(eng):
    """100 / 100 / 0.05 / 0.2 / 1 on 64 dates, 1e6 fp64 paths, one fixed seed: the controlled estimate lies within the summed
    half-widths of the plain one and its half-width is below a tenth of it (the float64 model gives 0.043; the margin is for
    the sampling noise of a variance ratio at that size); every controlled path value is >= 0 up to its bound (AM >= GM)."""
    m, n = 64, 1_000_000
    try:
        plain = eng.asian(ATM, m, n, SEED, 0, "f64")
        estimator(eng, False, True)
        ctrl = eng.asian(ATM, m, n, SEED, 0, "f64")
        print(f"plain {plain.expected:.6f} +- {plain.confidence:.2g}, control {ctrl.expected:.6f} +- {ctrl.confidence:.2g}")
        assert abs(ctrl.expected - plain.expected) <= ctrl.confidence + plain.confidence
        assert ctrl.confidence < 0.1 * plain.confidence
        for X in ("f32", "f64"):
            k = 20_000
            vals = eng.asian_paths(ATM, m, k, SEED, 0, X).astype(np.float64)
            b = gr.bound(ar.asian(ATM, m, normals(eng, X, 0, k, m), True, False), TOL[X]["pay"])[0]
            assert np.all(vals >= -b), (X, float((vals + b).min()))
    finally:
        estimator(eng, False, False)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    o, m, n = ATM, 12, 50_000
    with mc.Engine(0) as fresh:
        want = fresh.asian(o, m, n, SEED, 0, "f64")
        want32 = fresh.asian(o, m, n, SEED, 0, "f32")

    def still_fine(e):
        got = e.asian(o, m, n, SEED, 0, "f64")
        assert (got.sum, got.sum2, got.n) == (want.sum, want.sum2, want.n)
        got = e.asian(o, m, n, SEED, 0, "f32")
        assert (got.sum, got.sum2, got.n) == (want32.sum, want32.sum2, want32.n)

    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, mc._lib.MAX_ASIAN_DATES + 1):
                with pytest.raises(mc.McError, match="mc error 1"):   # MC_ERR_INVALID
                    e.asian(o, bad_m, n, SEED, 0, X)
                still_fine(e)
            for bad in (dict(o, s=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf"))):
                with pytest.raises(mc.McError, match="mc error 1"):
                    e.asian(bad, m, n, SEED, 0, X)
            with pytest.raises(mc.McError, match="mc error 1"):
                e.asian(o, m, 0, SEED, 0, X)
            still_fine(e)
            e.set_control_variate(True)
            for bad, what in ((dict(o, k=0.0), "k > 0"), (dict(o, v=0.0), "v != 0")):
                with pytest.raises(mc.McError, match=what):
                    e.asian(bad, m, n, SEED, 0, X)
            e.set_control_variate(False)
            assert e.asian(dict(o, v=0.0), m, n, SEED, 0, X).sum2 > 0   # without the control v == 0 is a (deterministic) call
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match="mc error 4"):   # MC_ERR_UNSUPPORTED
                e.asian(o, m, n, SEED, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match="mc error 4"):
            e.asian(o, m, n, SEED, 0, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 8. driver --------------------------------------------------------------------------------------------------------
def test_driver_prints_plain_and_controlled_prices():
    exe = os.path.join(ROOT, "drivers", "asianOpt_f64")
    assert os.path.exists(exe), "drivers/asianOpt_f64 not built (build())"
    out = subprocess.run([exe, "64", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(plain|control) price=(\S+) ci=(\S+)", out.stdout, re.M)}
    assert set(row) == {"plain", "control"}, out.stdout
    geo = float(re.search(r"^geometric closed_form=(\S+)", out.stdout, re.M).group(1))
    assert abs(row["plain"][0] - row["control"][0]) <= row["plain"][1] + row["control"][1], out.stdout
    assert row["control"][1] < row["plain"][1]
    assert 0 < geo < row["control"][0]   # the arithmetic average is at least the geometric one
