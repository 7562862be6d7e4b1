"""Merton's jump-diffusion on the GPU (merton_kernel, mc_merton_*): every path against the independent float64 model merton_ref.py on
the kernels' own normals (Engine.normals, domain 10) and their own Poisson counts, rebuilt exactly from the raw words
(Engine.words, domain 11) and the library's integer thresholds (mc_merton_thresholds_*) -- for both precisions, the three payoffs
and the four barrier types, antithetic off and on, date counts around every loop boundary (the fp32 loop takes 4 dates per trip, the
fp64 loop 8 then 2; a raw block holds 4 fp32 and 2 fp64 count words) and path ranges across the 2^32-unit seam; identities per path;
the sums of a call of many grid-stride trips; the bit rules of the stream; the launch form; the exact price; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of merton_ref's forward-error scale, per path; the bound on a sum is
the sum of the per-path bounds.  The barrier payoff has a step: a path farther from it than the tolerance (in units of the error of
its distance) must match the model's value; a nearer one must match one of the two values it can take, knocked or not -- no path is
left out.  tests/test_merton_ref.py caps how many paths are that near."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import greeks_ref as gr
import merton_ref as mr
from greeks_ref import trip_guard
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
ATM = mr.br.ATM
JP = mr.JUMPS[0]


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


def draws(mc, e, X, o, jp, first, n, m):
    """The kernels' own normals and counts of paths first ... first + n - 1."""
    return mr.merton_draws(e, SEED, X, first, n, m, mc.merton_thresholds(o, jp, m, X))


def forms(o, B):
    """(payoff, barrier type) of every product on this market."""
    return [("european", None), ("asian", None)] + [("barrier", kind) for kind in mr.kinds_of(o, B)]


def paths(e, o, jp, B, m, n, first, X, payoff, kind):
    if payoff == "european":
        return e.merton_paths(o, jp, m, n, SEED, first, X)
    if payoff == "asian":
        return e.merton_asian_paths(o, jp, m, n, SEED, first, X)
    return e.merton_barrier_paths(o, jp, B, m, n, SEED, first, X, kind)


def run(e, o, jp, B, m, n, first, X, payoff, kind):
    if payoff == "european":
        return e.merton(o, jp, m, n, SEED, first, X)
    if payoff == "asian":
        return e.merton_asian(o, jp, m, n, SEED, first, X)
    return e.merton_barrier(o, jp, B, m, n, SEED, first, X, kind)


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", mr.DATES)
def test_every_path_against_the_reference(mc, eng, X, m):
    assert mr.DATES[-1] == mc._lib.MAX_MERTON_DATES
    n, tol = mr.N_PATHS, TOL[X]["pay"]
    kinds, jumped = set(), []
    cases = list(zip((0, 12345, U32 - 100), mr.CASES)) + ([(777, mr.HEAVY)] if m in mr.HEAVY_DATES else [])
    try:
        for first, (o, B, jp) in cases:
            z, N = draws(mc, eng, X, o, jp, first, n, m)
            jumped.append(float((N.sum(axis=1) > 0).mean()))
            for anti in (False, True):
                eng.set_antithetic(anti)
                c, sides = mr.walk(o, jp, m, z, N, B, B > o["s"], anti)
                for payoff, kind in forms(o, B):
                    got = paths(eng, o, jp, B, m, n, first, X, payoff, kind).astype(np.float64)
                    worst, near = mr.check_paths(got, c, sides, payoff, bool(kind) and kind.endswith("in"), tol)
                    print(f"{X} m={m} first={first} {payoff} {kind} anti={anti}: worst err/bound {worst:.3g}, {near} near paths, most jumps on a date {int(N.max())}")
                    kinds.add(kind)
    finally:
        eng.set_antithetic(False)
    assert kinds == set(mr.KINDS) | {None}
    # the shares of the paths that jump, as the cases were chosen: about 64 %, 95 % and 22 %
    assert 0.55 < jumped[0] < 0.72 and 0.90 < jumped[1] < 0.98 and 0.15 < jumped[2] < 0.30, jumped


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 7, 64, 257])
def test_identities_per_path(mc, eng, X, m):
    n, first, tol = mr.N_PATHS, 4242, TOL[X]["pay"]
    try:
        for (o, B, jp), anti in itertools.product(mr.CASES, (False, True)):
            eng.set_antithetic(anti)
            z, N = draws(mc, eng, X, o, jp, first, n, m)
            # no jumps: the model at N = 0 (the constant-volatility walk on this product's own normals), whatever mu_j and delta
            j0 = dict(jp, **{"lambda": 0.0})
            assert len(mc.merton_thresholds(o, j0, m, X)) == 0
            c0, sides0 = mr.walk(o, j0, m, z, np.zeros_like(N), B, B > o["s"], anti)
            for payoff, kind in forms(o, B):
                got = paths(eng, o, j0, B, m, n, first, X, payoff, kind).astype(np.float64)
                mr.check_paths(got, c0, sides0, payoff, bool(kind) and kind.endswith("in"), tol)
            # knock-in + knock-out = the European value: the knocked weight cancels exactly
            c, sides = mr.walk(o, jp, m, z, N, B, B > o["s"], anti)
            k_out, k_in = mr.kinds_of(o, B)
            v_out, v_in = (paths(eng, o, jp, B, m, n, first, X, "barrier", k).astype(np.float64) for k in (k_out, k_in))
            eu = paths(eng, o, jp, B, m, n, first, X, "european", None).astype(np.float64)
            b = tol * (mr.value(c, sides, "barrier", False).scale[0] + mr.value(c, sides, "barrier", True).scale[0] + mr.value(c, sides, "european").scale[0])
            assert np.all(np.abs(v_out + v_in - eu) <= b), (o, B, anti)
            assert np.all(v_out >= 0.0) and np.all(v_in >= 0.0)
            if m == 1:   # one date: the average is the terminal spot
                asian = paths(eng, o, jp, B, m, n, first, X, "asian", None).astype(np.float64)
                assert np.all(np.abs(asian - eu) <= 2 * tol * mr.value(c, sides, "european").scale[0])
    finally:
        eng.set_antithetic(False)


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(mc, eng, few, X):
    """On the default engine (one trip a lane at this size) and on the engine of 16 blocks (48 trips a lane and part of a 49th)."""
    m, n, first, chunk = 16, 300_000, 777, 50_000
    o, B, jp = mr.CASES[0]
    ds = [draws(mc, eng, X, o, jp, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for anti in (False, True):
            eng.set_antithetic(anti), few.set_antithetic(anti)
            walks = [mr.walk(o, jp, m, z, N, B, True, anti) for z, N in ds]
            for payoff, kind in forms(o, B):
                parts = [mr.value(c, sides, payoff, bool(kind) and kind.endswith("in")) for c, sides in walks]
                p = gr.Paths(*(np.concatenate([getattr(q, k) for q in parts], axis=-1) for k in gr.Paths._fields))
                b, v = gr.bound(p, TOL[X]["pay"])[0], p.value[0]
                tol, tol2 = b.sum(), (2 * np.abs(v) * b + b * b).sum()
                for e in (eng, few):
                    g = run(e, o, jp, B, m, n, first, X, payoff, kind)
                    if e is few:
                        assert trip_guard(e, 16, n) == 48   # full trips a lane
                    assert g.n == v.size == n
                    print(f"{X} {payoff} {kind} anti={anti} blocks={e.blocks}: sum err {abs(g.sum - v.sum()):.3g} (tol {tol:.3g}), sum2 err {abs(g.sum2 - (v * v).sum()):.3g} (tol {tol2:.3g})")
                    assert abs(g.sum - v.sum()) <= tol, (payoff, kind, anti, e.blocks, g.sum, v.sum(), tol)
                    assert abs(g.sum2 - (v * v).sum()) <= tol2, (payoff, kind, anti, e.blocks, g.sum2, (v * v).sum(), tol2)
    finally:
        eng.set_antithetic(False), few.set_antithetic(False)


# ---- 4. bit rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    o, B, jp, m, f, n = dict(s=87.0, k=91.0, r=0.02, v=0.45, t=0.75), 110.0, dict([("lambda", 2.5), ("mu_j", -0.07), ("delta", 0.2)]), 13, 3001, 2500
    other = mc.Engine(0, blocks=96)
    try:
        for anti, (payoff, kind) in itertools.product((False, True), forms(o, B)):
            for e in (eng, other):
                e.set_antithetic(anti)
            whole = paths(eng, o, jp, B, m, f + n, 0, X, payoff, kind)
            part = paths(eng, o, jp, B, m, n, f, X, payoff, kind)
            assert np.array_equal(part, whole[f:])                                            # a path's value depends on its global index only
            assert np.array_equal(paths(other, o, jp, B, m, n, f, X, payoff, kind), part)     # not on the grid
            fused = run(eng, o, jp, B, m, 123_457, f, X, payoff, kind)
            eng.set_finish(False)
            two = run(eng, o, jp, B, m, 123_457, f, X, payoff, kind)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)             # the fused finish against the two-launch finish
            eng.set_timing(False)
            quiet = run(eng, o, jp, B, m, 123_457, f, X, payoff, kind)
            eng.set_timing(True)
            assert (quiet.sum, quiet.sum2, quiet.n) == (fused.sum, fused.sum2, fused.n) and quiet.kernel_ms == 0   # timing off
    finally:
        eng.set_finish(True)
        eng.set_timing(True)
        eng.set_antithetic(False)
        other.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_ranges_add_up(eng, X):
    o, B, jp, m, n, a = dict(s=120.0, k=100.0, r=0.01, v=0.3, t=1.5), 95.0, mr.JUMPS[1], 24, 400_000, 150_001
    try:
        for anti, (payoff, kind) in itertools.product((False, True), forms(o, B)):
            eng.set_antithetic(anti)
            whole, lo, hi = (run(eng, o, jp, B, m, cnt, first, X, payoff, kind) for cnt, first in ((n, 0), (a, 0), (n - a, a)))
            assert lo.n + hi.n == whole.n == n
            rel = TOL[X]["rel"]   # the same per-path values either way (bit rules): only the order of the fp64 additions differs
            assert lo.sum + hi.sum == pytest.approx(whole.sum, rel=rel)
            assert lo.sum2 + hi.sum2 == pytest.approx(whole.sum2, rel=rel)
    finally:
        eng.set_antithetic(False)


# ---- 5. launch form, armed slot ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_returns_the_run_forms_triple(eng, X):
    import torch
    o, B, jp, m, n = dict(s=95.0, k=100.0, r=0.03, v=0.25, t=1.0), 125.0, JP, 12, 200_000
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti, (payoff, kind) in itertools.product((False, True), forms(o, B)):
            eng.set_antithetic(anti)
            inputs = dict(o, **jp, n_dates=m, payoff=payoff)
            if kind:
                inputs.update(barrier=B, kind=kind)
            struct, keep = eng.prepared("merton", X, inputs)
            want = run(eng, o, jp, B, m, n, 5, X, payoff, kind)
            stream = torch.cuda.current_stream().cuda_stream
            eng.launch("merton", X, struct, SEED, 5, n, triple.data_ptr(), stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_an_armed_slot_receives_the_triple(eng, X):
    """mc_context_arm_direct: the next launch also delivers its triple into the armed pinned host slot."""
    import torch
    o, B, jp, m, n = ATM, 120.0, JP, 9, 100_000
    triple = torch.zeros(3, dtype=torch.float64, device="cuda")
    for payoff, kind in forms(o, B):
        want = run(eng, o, jp, B, m, n, 11, X, payoff, kind)
        inputs = dict(o, **jp, n_dates=m, payoff=payoff)
        if kind:
            inputs.update(barrier=B, kind=kind)
        struct, keep = eng.prepared("merton", X, inputs)
        slot = eng.arm_direct()
        assert slot[2] == -1.0
        eng.launch("merton", X, struct, SEED, 11, n, triple.data_ptr(), eng.stream)
        assert eng.wait_slot(slot) == (want.sum, want.sum2, float(n))
        torch.cuda.synchronize()


# ---- 6. the exact price -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16])
def test_the_walk_prices_the_closed_form(mc, eng, X, m):
    """One fixed seed, 1e7 paths, 3 half-widths (5.9 sigma: the margin is for sampling noise alone).  The walk is exact in law at
    any number of dates: there is no bias term."""
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            e = eng.merton(ATM, JP, m, 10_000_000, SEED, 0, X)
            exact = mc.merton_closed_form(ATM, JP)
            print(f"{X} m={m} anti={anti}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence
    finally:
        eng.set_antithetic(False)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    o, B, jp, m, n = ATM, 120.0, JP, 12, 50_000
    with mc.Engine(0) as fresh:
        want = {(X, payoff, kind): run(fresh, o, jp, B, m, n, 0, X, payoff, kind) for X in ("f32", "f64") for payoff, kind in forms(o, B)}

    def still_fine(e):
        for (X, payoff, kind), w in want.items():
            got = run(e, o, jp, B, m, n, 0, X, payoff, kind)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, -1, mc._lib.MAX_MERTON_DATES + 1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.merton(o, jp, bad_m, n, SEED, 0, X)
            for payoff in (3, -1):
                with pytest.raises(mc.McError, match=INVALID):
                    e._run("merton", X, mc.engine._as_merton(X, o, jp, m, payoff), SEED, 0, n)
            for kind in (4, -1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.merton_barrier(o, jp, B, m, n, SEED, 0, X, kind)
            still_fine(e)
            for bad in (dict(o, s=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf")), dict(o, k=float("nan"))):
                with pytest.raises(mc.McError, match=INVALID):
                    e.merton_asian(bad, jp, m, n, SEED, 0, X)
            for bad in (dict(jp, **{"lambda": -0.5}), dict(jp, delta=-0.1), dict(jp, mu_j=float("nan")), dict(jp, delta=float("inf"))):
                with pytest.raises(mc.McError, match=INVALID):
                    e.merton(o, bad, m, n, SEED, 0, X)
            for bad_b in (0.0, -1.0, float("inf"), float("nan")):
                with pytest.raises(mc.McError, match=INVALID):
                    e.merton_barrier(o, jp, bad_b, m, n, SEED, 0, X, "down-and-out" if bad_b <= 0 else "up-and-out")
            for bad_b, kind in ((100.0, "up-and-out"), (90.0, "up-and-in"), (100.0, "down-and-out"), (110.0, "down-and-in")):
                with pytest.raises(mc.McError, match="vanilla call or nothing"):
                    e.merton_barrier(o, jp, bad_b, m, n, SEED, 0, X, kind)
            with pytest.raises(mc.McError, match="Poisson thresholds"):   # lambda dt = 13: beyond the cap in both widths
                e.merton(o, dict(jp, **{"lambda": 13.0}), 1, n, SEED, 0, X)
            with pytest.raises(mc.McError, match="outside the range of a double"):
                e.merton(o, dict(jp, mu_j=-1.0e6, **{"lambda": 5.0}), 1, n, SEED, 0, X)
            with pytest.raises(mc.McError, match=INVALID):
                e.merton(o, jp, m, 0, SEED, 0, X)
            # valid corners: no diffusion with and without jump noise, jumps of size 1
            assert e.merton(dict(o, v=0.0), jp, m, n, SEED, 0, X).sum2 > 0
            assert e.merton(dict(o, v=0.0), dict(jp, delta=0.0), m, n, SEED, 0, X).sum2 > 0
            assert e.merton_asian(o, dict(jp, mu_j=0.0, delta=0.0), m, n, SEED, 0, X).sum2 > 0
            still_fine(e)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.merton_asian(o, jp, m, n, SEED, 0, X)
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                e.merton(o, jp, m, n, SEED, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.merton(o, jp, m, n, SEED, 0, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 8. driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prints_the_products_and_the_closed_form(mc, X):
    exe = os.path.join(ROOT, "drivers", f"mertonOpt_{X}")
    assert os.path.exists(exe), f"drivers/mertonOpt_{X} not built (build())"
    out = subprocess.run([exe, "64", "500000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {(k, f): (float(p), float(c)) for k, f, p, c in re.findall(r"^(\S+) (plain|antithetic|closed_form) price=(\S+) ci=(\S+)", out.stdout, re.M)}
    assert set(row) == {(k, f) for k in ("european-1", "european-16", "asian", "up-and-out") for f in ("plain", "antithetic")} | {("european", "closed_form")}, out.stdout
    exact = row["european", "closed_form"][0]
    assert exact == pytest.approx(mc.merton_closed_form(ATM, JP, X), rel=1e-12)   # the struct of this precision rounds the inputs
    for k, f in itertools.product(("european-1", "european-16"), ("plain", "antithetic")):
        assert abs(row[k, f][0] - exact) <= 3 * row[k, f][1], out.stdout
    assert row["asian", "plain"][0] < exact and row["up-and-out", "plain"][0] < exact
