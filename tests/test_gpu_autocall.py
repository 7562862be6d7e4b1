"""The worst-of autocallable notes on the GPU (autocall_kernel, mc_autocall_*): every path against the independent float64 model
autocall_ref.py on the kernels' own normals (Engine.normals, domain 15), for both precisions, every basket size class of the flat
(date, factor) layout, antithetic off and on, (dates, observations) around every loop boundary and up to the table's cap, and path
ranges across the 2^32-unit seam; the three knock-in modes; the sums of a call; a call of many grid-stride trips, where a lane
walks paths of different lifetimes; waves that leave at the first observation and waves that never do; shards and the launch
form; exact prices; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) per unit of autocall_ref's forward-error scale, per path.  Every decision is a
step: a path all of whose decisions are farther than the tolerance must match the model's value; a nearer one must match one of
the values the model enumerates for it -- no path is left out.  tests/test_autocall_ref.py caps how many paths are that near."""
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import autocall_ref as ar
import greeks_ref as gr
import rainbow_ref as rr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
WORST = {"f32": 0.0, "f64": 0.0}
INF = math.inf


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
    draw = lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X)
    return np.concatenate([ar.autocall_normals(draw, f, min(4096, first + n - f), n_assets, m, gr.NPB[X]) for f in range(first, first + n, 4096)])


def run_paths(e, b, m, n, con, first, X):
    return e.autocall_paths(b, m, n, con["autocall"], con["coupon_barrier"], con["coupon"], con["barrier"], con["ki"], con["gearing"], con["memory"],
                            SEED, first, X).astype(np.float64)


def run(e, b, m, n, con, first, X):
    return e.autocall(b, m, n, con["autocall"], con["coupon_barrier"], con["coupon"], con["barrier"], con["ki"], con["gearing"], con["memory"],
                      SEED, first, X)


def check_case(e, X, b, m, con, first, n, z=None, antis=(False, True)):
    """Every path of the range against the model, antithetic off and on.  Returns the worst error / bound."""
    tol = TOL[X]["pay"]
    z = normals(e, X, first, n, len(b["s"]), m) if z is None else z
    both = ar.walk(b, m, z, anti=True)
    worst = 0.0
    try:
        for anti in antis:
            e.set_antithetic(anti)
            p, cands = ar.value(b, m, con, both if anti else both[:1], tol, full=True)
            w, near = ar.check(run_paths(e, b, m, n, con, first, X), p, cands, tol)
            worst = max(worst, w)
            WORST[X] = max(WORST[X], w)
            print(f"{X} n={len(b['s'])} ({m},{con['autocall'].size}) first={first} ki={con['ki']} anti={anti}: worst err/bound {w:.3g}, {near} near paths; "
                  f"worst so far {WORST[X]:.3g}")
    finally:
        e.set_antithetic(False)
    return worst


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets,m,n_obs", [(a, m, k) for a in ar.ASSETS for m, k in ar.SHAPES(a)])
def test_every_path_against_the_reference(eng, X, n_assets, m, n_obs):
    cases = [(rr.market(n_assets), ar.contract_a(n_obs))] + ([(rr.ABSOLUTE[0], ar.contract_b(n_obs))] if n_assets == 3 else [])
    firsts = (U32 - 1000, 12345, 0)   # the first range straddles the 2^32-unit seam
    for i, (b, con) in enumerate(cases):
        check_case(eng, X, b, m, con, firsts[(i + m) % 3], ar.N_PATHS)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_three_knock_in_modes(eng, X):
    n_assets, m, n_obs, first = 3, 16, 4, 777
    b = rr.market(n_assets)
    z = normals(eng, X, first, ar.N_PATHS, n_assets, m)
    values = {}
    for ki, B in (("dates", 0.8), ("maturity", 0.8), (None, None)):
        con = dict(ar.contract_a(n_obs), ki=ki, barrier=B)
        check_case(eng, X, b, m, con, first, ar.N_PATHS, z)
        values[ki] = run_paths(eng, b, m, ar.N_PATHS, con, first, X)
    # the put is live on more paths from one mode to the next
    assert np.all(values[None] <= values["dates"]) and np.all(values["dates"] <= values["maturity"])
    assert np.any(values[None] < values["dates"]) and np.any(values["dates"] < values["maturity"])


# ---- 2. sums, many trips ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_match_the_dumped_paths(mc, eng, X):
    """(sum x, sum x^2) and expected of mc_autocall_run_* against the fp64 sums of the dumped paths; again on an engine of 16 blocks,
    where a lane walks several paths with different lifetimes: bit for bit the same paths, each against the model."""
    small = mc.Engine(0, blocks=16)
    n, first = 16 * 256 * 5 + 77, 4242
    try:
        for (n_assets, m, n_obs), anti in itertools.product(((3, 16, 4), (8, 5, 5), (2, 12, 4)), (False, True)):
            b, con = rr.market(n_assets), ar.contract_a(n_obs)
            for e in (eng, small):
                e.set_antithetic(anti)
            v, v_small = run_paths(eng, b, m, n, con, first, X), run_paths(small, b, m, n, con, first, X)
            assert np.array_equal(v_small, v)
            check_case(small, X, b, m, con, first, n, antis=(anti,))
            for e in (eng, small):
                e.set_antithetic(anti)
                g = run(e, b, m, n, con, first, X)
                assert g.n == n
                assert g.sum == pytest.approx(v.sum(), rel=TOL[X]["rel"]) and g.sum2 == pytest.approx((v * v).sum(), rel=TOL[X]["rel"])
                assert g.expected == pytest.approx(v.mean(), rel=TOL[X]["rel"])   # a present value: no discount on top
    finally:
        eng.set_antithetic(False)
        small.close()


# ---- 3. early exit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", [1, 3, 4])
def test_waves_that_leave_at_once_and_waves_that_never_leave(mc, eng, X, n_assets):
    """Every path called at observation 1 (a tiny trigger): the value is D_1 (c + 1) on every path, and the model's.  No path ever
    called: every wave walks to the end.  Both on the default grid and on 16 blocks (several paths per lane)."""
    m, n_obs = 64, 8
    b = rr.market(n_assets)
    small = mc.Engine(0, blocks=16)
    try:
        for e, n in ((eng, ar.N_PATHS), (small, 16 * 256 * 2 + 33)):
            z = normals(e, X, 5, n, n_assets, m)
            at_once = ar.contract(1e-6, 0.8, 0.02, barrier=0.6, ki="dates", gearing=1.0, n_obs=n_obs)
            assert check_case(e, X, b, m, at_once, 5, n, z) <= 1.0
            got = run_paths(e, b, m, n, at_once, 5, X)
            assert np.all(got == got[0]) and got[0] == pytest.approx(math.exp(-b["r"] * b["t"] / n_obs) * 1.02, rel=TOL[X]["pay"] * 4)
            never = ar.contract(INF, 0.8, 0.02, barrier=0.6, ki="dates", gearing=1.0, n_obs=n_obs)
            check_case(e, X, b, m, never, 5, n, z)
            mixed = ar.contract([INF, 1.0, 1.0, 1.0, INF, 0.9, 0.9, 0.9], 0.8, 0.02, barrier=0.6, ki="dates", gearing=1.0)
            check_case(e, X, b, m, mixed, 5, n, z)
    finally:
        small.close()


# ---- 4. shards, the launch form, the grid -----------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_two_shards_and_the_launch_form(mc, eng, X):
    import torch
    n_assets, m, n_obs, n, first = 4, 12, 4, 200_001, 5
    b, con = rr.market(n_assets), ar.contract_a(n_obs)
    other = mc.Engine(0, blocks=96)
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    struct, keep = eng.prepared("autocall", X, dict(b, n_dates=m, **con))
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            want = run(eng, b, m, n, con, first, X)
            eng.launch("autocall", X, struct, SEED, first, n, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
            assert mc.closing(want.sum, want.sum2, n, 1.0) == (want.expected, want.confidence)   # the discount of the closing is 1
            # two shards of the range, each through the launch form, add up to the single call
            sums = [0.0, 0.0, 0.0]
            for rank in range(2):
                lo, cnt = mc.shard_range(n, rank, 2)
                eng.launch("autocall", X, struct, SEED, first + lo, cnt, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                sums = [a + c for a, c in zip(sums, triple.tolist())]
            assert sums[2] == n and sums[0] == pytest.approx(want.sum, rel=TOL[X]["rel"]) and sums[1] == pytest.approx(want.sum2, rel=TOL[X]["rel"])
            # a path's value depends on its global index only, not on the grid
            part, whole = run_paths(eng, b, m, 2500, con, 3001, X), run_paths(eng, b, m, 5501, con, 0, X)
            assert np.array_equal(part, whole[3001:]) and np.array_equal(run_paths(other, b, m, 2500, con, 3001, X), part)
            seam = run(eng, b, m, 5000, con, U32 - 2500, X)   # a range across 2^32: two segments
            a, c = run(eng, b, m, 2500, con, U32 - 2500, X), run(eng, b, m, 2500, con, U32, X)
            assert a.sum + c.sum == pytest.approx(seam.sum, rel=TOL[X]["rel"]) and seam.n == 5000
    finally:
        eng.set_antithetic(False)
        other.close()


# ---- 5. prices --------------------------------------------------------------------------------------------------------
PRICE_PATHS = 10_000_000


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m,n_obs", [(4, 4), (16, 4)])
def test_one_asset_prices_the_exact_value(eng, X, m, n_obs):
    """One fixed seed, 1e7 paths, 3 half-widths, against the density propagation of autocall_ref (1e-7 of the notional)."""
    b, con = rr.market(1), ar.contract_a(n_obs)
    exact = ar.exact_single(b, m, con)
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            e = run(eng, b, m, PRICE_PATHS, con, 0, X)
            print(f"{X} ({m},{n_obs}) anti={anti}: expected {e.expected:.6f} exact {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [1, 16])
def test_two_assets_without_triggers_price_the_stulz_put(mc, eng, X, m):
    b, g = rr.market(2), 0.8
    con = ar.contract(INF, 0.8, 0.0, barrier=None, ki=None, gearing=g, n_obs=1)
    exact = math.exp(-b["r"] * b["t"]) - g * mc.rainbow_closed_form(b, "put-on-min")
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            e = run(eng, b, m, PRICE_PATHS, con, 0, X)
            print(f"{X} m={m} anti={anti}: expected {e.expected:.6f} closed form {exact:.6f} confidence {e.confidence:.2g}")
            assert abs(e.expected - exact) <= 3 * e.confidence
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_three_assets_without_triggers_price_the_rainbow_knock_in_put(eng, X):
    """The same contract from two domains of the stream: within 3 combined half-widths."""
    b, g, B, m = rr.market(3), 1.0, 0.7, 16
    con = ar.contract(INF, 0.8, 0.0, barrier=B, ki="dates", gearing=g, n_obs=4)
    e, ref = run(eng, b, m, PRICE_PATHS, con, 0, X), eng.rainbow(b, m, PRICE_PATHS, "put-on-min", B, "down-and-in", SEED, 0, X)
    want = math.exp(-b["r"] * b["t"]) - g * ref.expected
    print(f"{X}: autocall {e.expected:.6f} +- {e.confidence:.2g}, from the rainbow put {want:.6f} +- {g * ref.confidence:.2g}")
    assert abs(e.expected - want) <= 3 * (e.confidence + g * ref.confidence)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    b, m, n_obs, n = rr.market(3), 12, 4, 50_000
    con = ar.contract_a(n_obs)
    with mc.Engine(0) as fresh:
        want = {X: run(fresh, b, m, n, con, 0, X) for X in ("f32", "f64")}

    def still_fine(e):
        for X, w in want.items():
            got = run(e, b, m, n, con, 0, X)
            assert (got.sum, got.sum2, got.n) == (w.sum, w.sum2, w.n)

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    L = mc._lib
    A, Cb = con["autocall"], con["coupon_barrier"]
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            call = lambda b=b, m=m, n=n, A=A, Cb=Cb, c=0.02, B=0.6, ki="dates", g=1.0, mem=True, **kw: e.autocall(b, m, n, A, Cb, c, B, ki, g, mem, precision=X, **kw)
            bad_calls = [lambda: call(b=rr.market(9)), lambda: call(m=0), lambda: call(m=-4),
                         lambda: call(m=10),                                            # n_obs = 4 does not divide 10
                         lambda: call(A=1.0, Cb=0.8, n_obs=0), lambda: call(A=1.0, Cb=0.8, n_obs=-1),
                         lambda: call(m=1364, A=1.0, Cb=0.8, n_obs=2),                  # 3 * 1364 + 6 = 4098 values
                         lambda: call(A=A * np.array([1, 0, 1, 1])), lambda: call(A=A * np.array([1, -1, 1, 1])),
                         lambda: call(A=A * np.array([1, np.nan, 1, 1])),
                         lambda: call(Cb=Cb * np.array([1, -1, 1, 1])), lambda: call(Cb=Cb * np.array([1, np.nan, 1, 1])),
                         lambda: call(Cb=Cb * np.array([1, INF, 1, 1])),
                         lambda: call(c=-0.01), lambda: call(g=-1.0), lambda: call(c=float("nan")),
                         lambda: call(b=dict(b, k=0.0)), lambda: call(b=dict(b, k=-1.0)), lambda: call(b=dict(b, k=float("nan"))),
                         lambda: call(ki=2), lambda: call(ki=-2), lambda: call(mem=2), lambda: call(mem=-1),
                         lambda: call(B=0.0), lambda: call(B=-0.5), lambda: call(B=1.0), lambda: call(B=1.2),   # the initial worst level is 1
                         lambda: call(B=1.0, ki="maturity"),
                         lambda: call(b=dict(b, s=b["s"] * np.array([1.0, 0.0, 1.0]))), lambda: call(b=dict(b, w=-b["w"])),
                         lambda: call(b=dict(b, v=b["v"] * np.array([1.0, -1.0, 1.0]))), lambda: call(b=dict(b, t=0.0)),
                         lambda: call(b=dict(b, r=float("inf"))), lambda: call(b=dict(b, d=np.array([0.0, 0.0, 0.5]))),
                         lambda: call(n=0)]
            for i, bad in enumerate(bad_calls):
                with pytest.raises(mc.McError, match=INVALID):
                    bad()
                    print(f"bad call {i} ({X}) was served")
            h = e.prepared("autocall", X, dict(b, n_dates=m, **con))
            h[0].autocall = None   # a NULL array
            with pytest.raises(mc.McError, match=INVALID):
                e._run("autocall", X, h[0], SEED, 0, n)
            assert call(m=1364, A=1.0, Cb=0.8, n_obs=1, n=1000).n == 1000             # the largest table is served: 3 * 1364 + 3 = 4095
            assert call(m=682, A=1.0, Cb=0.8, n_obs=682, n=1000).n == 1000            # 682 * 6 = 4092
            assert call(B=None, ki=None, n=1000).n == 1000 and call(g=0.0, c=0.0, n=1000).n == 1000
            assert call(A=INF, Cb=0.0, n_obs=4, n=1000).n == 1000
            still_fine(e)
            e.set_control_variate(True)
            with pytest.raises(mc.McError, match=INVALID):
                call()
            e.set_control_variate(False)
            still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=UNSUPPORTED):
                run(e, b, m, n, con, 0, X)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            run(e, b, m, n, con, 0, "f64")
        e.set_normals("native")
        still_fine(e)


# ---- 7. driver --------------------------------------------------------------------------------------------------------
def driver_market():
    s = np.array([100.0, 50.0, 200.0])
    corr = np.array([[1.0, 0.5, 0.4], [0.5, 1.0, 0.6], [0.4, 0.6, 1.0]])
    return dict(s=s, v=np.array([0.2, 0.3, 0.25]), w=1.0 / s, p=np.linalg.cholesky(corr), d=np.zeros(3), k=1.0, t=5.0, r=0.03)


def test_driver_prints_prices_that_agree_with_the_engine(mc, eng):
    exe = os.path.join(ROOT, "drivers", "autocallOpt_f64")
    assert os.path.exists(exe), "drivers/autocallOpt_f64 not built (build())"
    n = 200_000
    out = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    row = {k: (float(p), float(c)) for k, p, c in re.findall(r"^(\w+) price=(\S+) ci=(\S+)", out.stdout, re.M)}
    names = ["note", "note_ki_maturity", "no_trigger_no_coupon"]
    assert set(row) == {k + a for k in names for a in ("", "_antithetic")} | {"from_rainbow_put"}, out.stdout
    b, m, n_obs = driver_market(), 1260, 20
    A = np.where(np.arange(n_obs) < 2, INF, 1.0 - 0.01 * np.arange(n_obs))
    note = ar.contract(A, 0.7, 0.02, barrier=0.6, ki="dates", gearing=1.0, memory=True)
    forms = {"note": note, "note_ki_maturity": dict(note, ki="maturity"),
             "no_trigger_no_coupon": dict(note, autocall=np.full(n_obs, INF), coupon=0.0)}
    try:
        for (name, con), anti in itertools.product(forms.items(), (False, True)):
            eng.set_antithetic(anti)
            e = run(eng, b, m, n, con, 0, "f64")
            got = row[name + ("_antithetic" if anti else "")]
            assert got[0] == pytest.approx(e.expected, rel=1e-9) and got[1] == pytest.approx(e.confidence, rel=1e-5), (name, anti, out.stdout)
    finally:
        eng.set_antithetic(False)
    assert abs(row["no_trigger_no_coupon"][0] - row["from_rainbow_put"][0]) <= 3 * (row["no_trigger_no_coupon"][1] + row["from_rainbow_put"][1])
    assert row["note_ki_maturity"][0] > row["note"][0]
