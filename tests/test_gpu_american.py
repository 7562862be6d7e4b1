"""The Bermudan put and call on the GPU (american_kernel, mc_american_*): every path against the independent float64 model
american_ref.py on the kernels' own normals (Engine.normals, domain 12), for both precisions, antithetic off and on, put and call,
date counts around every loop boundary (the fp32 loop takes 4 dates per trip, the fp64 loop 8 then 2) up to
MC_MAX_AMERICAN_DATES and path ranges across the 2^32-unit seam; identities; the sums of a call of many grid-stride trips; the bit
rules; the launch form, timing off, an armed slot; the fit (american_fit_kernel, american_solve_kernel, mc_american_fit_*): one date
launch on model-made state, the whole fit against the model's, fp32 against fp64; prices against the lattice; refusals; the C driver.

Tolerances: TOL[X]["pay"] (tests/test_gpu_parity.py) in american_ref's forward-error bound, per path.  A path that is not near
(american_ref) matches the model within its bound; a near path matches, within the bound, one of the values it can take; no path is
left out.  The share of near paths is capped at 5 % (tests/test_american_ref.py does the same on numpy normals)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import american_ref as am
import greeks_ref as gr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
NEAR_CAP = 0.05
FEW_BLOCKS = 16


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
    """An engine of 16 blocks: the pricing pass then runs at most 24 workgroups (6144 lanes) and a date launch of the fit at most 16
    (4096 lanes), so that the shapes below make every lane walk several paths -- the grid-stride trips the default engine's grid
    (3072 and 2048 workgroups) never needs below 786 432 and 524 288 paths."""
    e = mc.Engine(0, blocks=FEW_BLOCKS)
    yield e
    e.close()


def normals(e, X, first, n, m):
    return am.american_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, gr.NPB[X])


def check_paths(got, P, anti, what):
    ok = am.admissible(got.astype(np.float64), P, anti)
    share = float(P.near.mean())
    far = ~P.near
    worst = float((np.abs(got - P.value)[far] / np.maximum(P.bound[far], 1e-300)).max()) if far.any() else 0.0
    print(f"{what}: near {share:.4f}, worst err/bound off the near paths {worst:.3g}")
    assert share <= NEAR_CAP, (what, share)
    assert ok.all(), (what, int((~ok).sum()), np.flatnonzero(~ok)[:5], got[~ok][:5], P.value[~ok][:5], P.bound[~ok][:5])


# ---- 1. per path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("mi", range(len(am.DATES)))
def test_every_path_against_the_reference(mc, eng, X, mi):
    m, n = am.DATES[mi], am.GPU_PATHS
    assert am.DATES[-1] == mc._lib.MAX_AMERICAN_DATES and mc._lib.DOMAIN_AMERICAN == am.DOMAIN_AMERICAN
    try:
        for kind, first in (("put", 0), ("call", U32 - 100), ("put", 12345 + (U32 if m % 2 else 0))):
            o, beta = am.MARKETS[kind], am.rule(kind, m)
            z = normals(eng, X, first, n, m)
            for anti in (False, True):
                eng.set_antithetic(anti)
                got = eng.american_paths(o, m, beta, n, SEED, first, X, kind)
                P = am.price(o, m, kind, beta, z, anti, TOL[X]["pay"], am.U[X])
                check_paths(got, P, anti, f"{X} {kind} m={m} first={first} anti={anti}")
    finally:
        eng.set_antithetic(False)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", [5, 64])
def test_every_path_of_several_grid_stride_trips(few, X, m):
    """20 000 paths on the engine of 16 blocks: 6144 lanes, so a lane walks three or four paths and writes out[i] for i beyond the stride."""
    n, first = 20_000, U32 - 7000
    few.american_paths(am.MARKETS["put"], m, am.rule("put", m), 1000, SEED, 0, X, "put")
    grid, group = few.last_launch()
    assert grid * group == 1024 and FEW_BLOCKS * 3 // 2 * 256 < n // 3      # a small call takes what it needs; the cap is 6144 lanes
    try:
        for kind in ("put", "call"):
            o, beta = am.MARKETS[kind], am.rule(kind, m)
            z = normals(few, X, first, n, m)
            for anti in (False, True):
                few.set_antithetic(anti)
                got = few.american_paths(o, m, beta, n, SEED, first, X, kind)
                P = am.price(o, m, kind, beta, z, anti, TOL[X]["pay"], am.U[X])
                check_paths(got, P, anti, f"{X} {kind} m={m} several trips anti={anti}")
    finally:
        few.set_antithetic(False)


# ---- 2. identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_identities(eng, X):
    """Rows that never exercise leave the vanilla payoff of the same walk; all-zero rows exercise at the first date in the
    money; one date is the vanilla payoff whatever the rule holds."""
    n, first = 3000, 4242
    for kind in ("put", "call"):
        o, q = am.MARKETS[kind], am.sign(kind)
        for m in (1, 6, 21):
            z = normals(eng, X, first, n, m)
            xk, bx, g = am.constants(o, m)
            e = np.exp(xk + bx * np.cumsum(z.astype(np.float64), axis=1))
            p = np.maximum(q * (e - 1.0), 0.0)
            never = np.tile(am.NEVER, (m, 1))
            junk = np.full((m, 4), 123.0)
            for beta, want in ((never, p[:, m - 1]), (np.zeros((m, 4)), None), (junk if m == 1 else None, p[:, m - 1])):
                if beta is None:
                    continue
                if want is None:   # the first date in the money
                    itm = p > 0
                    j = np.where(itm.any(axis=1), itm.argmax(axis=1), m - 1)
                    want = (p * g)[np.arange(n), j]
                got = eng.american_paths(o, m, beta, n, SEED, first, X, kind)
                P = am.price(o, m, kind, beta, z, False, TOL[X]["pay"], am.U[X])
                assert np.allclose(P.value, want, rtol=1e-13, atol=0), (kind, m)
                check_paths(got, P, False, f"{X} {kind} m={m} identity")


# ---- 3. sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_sums_of_a_call_of_many_trips(few, X):
    """300 000 paths on the engine of 16 blocks, 48 or 49 grid-stride trips per lane: the call's sums are the model's, scaled by k and
    k^2; a near path may add the spread of its admissible values."""
    eng = few
    m, n, first, chunk, kind = 16, 300_000, 777, 50_000, "put"
    o, beta, k = am.MARKETS[kind], am.rule(kind, 16), am.MARKETS[kind]["k"]
    zs = [normals(eng, X, f, min(chunk, first + n - f), m) for f in range(first, first + n, chunk)]
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            g = eng.american(o, m, beta, n, SEED, first, X, kind)
            parts = [am.price(o, m, kind, beta, z, anti, TOL[X]["pay"], am.U[X]) for z in zs]
            v, b = np.concatenate([p.value for p in parts]), np.concatenate([p.bound for p in parts])
            near = np.concatenate([p.near for p in parts])
            top = np.concatenate([np.maximum(*(c.max(axis=1) for c in p.cand)) if anti else p.cand.max(axis=1) for p in parts])
            b = np.where(near, top + b, b)
            assert g.n == v.size == n and near.mean() <= NEAR_CAP
            assert eng.last_launch()[0] == FEW_BLOCKS * 3 // 2
            tol, tol2 = k * b.sum(), k * k * (2 * np.abs(v) * b + b * b).sum()
            print(f"{X} anti={anti}: sum err {abs(g.sum - k * v.sum()):.3g} (tol {tol:.3g}), sum2 err {abs(g.sum2 - k * k * (v * v).sum()):.3g} (tol {tol2:.3g})")
            assert abs(g.sum - k * v.sum()) <= tol
            assert abs(g.sum2 - k * k * (v * v).sum()) <= tol2
            r = float(np.float32(o["r"])) if X == "f32" else o["r"]   # the discount is folded from the struct's own r
            assert g.expected == pytest.approx(math.exp(-r * o["t"]) * g.sum / n, rel=1e-14)
    finally:
        eng.set_antithetic(False)


# ---- 4. bit rules, launch form, timing off, armed slot ----------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_bit_rules(mc, eng, X):
    kind, m, f, n = "put", 13, 3001, 2500
    o, beta = am.MARKETS[kind], am.rule(kind, 16)[:13]
    other = mc.Engine(0, blocks=96)
    try:
        for anti in (False, True):
            for e in (eng, other):
                e.set_antithetic(anti)
            whole = eng.american_paths(o, m, beta, f + n, SEED, 0, X, kind)
            part = eng.american_paths(o, m, beta, n, SEED, f, X, kind)
            assert np.array_equal(part, whole[f:])                                              # a path's value depends on its global index only
            assert np.array_equal(other.american_paths(o, m, beta, n, SEED, f, X, kind), part)  # not on the grid
            fused = eng.american(o, m, beta, 123_457, SEED, f, X, kind)
            eng.set_finish(False)
            two = eng.american(o, m, beta, 123_457, SEED, f, X, kind)
            eng.set_finish(True)
            assert (fused.sum, fused.sum2, fused.n) == (two.sum, two.sum2, two.n)
            eng.set_timing(False)
            quiet = eng.american(o, m, beta, 123_457, SEED, f, X, kind)
            eng.set_timing(True)
            assert (quiet.sum, quiet.sum2, quiet.n, quiet.kernel_ms) == (fused.sum, fused.sum2, fused.n, 0.0)
            lo, hi = eng.american(o, m, beta, 50_001, SEED, f, X, kind), eng.american(o, m, beta, 123_457 - 50_001, SEED, f + 50_001, X, kind)
            assert lo.sum + hi.sum == pytest.approx(fused.sum, rel=TOL[X]["rel"]) and lo.sum2 + hi.sum2 == pytest.approx(fused.sum2, rel=TOL[X]["rel"])
    finally:
        eng.set_finish(True)
        eng.set_timing(True)
        eng.set_antithetic(False)
        other.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_launch_form_and_armed_slot(eng, X):
    import torch
    kind, m, n = "call", 12, 200_000
    o, beta = am.MARKETS[kind], am.rule(kind, 16)[:12]
    struct, keep = eng.prepared("american", X, dict(o, n_dates=m, kind=kind, beta=beta))
    triple = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            want = eng.american(o, m, beta, n, SEED, 5, X, kind)
            eng.launch("american", X, struct, SEED, 5, n, triple.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(triple.tolist()) == (want.sum, want.sum2, float(want.n))
            slot = eng.arm_direct()
            assert slot[2] == -1.0
            eng.launch("american", X, struct, SEED, 5, n, triple.data_ptr(), eng.stream)
            assert eng.wait_slot(slot) == (want.sum, want.sum2, float(n))
            torch.cuda.synchronize()
    finally:
        eng.set_antithetic(False)


def test_the_table_is_cached_by_content(eng):
    kind, m, n = "put", 16, 10_000
    o, beta = am.MARKETS[kind], am.rule(kind, 16)
    first = eng.american(o, m, beta, n, SEED, 0, "f64", kind)
    again = eng.american(o, m, beta, n, SEED, 0, "f64", kind)
    assert eng.last_call_stats()["table_upload_ms"] == 0.0
    changed = beta.copy()
    changed[3, 0] *= 1.5
    eng.american(o, m, changed, n, SEED, 0, "f64", kind)
    assert eng.last_call_stats()["table_upload_ms"] > 0.0
    assert (first.sum, first.sum2) == (again.sum, again.sum2)


# ---- 5. the fit ---------------------------------------------------------------------------------------------------------
def fit_normals(e, X, first, n, m):
    return am.fit_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, m, gr.NPB[X])


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n", [8192, 8192 + 37])
@pytest.mark.parametrize("which", ["default", "few"])
def test_one_date_launch_of_the_fit(mc, eng, few, which, X, n):
    """mc_american_fit_date_* on model-made state at dates m, m - 1, a middle date and 0: W within its bound; V by the per-path
    rule (a near path may take either value, and their share is capped); the sums, recomputed by the model from the state the
    launch returned, within 1e-12 relative (fp64) or the tolerance times the sum of absolute terms (fp32: american_ref.date_sums).
    On the engine of 16 blocks a lane takes two or three paths: the state's round trip and the sums beyond the first trip."""
    assert mc._lib.DOMAIN_AMERICAN_FIT == am.DOMAIN_AMERICAN_FIT
    eng = few if which == "few" else eng
    kind, m, first = "put", 12, 5_000_000_000
    o, tol, T = am.MARKETS[kind], TOL[X]["pay"], np.float32 if X == "f32" else np.float64
    beta = am.rule(kind, 16)[:m]
    z = fit_normals(eng, X, first, n, m)
    W_all = am.bridge(z)                                     # the model's own backward walk: state for every date
    rng = np.random.default_rng(5)
    for j in (m, m - 1, 5, 0):
        W_in = (W_all[:, j] if j < m else np.zeros(n)).astype(T)          # W_{j+1}
        V_in = np.abs(rng.standard_normal(n) * 0.05).astype(T)            # any continuation values will do
        b_next = beta[j] if j + 1 < m else np.zeros(4)
        zj = z[:, j - 1] if j > 0 else None
        F = am.fit_date(o, m, kind, j, W_in, V_in, b_next.astype(T), zj, tol)
        W, V, S = eng.american_fit_date(o, m, j, W_in, V_in, b_next, kind, 3, SEED, first, X)
        W, V = W.astype(np.float64), V.astype(np.float64)
        assert eng.last_launch()[0] == (FEW_BLOCKS if which == "few" else (n + 255) // 256)
        share = float(F.near.mean())
        print(f"{X} n={n} j={j}: near {share:.4f}")
        assert share <= NEAR_CAP
        if j > 0:
            assert np.all(np.abs(W - F.W) <= F.W_bound + 1e-300), (j, float(np.abs(W - F.W).max()))
            ok = (np.abs(V - F.V) <= F.V_bound) | (F.near & (np.abs(V - F.V_alt) <= F.V_bound + tol * np.abs(F.V_alt)))
            assert ok.all(), (j, int((~ok).sum()), V[~ok][:4], F.V[~ok][:4])
            kept = ~F.near & (F.V_bound == 0) & (j < m)
            assert np.array_equal(V[kept], V_in.astype(np.float64)[kept])   # a path that does not exercise keeps its bits
        if 0 < j < m:
            want, bound = am.date_sums(o, m, kind, j, W, V, tol)
            assert S[11] == 0 and np.all(np.abs(S - want) <= bound), (j, S, want, bound)
            assert S[0] == round(S[0]) and S[0] > n / 3
        elif j == m:
            assert np.all(S == 0)
        else:
            v, va = F.V, np.where(F.near, F.V_alt, F.V)
            lo, hi = np.minimum(v, va) - F.V_bound, np.maximum(v, va) + F.V_bound
            assert lo.sum() * (1 - 1e-12) <= S[0] <= hi.sum() * (1 + 1e-12) and np.all(S[2:] == 0)
            assert (lo * lo).sum() * (1 - 1e-12) <= S[1] <= (hi * hi).sum() * (1 + 1e-12)


@pytest.mark.parametrize("which", ["default", "few"])
def test_whole_fit_against_the_model(eng, few, which):
    """fp64, 50 dates x 2^16 paths on the fit's own normals: the curves C_j(p) on a grid over the in-the-money range agree with
    the model's.  The tolerance is 16 times what the model's own curves move between two summation orders and a long-double
    solve on the same normals, relative to the curves' size (the test prints the figure; DESIGN 4.13 records it).  On the engine
    of 16 blocks every lane carries 16 paths through each of the 51 date launches."""
    eng = few if which == "few" else eng
    o, m, n, kind = am.TABLE1[0][0], 50, 1 << 16, "put"
    z = fit_normals(eng, "f64", 0, n, m)
    base, ins = am.fit(o, m, kind, 3, z, n)
    grid = np.linspace(0.01, 0.35, 35)
    want = am.curves(base, grid)
    assert np.all(np.isfinite(want))
    own = max(float(np.abs(am.curves(am.fit(o, m, kind, 3, z, n, v)[0], grid) - want).max()) for v in ("reversed", "longdouble"))
    beta, est = eng.american_fit(o, m, n, kind, 3, SEED, 0, "f64")
    err = float(np.abs(am.curves(beta, grid) - want).max())
    print(f"curves: model's own movement {own:.3g}, device against model {err:.3g} (allowed {16 * own:.3g}); curve size {np.abs(want).max():.3g}")
    assert np.all(beta[m - 1] == 0)
    assert err <= 16 * own
    k, disc = o["k"], math.exp(-o["r"] * o["t"])
    assert est.n == n and est.expected == pytest.approx(k * disc * ins[0], rel=1e-9)
    assert est.confidence == pytest.approx(k * ins[1], rel=1e-6)   # mc_closing: the half-width is not discounted


def test_fp32_fit_agrees_with_fp64(eng):
    """Same seed, 50 dates x 2^16 paths: the fp32 fit's in-sample estimate, and the price of its rule on 2^20 fresh paths, within
    3 combined half-widths of the fp64 fit's."""
    o, m, n, kind = am.TABLE1[0][0], 50, 1 << 16, "put"
    b64, e64 = eng.american_fit(o, m, n, kind, 3, SEED, 0, "f64")
    b32, e32 = eng.american_fit(o, m, n, kind, 3, SEED, 0, "f32")
    p64, p32 = eng.american(o, m, b64, 1 << 20, SEED, 0, "f64", kind), eng.american(o, m, b32, 1 << 20, SEED, 0, "f64", kind)
    print(f"in-sample {e64.expected:.5f} / {e32.expected:.5f} +- {e64.confidence:.2g}; price {p64.expected:.5f} / {p32.expected:.5f} +- {p64.confidence:.2g}")
    assert abs(e32.expected - e64.expected) <= 3 * (e32.confidence + e64.confidence)
    assert abs(p32.expected - p64.expected) <= 3 * (p32.confidence + p64.confidence)
    again = eng.american_fit(o, m, n, kind, 3, SEED, 0, "f32")[0]
    assert np.array_equal(again, b32)                                                       # a fit is reproducible
    assert not np.array_equal(eng.american_fit(o, m, n, kind, 3, SEED, n, "f32")[0], b32)   # and another range is another sample
    for degree in (1, 2):
        b = eng.american_fit(o, m, 4096, kind, degree, SEED, 0, "f64")[0]
        assert np.all(b[:, degree + 1:] == 0) and np.all(b[:m - 1, degree] != 0)


def test_fit_refusals(mc, eng):
    o, m, n = am.MARKETS["put"], 12, 4096
    INVALID = "mc error 1"
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad in (dict(n_dates=0), dict(n_dates=mc._lib.MAX_AMERICAN_DATES + 1), dict(n_dates=2 ** 31 - 1), dict(n_dates=-5), dict(degree=0), dict(degree=4), dict(kind=2), dict(n_paths=(1 << 24) + 1),
                        dict(n_paths=0)):
                with pytest.raises(mc.McError, match=INVALID):
                    e.american_fit(o, bad.get("n_dates", m), bad.get("n_paths", n), bad.get("kind", "put"), bad.get("degree", 3), SEED, 0, X)
            with pytest.raises(mc.McError, match=INVALID):
                e.american_fit(dict(o, k=-1.0), m, n, "put", 3, SEED, 0, X)
        e.set_control_variate(True)
        with pytest.raises(mc.McError, match=INVALID):
            e.american_fit(o, m, n)
        e.set_control_variate(False)
        e.set_generator("xorwow")
        with pytest.raises(mc.McError, match=INVALID):
            e.american_fit(o, m, n)
        e.set_generator("philox")
        beta, est = e.american_fit(o, 1, n)          # one date: nothing to fit, the European estimate
        assert np.all(beta == 0) and est.expected > 0
        want = eng.american_fit(o, m, n)[0]
        assert np.array_equal(e.american_fit(o, m, n)[0], want)


# ---- 6. prices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("case", range(3))
def test_prices_against_the_lattice(mc, eng, X, case):
    """Table 1's puts: the rule fitted on 2^18 paths, then 1e7 fresh paths, one fixed seed.  The price is a lower bound: never more
    than 3 half-widths above the lattice price; not more than 3 half-widths below the lattice price less the rule's shortfall, which
    the float64 model measured for a fit of that size on antithetic pairs of its own (american_ref.SHORTFALL, with a half-width a
    tenth of this test's); and above the European price by more than 3."""
    o, m, _, _ = am.TABLE1[case]
    lat, eu = mc.american_lattice(o, m, 64, "put"), am.black_scholes(o, "put")
    short, short_hw = am.SHORTFALL[case]
    beta, ins = eng.american_fit(o, m, am.TABLE1_FIT_PATHS, "put", 3, SEED, 0, X)
    try:
        for anti in (False, True):
            eng.set_antithetic(anti)
            e = eng.american(o, m, beta, 10_000_000, SEED, 0, X, "put")
            print(f"{X} case {case} anti={anti}: price {e.expected:.5f} +- {e.confidence:.2g}, in-sample {ins.expected:.5f}, lattice {lat:.5f}, "
                  f"shortfall {short:.5f} +- {short_hw:.2g}, european {eu:.5f}, fit {ins.kernel_ms:.2f} ms, price {e.kernel_ms:.2f} ms")
            assert e.expected <= lat + 3 * e.confidence
            assert e.expected >= lat - short - 3 * e.confidence
            assert e.expected > eu + 3 * e.confidence
    finally:
        eng.set_antithetic(False)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(mc, eng):
    kind, m, n = "put", 12, 50_000
    o, beta = am.MARKETS[kind], am.rule(kind, 16)[:12]
    with mc.Engine(0) as fresh:
        want = {X: fresh.american(o, m, beta, n, SEED, 0, X, kind) for X in ("f32", "f64")}

    def still_fine(e):
        for X in ("f32", "f64"):
            got = e.american(o, m, beta, n, SEED, 0, X, kind)
            assert (got.sum, got.sum2, got.n) == (want[X].sum, want[X].sum2, want[X].n)

    def rule_with(i, j, x):
        b = beta.copy()
        b[i, j] = x
        return b

    INVALID, UNSUPPORTED = "mc error 1", "mc error 4"
    with mc.Engine(0) as e:
        for X in ("f32", "f64"):
            for bad_m in (0, mc._lib.MAX_AMERICAN_DATES + 1):
                with pytest.raises(mc.McError, match=INVALID):
                    e.american(o, bad_m, np.zeros((max(bad_m, 0), 4)), n, SEED, 0, X, kind)
            for bad in (dict(o, s=0.0), dict(o, k=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf")), dict(o, v=float("nan"))):
                with pytest.raises(mc.McError, match=INVALID):
                    e.american(bad, m, beta, n, SEED, 0, X, kind)
            for bad_kind in (-1, 2):
                with pytest.raises(mc.McError, match=INVALID):
                    e.american(o, m, beta, n, SEED, 0, X, bad_kind)
            for degree in (0, 4):
                struct, keep = e.prepared("american", X, dict(o, n_dates=m, kind=kind, degree=degree, beta=beta))
                with pytest.raises(mc.McError, match=INVALID):
                    e.launch("american", X, struct, SEED, 0, n, 0, 0)
            for b in (rule_with(2, 1, float("nan")), rule_with(0, 0, -float("inf")), rule_with(5, 3, float("inf")), rule_with(10, 2, -float("inf"))):
                with pytest.raises(mc.McError, match=INVALID):
                    e.american(o, m, b, n, SEED, 0, X, kind)
            with pytest.raises(mc.McError, match=INVALID):
                e.american(o, m, beta, 0, SEED, 0, X, kind)
            with pytest.raises(mc.McError, match=INVALID):   # the exponent-range guard of the Asian call
                e.american(dict(o, v=2e4), m, beta, n, SEED, 0, X, kind)
            still_fine(e)
            # what the rule allows: +inf in column 0 ("never"), anything at all in the last row
            e.american(o, m, rule_with(4, 0, float("inf")), n, SEED, 0, X, kind)
            last = e.american(o, m, rule_with(m - 1, 2, float("nan")), n, SEED, 0, X, kind)
            assert (last.sum, last.sum2) == (want[X].sum, want[X].sum2)
        e.set_control_variate(True)
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=INVALID):
                e.american(o, m, beta, n, SEED, 0, X, kind)
        e.set_control_variate(False)
        still_fine(e)
        e.set_generator("xorwow")
        for X in ("f32", "f64"):
            with pytest.raises(mc.McError, match=INVALID):
                e.american(o, m, beta, n, SEED, 0, X, kind)
        e.set_generator("philox")
        still_fine(e)
        e.set_normals("f32")
        with pytest.raises(mc.McError, match=UNSUPPORTED):
            e.american(o, m, beta, n, SEED, 0, "f64", kind)
        e.set_normals("native")
        still_fine(e)


# ---- 8. driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_driver_prices_table_1(X):
    exe = os.path.join(ROOT, "drivers", f"americanOpt_{X}")
    assert os.path.exists(exe), f"drivers/americanOpt_{X} not built (build())"
    out = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^case (\d) (plain|antithetic|in-sample|lattice|european) price=(\S+) ci=(\S+)", out.stdout, re.M)
    assert len(rows) == 15, out.stdout
    got = {(int(c), f): (float(p), float(ci)) for c, f, p, ci in rows}
    for case, (o, m, _, _) in enumerate(am.TABLE1):
        lat, eu = got[case, "lattice"][0], got[case, "european"][0]
        assert lat == pytest.approx(am.lattice(o, m, 16, "put"), rel=1e-6 if X == "f32" else 1e-12)
        assert eu == pytest.approx(am.black_scholes(o, "put"), rel=1e-6 if X == "f32" else 1e-12)
        for form in ("plain", "antithetic"):
            p, ci = got[case, form]
            assert eu < p <= lat + 3 * ci, out.stdout
        assert abs(got[case, "in-sample"][0] - lat) <= 0.02 * lat
