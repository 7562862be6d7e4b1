"""The local-volatility products without a GPU: the lookup rule of the header against mc_localvol_sigma_* (plain C in mc_hostmath.c);
the float64 reference model localvol_ref.py itself -- a flat surface is the constant-volatility models, a time-only surface the
log-normal at the root-mean-square volatility, a float32 evaluation of the same formulas stays within the per-path bound at every
date and seven mutations break it; the near-barrier paths of the GPU test's shapes stay under their cap (a condition, not a
measurement) and the narrow grid clamps on both ends; the refusals that need no device; the structs' layout."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import asian_ref
import barrier_ref
import localvol_ref as lv
from test_gpu_parity import TOL

NPX = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def numpy_normals(m, n, seed):
    return np.random.default_rng(seed).standard_normal((n, m))


# ---- the lookup rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(6, 3, 5), (4, 1, 2), (8, 8, 3), (64, 32, 64), (12, 2, 65)], ids=str)
def test_the_lookup_rule_is_the_headers(mc, X, shape):
    """At the nodes, at the midpoints, beyond both clamps, at n_nodes = 2 and at every slice boundary step: the header's formula in
    float64 on the table as rounded for X, to the last few ulps."""
    m, nt, nn = shape
    lo, hi = -0.5, 0.75   # exact in float32: the nodes below are the nodes of both precisions
    surf = lv.wavy_surface(nt, nn, lo, hi)
    a, b = lv.tables(surf, NPX[X])
    h = (hi - lo) / (nn - 1)
    nodes = lo + h * np.arange(nn)
    ys = np.concatenate([nodes, nodes[:-1] + 0.5 * h, nodes[:-1] + 0.25 * h, [lo - 1.0, lo - 1e-9, hi + 1e-9, hi + 3.0, 0.0]])
    per = m // nt
    steps = sorted({1, m} | {q * per for q in range(1, nt + 1)} | {q * per + 1 for q in range(nt)})
    for step in steps:
        q = (step - 1) // per
        for y in ys:
            got = mc.localvol_sigma(surf, m, step, float(y), X)
            assert got == pytest.approx(lv.sigma_at(surf, m, step, float(y), NPX[X]), rel=1e-13, abs=1e-15), (step, y)
        for i, y in enumerate(nodes):                                       # at a node: its value; the last one through the rounded slope
            want = a[q, i] if i < nn - 1 else a[q, nn - 2] + b[q, nn - 2]
            assert mc.localvol_sigma(surf, m, step, float(y), X) == pytest.approx(want, rel=1e-12)
            assert want == pytest.approx(a[q, i], rel=2.0 ** -23)
        for i in range(nn - 1):                                             # at a midpoint: the mean with the ROUNDED slope
            assert mc.localvol_sigma(surf, m, step, float(nodes[i] + 0.5 * h), X) == pytest.approx(a[q, i] + 0.5 * b[q, i], rel=1e-12)
        assert mc.localvol_sigma(surf, m, step, lo - 5.0, X) == a[q, 0]       # flat beyond both ends
        assert mc.localvol_sigma(surf, m, step, hi + 5.0, X) == pytest.approx(a[q, nn - 2] + b[q, nn - 2], rel=1e-15)
    # the slice rule is the integer one: the last step of a slice reads that slice, the next step the next
    if nt > 1:
        assert mc.localvol_sigma(surf, m, per, lo, X) == a[0, 0] and mc.localvol_sigma(surf, m, per + 1, lo, X) == a[1, 0]
        assert a[0, 0] != a[1, 0]


def test_the_interpolant_is_continuous_across_nodes_and_clamps(mc):
    surf = lv.wavy_surface(2, 5, -0.3, 0.3)
    h = 0.6 / 4
    for k in range(5):
        y = -0.3 + k * h
        below, at, above = (mc.localvol_sigma(surf, 4, 3, y + e) for e in (-1e-12, 0.0, 1e-12))
        assert abs(below - at) < 1e-11 and abs(above - at) < 1e-11


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 5, 16])
def test_a_flat_surface_is_the_constant_volatility_models(nd):
    o = dict(lv.MKT, v=0.23)
    z = numpy_normals(nd, 2000, 3)
    for nt, nn in ((1, 2), (1, 7), (nd, 3)):
        surf = lv.make_surface(np.full((nt, nn), o["v"]), -0.2, 0.3)
        sides = lv.walk(o, surf, nd, 1, z)
        assert np.allclose(lv.asian(sides), asian_ref.asian(o, nd, z).value[0], rtol=1e-12, atol=1e-12)
        for B, kind in ((lv.UP, "up-and-out"), (lv.UP, "up-and-in"), (lv.DOWN, "down-and-out"), (lv.DOWN, "down-and-in")):
            assert np.allclose(lv.barrier(sides, B, kind), barrier_ref.barrier(o, B, nd, z, kind).value[0], rtol=1e-12, atol=1e-12)
        one = lv.walk(o, surf, 1, nd, z)
        w = z.sum(axis=1) / math.sqrt(nd)
        S = o["s"] * np.exp((o["r"] - 0.5 * o["v"] ** 2) * o["t"] + o["v"] * math.sqrt(o["t"]) * w)
        assert np.allclose(lv.european(one, "call"), np.maximum(S - o["k"], 0.0), rtol=1e-12, atol=1e-12)
        assert np.allclose(lv.european(one, "put"), np.maximum(o["k"] - S, 0.0), rtol=1e-12, atol=1e-12)


def test_a_time_only_surface_is_the_log_normal_at_the_rms_volatility():
    """n_nodes = 2 with equal columns: the step is exact in law, y_m = (r - rms^2/2) T + sqrt(dt) sum_j sigma_j z_j on every path."""
    o, m, rows = lv.MKT, 12, np.array([0.15, 0.3, 0.22, 0.4])
    surf = lv.make_surface(np.stack([rows, rows], axis=1), -0.1, 0.1)
    z = numpy_normals(m, 3000, 4)
    sig = np.repeat(rows, m // 4)
    rms2 = (sig ** 2).mean()
    y = (o["r"] - 0.5 * rms2) * o["t"] + math.sqrt(o["t"] / m) * (z * sig[None, :]).sum(axis=1)
    got = lv.walk(o, surf, 1, m, z)[0]["y"][-1]
    assert np.allclose(got, y, rtol=1e-12, atol=1e-13)
    assert np.var(got) == pytest.approx(rms2 * o["t"], rel=0.1)


GRIDS = {"wide": lv.WIDE, "narrow": lv.NARROW}


@pytest.mark.parametrize("grid", ["wide", "narrow"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (5, 1, 5, 3), (9, 3, 3, 65), (16, 16, 1, 65), (64, 2, 2, 65), (64, 32, 2, 64)], ids=str)
def test_a_float32_evaluation_stays_within_the_bound_on_every_path_and_date(shape, grid):
    """The same formulas in numpy float32 (no fma: two roundings where the kernel has one) on float32 normals: y at every date within E
    plus the date's own term, and the three payoffs within their bounds."""
    m, nt, spd, nn = shape
    tol = TOL["f32"]["pay"]
    surf = lv.surface_for(shape, GRIDS[grid])
    z = numpy_normals(m, 4000, 21).astype(np.float32).astype(np.float64)
    nd = m // spd
    for anti in (False, True):
        p = lv.walk(lv.MKT, surf, nd, spd, z, anti, tol=tol, table=np.float32)   # the model: float64 on the float32 table
        q = lv.walk(lv.MKT, surf, nd, spd, z, anti, dtype=np.float32)
        for a, b in zip(p, q):
            r = np.abs(a["y"] - b["y"]) / (a["E"] + tol * (1.0 + np.abs(a["y"])))
            assert np.all(r <= 1.0), (anti, float(r.max()))
        for right in ("call", "put"):
            assert np.all(np.abs(lv.european(q, right) - lv.european(p, right)) <= lv.european_bound(p, right))
            assert np.all(np.abs(lv.asian(q, right) - lv.asian(p, right)) <= lv.asian_bound(p, right))
            for B, kind in ((lv.UP, "up-and-out"), (lv.DOWN, "down-and-in")):
                r, near = lv.barrier_errors(lv.barrier(q, B, kind, right), p, B, kind, right)
                assert np.all(r <= 1.0), (anti, right, kind, float(r.max()))


MUTATION_CASES = {   # mutation: (shape, grid, payoff): an in-the-money call (k = 40) so that every path carries the change
    "slice_late": ((16, 16, 1, 65), lv.WIDE, "european"),
    "round_nearest": ((16, 2, 2, 65), lv.WIDE, "european"),
    "no_half": ((16, 2, 2, 65), lv.WIDE, "european"),
    "clamp_n": ((16, 2, 2, 3), lv.NARROW, "european"),
    "date_late": ((16, 2, 2, 65), lv.WIDE, "asian"),
    "one_more": ((16, 2, 2, 65), lv.WIDE, "asian"),
    "put_as_call": ((16, 2, 2, 65), lv.WIDE, "european_put"),
}


@pytest.mark.parametrize("mutation", lv.MUTATIONS)
def test_the_bound_rejects_a_mutation(mutation):
    shape, grid, payoff = MUTATION_CASES[mutation]
    m, nt, spd, nn = shape
    o = dict(lv.MKT, k=40.0, t=2.0)
    surf = lv.surface_for(shape, grid)
    z = numpy_normals(m, 4000, 31)
    p = lv.walk(o, surf, m // spd, spd, z, tol=TOL["f32"]["pay"])
    q = lv.walk(o, surf, m // spd, spd, z, mutation=mutation)
    if payoff == "asian":
        diff, b = np.abs(lv.asian(q, "call", mutation) - lv.asian(p)), lv.asian_bound(p)
    else:
        right = "put" if payoff == "european_put" else "call"
        diff, b = np.abs(lv.european(q, right, mutation) - lv.european(p, right)), lv.european_bound(p, right)
    share = (diff > b).mean()
    print(mutation, share)
    assert share > lv.MUTATION_SHARE, (mutation, share)


@pytest.mark.parametrize("shape", lv.SHAPES + [lv.BIG_SHAPE], ids=str)
def test_near_barrier_paths_stay_under_the_cap_on_the_shapes_of_the_gpu_test(shape):
    """A condition on the test's shapes, not a measurement: exactly the (shape, grid, precision) set of the GPU test, on numpy normals,
    both path directions, both barriers."""
    m, nt, spd, nn = shape
    n = lv.N_PATHS if m > 64 else 4 * lv.N_PATHS
    z = numpy_normals(m, n, 1000 + m)
    for grid in (lv.WIDE, lv.NARROW):
        surf = lv.surface_for(shape, grid)
        for X in ("f32", "f64"):
            if X == "f32" and m > lv.F32_BARRIER_MAX_STEPS:
                continue
            sides = lv.walk(lv.MKT, surf, m // spd, spd, z, anti=True, tol=TOL[X]["pay"], table=NPX[X])
            for B, kind in ((lv.UP, "up-and-out"), (lv.DOWN, "down-and-in")):
                _, near = lv.barrier_errors(lv.barrier(sides, B, kind), sides, B, kind)
                print(f"{shape} {grid} {X} {kind}: {near.mean():.3%} near")
                assert near.mean() <= lv.NEAR_CAP, (shape, grid, X, kind, near.mean())
                assert np.all(np.isfinite(lv.european_bound(sides)))


@pytest.mark.parametrize("shape", [s for s in lv.SHAPES if s[0] >= 2], ids=str)
def test_the_narrow_grid_clamps_on_both_ends(shape):
    """On every shape of the GPU test but the one of a single step: there the only lookup is at y_0 = 0, inside any grid around 0, so no
    clamp can run (the GPU test's one-step shape checks the first lookup and the payoffs, not the clamps)."""
    m, nt, spd, nn = shape
    s = lv.walk(lv.MKT, lv.surface_for(shape, lv.NARROW), m // spd, spd, numpy_normals(m, 4000, 7), tol=1e-14)[0]
    lo, hi = s["clamped"].mean(axis=1)
    print(shape, lo, hi)
    assert lo >= 0.10 and hi >= 0.10, (shape, lo, hi)


def test_the_displaced_price_obeys_parity_and_its_flat_limit():
    for k in (80.0, 100.0, 120.0):
        c, p = lv.displaced_price(100.0, k, 0.03, 1.0, 0.2, 50.0), lv.displaced_price(100.0, k, 0.03, 1.0, 0.2, 50.0, "put")
        assert c - p == pytest.approx(100.0 - k * math.exp(-0.03))
        assert lv.displaced_price(100.0, k, 0.03, 1.0, 0.2, 0.0) == pytest.approx(lv.black_scholes_call(dict(s=100.0, k=k, r=0.03, v=0.2, t=1.0)), rel=1e-12)
    surf = lv.displaced_surface(0.2, 50.0, 0.03, 1.0, 8, 65, -1.5, 1.5)
    assert surf["sigma"].shape == (8, 65) and surf["sigma"][7, 32] == pytest.approx(0.2 * (100.0 + 50.0 * math.exp(-0.03 / 16)) / 100.0)
    assert set(lv.BIAS) == {80.0, 100.0, 120.0} and all(h > 0 for _, h in lv.BIAS.values())


# ---- the refusals that need no device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_refusals(mc, X):
    from montecarlocuda_amd.engine import _LocalVolHolder, check
    L = mc._lib
    INVALID = "mc error 1"
    nan, inf = float("nan"), float("inf")
    o = dict(s=100.0, k=100.0, r=0.03, t=1.0)
    good = lv.wavy_surface(2, 5, -0.5, 0.5)

    def sigma(opt=o, surface=good, nd=4, spd=3, payoff="european", right="call", barrier=130.0, kind="up-and-out", n_steps=None, step=1, y=0.0,
              null=False, n_times=None, n_nodes=None):
        h = _LocalVolHolder(X, opt, surface, nd, spd, payoff, right, barrier, kind)
        if n_steps is not None:
            h.struct.n_steps = n_steps
        if n_times is not None:
            h.struct.n_times = n_times
        if n_nodes is not None:
            h.struct.n_nodes = n_nodes
        if null:
            h.struct.sigma = C.POINTER(L.CT[X])()
        out = C.c_double()
        check(getattr(L.lib(), f"mc_localvol_sigma_{X}")(C.byref(h.struct), step, y, C.byref(out)))
        return out.value

    assert sigma() == pytest.approx(mc.localvol_sigma(good, 12, 1, 0.0, X))
    for bad_steps in (0, -3, L.MAX_LOCALVOL_STEPS + 1):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(n_steps=bad_steps)
    for nt, nn in ((0, 5), (-1, 5), (2, 1), (2, 0), (2, 1025), (1, 2049), (4096, 2)):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(n_times=nt, n_nodes=nn, n_steps=4096 if nt > 0 and 4096 % nt == 0 else None)
    assert np.isfinite(sigma(surface=lv.wavy_surface(32, 64, -1.0, 1.0), nd=64, spd=1))           # the cap itself
    with pytest.raises(mc.McError, match="does not divide"):
        sigma(surface=lv.wavy_surface(5, 3, -0.5, 0.5))                                            # 12 steps, 5 slices
    for bad_spd in (0, -1, 5, 7, 13):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(spd=bad_spd, n_steps=12)
    with pytest.raises(mc.McError, match="NULL sigma"):
        sigma(null=True)
    for v in (-0.01, nan, inf):
        s = good["sigma"].copy()
        s[1, 3] = v
        with pytest.raises(mc.McError, match=r"sigma\[1\]\[3\]"):
            sigma(surface=dict(good, sigma=s))
    for lo, hi in ((0.5, 0.5), (0.5, -0.5), (nan, 0.5), (-0.5, inf), (-inf, 0.5)):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(surface=dict(good, y_lo=lo, y_hi=hi))
    tiny = 1e-45 if X == "f32" else 5e-324                                                       # 1 / h overflows the precision
    for lo, hi in ((0.0, 4 * tiny), (-2 * tiny, 2 * tiny)):
        with pytest.raises(mc.McError, match="too small"):
            sigma(surface=dict(good, y_lo=lo, y_hi=hi))
    for bad in (-1, 3, 7):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(payoff=bad)
    for bad in (-1, 2):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(right=bad)
    for bad in (-1, 4):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(payoff="barrier", kind=bad)
    assert np.isfinite(sigma(payoff="asian", kind=99, barrier=nan))                               # ignored by the other payoffs
    for bad_b in (0.0, -5.0, nan, inf):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(payoff="barrier", barrier=bad_b)
    for bad_b, kind in ((100.0, "up-and-out"), (90.0, "up-and-in"), (100.0, "down-and-out"), (110.0, "down-and-in")):
        with pytest.raises(mc.McError, match="on or beyond"):
            sigma(payoff="barrier", barrier=bad_b, kind=kind)
    for bad in (dict(o, s=0.0), dict(o, s=-3.0), dict(o, t=0.0), dict(o, t=-1.0), dict(o, r=inf), dict(o, k=nan), dict(o, s=inf), dict(o, t=nan)):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(opt=bad)
    with pytest.raises(mc.McError, match="outside the range of a double"):
        sigma(surface=dict(good, sigma=np.full((2, 5), 3e4)), nd=4096, spd=1)                      # the exponent-range guard
    for step, y in ((0, 0.0), (13, 0.0), (1, nan), (1, inf)):
        with pytest.raises(mc.McError, match=INVALID):
            sigma(step=step, y=y)
    assert np.isfinite(sigma(opt=dict(o, v=nan)))                                                  # option.v is ignored


def test_struct_layout(mc):
    L = mc._lib
    for X, R in (("f32", C.c_float), ("f64", C.c_double)):
        S = L.LOCALVOL[X]
        assert [f[0] for f in S._fields_] == ["option", "sigma", "n_times", "n_nodes", "y_lo", "y_hi", "n_steps", "steps_per_date", "payoff",
                                              "right", "barrier_type", "barrier"]
        assert S.sigma.offset == (24 if X == "f32" else 40) and S.barrier.size == C.sizeof(R)
    assert (L.LOCALVOL_PAYOFFS, L.LOCALVOL_RIGHTS, L.DOMAIN_LOCALVOL) == (dict(european=0, asian=1, barrier=2), dict(call=0, put=1), lv.DOMAIN_LOCALVOL)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mc_mi355x.h")).read()
    for text in ("#define MC_DOMAIN_LOCALVOL 16u", "#define MC_MAX_LOCALVOL_STEPS 4096", "#define MC_MAX_LOCALVOL_NODES 2048",
                 "enum { MC_LOCALVOL_EUROPEAN = 0, MC_LOCALVOL_ASIAN = 1, MC_LOCALVOL_BARRIER = 2 };", "enum { MC_LOCALVOL_CALL = 0, MC_LOCALVOL_PUT = 1 };"):
        assert text in header
    assert (L.MAX_LOCALVOL_STEPS, L.MAX_LOCALVOL_NODES) == (4096, 2048)
