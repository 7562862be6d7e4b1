"""The CVA PRICING kernels -- cva_kernel (one lane per path), cva_dates_kernel (a path's dates shared by 2 ... 64 lanes) and
cva_split_kernel (both in one launch) -- per path against the float64 model cva_ref.price (greeks_ref.cva's own CVA), on random
ASYMMETRIC markets, on schedules of every ending (full, cut, intrinsic) and parity, on the device's own normals (Engine.normals).

Why: test_gpu_parity.py, test_gpu_cva_dates.py and test_gpu_hotloop.py compare these kernels with the oracle twin (the same
formulas in the same precision) on the one market CVA0 (s = k = 100, t = 1), whose grids never put the intrinsic-value date on an
even index of a date-parallel grid (cva_dates_role's `first` branch), never cross a host threshold of cva_enqueue, and whose
constant tolerance means something at that market's scale only.  test_cva_ref.py shows that the index errors of
cva_ref.MUTATIONS move almost every path of the markets priced here beyond the bound used here.

Tolerances: per path greeks_ref.bound(p, TOL[X]["pay"]), the eps of the Greeks tests, per unit of the model's forward-error scale.
Sums are held to the same call's own per-path dump: the values of a call share one sign and are added in fp64 in some order, so
|sum - S p| <= n 2^-53 S |p| and |sum2 - S p^2| <= (n + 1) 2^-53 S p^2 (p^2 is exact inside the device's fma, rounded once on
the host), with S taken exactly (math.fsum).  Every family prints its worst err/bound.
"""
import contextlib

import numpy as np
import pytest

import cva_ref as cr
import greeks_ref as gr
from greeks_ref import check_sums
from test_gpu_parity import SEED

pytestmark = pytest.mark.gpu

U32 = 1 << 32
N_PATHS = 3001                 # no multiple of a lane-group count: dead path slots at every lane count
FIRSTS = (11, U32 - 1000)      # the second crosses the 2^32-unit seam: two segments
GROUP = 256


# ---- plumbing -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def setting(e, lanes, anti=False):
    e.set_cva_date_lanes(lanes), e.set_antithetic(anti)
    try:
        yield
    finally:
        e.set_cva_date_lanes(0), e.set_antithetic(False)


_normals = {}


def device_normals(e, X, first, n, n_dates):
    """The device's own CVA normals of paths first .. first + n - 1, (n, n_dates) in fp64: one draw per (precision, mode, range),
    shared by every market (the stream does not depend on the market)."""
    npb = 4 if (X == "f32" or e._normals_f32) else 8
    key = (X, npb, first, n)
    if key not in _normals or _normals[key].shape[1] < n_dates:
        cols = max(n_dates, 520 if n <= N_PATHS else 0)
        z = gr.cva_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, cols, npb)
        z.setflags(write=False)
        _normals[key] = z
    return _normals[key][:, :n_dates]


def check_paths(got, p, X, what):
    """Per path within the bound; returns the worst err/bound (0 where model and kernel are both exactly 0)."""
    bnd, v = cr.bound(p, X), p.value[0]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == v.shape, what
    err = np.abs(got - v)
    assert np.all(err <= bnd), (what, int(np.argmax(err - bnd)), float(err.max()), float(bnd.min()), int((err > bnd).sum()))
    return float(np.max(np.where(err > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)))


def models(c, z, X):
    """(plain, antithetic) model Paths on normals z."""
    return cr.price(c, z, X), cr.price(c, z, X, anti=True)


def form(e, n, first=0):
    """'one' (ceil(n / 256) workgroups per segment: one lane per path) or 'dates' (more), of the last launch (the last segment's)."""
    room = U32 - (first & (U32 - 1))
    last = n if n <= room else n - room
    one = min(-(-last // GROUP), e.blocks * 3 // 2)      # grid_for at GRID_SCALE_CVA
    wgs = e.last_launch()[0]
    assert wgs >= one, (wgs, one)
    return "one" if wgs == one else "dates"


worst_by_family = {}


def note(family, X, ratio):
    worst_by_family[(family, X)] = max(worst_by_family.get((family, X), 0.0), ratio)


def family_of(lanes_used, split=False):
    return "split" if split else ("one lane" if lanes_used == 1 else "date-parallel")


def report(test, X):
    print(f"cva_ref {test} {X}: worst err/bound so far " + ", ".join(f"{f} {r:.4f}" for (f, x), r in sorted(worst_by_family.items()) if x == X))


# ---- a, b. every family per path, sums against the call's own dump ------------------------------------------------------
def sweep(e, c, X, what):
    """Every lane count x {plain, antithetic} x both first paths: per path within the bound, sums against the dump, and the
    form that ran what cva_plan says."""
    nd = cr.schedule(c, X).n_dates
    for first in FIRSTS:
        z = device_normals(e, X, first, N_PATHS, nd)
        for anti, p in zip((False, True), models(c, z, X)):
            for lanes in cr.LANES:
                with setting(e, lanes, anti):
                    got = e.cva_paths(c, N_PATHS, SEED, first, X)
                    L = cr.lanes_used(lanes, nd)
                    assert form(e, N_PATHS, first) == ("one" if L == 1 else "dates"), (what, lanes, L)
                    est = e.cva(c, N_PATHS, SEED, first, X)
                tag = (what, X, first, lanes, anti)
                note(family_of(L), X, check_paths(got, p, X, tag))
                check_sums(est, got, N_PATHS, tag)
                if not (c["lgd"] and c["defint"]):
                    assert not np.any(got) and est.sum == 0.0 and est.sum2 == 0.0, tag


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("case", cr.CASES, ids=lambda k: f"t{k[0]}-n{k[1]}")
def test_every_family_on_every_schedule(eng, X, case):
    sweep(eng, cr.market(case), X, case)
    report("a", X)


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("i", range(cr.N_EXTRA))
def test_every_family_on_unconstrained_markets(eng, X, i):
    sweep(eng, cr.extra_market(X, i), X, ("extra", i))
    report("a", X)


# ---- c. bit rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("blocks,n", [(0, N_PATHS), (16, 7001)], ids=["default", "16-workgroups"])
def test_a_path_has_the_same_bits_wherever_its_call_starts(mc, X, blocks, n):
    """cva_paths(c, n, SEED, f) == cva_paths(c, f + n, SEED, 0)[f:] bitwise at every lane count; on 16 workgroups (24 in the
    CVA's grid) the paths outnumber the slots of every form and the loops go grid-stride."""
    f = 1234
    word = np.uint32 if X == "f32" else np.uint64
    with mc.Engine(0, blocks) as e:
        for case in ((8.125, 65), (1.0, 129)):      # intrinsic on an even index; cut
            c = cr.market(case)
            for anti in (False, True):
                for lanes in cr.LANES:
                    with setting(e, lanes, anti):
                        a = e.cva_paths(c, n, SEED, f, X)
                        b = e.cva_paths(c, f + n, SEED, 0, X)[f:]
                    assert np.array_equal(a.view(word), b.view(word)), (case, X, lanes, anti)
                    assert np.any(a), (case, X)


# ---- d. thresholds and fallbacks --------------------------------------------------------------------------------------
N_BIG = 1301    # long grids: fewer paths keep the numpy model to a second


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_table_beyond_lds_keeps_one_lane_per_path(eng, X):
    """Forced to 8 lanes: the per-date table fits 48 KB of LDS up to 1024 dates in fp64 and 2048 in fp32; one date more runs one
    lane per path."""
    for n_grid, parallel in cr.THRESHOLD_GRIDS[X]:
        c = cr.threshold_market(n_grid)
        nd = cr.schedule(c, X).n_dates
        assert (nd <= cr.DATES_MAX[X]) == parallel
        z = device_normals(eng, X, FIRSTS[0], N_BIG, nd)
        with setting(eng, 8):
            got = eng.cva_paths(c, N_BIG, SEED, FIRSTS[0], X)
            assert form(eng, N_BIG) == ("dates" if parallel else "one"), (X, n_grid)
            est = eng.cva(c, N_BIG, SEED, FIRSTS[0], X)
        note(family_of(8 if parallel else 1), X, check_paths(got, cr.price(c, z, X), X, (X, n_grid)))
        check_sums(est, got, N_BIG, (X, n_grid))
    report("d", X)


def test_fp32_pair_rows_from_lds_and_from_scalar_registers(eng):
    """fp32, one lane per path: the date pairs' rows come from LDS while they fit 16 KB (n_bs / 2 <= 341: n_bs = 682, 683) and
    from scalar registers beyond (684)."""
    for n_grid in cr.PAIR_ROW_GRIDS:
        c = cr.threshold_market(n_grid)
        s = cr.schedule(c, "f32")
        assert s.n_bs == n_grid
        z = device_normals(eng, "f32", FIRSTS[0], N_BIG, s.n_dates)
        with setting(eng, 1):
            got = eng.cva_paths(c, N_BIG, SEED, FIRSTS[0], "f32")
            assert form(eng, N_BIG) == "one"
            est = eng.cva(c, N_BIG, SEED, FIRSTS[0], "f32")
        note("one lane", "f32", check_paths(got, cr.price(c, z, "f32"), "f32", n_grid))
        check_sums(est, got, N_BIG, n_grid)
    report("d", "f32")


# ---- e. the split launch under the automatic rule -----------------------------------------------------------------------
def split_shapes(X):
    """(market, remainder in paths (None: 60 % of a trip), one more path, split expected)."""
    yield cr.market((8.125, 65)), 1000, 0, True
    yield cr.market((8.125, 65)), None, 0, True           # 100 r <= 60 trip, at the largest such r
    yield cr.market((8.125, 65)), None, 1, False
    yield cr.market((1.0, 63)), 1000, 0, False            # fewer than 64 dates
    for n_grid, fits in cr.SPLIT_GRIDS[X]:                # either side of 24 KB of table
        yield cr.threshold_market(n_grid), 1000, 0, fits


def grid_one(e, n):
    return min(-(-n // GROUP), e.blocks * 3 // 2)


def grid_dates(e, n, L):
    return min(-(-n * L // GROUP), e.blocks * 3 // 2)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_split_launch_under_the_automatic_rule(eng, X):
    """n = 2 trips + r: the leading trips one lane per path, the remainder date-parallel, in one launch of grid_for(main) + g_tail
    workgroups -- when r is at most 60 % of a trip (100 r == 60 trip where a trip is a multiple of 5 paths, the largest r below
    that otherwise), the grid has 64 dates or more and the table fits 24 KB; one launch of one lane per path otherwise.  The
    antithetic estimator and a range that crosses 2^32 fall back to one lane per path."""
    trip = 256 * eng.info()["compute_units"]
    for c, r, more, split in split_shapes(X):
        r = (60 * trip // 100 if r is None else r) + more
        n, main = 2 * trip + r, 2 * trip
        s = cr.schedule(c, X)
        assert split == (100 * r <= 60 * trip and s.n_dates >= 64 and s.n_dates <= cr.SPLIT_MAX[X]), (X, c["n_grid"], r)
        L = cr.lanes_used(1 << max(1, ((2 * trip + r - 1) // r - 1).bit_length()), s.n_dates)     # cva_plan: ~two waves per SIMD
        want_grid = grid_one(eng, main) + grid_dates(eng, r, L) if split else grid_one(eng, n)
        lo = main - 700
        z = device_normals(eng, X, lo, n - lo, s.n_dates)
        p = cr.price(c, z, X)
        tag = (X, c["n_grid"], r, split)
        with setting(eng, 0):
            for rep in range(3):        # repeated: the tickets must be back at zero
                est = eng.cva(c, n, SEED, 0, X)
                assert eng.last_launch()[0] == want_grid, (tag, eng.last_launch(), want_grid)
                got = eng.cva_paths(c, n, SEED, 0, X)
                assert eng.last_launch()[0] == want_grid, tag
                check_sums(est, got, n, (tag, rep))
            ratio = check_paths(got[lo:], p, X, tag)
            note(family_of(L, split), X, ratio)
        if split and r == 1000:
            with setting(eng, 0, anti=True):        # the split kernel is compiled for the plain estimator
                got = eng.cva_paths(c, n, SEED, 0, X)
                assert eng.last_launch()[0] == grid_one(eng, n), tag
                check_sums(eng.cva(c, n, SEED, 0, X), got, n, (tag, "anti"))
                note("one lane", X, check_paths(got[lo:], cr.price(c, z, X, anti=True), X, (tag, "anti")))
            first = U32 - main - 300                # the tail would cross 2^32: two segments
            with setting(eng, 0):
                got = eng.cva_paths(c, n, SEED, first, X)
                assert eng.last_launch()[0] == grid_one(eng, r - 300), tag
                check_sums(eng.cva(c, n, SEED, first, X), got, n, (tag, "seam"))
                zs = device_normals(eng, X, first + lo, n - lo, s.n_dates)
                note("one lane", X, check_paths(got[lo:], cr.price(c, zs, X), X, (tag, "seam")))
    report("e", X)


# ---- f. fp32 normals in the fp64 kernels ------------------------------------------------------------------------------
def test_fp32_normals_mode_is_fp64_downstream(mc):
    """set_normals("f32"): the normal is a widened float, everything downstream of it fp64, so on the mode's own normals the fp64
    bound holds per path -- one lane per path, date-parallel and split."""
    with mc.Engine(0) as e:
        e.set_normals("f32")
        for case in ((8.125, 65), (1.0, 129), (1.0, 256)):
            c = cr.market(case)
            nd = cr.schedule(c, "f64").n_dates
            z = device_normals(e, "f64", FIRSTS[0], N_PATHS, nd)
            assert np.array_equal(z, z.astype(np.float32).astype(np.float64)) and np.abs(z).max() < 6.77
            for anti, p in zip((False, True), models(c, z, "f64")):
                for lanes in (1, 4, 64):
                    with setting(e, lanes, anti):
                        got = e.cva_paths(c, N_PATHS, SEED, FIRSTS[0], "f64")
                        est = e.cva(c, N_PATHS, SEED, FIRSTS[0], "f64")
                    note("fp32 normals", "f64", check_paths(got, p, "f64", (case, lanes, anti)))
                    check_sums(est, got, N_PATHS, (case, lanes, anti))
        trip = 256 * e.info()["compute_units"]
        c = cr.market((8.125, 65))
        n, main, lo = 2 * trip + 1000, 2 * trip, 2 * trip - 700
        with setting(e, 0):
            got = e.cva_paths(c, n, SEED, 0, "f64")
            assert e.last_launch()[0] == grid_one(e, main) + grid_dates(e, 1000, 16)
            check_sums(e.cva(c, n, SEED, 0, "f64"), got, n, "split")
        z = device_normals(e, "f64", lo, n - lo, 65)
        note("fp32 normals", "f64", check_paths(got[lo:], cr.price(c, z, "f64"), "f64", "split"))
    print(f"cva_ref f: worst err/bound fp32 normals {worst_by_family[('fp32 normals', 'f64')]:.4f}")


# ---- g. chosen normals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_chosen_normals_through_the_from_normals_hook(eng, X):
    """Values compared, nothing provoked: every normal is one the generator can draw, every market passes build_cva_table's range
    check, every model value is finite."""
    for case in cr.CHOSEN_CASES:
        c = cr.market(case)
        z = cr.chosen_normals(c, X, np.random.default_rng(77))
        full = np.zeros((z.shape[0], c["n_grid"]), dtype=z.dtype)         # the hook takes n_grid normals per path
        full[:, :z.shape[1]] = z
        p = cr.price(c, z.astype(np.float64), X)
        assert np.isfinite(p.value).all() and np.isfinite(p.scale).all()
        for lanes in (1, 4, 64):
            with setting(eng, lanes):
                est, vals = eng.cva_from_normals(c, full, X)
            note("external", X, check_paths(vals, p, X, (case, X, lanes)))
            check_sums(est, vals, z.shape[0], (case, X, lanes))
    report("g", X)


# ---- h. table reuse -----------------------------------------------------------------------------------------------------
def test_table_reuse_sees_every_field(mc):
    """cva_table_ready reuses the uploaded table when its key matches: one context, one lane setting, a market, then copies that
    differ in exactly one field, then the first again, fp32 and fp64 alternately.  Every call meets its own model; the repeat has
    its first run's bits."""
    base = cr.market((1.0, 65))
    changes = [dict(defint=base["defint"] * 1.5), dict(lgd=base["lgd"] * 0.5), dict(s=base["s"] * 1.01), dict(k=base["k"] * 0.99),
               dict(r=base["r"] + 0.004), dict(v=base["v"] * 1.02), dict(t=1.25), dict(n_grid=66)]
    n = 1001
    for lanes in (1, 8):
        with mc.Engine(0) as e, setting(e, lanes):
            first_run = {}
            for c in [base] + [dict(base, **ch) for ch in changes] + [base]:
                for X in ("f32", "f64"):
                    nd = cr.schedule(c, X).n_dates
                    got = e.cva_paths(c, n, SEED, FIRSTS[0], X)
                    z = device_normals(e, X, FIRSTS[0], N_PATHS, nd)[:n]
                    check_paths(got, cr.price(c, z, X), X, (lanes, X, c))
                    check_sums(e.cva(c, n, SEED, FIRSTS[0], X), got, n, (lanes, X, c))
                    if c is base:
                        assert np.array_equal(first_run.setdefault(X, got).view(np.uint8), got.view(np.uint8)), (lanes, X)
