"""The float64 CVA pricing model (cva_ref.py) on the CPU: that the oracle twin of the pricing kernels stays inside its bound on
every market test_gpu_cva_ref.py prices, that those markets' schedules cover what the kernels branch on, that the bound has power
-- the index errors of cva_ref.MUTATIONS move almost every path beyond the fp32 bound -- and that the model prices what the
closed form does."""
import math

import numpy as np
import pytest

import cva_ref as cr
import greeks_ref as gr
from test_gpu_parity import SEED, cva_analytic

N_TWIN, FIRST = 1500, 11


def all_cases(X):
    """(name, market, paths of the twin test) of everything test_gpu_cva_ref.py prices in precision X."""
    out = [(f"t{t}-n{g}", cr.market((t, g)), N_TWIN) for t, g in cr.CASES]
    out += [(f"extra{i}", cr.extra_market(X, i), N_TWIN) for i in range(cr.N_EXTRA)]
    grids = [g for g, _ in cr.THRESHOLD_GRIDS[X] + cr.SPLIT_GRIDS[X]] + (cr.PAIR_ROW_GRIDS if X == "f32" else [])
    return out + [(f"threshold-n{g}", cr.threshold_market(g), 150) for g in sorted(set(grids))]      # long grids: fewer paths


_normals = {}


def twin_normals(po, X, n, n_dates):
    """The oracle's own CVA normals of paths FIRST .. FIRST + n - 1: drawn once per precision (the stream does not depend on the market)."""
    key = (X, n)
    if key not in _normals:
        cols = max(cr.schedule(c, X).n_dates for _, c, m in all_cases(X) if m == n)
        _normals[key] = gr.cva_normals(lambda dom, u0, cnt, blk: np.array([po.dev_normals(X, SEED, dom, u0 + u, blk) for u in range(cnt)]),
                                       FIRST, n, cols, gr.NPB[X])
    return _normals[key][:, :n_dates]


# ---- the twin stays inside the bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_oracle_twin_stays_inside_the_bound(po, X):
    """po.dev_cva evaluates the kernels' formulas in the kernels' precision with the host's libm: within the per-path bound of the
    model on every GPU-tested market, plain and antithetic, using a small part of it -- the bound holds without a GPU and leaves
    the hardware's exp2 / log2 room."""
    worst = (0.0, None)
    for name, c, n in all_cases(X):
        z = twin_normals(po, X, n, cr.schedule(c, X).n_dates)
        for anti in (False, True):
            got, o = po.dev_cva(X, c, SEED, FIRST, n, antithetic=anti)
            p = cr.price(c, z, X, anti)
            err, bnd = np.abs(got.astype(np.float64) - p.value[0]), cr.bound(p, X)
            assert np.all(err <= bnd), (name, anti, float((err / bnd).max()))
            ratio = float(np.max(np.where(err > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)))
            worst = max(worst, (ratio, (name, anti)))
            if not (c["lgd"] and c["defint"]):
                assert not np.any(got) and not np.any(p.value) and o["sum"] == 0.0 and o["sum2"] == 0.0, name
    print(f"cva twin {X}: worst err/bound {worst[0]:.4f} at {worst[1]}")
    assert worst[0] <= 1


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_twin_stays_inside_the_bound_on_the_chosen_normals(po, X):
    """The normals test_gpu_cva_ref.py sends through cva_from_normals: d1 or d2 within a few ulp of 0, the last spot within a few
    ulp of K, single normals at the generator's extremes."""
    worst = 0.0
    for case in cr.CHOSEN_CASES:
        c = cr.market(case)
        z = cr.chosen_normals(c, X, np.random.default_rng(77))
        full = np.zeros((z.shape[0], c["n_grid"]), dtype=z.dtype)
        full[:, :z.shape[1]] = z
        p = cr.price(c, z.astype(np.float64), X)
        assert np.isfinite(p.value).all() and np.isfinite(p.scale).all()
        for anti in (False, True):
            got, _ = po.dev_cva_on_normals(X, c, full, antithetic=anti)
            p = cr.price(c, z.astype(np.float64), X, anti)
            ratio = np.abs(got.astype(np.float64) - p.value[0]) / cr.bound(p, X)
            worst = max(worst, float(ratio.max()))
    print(f"cva twin on chosen normals {X}: worst err/bound {worst:.4f}")
    assert worst <= 1


# ---- the model organised as the kernel is the model ---------------------------------------------------------------------
def test_lanes_model_is_the_price_at_every_lane_count():
    rng = np.random.default_rng(3)
    for case in cr.CASES:
        c = cr.market(case)
        for X in ("f32", "f64"):
            z = rng.standard_normal((200, cr.schedule(c, X).n_dates))
            for anti in (False, True):
                p = cr.price(c, z, X, anti)
                for lanes in cr.LANES:
                    assert np.all(np.abs(cr.lanes_model(c, z, X, lanes, anti) - p.value[0]) <= 1e-14 * p.scale[0]), (case, X, lanes, anti)
    assert [cr.lanes_used(l, 65) for l in cr.LANES] == [1, 2, 4, 8, 16, 16, 16] and cr.lanes_used(64, 257) == 64 and cr.lanes_used(64, 256) == 32
    assert cr.lanes_used(2, 8) == 1 and cr.lanes_used(2, 9) == 2


def test_antithetic_price_is_the_pair_mean():
    c = cr.market((1.625, 13))
    z = np.random.default_rng(4).standard_normal((300, 13))
    a, p, m = cr.price(c, z, "f64", anti=True), cr.price(c, z, "f64"), cr.price(c, -z, "f64")
    assert a.value.shape == (1, 300) and np.array_equal(a.value, 0.5 * (p.value + m.value)) and np.array_equal(a.scale, 0.5 * (p.scale + m.scale))
    assert np.array_equal(p.value[0], gr.cva(c, z, "f64").value[0]) and np.array_equal(p.scale[0], gr.cva(c, z, "f64").scale[0])
    # the only jump is the Hastings cnd's own step at d = 0: 1e-9 of the terms in play, on paths within eps of it
    assert p.jump.shape == (1, 300) and np.all(p.jump > 0) and np.all(p.jump <= 1.1e-9 * p.scale) and gr.kink_free(p, 1e-10)
    assert 1.0e-9 < cr.HASTINGS_STEP < 1.1e-9


# ---- guard on the lists -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_cases_cover_what_the_kernels_branch_on(X):
    sch = {case: cr.schedule(cr.market(case), X) for case in cr.CASES}
    assert {(s.ending, s.parity) for s in sch.values()} == {(e, q) for e in ("full", "cut", "intrinsic") for q in (0, 1)}
    # the classes as cva_ref lists them
    assert all(sch[k].ending == "intrinsic" and sch[k].parity == 0 for k in cr.INTRINSIC_EVEN)
    assert all(sch[k].ending == "intrinsic" and sch[k].parity == 1 for k in cr.INTRINSIC_ODD)
    assert all(sch[k].ending == "full" for k in cr.FULL) and {sch[k].parity for k in cr.FULL} == {0, 1}
    assert all(sch[k] == cr.Schedule(257, 257, "cut", 1, 0) for k in cr.CUT_LONG)
    cut = {k: sch[k].ending for k in cr.CUT}
    assert cut == ({(1.0, 250): "cut", (1.0, 129): "cut", (1.0, 500): "full", (0.7321, 37): "full", (0.7321, 100): "intrinsic"} if X == "f32" else
                   dict.fromkeys(cr.CUT, "cut"))
    # the intrinsic date (0-based index n_bs) on an even index: at a chunk's start, inside a chunk, at a round's start
    even = [s for s in sch.values() if s.ending == "intrinsic" and s.parity == 0]
    assert any(s.n_bs % cr.CH == 0 for s in even) and any(s.n_bs % cr.CH not in (0, cr.CH - 1) for s in even)
    for lanes in (8, 16):
        assert any(cr.lanes_used(lanes, s.n_dates) == lanes and s.n_bs == cr.CH * lanes for s in even), lanes
    # at every lane count that a forced call really runs: a last date pair with one date and with two, a cut and a full schedule
    for lanes in cr.LANES[1:]:
        at = [s for s in sch.values() if cr.lanes_used(lanes, s.n_dates) == lanes]
        assert {s.n_dates % 2 for s in at} == {0, 1}, lanes
        assert {"cut", "full"} <= {s.ending for s in at}, lanes
        assert any(s.n_dates > cr.CH * lanes for s in at), lanes      # more than one round
    # the host thresholds of cva_enqueue, from both sides
    for grids, limit in ((cr.THRESHOLD_GRIDS[X], cr.DATES_MAX[X]), (cr.SPLIT_GRIDS[X], cr.SPLIT_MAX[X])):
        (g_in, fits), (g_out, beyond) = grids
        assert fits and not beyond
        assert cr.schedule(cr.threshold_market(g_in), X).n_dates == limit and cr.schedule(cr.threshold_market(g_out), X).n_dates in (limit + 1, limit + 2)
    if X == "f32":
        assert [cr.schedule(cr.threshold_market(g), X).n_bs for g in cr.PAIR_ROW_GRIDS] == [682, 683, 684]      # 48 * (n_bs // 2) <= 16 KB up to 683
    # the extra markets
    ex = [cr.extra_market(X, i) for i in range(cr.N_EXTRA)]
    assert ex[5]["lgd"] < 0 and ex[6]["lgd"] == 0 and ex[7]["defint"] == 0 and all(c["lgd"] > 0 and c["defint"] > 0 for c in ex[:5])


def test_the_older_grids_never_price_the_intrinsic_date_on_an_even_index():
    """test_gpu_cva_dates.GRIDS at t = 1 (and the Greeks tests' two intrinsic grids): no intrinsic schedule with an even n_bs and
    more than 8 dates, so cva_dates_role's `first = ja == o.n_bs` branch was run by none of them."""
    from test_gpu_cva_dates import CVA0, GRIDS
    for X in ("f32", "f64"):
        intrinsic = []
        for t, n_grid in [(1.0, g) for g in GRIDS] + [(1.0, 64), (3.0, 300)]:
            s = cr.schedule(dict(CVA0, t=t, n_grid=n_grid), X)
            if s.ending == "intrinsic":
                intrinsic.append(n_grid)
                assert s.parity == 1 or s.n_dates <= cr.CH, (X, n_grid, s)
        assert {1, 2, 8, 16, 64, 256} <= set(intrinsic) <= {1, 2, 8, 16, 64, 256, 300}, X


# ---- power --------------------------------------------------------------------------------------------------------------
LANE_MUTATIONS = ("lane_first_date_misses_chunk_below", "second_round_misses_first_total")
# The power list: the schedule cases (all GPU-tested, at every lane count, plain and antithetic) on which a mutation applies in
# BOTH precisions' schedules unless marked, and on which it must move at least 90 % of 2000 paths beyond the fp32 bound.  A case
# is absent from a mutation's list where no correct fp32 test could see it on 90 % of the paths: paths out of the money at the
# last date carry no intrinsic value, and on long grids the exchange of two adjacent rows changes a path by less than the bound.
SMALL = [(1.125, 9), (1.375, 11), (1.625, 13), (2.125, 17), (1.0, 16), (0.375, 24)]      # dt >= 1 / 64: the intrinsic date's own share of the bound is large
POWER = {
    "intrinsic_neighbour_xk": SMALL,
    "pair_rows_exchanged": [(1.125, 9), (1.375, 11), (1.625, 13)],
    "lane_first_date_misses_chunk_below": SMALL + [(8.125, 65), (16.125, 129), (1.0, 64), (0.7321, 37), (1.0, 63), (1.0, 65)],
    "second_round_misses_first_total": [(2.125, 17), (0.375, 24), (1.0, 64), (1.0, 256), (1.0, 250), (1.0, 129), (0.7321, 100), (1.0, 500),
                                        (0.7321, 37), (1.0, 63), (1.0, 127)],
    "date_beyond_cut_contributes": cr.CUT + cr.CUT_LONG,       # (three of them are cut in fp64 only)
    "anti_mirror_spot_only": SMALL + [(8.125, 65), (16.125, 129), (1.0, 64), (1.0, 256), (1.0, 250), (1.0, 129), (0.7321, 100), (0.7321, 37),
                                      (1.0, 63), (1.0, 65), (1.0, 127), (1.0, 258), (2.0, 514)],
}


def power_params():
    return [(name, case) for name, cases in POWER.items() for case in cases]


def test_every_mutation_has_its_cases():
    assert set(POWER) == set(cr.MUTATIONS)
    for name, cases in POWER.items():
        assert len(cases) >= 3 and set(cases) <= set(cr.CASES), name
    assert set(POWER["intrinsic_neighbour_xk"]) & set(cr.INTRINSIC_EVEN) and set(POWER["intrinsic_neighbour_xk"]) & set(cr.INTRINSIC_ODD)


@pytest.mark.parametrize("name,case", power_params(), ids=lambda v: v if isinstance(v, str) else f"t{v[0]}-n{v[1]}")
def test_every_mutation_moves_almost_every_path(name, case):
    """In each precision's schedule in which the mutation applies, under each estimator, and for the two mutations of the running
    sum at every lane count that a forced call runs (the others do not depend on it): at least 90 % of 2000 paths move beyond the
    fp32 bound.  (A market that fails this is reseeded in cva_ref.RESEEDED; the 90 % stays.)"""
    c = cr.market(case)
    ran = 0
    for X in ("f32", "f64"):
        s = cr.schedule(c, X)
        z = np.random.default_rng(cr.seed_of(case)).standard_normal((2000, s.n_dates))
        for anti in (False, True):
            if name in LANE_MUTATIONS:
                Ls = sorted({cr.lanes_used(l, s.n_dates) for l in cr.LANES if cr.applies(name, s, l, anti)})
            else:
                Ls = [1] if cr.applies(name, s, 1, anti) else []
            if not Ls:
                continue
            bnd = cr.bound(cr.price(c, z, X, anti), "f32")
            clean = cr.lanes_model(c, z, X, 1, anti)       # (test_lanes_model_is_the_price_at_every_lane_count: the same at every L)
            for L in Ls:
                moved = np.abs(cr.lanes_model(c, z, X, L, anti, name) - clean) > bnd
                assert moved.mean() >= 0.9, (name, case, X, anti, L, int(moved.sum()))
                ran += 1
    assert ran, (name, case)


def test_mutations_apply_where_they_say():
    s9, s8, s65 = cr.Schedule(9, 8, "intrinsic", 0, 0), cr.Schedule(8, 8, "cut", 0, 7), cr.Schedule(65, 65, "full", 1, 0)
    assert cr.applies("intrinsic_neighbour_xk", s9, 1, False) and not cr.applies("intrinsic_neighbour_xk", s65, 1, False)
    assert cr.applies("date_beyond_cut_contributes", s8, 4, True) and not cr.applies("date_beyond_cut_contributes", s9, 4, True)
    assert cr.applies("lane_first_date_misses_chunk_below", s9, 2, False) and not cr.applies("lane_first_date_misses_chunk_below", s8, 2, False)
    assert not cr.applies("lane_first_date_misses_chunk_below", s65, 1, False)
    assert cr.applies("second_round_misses_first_total", s65, 8, False) and not cr.applies("second_round_misses_first_total", s65, 16, False)
    assert cr.applies("anti_mirror_spot_only", s65, 1, True) and not cr.applies("anti_mirror_spot_only", s65, 1, False)
    assert cr.applies("pair_rows_exchanged", s8, 64, False)


# ---- the price is the closed form's -------------------------------------------------------------------------------------
def test_price_meets_the_closed_form():
    """E[CVA] = LGD sum_j dp_j C_0 e^{r t_j} (test_gpu_parity.cva_analytic): within 3.5 sigma at 2e5 paths (the Hastings cnd's
    1e-7-level price error is far below it)."""
    c = dict(gr.random_cva(np.random.default_rng(31)), t=1.5, n_grid=12)
    assert cr.schedule(c, "f64").ending == "intrinsic"
    z = np.random.default_rng(32).standard_normal((200_000, 12))
    for anti in (False, True):
        v = cr.price(c, z, "f64", anti).value[0]
        assert abs(v.mean() - cva_analytic(c)) <= 3.5 * v.std() / math.sqrt(v.size) + 2e-6, anti
