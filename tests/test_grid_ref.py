"""The launch-geometry mode's sample definition (grid_ref.py) on the CPU, on the oracle's streams (pyoracle.grid_normals, bit-equal to
rocRAND's host-callable engine: test_rocrand_xcheck.py):
  (a) unmutated, the model's arrangement IS pyoracle.grid_path_normals, bit for bit, on every geometry test_gpu_grid_ref.py runs --
      the model was written from the header's paragraph, the oracle's by the kernels' hand: where the two agree here and the
      kernels agree with the model on the GPU, all three do; and by hand on a launch small enough to write down;
  (b) the draws rule as the header states it equals cva_ref.schedule(c, X).n_dates on every CVA market in use;
  (c) the bound has power: on every family's in-the-money markets and every geometry, each wrong sample of grid_ref.MUTATIONS
      moves at least 90 % of the paths it reaches beyond the fp32 bound (and no path it cannot reach at all);
  (d) the geometry list meets the conditions it was chosen for, under the piece rule of grid_pieces (csrc/mc_launch_shape.hpp)
      restated here -- here only, to guard the list; the GPU module reads the count from the launch.
"""
import numpy as np
import pytest

import cva_ref as cr
import grid_ref as gf
import xorwow_ref as xr

POWER = 0.9
SEG_ALIGN = 8


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


# ---- the oracle's streams, by seed -------------------------------------------------------------------------------------------
_STREAMS = {}


def seed_streams(po, seed, T, count):
    """(T, count) float32: the first `count` normals of threads 0 .. T - 1 of the block seeded `seed` (orc_grid_normals seeds block b
    of G with b + G: block `seed` of 0)."""
    have = _STREAMS.get((seed, T))
    if have is None or have.shape[1] < count:
        import ctypes as C
        L = po.lib()
        L.orc_grid_normals.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
        L.orc_grid_normals.restype = None
        n = max(count, 2 * have.shape[1] if have is not None else 0)
        have = np.empty((T, n), dtype=np.float32)
        row = (C.c_float * n)()
        for t in range(T):
            L.orc_grid_normals(0, seed, t, n, row)
            have[t] = np.frombuffer(row, dtype=np.float32)
        _STREAMS[(seed, T)] = have
    return have[:, :count]


def streams_of(po, c, p):
    count = gf.count_needed(c, p)
    return np.stack([seed_streams(po, int(s), c.T, count) for s in p.seeds])


def pieces_rule(G, T, per_block):
    """(sub, seg) of grid_pieces as it stands: doubled while the launch stays within 8 waves a SIMD's worth of lanes (8 x 1024 x 64,
    threads rounded up to whole waves) and a piece keeps 16 paths of thread 0, up to 32; seg = thread 0's share rounded up to 8."""
    n_max = -(-per_block // T)
    lanes, want, s = G * (-(-T // 64) * 64), 8 * 1024 * 64, 1
    while s < 32 and lanes * s * 2 <= want and n_max >= 16 * s * 2:
        s *= 2
    return s, -(-(-(-n_max // s)) // SEG_ALIGN) * SEG_ALIGN


# ---- (a) the arrangement -----------------------------------------------------------------------------------------------------------
def test_seed_streams_are_the_oracle_s(po):
    want = po.grid_normals(3, 5, 10)
    for b in range(3):
        assert np.array_equal(seed_streams(po, b + 3, 5, 10).view(np.uint32), want[b].view(np.uint32))
    assert not np.array_equal(seed_streams(po, 0, 5, 10), want[0])


@pytest.mark.parametrize("geom", list(gf.GEOMS))
def test_the_arrangement_is_the_oracle_s_bit_for_bit(po, geom):
    G, T, per_block = geom
    for draws in (1, 2, 3, 5, 8, 13, 16, 17, 33, 65):
        c = gf.Call("basket", G, T, per_block, draws, draws)
        s = po.grid_normals(G, T, gf.count_needed(c))
        assert gf.count_needed(c) - po.grid_draws_per_thread(T, per_block, draws) in (0, 1)
        got, want = gf.arrange(s, c), po.grid_path_normals(s, per_block, draws)
        assert got.shape == want.shape == (G * per_block, draws)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (geom, draws)


def test_the_arrangement_and_every_mutation_by_hand():
    """Two blocks of two threads, five paths a block, three normals a path; stream entry = 1000 seed + 100 thread + position."""
    c = gf.Call("basket", 2, 2, 5, 3, 3)

    def s(seeds, count=16, T=2):
        return np.array([[[1000 * sd + 100 * t + q for q in range(count)] for t in range(T)] for sd in seeds])
    z = gf.arrange(s([2, 3]), c)
    # block 0 (seed 2): thread 0 prices paths 0, 2, 4 from positions 0, 3, 6; thread 1 paths 1, 3 from 0, 3; block 1 is seed 3
    assert z[:5].tolist() == [[2000, 2001, 2002], [2100, 2101, 2102], [2003, 2004, 2005], [2103, 2104, 2105], [2006, 2007, 2008]]
    assert z[5:7].tolist() == [[3000, 3001, 3002], [3100, 3101, 3102]]
    assert gf.thread_paths(c).tolist() == [3, 2] and gf.count_needed(c) == 10

    def m(name, cc=c, sub=1, seg=0):
        p = gf.plan(cc, name, sub, seg)
        return gf.arrange(s(p.seeds, 96, cc.T), cc, p), gf.reach(name, cc, sub, seg)
    z1, r = m("block_contiguous_map")          # thread 0: paths 0, 1, 2; thread 1: paths 3, 4
    assert z1[:5, 0].tolist() == [2000, 2003, 2006, 2100, 2103] and r[:5].tolist() == [False, True, True, True, True]
    z1, r = m("kept_member_dropped_between_paths")
    assert z1[:5, 0].tolist() == [2000, 2100, 2004, 2104, 2008] and r[:5].tolist() == [False, False, True, True, True]
    z1, r = m("cosine_member_first")
    assert z1[:3].tolist() == [[2001, 2000, 2003], [2101, 2100, 2103], [2002, 2005, 2004]] and r.all()
    z1, r = m("block_seeded_without_grid_size")
    assert z1[[0, 5], 0].tolist() == [0, 1000] and r.all()
    z1, r = m("padded_basket_draws_compiled_size")
    assert z1[:5, 0].tolist() == [2000, 2100, 2004, 2104, 2008]
    cva = gf.Call("cva", 2, 2, 5, 3, 5)         # three of five dates draw
    z1, r = m("cva_draws_for_every_grid_date", cva)
    assert z1[:5].tolist() == [[2000, 2001, 2002], [2100, 2101, 2102], [2005, 2006, 2007], [2105, 2106, 2107], [2010, 2011, 2012]]
    assert r[:5].tolist() == [False, False, True, True, True]
    assert not gf.applies("cva_draws_for_every_grid_date", gf.Call("cva", 2, 2, 5, 5, 5))
    # one block of one thread, 20 paths of three normals in two pieces of 16: piece 1 = paths 16 .. 19, its state at word 48
    one = gf.Call("basket", 1, 1, 20, 3, 3)
    assert gf.arrange(s([1], 64, 1), one)[[15, 16, 19], 0].tolist() == [1045, 1048, 1057]
    z1, r = m("piece_starts_unaligned", one, 2, 16)      # piece 1 begins at path ceil(20 / 2) = 10, from word 48
    assert z1[[9, 10, 11, 19], 0].tolist() == [1027, 1048, 1051, 1075] and r.tolist() == [False] * 10 + [True] * 10
    z1, r = m("piece_state_advanced_by_paths", one, 2, 16)      # piece 1's state at word 16
    assert z1[[15, 16, 17], 0].tolist() == [1045, 1016, 1019] and r.tolist() == [False] * 16 + [True] * 4
    assert not gf.applies("piece_starts_unaligned", gf.Call("basket", 1, 1, 32, 3, 3), 2, 16)      # ceil(32 / 2) is the aligned 16


def test_box_muller_is_the_oracle_s_stream(po):
    """grid_ref.box_muller of the oracle's words is the oracle's normal stream within the float functions' error (the GPU module
    ties Engine.grid_normals to Engine.xorwow_words through it, at the same 4e-6)."""
    for G, b, T, count in ((1, 0, 3, 400), (5, 2, 2, 400)):
        want = po.grid_normals(G, T, count)[b].astype(np.float64)
        got = gf.box_muller(np.array([po.xorwow_words(b + G, t, count) for t in range(T)], dtype=np.uint32))
        assert np.abs(got - want).max() <= 4e-6, float(np.abs(got - want).max())
    w = np.array([[0, 0, 0xFFFFFFFF, 0x40000000]], dtype=np.uint32)      # u = 2^-32 and v = c; u rounds to 1: both members 0
    z = gf.box_muller(w)[0]
    assert z[0] == pytest.approx(np.sqrt(64 * np.log(2.0)) * 1.46291807e-09, rel=1e-6) and z[1] == pytest.approx(np.sqrt(64 * np.log(2.0)))
    assert z[2] == 0.0 and z[3] == 0.0


# ---- (b) the draws rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", gf.PRECISIONS)
def test_the_draws_rule_is_the_schedule_s_date_count(X):
    markets = [xr.cva_market(X, d) for d in xr.CVA_DATES] + [cr.market(case) for case in cr.CASES]
    markets += [m for d in gf.CVA_DATES + ["long"] for _, m in gf.cva_markets(X, d)]
    for c in markets:
        assert gf.cva_draws(c, X) == cr.schedule(c, X).n_dates, (X, c)
    # what the GPU module's subset covers, in this precision: every ending, one date, odd and even counts, a cut long schedule
    sch = [cr.schedule(xr.cva_market(X, d), X) for d in gf.CVA_DATES]
    assert [s.n_dates for s in sch] == gf.CVA_DATES and {s.ending for s in sch} == set(xr.ENDINGS)
    assert 1 in gf.CVA_DATES and {d % 2 for d in gf.CVA_DATES} == {0, 1}
    long = cr.schedule(cr.market(gf.CVA_LONG), X)
    assert (long.n_dates, long.ending) == (257, "cut")
    cut = [d for d, s in zip(gf.CVA_DATES, sch) if s.ending == "cut"]
    assert cut and all(gf.cva_draws(xr.cva_market(X, d), X) == d < xr.cva_market(X, d)["n_grid"] for d in cut)


# ---- (d) the geometries ----------------------------------------------------------------------------------------------------------
def test_the_geometries_meet_their_conditions():
    geoms = list(gf.GEOMS)
    Ts = {T for _, T, _ in geoms}
    assert {1, 64, 100, 512, 1024} <= Ts and any(T % 2 == 1 and 1 < T < 64 for T in Ts)
    assert any(per < T for _, T, per in geoms) and any(per % T != 0 and per > T and gf.GEOMS[(G, T, per)] > 1 for G, T, per in geoms) and any(G > 1 for G, _, _ in geoms)
    assert all(G * per <= 16000 for G, _, per in geoms) and len(geoms) <= 9
    rule = {g: pieces_rule(*g) for g in geoms}
    assert {g: sub for g, (sub, _) in rule.items()} == gf.GEOMS
    assert {sub for sub, _ in rule.values()} == {1, 2, 4, 8, 16, 32}
    empty = [g for g, (sub, seg) in rule.items() if (sub - 1) * seg >= -(-g[2] // g[1])]      # thread 0 has nothing for the last piece
    assert empty, rule
    # every piece but the last is whole and pair-aligned whatever a path draws; a piece's offset fits the 32-bit offset matrices
    assert all(seg % SEG_ALIGN == 0 and sub * seg * 257 < 1 << 32 for sub, seg in rule.values())
    # baskets and the CVA run every geometry (the long schedule: SMALL_GEOM), so each meets 1024 threads, 16 and 32 pieces, and odd
    # draws with more than one piece
    assert rule[gf.SMALL_GEOM][0] == 16 and gf.cva_geoms("long") == [gf.SMALL_GEOM] and gf.cva_geoms(5) == geoms
    assert any(n % 2 for n in gf.BASKET_FUSED) and any(d % 2 for d in gf.CVA_DATES)
    assert gf.BASKET_FUSED == [1, 2, 3, 4, 5, 7, 8, 9, 13, 16] and gf.BASKET_STAGED_ONLY == [17, 33]


# ---- (c) the bound has power --------------------------------------------------------------------------------------------------------
def family_markets(mc, family, X):
    """(tag, in-the-money market, geometries)"""
    if family == "vanilla":
        return [(i, gf.vanilla_markets(i)[1][1], list(gf.GEOMS)) for i in range(gf.N_VANILLA_MARKETS)]
    if family == "basket":
        return [(n, gf.basket_markets(mc, n)[1][1], list(gf.GEOMS)) for n in gf.BASKET_FUSED + gf.BASKET_STAGED_ONLY]
    return [(d, gf.cva_markets(X, d)[1][1], gf.cva_geoms(d)) for d in gf.CVA_DATES + ["long"]]


@pytest.mark.parametrize("family", ["vanilla", "basket", "cva"])
@pytest.mark.parametrize("X", gf.PRECISIONS)
def test_every_wrong_sample_moves_the_paths_it_reaches(mc, po, X, family):
    """Struck in the money: |mutated model - model| beyond the fp32 bound on at least 90 % of the paths the mutation reaches, nothing
    else moved at all; every mutation that can act on the family acts."""
    weakest = {}
    for tag, market, geoms in family_markets(mc, family, X):
        for geom in geoms:
            c = gf.call(family, geom, market, X)
            sub, seg = pieces_rule(*geom) if c.size <= 16 else (1, 0)      # (no fused kernel beyond 16 assets: no pieces)
            names = [k for k in gf.MUTATIONS if gf.applies(k, c, sub, seg)]
            p0 = gf.plan(c)
            p = gf.value(c, market, gf.arrange(streams_of(po, c, p0), c, p0), X)
            bnd = gf.bound(p, "f32")
            for name in names:
                pm = gf.plan(c, name, sub, seg)
                q = gf.value(c, market, gf.arrange(streams_of(po, c, pm), c, pm), X)
                reach = gf.reach(name, c, sub, seg)
                assert reach.sum() >= min(32, c.G * c.per_block // 2), (name, geom, tag, int(reach.sum()))
                moved = np.abs(q.value[0] - p.value[0]) > bnd
                share = float(moved[reach].mean())
                assert share >= POWER, (name, geom, tag, share, int(reach.sum()))
                assert np.array_equal(q.value[0][~reach], p.value[0][~reach]), (name, geom, tag)
                weakest[name] = min(weakest.get(name, (2.0, None)), (share, (geom, tag)), key=lambda w: w[0])
    want = {"block_contiguous_map", "cosine_member_first", "block_seeded_without_grid_size", "piece_starts_unaligned"}
    want |= {"vanilla": set(), "basket": {"kept_member_dropped_between_paths", "padded_basket_draws_compiled_size", "piece_state_advanced_by_paths"},
             "cva": {"kept_member_dropped_between_paths", "cva_draws_for_every_grid_date", "piece_state_advanced_by_paths"}}[family]
    if family == "vanilla":
        want |= {"kept_member_dropped_between_paths"}      # one draw a path is an odd number of draws
    assert set(weakest) == want, (sorted(weakest), sorted(want))
    for name, (share, where) in sorted(weakest.items()):
        print(f"grid power {family} {X} {name}: weakest share {share:.3f} at {where}")
