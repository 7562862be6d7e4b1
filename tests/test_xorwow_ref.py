"""The XORWOW mode's sample definition (xorwow_ref.py) on the CPU: on the oracle's words (po.xorwow_words, which
test_rocrand_xcheck.py pins to rocRAND) the model -- assignment from xorwow_ref, values from greeks_ref.vanilla, basket_ref.value
and cva_ref.price -- meets the oracle's XORWOW twin (po.dev_* under po.xorwow_mode) per path on every shape
test_gpu_xorwow_ref.py runs, in both precisions, plain and antithetic (baskets: the control variate too); and the bound has power:
struck in the money, every wrong assignment of xorwow_ref.MUTATIONS moves at least 90 % of the later-trip paths it can reach
beyond the bound.  The twin restates the lane bookkeeping by the kernels' hand; the model was written from the header's sentence:
where the two agree here and the kernels agree with the model on the GPU, all three do.
"""
import functools

import numpy as np
import pytest

import xorwow_ref as xr
from test_gpu_parity import TOL

POWER = 0.9
# (blocks, lanes, units) of test_gpu_xorwow_ref.py's three engines as the launches the twin is asked to mirror (the default
# engine: nine workgroups for 2121 units), and one launch no current grid rule produces -- fewer workgroups than the context's
# blocks AND several trips -- the only kind on which "L from the context's blocks" differs from the launch
LAUNCHES = [(1, 256, xr.UNITS[1]), (2, 512, xr.UNITS[2]), (1024, 9 * 256, xr.UNITS[0])]
HYPOTHETICAL = (4, 512, xr.UNITS[2])
WORDS_MAX = 5 * 9 * 12     # a lane's words: at most four trips (and one unit of slack) of nine fp64 blocks


def seed_base(launch):
    i = (LAUNCHES + [HYPOTHETICAL]).index(launch)
    return xr.SEEDS[i % 2], xr.BASES[(i + 1) % 3]


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@functools.lru_cache(maxsize=None)
def _lane_words(po, seed, base, lanes, count):
    return np.array([po.xorwow_words(seed, base + l, count) for l in range(lanes)], dtype=np.uint32)


def words_of(po, launch):
    seed, base = seed_base(launch)
    per_lane = min(WORDS_MAX, (-(-launch[2] // launch[1]) + 1) * 9 * 12)

    def f(lanes, K):
        assert K <= per_lane, (K, per_lane)
        return _lane_words(po, seed, base, lanes, per_lane)[:, :K]
    return f


def calls(mc, X, family, launch):
    """(call, first path, paths, market, estimators) of one family on one launch."""
    blocks, lanes, units = launch
    if family == "vanilla":
        for i, head in enumerate(xr.VANILLA_HEADS[X]):
            first = xr.NPB[X] * (1000 + 7 * i) + head
            n = units * xr.NPB[X] - head - (1 + i)           # ends inside the last unit
            c = xr.vanilla_call(X, blocks, lanes, first, n)
            assert c.n_units == units and c.head == head
            yield c, first, n, xr.vanilla_market(i), [(False, False), (True, False)]
    elif family == "basket":
        for n_assets in xr.BASKET_SIZES:
            yield (xr.Call("basket", X, blocks, lanes, units, n_assets, 0), 4242 + n_assets, units, xr.basket_market(mc, n_assets),
                   [(False, False), (True, False), (False, True), (True, True)])
    else:
        for d in xr.CVA_DATES:
            yield xr.Call("cva", X, blocks, lanes, units, d, 0), 777 + d, units, xr.cva_market(X, d), [(False, False), (True, False)]


def in_the_money(family, m):
    return {"vanilla": xr.vanilla_in_the_money, "basket": xr.br.in_the_money, "cva": xr.cva_in_the_money}[family](m)


def twin(po, c, market, launch, first, n, anti, control):
    seed, base = seed_base(launch)
    unit0 = first // xr.NPB[c.X] if c.family == "vanilla" else first
    with po.xorwow_mode(seed, base, c.lanes, unit0):
        if c.family == "vanilla":
            got, _ = po.dev_vanilla(c.X, market, seed, first, n, antithetic=anti)
        elif c.family == "basket":
            got, _ = po.dev_basket(c.X, market, seed, first, n, antithetic=anti, control=control)
        else:
            got, _ = po.dev_cva(c.X, market, seed, first, n, antithetic=anti)
    return got.astype(np.float64)


# ---- the model is the twin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["vanilla", "basket", "cva"])
@pytest.mark.parametrize("X", xr.PRECISIONS)
def test_the_model_meets_the_oracle_twin_on_every_path(mc, po, X, family):
    worst = (0.0, None)
    for launch in LAUNCHES:
        for c, first, n, market, estimators in calls(mc, X, family, launch):
            z = xr.product_normals(xr.draw(c, words_of(po, launch), xr.cpu_normals), c, n)
            for m, tag in ((market, "drawn"), (in_the_money(family, market), "itm")):
                for anti, control in estimators:
                    p = xr.value(c, m, z, anti, control)
                    got = twin(po, c, m, launch, first, n, anti, control)
                    err, bnd = np.abs(got - p.value[0]), xr.bound(c, p, TOL)
                    r = xr.ratio(err, bnd)
                    what = (launch, c.size, c.head, tag, anti, control)
                    assert np.all(err <= bnd), (what, int(np.argmax(r)), float(r.max()), int((err > bnd).sum()))
                    worst = max(worst, (float(r.max()), what), key=lambda w: w[0])
    print(f"xorwow twin {family} {X}: worst err/bound {worst[0]:.4f} at {worst[1]}")


# ---- the bound has power ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["vanilla", "basket", "cva"])
@pytest.mark.parametrize("X", xr.PRECISIONS)
def test_every_wrong_assignment_moves_the_later_trips(mc, po, X, family):
    """Struck in the money, plain estimator: |mutated model - model| beyond the bound on at least 90 % of the later-trip paths the
    mutation can reach.  The applicable (mutation, shape) pairs are counted: every mutation of this family and precision acts."""
    seen, weakest = {}, (2.0, None)
    for launch in LAUNCHES + [HYPOTHETICAL]:
        for c, first, n, market, _ in calls(mc, X, family, launch):
            names = [k for k in xr.MUTATIONS if xr.applies(k, c)]
            if not names:
                continue
            m = in_the_money(family, market)
            p = xr.value(c, m, xr.product_normals(xr.draw(c, words_of(po, launch), xr.cpu_normals), c, n))
            bnd = xr.bound(c, p, TOL)
            unit = xr.unit_of_path(c, n)
            for name in names:
                q = xr.value(c, m, xr.product_normals(xr.draw(c, words_of(po, launch), xr.cpu_normals, name), c, n))
                reach = xr.reach(name, c)[unit]
                assert reach.sum() >= xr.NPB[X] if family == "vanilla" else reach.sum() >= 64, (name, launch, c)
                share = float((np.abs(q.value[0] - p.value[0]) > bnd)[reach].mean())
                assert share >= POWER, (name, launch, c.size, c.head, share, int(reach.sum()))
                # ... and nothing it cannot reach moves at all
                assert np.array_equal(q.value[0][~xr.MUTATIONS[name].reach(c)[unit]], p.value[0][~xr.MUTATIONS[name].reach(c)[unit]]), name
                seen[name] = seen.get(name, 0) + 1
                weakest = min(weakest, (share, (name, launch, c.size, c.head)), key=lambda w: w[0])
    want = {"lanes_from_context_blocks", "partial_last_trip_drawn_first"}
    want |= {"vanilla": {"partial_vanilla_unit_skips_dead_paths"}, "basket": {"fp64_basket_without_whole_blocks"} if X == "f64" else set(),
             "cva": {"fp64_cva_without_round_up_after_last_pair"} if X == "f64" else set()}[family]
    assert set(seen) == want, (seen, want)
    print(f"xorwow power {family} {X}: {seen}, weakest share {weakest[0]:.3f} at {weakest[1]}")


# ---- the rules themselves -----------------------------------------------------------------------------------------------------
def test_padding_to_tiles_then_blocks_is_padding_to_blocks():
    """The basket kernel pads n to 4 ceil(n / 4) normals and then to whole blocks; nested ceilings: that IS ceil(n / NPB) blocks, for
    every n -- so "padding to blocks only" is no wrong assignment, and none of that name is listed."""
    for X in xr.PRECISIONS:
        assert all(xr.basket_blocks(n, X) == -(-n // xr.NPB[X]) for n in range(1, 257))
    assert [xr.basket_blocks(n, "f64") for n in (1, 4, 5, 8, 9, 64)] == [1, 1, 1, 1, 2, 8]
    assert [xr.cva_blocks(d, "f32") for d in (1, 4, 5, 65)] == [1, 1, 2, 17] and [xr.cva_blocks(d, "f64") for d in (1, 8, 9, 65)] == [1, 1, 2, 9]


def test_unit_words_by_hand():
    """Three lanes, eight units of two words: lane 1 prices units 1, 4, 7 from words 0-1, 2-3, 4-5 of its sequence."""
    words = np.arange(3 * 10).reshape(3, 10)
    w = xr.unit_words(words, 8, 2)
    assert w.tolist() == [[0, 1], [10, 11], [20, 21], [2, 3], [12, 13], [22, 23], [4, 5], [14, 15]]
    # unit 0 moves its lane on by one word only
    assert xr.unit_words(words, 8, 2, advance=[1] + [2] * 7)[[0, 3, 6]].tolist() == [[0, 1], [1, 2], [3, 4]]
    # the partial last trip (units 6, 7: lanes 0, 1) first
    assert xr.unit_words(words, 8, 2, order=[2, 0, 1]).tolist() == [[2, 3], [12, 13], [20, 21], [4, 5], [14, 15], [22, 23], [0, 1], [10, 11]]
    with pytest.raises(AssertionError):
        xr.unit_words(words[:, :5], 8, 2)


def test_vanilla_ranges_start_and_end_inside_a_unit():
    for X in xr.PRECISIONS:
        c = xr.vanilla_call(X, 1, 256, xr.NPB[X] * 10 + 3, 2 * xr.NPB[X])
        assert (c.n_units, c.head) == (3, 3)
        z = np.arange(3 * xr.NPB[X], dtype=np.float64).reshape(3, -1)
        assert xr.vanilla_z(z, c, 2 * xr.NPB[X]).tolist() == list(range(3, 3 + 2 * xr.NPB[X]))
        assert xr.unit_of_path(c, 2 * xr.NPB[X])[[0, xr.NPB[X] - 4, xr.NPB[X] - 3, -1]].tolist() == [0, 0, 1, 2]


@pytest.mark.parametrize("X", xr.PRECISIONS)
def test_the_cva_grids_price_the_listed_dates_with_every_ending(X):
    sch = xr.cva_schedules(X)
    assert sorted(sch) == xr.CVA_DATES and {e for _, _, e in sch.values()} == set(xr.ENDINGS)
    for d, (t, g, ending) in sch.items():
        s = xr.cr.schedule(xr.cva_market(X, d), X)
        assert (s.n_dates, s.ending) == (d, ending)
    assert xr.later_trips(xr.Call("cva", X, 1, 256, xr.UNITS[1], 5, 0)).sum() == xr.UNITS[1] - 256
    assert all(xr.UNITS[b] >= 2 * b * 256 for b in (1, 2)) and xr.UNITS[1] % 256 % 64 != 0
