"""The blocked fp32 vanilla kernel on a real MI355X (csrc/mc_kernels.hpp: vanilla_f32_blocked_kernel).

From one full sweep of the grid on, a lane of the hot kernel takes whole 8-aligned blocks of 8 units where the segment has them
and single units elsewhere (csrc/mc_launch_shape.hpp: vanilla_blocking); the eight units of a block share the front of Philox
(csrc/mc_rng.hpp: PhiloxBlock8).  Smaller calls run the unit-strided kernel as before.  Every path's payoff
must be what it was -- the same words, the same arithmetic -- and only the grouping of the fp32 partial sums may differ.

Reference: the per-path route (vanilla_paths: the masked kernel, one unit per lane and trip through philox_unit, which the blocked
form does not touch), its payoffs added up in float64 on the host.  The hot kernel's {sum, sum2, n} against that, plain and
antithetic, over ranges chosen to hit every branch of the split.

BOUNDS.  `n` is exact.  For the sums both sides hold the same payoffs; they differ in
  * the hot kernel's fp32 partials: 16 scaled payoffs (each >= 0) are added in fp32 before each flush to fp64, at most 16
    roundings of 2^-24 relative to the partial: |error| <= 16 * 2^-24 of the partial, zero-mean;
  * the dump's scaling: the per-path route stores payoff * (S 2^k) rounded to fp32: 2^-24 relative per path (the squares: twice).
  >= 1e6 paths: relative 2e-9, the summation-order bound of test_gpu_parity.py::test_vanilla_shards_add_up_and_geometry_does_not_matter
    (independent zero-mean errors over >= 6e4 partials);
  <  1e6 paths: no averaging is assumed: the worst case of the above, 17 * 2^-24 relative for the sum and 19 * 2^-24 for the
    sum of squares (every term is >= 0, so the errors of the parts are bounded by the same fraction of the whole), and never more
    than the per-path absolute bound of test_gpu_parity.py's TOL (2e-6 * spot per path) times the number of paths.
"""
import numpy as np
import pytest

from test_gpu_parity import SEED, TOL, VAN

pytestmark = pytest.mark.gpu

GROUP = 256
DEFAULT_BLOCKS = 2048


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def engines(mc):
    """grids of 4, 7, 16, 311 and the default 2048 workgroups"""
    engs = {b: mc.Engine(0, blocks=b) for b in (4, 7, 16, 311)}
    engs[DEFAULT_BLOCKS] = mc.Engine(0)
    yield engs
    for e in engs.values():
        e.close()


def case_list():
    """(name, blocks, first path, paths).  The stride of a grid of b workgroups is S = 256 b units once the call has that many
    units; a sweep of blocks is 8 S units = 32 S paths."""
    S16, S4, S7, S311, SD = 16 * GROUP, 4 * GROUP, 7 * GROUP, 311 * GROUP, DEFAULT_BLOCKS * GROUP
    cases = []
    # a segment start at every residue mod 8 units, the first path inside a unit (an edge launch in front), two sweeps and a bit
    for r in range(8):
        cases.append((f"start_residue_{r}", 16, 4 * (8 * 1000 + r) + 1, 4 * (2 * 8 * S16 + 37) + 2))
    cases += [
        ("three_units", 16, 4 * 5, 4 * 3),                                     # fewer than 8 units in total
        ("seven_units_over_a_block_boundary", 16, 4 * 12 + 2, 4 * 7 + 1),
        ("less_than_a_unit", 16, 9, 2),
        ("one_block_per_lane", 16, 0, 32 * S16),                               # exactly one block per lane
        ("one_block_per_lane_default_grid", DEFAULT_BLOCKS, 0, 32 * SD),
        ("one_sweep_minus_one_unit", 16, 0, 32 * S16 - 4),                     # one sweep +- 1 unit
        ("one_sweep_plus_one_unit", 16, 0, 32 * S16 + 4),
        ("one_sweep_plus_one_unit_default_grid", DEFAULT_BLOCKS, 0, 32 * SD + 4),
        ("one_sweep_minus_one_unit_default_grid", DEFAULT_BLOCKS, 4 * 8, 32 * SD - 4),
        ("partial_sweep", 16, 4 * 3, 4 * (8 * S16 + 7 * S16 + S16 // 2 + 100) + 3),   # more than 7.5 strides after the last full sweep
        ("partial_sweep_default_grid", DEFAULT_BLOCKS, 0, 4 * (8 * SD + 7 * SD + 3 * SD // 4)),
        ("seven_strides_left", 16, 0, 4 * (8 * S16 + 7 * S16)),                # exactly 7: unit-strided
        ("almost_a_sweep", 16, 0, 4 * (8 * S16 - 9)),                          # below one full sweep: the unit-strided kernel
        ("across_2_32_units", 4, 4 * ((1 << 32) - 50_000) - 3, 4 * 100_000 + 5),   # two segments, the first ends at 2^32 units
        ("across_2_32_units_odd_start", 7, 4 * ((1 << 32) - 8 * S7 * 2 - 3), 4 * (8 * S7 * 5 + 11)),
        ("high_word_set", 4, 4 * ((5 << 32) + 8 * 77 + 5) + 1, 4 * (8 * S4 * 3 + 9)),
        ("blocks_311", 311, 7, 4 * (3 * 8 * S311 + 12345) + 1),                # odd grids
        ("blocks_311_partial_sweep", 311, 4 * 6, 4 * (8 * S311 + 7 * S311 + 3 * S311 // 4)),
        ("blocks_7", 7, 4 * 2 + 3, 4 * (4 * 8 * S7 + 7 * S7 + 5) + 2),
        ("blocks_7_small", 7, 0, 4 * (S7 * 3 + 1)),
    ]
    return cases


CASES = case_list()


def test_cases_reach_every_branch_of_the_split():
    """Guard on the test itself (no GPU work): the list holds blocked calls with a head, with a partial sweep, without one, and
    unblocked ones; the rule is csrc/mc_launch_shape.hpp: vanilla_blocking (restated here for whole-unit ranges)."""
    seen = set()
    for name, blocks, first, n in CASES:
        u0, u1 = -(-first // 4), (first + n) // 4
        units = max(u1 - u0, 0)
        grid = min(blocks, max(-(-units // GROUP), 1))
        stride = grid * GROUP
        lo, segs = u0, []
        while lo < u1:
            hi = min(u1, ((lo >> 32) + 1) << 32)
            segs.append((lo & 0xFFFFFFFF, hi - lo))
            lo = hi
        for lo32, cnt in segs:
            if blocks == DEFAULT_BLOCKS and cnt < 2_100_000:
                continue   # the default grid shrinks for small calls (grid_for_vanilla); those cases are not counted here
            head = min((-lo32) % 8, cnt)
            nb = (cnt - head) // 8
            sweeps, left = nb // stride, (cnt - head) - 8 * (nb // stride) * stride
            extra = nb - sweeps * stride if 2 * left > 15 * stride else 0
            if sweeps < 1:
                sweeps = extra = 0
            seen.add(("blocked" if sweeps or extra else "unit-strided", "head" if head and (sweeps or extra) else "", "extra" if extra else "",
                      "rest" if (sweeps or extra) and cnt - 8 * (sweeps * stride + extra) - head > 0 else ""))
    assert {("blocked", "head", "", "rest"), ("blocked", "", "extra", ""), ("blocked", "head", "extra", "rest"), ("blocked", "", "", ""),
            ("unit-strided", "", "", "")} <= seen, seen
    assert {(-(-first // 4)) % 8 for name, _, first, _ in CASES if name.startswith("start_residue")} == set(range(8))


@pytest.mark.parametrize("anti", [False, True], ids=["plain", "antithetic"])
@pytest.mark.parametrize("name,blocks,first,n", CASES, ids=[c[0] for c in CASES])
def test_hot_kernel_sums_equal_the_per_path_route(engines, name, blocks, first, n, anti):
    eng = engines[blocks]
    eng.set_antithetic(anti)
    try:
        e = eng.vanilla(VAN, n, SEED, first, "f32")
        again = eng.vanilla(VAN, n, SEED, first, "f32")
        pay = eng.vanilla_paths(VAN, n, SEED, first, "f32").astype(np.float64)
    finally:
        eng.set_antithetic(False)
    want_s, want_q = float(pay.sum()), float((pay * pay).sum())
    ds, dq = abs(e.sum - want_s), abs(e.sum2 - want_q)
    print(f"{name} anti={anti}: n={n} sum {e.sum!r} vs {want_s!r} rel {ds / max(want_s, 1e-300):.3g}; "
          f"sum2 {e.sum2!r} vs {want_q!r} rel {dq / max(want_q, 1e-300):.3g}")
    assert e.n == n == pay.size
    assert (again.sum, again.sum2, again.n) == (e.sum, e.sum2, e.n)   # run-to-run bitwise, fixed grid
    if n >= 1_000_000:
        assert ds <= 2e-9 * want_s and dq <= 2e-9 * want_q
    else:
        per_path = TOL["f32"]["pay"] * VAN["s"]
        assert ds <= min(17 * 2.0 ** -24 * want_s, n * per_path)
        assert dq <= min(19 * 2.0 ** -24 * want_q, n * 2 * per_path * float(pay.max(initial=0.0)) + n * per_path ** 2)


def test_blocked_payoffs_are_the_oracles(engines, po):
    """the same blocked call against the oracle's sequential fp64 sums over the same counters (the stated sum tolerance of
    test_gpu_parity.py): the shared front of Philox yields the stream the oracle pins"""
    first, n = 4 * 11 + 1, 4 * (2 * 8 * 16 * GROUP + 21) + 2
    for anti in (False, True):
        eng = engines[16]
        eng.set_antithetic(anti)
        try:
            e = eng.vanilla(VAN, n, SEED, first, "f32")
        finally:
            eng.set_antithetic(False)
        _, o = po.dev_vanilla("f32", VAN, SEED, first, n, want_paths=False, antithetic=anti)
        assert e.n == n == o["n"]
        assert e.sum == pytest.approx(o["sum"], rel=TOL["f32"]["rel"]) and e.sum2 == pytest.approx(o["sum2"], rel=TOL["f32"]["rel"])
