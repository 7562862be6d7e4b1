"""tests/math_ref.py checked without a GPU: against Python's libm at double precision, against identities at long-double
precision, against the project's host twin of the device arithmetic (tools/check_f64_tables.c, compiled as a library), and --
guards on tests/test_gpu_math_edges.py itself -- that the input lists hold the edges they claim.

The host twin runs the very lists the GPU tests run, at the GPU tests' bounds (4e-16 relative for -2 ln u, 2e-16 absolute for
sin / cos, 3e-16 relative for exp): the log / sincos / exp arithmetic is the same C99 fma sequence on both sides, so a list
entry that broke a bound would show here first."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import math_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not mr.available(), reason="numpy longdouble has no 64-bit mantissa here")
LD = mr.LD


def test_longdouble_is_extended():
    assert np.finfo(LD).nmant >= 63


# ---- against libm at double precision -----------------------------------------------------------------------------------------
def test_functions_agree_with_libm_at_double_precision():
    g = np.random.default_rng(11)
    J = g.integers(0, 1 << 52, size=2000, dtype=np.uint64)
    u = mr.u_of_J(J)
    assert [float(x) for x in mr.neg2log(u)] == pytest.approx([-2 * math.log(x) for x in u], rel=4e-16)
    s, c = mr.sincos_J(J)
    # libm sees fl(2 pi u): the argument carries up to 2 pi * 2^-53 relative, 7e-16 absolute at a full turn
    assert np.abs(s.astype(np.float64) - np.sin(2 * math.pi * u)).max() < 1.5e-15
    assert np.abs(c.astype(np.float64) - np.cos(2 * math.pi * u)).max() < 1.5e-15
    x = g.uniform(-700, 700, 2000)
    assert [float(v) for v in mr.exp(x)] == pytest.approx([math.exp(v) for v in x], rel=4e-16)
    p = 2.0 ** g.uniform(-80, 10, 2000)
    assert [float(v) for v in mr.sqrt(p)] == pytest.approx([math.sqrt(v) for v in p], rel=2.3e-16)
    assert [float(v) for v in mr.recip(p)] == pytest.approx([1 / v for v in p], rel=2.3e-16)


def test_identities_at_long_double_precision():
    g = np.random.default_rng(12)
    N = np.concatenate([g.integers(0, 1 << 53, size=4000, dtype=np.uint64), np.array(mr.quarter_turn_words(), dtype=np.uint64) >> np.uint64(11)])
    s, c = mr.sincos_N(N)
    assert np.abs(s * s + c * c - 1).max() < 1e-18
    x = g.uniform(-700, 700, 4000)
    assert np.abs(mr.exp(x) * mr.exp(-x) - 1).max() < 1e-18
    p = 2.0 ** g.uniform(-80, 10, 4000)
    assert np.abs(mr.sqrt(p) ** 2 / p.astype(LD) - 1).max() < 1e-18
    assert np.abs(mr.recip(p) * p.astype(LD) - 1).max() < 1e-18
    u = mr.u_of_J(g.integers(0, 1 << 52, size=4000, dtype=np.uint64))
    assert np.abs(np.exp(-mr.neg2log(u) / 2) / u.astype(LD) - 1).max() < 1e-17     # |ln u| <= 37 amplifies the log's rounding


def test_octant_reduction_is_exact_at_the_eighth_turns():
    s, c = mr.sincos_N(np.array([k << 50 for k in range(8)], dtype=np.uint64))
    h = np.sqrt(LD(0.5))
    want_s = np.array([0, h, 1, h, 0, -h, -1, -h], dtype=LD)
    want_c = np.array([1, h, 0, -h, -1, -h, 0, h], dtype=LD)
    assert np.abs(s - want_s).max() < 1e-19 and np.abs(c - want_c).max() < 1e-19
    # and it is continuous across every octant boundary: one step of 2^-53 revolutions moves sin and cos by at most 2 pi 2^-53
    for k in range(1, 8):
        a, b = mr.sincos_N(np.array([(k << 50) - 1, k << 50, (k << 50) + 1], dtype=np.uint64))
        assert np.abs(np.diff(a)).max() < 7.1e-16 and np.abs(np.diff(b)).max() < 7.1e-16


# ---- the bit constructions ----------------------------------------------------------------------------------------------------
def test_bit_constructions():
    assert mr.u_of_J([0])[0] == 2.0 ** -53 and mr.u_of_J([(1 << 52) - 1])[0] == 1 - 2.0 ** -53
    assert mr.J_of([0xfff, 0x1000, 0], [0, 0, 1]).tolist() == [0, 1, 1 << 20]
    g = np.random.default_rng(13)
    a, m, c = (mr.rand_words(g, 1000) for _ in range(3))
    jr, ja = mr.pair_J(a, m, c)
    # the header's wording: the radius is u01_f64(lo = m, hi = a), the angle takes (lo = m << 20, hi = c)
    assert np.array_equal(jr, mr.J_of(m, a)) and np.array_equal(ja, mr.J_of((m << np.uint64(20)) & np.uint64(0xffffffff), c))
    assert not np.any(ja & np.uint64(0xff)) and np.array_equal(ja >> np.uint64(8) & np.uint64(0xfff), m & np.uint64(0xfff))
    assert np.array_equal(jr & np.uint64(0xfffff), m >> np.uint64(12))
    # fp32: x = 2^32 - 1 rounds up to 1, x = 0 is the smallest uniform; 2^31 - 1 and 2^31 straddle a rounding of the sum
    assert mr.u01_f32([0, 0xffffffff, 0x7fffffff, 0x80000000, 0xffffff7f, 0xffffff80]).tolist() == [
        2.0 ** -33, 1.0, 0.5, 0.5, 1 - 2.0 ** -24, 1.0]
    assert mr.angle_f32_bits([0, 0x1ff, 0x200, 0xffffffff]).tolist() == [0x3f800000, 0x3f800000, 0x3f800001, 0x3fffffff]
    assert mr.angle_f32_N([1 << 30])[0] == 1 << 51 and mr.angle_f32_N([0x1ff])[0] == 0


# ---- the host twin on the GPU tests' own lists ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    so = tmp_path_factory.mktemp("twin") / "libtwin.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-DCHECK_F64_TABLES_LIB", "-shared", "-fPIC", "-o", str(so),
                    os.path.join(ROOT, "tools", "check_f64_tables.c"), "-lm"], check=True, capture_output=True)
    L = C.CDLL(str(so))
    L.twin_u01.restype = L.twin_neg2log.restype = L.twin_exp.restype = C.c_double
    L.twin_u01.argtypes = [C.c_uint32, C.c_uint32]
    L.twin_neg2log.argtypes = L.twin_exp.argtypes = [C.c_double]
    L.twin_sincos.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.twin_sincos.restype = None
    return L


def test_twin_uniform_is_the_integer_restatement(twin):
    lo, hi = mr.u01_inputs()
    got = np.array([twin.twin_u01(int(a), int(b)) for a, b in zip(lo, hi)])
    assert np.array_equal(got, mr.u_of_J(mr.J_of(lo, hi)))


def test_twin_log_meets_the_device_bound_on_the_edge_list(twin):
    u = mr.neg2log_inputs()
    mr.check_neg2log(u, np.array([twin.twin_neg2log(float(x)) for x in u]))


@pytest.mark.parametrize("v2", [False, True])
def test_twin_sincos_meets_the_device_bound_on_the_edge_list(twin, v2):
    lo, hi = mr.sincos_inputs(v2)
    s, c = C.c_double(), C.c_double()
    got = []
    for a, b in zip(lo, hi):
        twin.twin_sincos(int(a), int(b), C.byref(s), C.byref(c))
        got.append((s.value, c.value))
    got = np.array(got).astype(LD)
    rs, rc = mr.sincos_J(mr.J_of(lo, hi))
    assert max(np.abs(got[:, 0] - rs).max(), np.abs(got[:, 1] - rc).max()) <= 2e-16


def test_twin_exp_meets_the_device_bound_on_the_edge_list(twin):
    x = mr.exp_inputs()
    got = np.array([twin.twin_exp(float(v)) for v in x])
    ref = mr.exp(x)
    normal = (ref >= LD(2.0 ** -1022)) & (ref < LD(np.finfo(np.float64).max))
    rel = np.abs((got[normal].astype(LD) - ref[normal]) / ref[normal])
    assert rel.max() <= 3e-16, (float(rel.max()), float(x[normal][rel.argmax()]))
    tiny = ref < LD(2.0 ** -1022)
    assert not np.isnan(got).any()
    assert np.abs(got[tiny].astype(LD) - ref[tiny]).max() <= 2 * LD(2.0 ** -1074)
    assert np.all(np.isposinf(got[x > 709.79]))


# ---- guards: the lists hold what tests/test_gpu_math_edges.py says they hold --------------------------------------------------------
def test_log_list_reaches_every_slot_the_seam_and_both_ends():
    u = mr.neg2log_inputs()
    assert np.all(u > 0) and np.all(np.isfinite(u)) and np.all(u >= 2.0 ** -1022)
    b = mr.dbl_bits(u)
    k, slot = mr.log_slot(u)
    off = ((b >> np.uint64(32)).astype(np.int64) - mr.LOG_SEAM) & 0x1fff
    lo = (b & np.uint64(0xffffffff)).astype(np.int64)
    seen = {(int(kk), int(ss), int(o), int(l)) for kk, ss, o, l in zip(k, slot, off, lo)}
    for e in mr.LOG_EXPONENTS:
        for i in range(mr.LOG_SLOTS):
            assert {(e, i, 0, 0), (e, i, 0x1000, 0), (e, i, 0x1fff, 0xffffffff)} <= seen, (e, i)
    # both sides of the seam: the last mantissa below it belongs to the exponent below, slot 127
    hi = (b >> np.uint64(32)).astype(np.int64)
    assert {mr.LOG_SEAM - 1, mr.LOG_SEAM, mr.LOG_SEAM + 1} <= set(hi.tolist())
    assert (-1, 127, 0x1fff, 0xffffffff) in seen and (0, 0, 0, 0) in seen
    # the ends of the generator's range, and powers of two with their neighbours
    assert 2.0 ** -53 in u and 1 - 2.0 ** -53 in u and 1.0 in u
    for e in range(-52, 0):
        assert {2.0 ** e, 2.0 ** e * (1 + 2.0 ** -52), 2.0 ** e * (1 - 2.0 ** -52)} <= set(u.tolist())
    kk, ss = mr.log_slot(np.array([1.0, 1 - 2.0 ** -53]))
    assert kk.tolist() == [0, 0] and ss[0] == ss[1]                      # the slot that holds m = 1 is hit from both sides
    assert len(u) < 8192


@pytest.mark.parametrize("v2", [False, True])
def test_angle_list_reaches_every_slot_and_the_quarter_turns(v2):
    lo, hi = mr.sincos_inputs(v2)
    J = mr.J_of(lo, hi)
    slot = (J >> np.uint64(44)).astype(np.int64)
    low44 = (J & np.uint64((1 << 44) - 1)).astype(np.int64)
    seen = set(zip(slot.tolist(), low44.tolist()))
    last = (1 << 44) - 1 if not v2 else ((1 << 44) - 1) & ~0xff
    for i in range(mr.ANGLE_SLOTS):
        assert {(i, 0), (i, 1 << 43), (i, last)} <= seen, i
    Js = set(J.tolist())
    for q in range(4):
        step = 256 if v2 else 1
        assert (q << 50) in Js and ((q << 50) - step) % (1 << 52) in Js and ((q << 50) + (0 if v2 else 1)) in Js, q
    if v2:
        assert not np.any(lo & np.uint64(0xfffff)) and not np.any(J & np.uint64(0xff))
    assert len(lo) < 8192


def test_exp_list_holds_the_ties_and_the_range_ends():
    x = mr.exp_inputs()
    assert np.all(np.abs(x) < 5.0e6)                                    # EXP_F64_ARG_LIMIT: every input is inside the precondition
    scaled = x.astype(LD) * LD(256) / mr.LN2
    for j in mr.EXP_TIES:
        near = scaled[np.abs(scaled - (j + 0.5)) < 1e-9] - LD(j + 0.5)
        assert (near < 0).any() and (near > 0).any() and len(near) >= 5, j     # both sides of the tie, within 1e-9 of it
    ref = mr.exp(x)
    assert (ref == 0).any() or (ref < LD(2.0 ** -1074)).any()
    assert ((ref > 0) & (ref < LD(2.0 ** -1022))).sum() > 50            # subnormal results
    assert {0.0, 700.0, -700.0, 709.7, -708.3, -745.0, -800.0, -1e4, 4.99e6, -4.99e6, 1e-300, -1e-300} <= set(x.tolist())


def test_sqrt_and_recip_lists():
    x = mr.sqrt_inputs()
    assert np.all(x >= 2.0 ** -1022) and np.all(np.isfinite(x))
    assert {2.0 ** -52, 73.47, 1e-24, 1e-16, 1e3} <= set(x.tolist()) and {2.0 ** k for k in range(-80, 11)} <= set(x.tolist())
    squares = {float(n * n) for n in range(1, 65)}
    assert squares <= set(x.tolist()) and {float(np.nextafter(s, np.inf)) for s in squares} <= set(x.tolist())
    r = mr.recip_inputs()
    assert r.shape[1] == 4 and r.min() == 1.0 and r.max() == 3.0
    for col in range(4):
        assert {1.0, 3.0, 1 + 2.0 ** -52, float(np.nextafter(3.0, 0))} <= set(r[:, col].tolist())


def test_pair_lists_put_the_radius_at_its_ends_and_split_the_middle_word():
    ex = mr.pair_extreme_inputs()
    jr, ja = mr.pair_J(ex[:, 0], ex[:, 1], ex[:, 2])
    combos = set(zip(jr.tolist(), ja.tolist()))
    for end in (0, (1 << 52) - 1):
        for q in range(4):
            assert {(end, q << 50), (end, ((q << 50) + 256)), (end, ((q << 50) - 256) % (1 << 52))} <= combos, (end, q)
    base, top, low = mr.pair_split_inputs()
    jb, jt, jl = (mr.pair_J(w[:, 0], w[:, 1], w[:, 2]) for w in (base, top, low))
    assert np.array_equal(jb[1], jt[1]) and np.all(jb[0] != jt[0])      # top 20 bits of m: the radius alone
    assert np.array_equal(jb[0], jl[0]) and np.all(jb[1] != jl[1])      # low 12 bits of m: the angle alone
    assert np.all(np.abs(mr.u_of_J(jb[0]) - mr.u_of_J(jt[0])) >= 2.0 ** -34)   # and the radius moves by something a double shows


def test_f32_list_is_the_cross_product():
    w = mr.f32_block_inputs()
    grid = {(a, b) for a in mr.F32_XA for b in mr.F32_XB}
    assert grid <= set(zip(w[:, 0].tolist(), w[:, 1].tolist())) and grid <= set(zip(w[:, 2].tolist(), w[:, 3].tolist()))
    assert {0, 1 << 9, 0xffffffff, 1 << 30, (1 << 30) - 512, (1 << 30) + 512, 1 << 31, 3 << 30, 0xfffffe00} <= set(mr.F32_XB)
    assert len(mr.F32_XA) == 8


def test_vanilla_extreme_markets_are_what_their_tests_need():
    """Guard on tests/test_gpu_vanilla_extremes.py."""
    zmax = mr.host_zmax_f32()
    assert mr.ZMAX_F32 < mr.NEAR_MAX["f32"] + 0.01 <= zmax and mr.ZMAX_F64 < mr.NEAR_MAX["f64"] + 0.01 <= mr.host_zmax_f64()
    k = mr.f32_rescale_exponent(mr.WIDE, zmax)
    assert k >= 20
    # sized for 6.7 the rescale is one order short, and the device's largest normal then leaves [0, 1]
    drift, vol = mr.drift_vol(mr.WIDE)
    assert mr.f32_rescale_exponent(mr.WIDE, 6.7) == k - 1
    assert (drift + vol * mr.ZMAX_F32) * mr.LOG2E - (k - 1) > 0.1 > mr.WIDE["k"] / mr.WIDE["s"] * 2.0 ** -(k - 1)
    assert (drift + vol * mr.ZMAX_F32) * mr.LOG2E - k < 0
    assert {o["k"] for o in mr.MARKETS.values()} >= {0.0, -20.0} and mr.MARKETS["deep_otm"]["k"] > 1.5 * mr.MARKETS["deep_otm"]["s"]
