"""The device's fp64 elementary functions and its words-to-normals plumbing at the edges of their domains.

Every fp64 kernel runs through csrc/mc_math_f64.hpp (exp_f64, neg2log_unit_tab, sincos_turns_tab, sqrt_pos, recip*_pos, the
register-constant F64K twins) and csrc/mc_rng.hpp (u01_f64, pair_normals_f64, box_muller_f32).  The generator hooks take
counters, so no search over counters reaches the smallest and largest radius uniform, a slot boundary of the log and angle
tables, the sqrt(1/2) seam, an exact quarter turn or a tie of the exponential's rounding.  The test hook mc_math_probe
(Engine.math_probe) evaluates the SHIPPING inline functions on chosen inputs -- 256-lane workgroups, LDS tables staged as
the kernels stage them, item i on lane i mod 256 -- and this file compares them with tests/math_ref.py: numpy long double
(64-bit mantissa) and integer restatements of the bit constructions.  The input lists live in math_ref.py;
tests/test_math_ref.py checks without a GPU that they hold every slot, seam and end they claim, and runs the host twin
(tools/check_f64_tables.c) over the same lists at the same bounds.

BOUNDS.  Bit-equal: the uniforms and the fp32 angle against the integer restatement; the F64K forms against the plain ones
(the header's claim).  Against the long-double reference, the bounds the project asserts for the host twin: -2 ln u 4e-16
relative on u <= 1 (math_ref.check_neg2log says what holds above 1, where no generator goes), sin / cos 2e-16 absolute, exp 3e-16
relative where the result is a normal double, the fp64 normal 4e-15 absolute.  sqrt_pos and recip_pos: the header's 2 ulp.
recip2_pos 2.5 ulp, recip4_pos 4 ulp (the roundings they add to recip_pos).  An exponential whose result is subnormal or zero: never
NaN, non-increasing as x falls, within 2 units of 2^-1074 (the product rounds, then v_ldexp_f64 rounds).  Above 709.78: +inf.

fp32 NORMALS.  The hardware's v_log / v_sqrt / v_sin / v_cos have no accuracy statement this project has measured against, so the
bound on |z - reference| is twice the maximum observed on this input list (the functions are deterministic: the factor covers a
compiler or library change, not noise): observed 4.787e-07 on MI355X (F32_Z_ERR_OBSERVED below, profiles/math_edges.log).

Every test prints its observed maxima (`math_edges ...` lines); profiles/math_edges.log is that output.
"""
import numpy as np
import pytest

import math_ref as mr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not mr.available(), reason="numpy longdouble has no 64-bit mantissa here")]

LD = mr.LD
U64 = np.uint64
F32_Z_ERR_OBSERVED = 4.787e-07     # max |z_device - z_reference| over f32_block_inputs() on MI355X (profiles/math_edges.log)


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


def note(name, value):
    print(f"math_edges {name} {float(value):.3e}")


def dbl(col):
    return np.ascontiguousarray(col, dtype=U64).view(np.float64)


def flt(col):
    return np.ascontiguousarray(col, dtype=U64).astype(np.uint32).view(np.float32)


def in_ulps(got, ref):
    return np.abs(got.astype(LD) - ref) / mr.ulp(ref)


def test_uniform_is_the_integer_restatement(eng):
    lo, hi = mr.u01_inputs()
    out = eng.math_probe("u01", np.stack([lo, hi], axis=1))
    assert np.array_equal(out[:, 0], mr.dbl_bits(mr.u_of_J(mr.J_of(lo, hi))))


def test_log_at_every_slot_the_seam_and_both_ends(eng):
    u = mr.neg2log_inputs()
    out = eng.math_probe("neg2log", mr.dbl_bits(u))
    assert np.array_equal(out[:, 0], out[:, 1])                        # F64K form: the same bits
    worst = mr.check_neg2log(u, dbl(out[:, 0]))
    note("neg2log_rel_u_le_1", worst["inside"])
    note("neg2log_rel_u_gt_1", worst["above_rel"])


@pytest.mark.parametrize("v2", [False, True], ids=["52-bit", "stream-v2-44-bit"])
def test_sincos_at_every_slot_and_quarter_turn(eng, v2):
    lo, hi = mr.sincos_inputs(v2)
    out = eng.math_probe("sincos", np.stack([lo, hi], axis=1))
    assert np.array_equal(out[:, 0:2], out[:, 2:4])                    # F64K form: the same bits
    rs, rc = mr.sincos_J(mr.J_of(lo, hi))
    es, ec = np.abs(dbl(out[:, 0]).astype(LD) - rs).max(), np.abs(dbl(out[:, 1]).astype(LD) - rc).max()
    note(f"sincos_abs_v2={int(v2)}", max(es, ec))
    assert max(es, ec) <= 2e-16


def test_exp_at_its_ties_and_range_ends(eng):
    x = mr.exp_inputs()
    got = dbl(eng.math_probe("exp", mr.dbl_bits(x))[:, 0])
    ref = mr.exp(x)
    assert not np.isnan(got).any()
    normal = (ref >= LD(2.0 ** -1022)) & (ref <= LD(np.finfo(np.float64).max))
    rel = np.abs((got[normal].astype(LD) - ref[normal]) / ref[normal])
    note("exp_rel_normal", rel.max())
    assert rel.max() <= 3e-16, float(x[normal][rel.argmax()])
    tiny = ref < LD(2.0 ** -1022)
    assert tiny.sum() > 50
    units = np.abs(got[tiny].astype(LD) - ref[tiny]) / LD(2.0 ** -1074)
    note("exp_subnormal_units", units.max())
    assert units.max() <= 2
    order = np.argsort(x[tiny])
    assert np.all(np.diff(got[tiny][order]) >= 0)                      # non-increasing as x falls
    assert np.all(got[x <= -800.0] == 0)
    over = x > 709.78
    assert over.any() and np.all(np.isposinf(got[over]))


def test_sqrt_on_the_callers_radicands(eng):
    x = mr.sqrt_inputs()
    got = dbl(eng.math_probe("sqrt", mr.dbl_bits(x))[:, 0])
    e = in_ulps(got, mr.sqrt(x))
    note("sqrt_ulp", e.max())
    assert np.all(np.isfinite(got)) and e.max() <= 2, float(x[e.argmax()])


def test_reciprocals_on_the_hastings_range(eng):
    """recip_pos: 2 ulp (header).  recip2_pos(a, b) = recip_pos(fl(a b)) b and recip4_pos (products of the pairs, their product,
    two more products per result) add roundings of half an ulp each on top of it: asserted 2.5 and 4 ulp; observed on MI355X
    0.5 (recip_pos: correctly rounded on this list), 1.8 and 2.8."""
    d = mr.recip_inputs()
    out = eng.math_probe("recip", mr.dbl_bits(d.reshape(-1)).reshape(-1, 4))
    ref = mr.recip(d)
    one = in_ulps(dbl(out[:, 0]), ref[:, 0])
    two = np.maximum(in_ulps(dbl(out[:, 1]), ref[:, 0]), in_ulps(dbl(out[:, 2]), ref[:, 1]))
    four = np.max([in_ulps(dbl(out[:, 3 + j]), ref[:, j]) for j in range(4)], axis=0)
    note("recip_ulp", one.max())
    note("recip2_ulp", two.max())
    note("recip4_ulp", four.max())
    assert one.max() <= 2 and two.max() <= 2.5 and four.max() <= 4


def test_pair_normals_at_the_radius_ends_and_the_split_of_the_middle_word(eng):
    z_max_host = mr.host_zmax_f64()
    ex = mr.pair_extreme_inputs()
    base, top, low = mr.pair_split_inputs()
    words = np.concatenate([ex, base, top, low, mr.pair_random_inputs()])
    out = eng.math_probe("pair", words)
    assert np.array_equal(out[:, 0:2], out[:, 2:4])                    # F64K form: the same bits
    zc, zs = dbl(out[:, 0]), dbl(out[:, 1])
    assert np.all(np.isfinite(zc)) and np.all(np.isfinite(zs))
    jr, ja = mr.pair_J(words[:, 0], words[:, 1], words[:, 2])
    rc, rs = mr.normals_J(jr, ja)
    err = max(np.abs(zc.astype(LD) - rc).max(), np.abs(zs.astype(LD) - rs).max())
    biggest = max(np.abs(zc).max(), np.abs(zs).max())
    note("normal_f64_abs", err)
    note("normal_f64_largest", biggest)
    assert err <= 4e-15
    assert biggest <= z_max_host
    # J = 0: the largest normal the stream can hold, on the axes of the four quarter turns
    at_zero = jr[:len(ex)] == 0
    assert at_zero.sum() == 12
    r0 = np.maximum(np.abs(zc[:len(ex)]), np.abs(zs[:len(ex)]))[at_zero]
    assert np.abs(r0 - mr.ZMAX_F64).max() <= 4e-15 and mr.ZMAX_F64 < z_max_host
    # the top 20 bits of m move the radius alone, its low 12 bits the angle alone
    n, o = len(base), len(ex)
    b, t, l = (slice(o + i * n, o + (i + 1) * n) for i in range(3))
    rad = np.hypot(zc, zs)
    cross = zc[b] * zs[t] - zs[b] * zc[t]
    # (each of the four components is within 4e-15 of a pair of parallel vectors; the products round at 1.1e-16 each)
    assert np.all(np.abs(cross) <= 4e-15 * 2 * (rad[b] + rad[t]) + 4e-16 * rad[b] * rad[t])
    assert np.all(np.abs(rad[b] - rad[t]) > 1e-11)
    assert np.all(np.abs(rad[b] - rad[l]) <= 1e-14)
    assert np.all((out[b, 0] != out[l, 0]) | (out[b, 1] != out[l, 1]))


def test_fp32_block_at_the_ends_of_both_uniforms(eng):
    zmax_host = mr.host_zmax_f32()
    w = mr.f32_block_inputs()
    out = eng.math_probe("f32_block", w)
    for col, word in ((4, 0), (6, 2)):
        assert np.array_equal(out[:, col].astype(np.uint32), mr.u01_f32(w[:, word]).view(np.uint32))
    for col, word in ((5, 1), (7, 3)):
        assert np.array_equal(out[:, col], mr.angle_f32_bits(w[:, word]))
    z = np.stack([flt(out[:, j]) for j in range(4)], axis=1).astype(np.float64)
    assert np.all(np.isfinite(z))                                      # x = 2^32 - 1: u rounds to 1, the radius is sqrt(-0)
    ref = np.stack(mr.normals_f32(w[:, 0], w[:, 1]) + mr.normals_f32(w[:, 2], w[:, 3]), axis=1)
    err = np.abs(z.astype(LD) - ref).max()
    biggest = np.abs(z).max()
    note("normal_f32_abs", err)
    note("normal_f32_largest", biggest)
    assert biggest < zmax_host and mr.ZMAX_F32 < zmax_host
    first = (w[:, 0] == 0) & (w[:, 1] == 0)
    assert first.any() and np.abs(np.abs(z[first, 0]) - mr.ZMAX_F32).max() <= 2 * F32_Z_ERR_OBSERVED   # x = 0, angle 0: the largest
    assert err <= 2 * F32_Z_ERR_OBSERVED


def test_probe_refuses_what_it_cannot_hold(mc, eng):
    with pytest.raises(mc.McError, match="mc error 1:"):
        eng.math_probe("exp", np.zeros((mc._lib.PROBE_MAX + 1, 1), dtype=U64))
    mc._lib.PROBE_OPS["nonsense"] = len(mc._lib.PROBE_OPS)
    try:
        with pytest.raises(mc.McError, match="mc error 1:"):
            eng.math_probe("nonsense", np.zeros((4, 1), dtype=U64))
    finally:
        del mc._lib.PROBE_OPS["nonsense"]
    full = eng.math_probe("sqrt", np.full((mc._lib.PROBE_MAX, 1), mr.dbl_bits(np.array([4.0]))[0], dtype=U64))
    assert np.all(dbl(full[:, 0]) == 2.0)
