"""The vanilla call at the generator's extremes, through the kernels' own payoff code (mc_vanilla_from_normals_*).

Two host constants assume how large a normal the device can draw: `zmax = 6.77` sizes the fp32 kernels' power-of-two rescale so that
the [0, 1] output clamp IS the payoff's max(., 0) (VanillaTraits<float>::prepare), and `Z_MAX_F64 = 8.58` stands behind every
exponent_in_range guard.  tests/test_gpu_math_edges.py pins the device's largest |z| (sqrt(2 * 33 ln 2) = 6.7637 and
sqrt(2 * 53 ln 2) = 8.5717); here normals of that size go through the masked kernel (per path) and through the hot kernels (sums of
whole units), on asymmetric markets, against the long-double payoff of tests/math_ref.py.  A clamp that saturates -- a rescale
sized for smaller normals -- shows as a deficit of the sums at the + extreme and nowhere else in the suite: the market `wide` is
chosen so that a rescale sized for |z| <= 6.7 would be one binary order short (guarded in tests/test_math_ref.py).

TOLERANCES: test_gpu_parity.py's TOL.  Per path TOL[X]["pay"] * s; in fp32 times 2^k, k the rescale exponent (the kernel computes
payoff / (s 2^k) in [0, 1] with fp32 roundings).  In fp64 the bound cannot stay below the resolution of the number it bounds: a path
with S_T > s is held to TOL["f64"]["pay"] * S_T (at the + extreme of `wide` S_T is 4e7 s and one ulp of it 6e-9 s).  Sums:
TOL[X]["rel"].  The reference prices the market as the kernel receives it: mc_option_f32 holds floats (math_ref.as_given), and at the
k = 99 boundary the rate is 67, whose float rounding alone is 4e-6 of every payoff.
"""
import math

import numpy as np
import pytest

import math_ref as mr
from test_gpu_parity import TOL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not mr.available(), reason="numpy longdouble has no 64-bit mantissa here")]

LD = mr.LD


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(mr.MARKETS))
def test_payoff_per_path_at_forced_extremes(eng, X, name):
    o = mr.MARKETS[name]
    z = mr.extreme_normals(o, X)
    assert len(z) % (4 if X == "f32" else 8)                           # a partial unit: the masked kernel
    e, vals = eng.vanilla_from_normals(o, z, X)
    want, st = mr.vanilla_payoff(o, z, X)
    if X == "f32":
        tol = TOL[X]["pay"] * o["s"] * 2.0 ** mr.f32_rescale_exponent(o, mr.host_zmax_f32())
    else:
        tol = LD(TOL[X]["pay"]) * np.maximum(LD(o["s"]), st)
    err = np.abs(vals.astype(LD) - want)
    print(f"vanilla_extremes {X} {name}: max err / tol {float((err / tol).max()):.3g}, largest payoff {float(want.max()):.6g}")
    assert np.all(np.isfinite(vals)) and np.all(err <= tol)
    assert e.n == len(z) and abs(LD(e.sum) - want.sum()) <= np.sum(tol * np.ones(len(z)))


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("pattern", ["plus", "alternating"])
@pytest.mark.parametrize("name", sorted(mr.MARKETS))
def test_hot_kernel_sums_at_the_extreme(eng, X, name, pattern):
    """1024 paths = whole units, no per-path output: the hot kernels."""
    o = mr.MARKETS[name]
    zx = mr.NP[X](mr.DEVICE_MAX[X])
    z = np.full(1024, zx, dtype=mr.NP[X])
    if pattern == "alternating":
        z[1::2] = -zx
    e, _ = eng.vanilla_from_normals(o, z, X, want_values=False)
    want, _ = mr.vanilla_payoff(o, z, X)
    s1, s2 = float(want.sum()), float((want * want).sum())
    print(f"vanilla_extremes {X} {name} {pattern}: sum {e.sum!r} vs {s1!r}, sum2 {e.sum2!r} vs {s2!r}")
    assert e.n == 1024
    assert abs(e.sum - s1) <= TOL[X]["rel"] * s1 and abs(e.sum2 - s2) <= 2 * TOL[X]["rel"] * s2


def _with_rate(target, v=0.2, t=1.0, bound=None):
    """the rate that puts the host's bound exactly at `target`: fp32 (r - v^2/2) t log2 e + v sqrt(t) log2 e zmax, fp64
    |(r - v^2/2) t| + v sqrt(t) Z_MAX_F64"""
    return (target - v * math.sqrt(t) * bound) / t + 0.5 * v * v


@pytest.mark.parametrize("inside_at,outside_at,k_inside", [(98.5, 99.5, 99), (-99.5, -100.5, -99)], ids=["k=99", "k=-99"])
def test_fp32_guard_accepts_k_99_and_refuses_k_100(mc, eng, inside_at, outside_at, k_inside):
    """|k| < 100: (drift + vol zmax) log2 e just below 99 (just above -100) is priced, just above 99 (below -100) refused."""
    zmax = mr.host_zmax_f32()
    inside = dict(s=100.0, k=100.0, v=0.2, t=1.0, r=_with_rate(inside_at / mr.LOG2E, bound=zmax))
    outside = dict(inside, r=_with_rate(outside_at / mr.LOG2E, bound=zmax))
    assert mr.f32_rescale_exponent(inside, zmax) == k_inside and abs(mr.f32_rescale_exponent(outside, zmax)) == 100
    z = np.resize(mr.extreme_normals(inside, "f32")[:6], 1024)     # the extremes and +-0; S_T = K lies far outside the generator's range here
    e, vals = eng.vanilla_from_normals(inside, z, "f32")
    assert np.all(np.isfinite(vals)) and all(math.isfinite(q) for q in (e.sum, e.sum2, e.expected, e.confidence))
    want, _ = mr.vanilla_payoff(inside, z, "f32")
    assert np.all(np.abs(vals.astype(LD) - want) <= TOL["f32"]["pay"] * inside["s"] * 2.0 ** k_inside)
    assert (want.max() > 1e30) == (k_inside > 0)
    with pytest.raises(mc.McError, match="mc error 1:"):
        eng.vanilla_from_normals(outside, z, "f32")
    with pytest.raises(mc.McError, match="mc error 1:"):
        eng.vanilla(outside, 4096, precision="f32")


def test_fp64_guard_accepts_an_exponent_below_700_and_refuses_one_above(mc, eng):
    z_max = mr.host_zmax_f64()
    inside = dict(s=1e-160, k=1e-160, v=0.2, t=1.0, r=_with_rate(699.9, bound=z_max))     # spot scaled so that the squares stay finite
    outside = dict(inside, r=_with_rate(700.1, bound=z_max))
    z = np.resize(mr.extreme_normals(inside, "f64")[:6], 1024)
    e, vals = eng.vanilla_from_normals(inside, z, "f64")
    want, st = mr.vanilla_payoff(inside, z, "f64")
    assert np.all(np.isfinite(vals)) and all(math.isfinite(q) for q in (e.sum, e.sum2)) and float(st.max()) > 1e143
    # the exponent is ~700: half an ulp of it, 5.7e-14, enters the payoff's relative error twice (the host's drift, the device's fma)
    assert np.all(np.abs(vals.astype(LD) - want) <= LD(2e-13) * st)
    with pytest.raises(mc.McError, match="mc error 1:"):
        eng.vanilla_from_normals(outside, z, "f64")
    with pytest.raises(mc.McError, match="mc error 1:"):
        eng.vanilla(outside, 4096, precision="f64")
