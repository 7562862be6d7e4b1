"""Plain high-precision reference of the device's fp64 elementary functions and Box-Muller plumbing (not a test module).

What csrc/mc_math_f64.hpp and csrc/mc_rng.hpp compute, restated from the definitions -- never from the device code:
  * the functions in numpy `longdouble` (x87 extended: 64-bit mantissa, unit roundoff 5.4e-20; `available()` says whether this
    platform has it): -2 ln u, sin / cos of 2 pi u, exp, sqrt, 1/x;
  * the bit constructions with integers: u = (J + 1/2) 2^-52 with J = hi:lo >> 12; stream version 2's pair (radius from
    (a : top 20 bits of m), angle from (c : low 12 bits of m) with eight zero bits below); fp32: u = fmaf((float) x, 2^-32, 2^-33),
    angle (x >> 9) 2^-23 revolutions;
  * the input lists of tests/test_gpu_math_edges.py as functions, so that tests/test_math_ref.py can check without a GPU that
    they hold what they claim.

ANGLES.  Every angle here is a binary fraction N 2^-53 of a revolution with an integer 0 <= N < 2^53.  Its octant is N >> 50 and
the offset inside the octant N mod 2^50 -- integer operations, exact -- so sinl / cosl only ever see 2 pi f 2^-53 <= pi / 4, where the
rounding of 2 pi itself (relative 2^-64) moves the result by less than 1e-19.
"""
import math
import os
import re

import numpy as np

LD = np.longdouble
U64 = np.uint64
TWO_PI = LD("6.283185307179586476925286766559005768394")
LN2 = LD("0.693147180559945309417232121458176568076")

# the generators' extremes: u >= 2^-53 (fp64: J = 0) and u >= 2^-33 (fp32: x = 0)
ZMAX_F64 = math.sqrt(2 * 53 * math.log(2))     # 8.5717...
ZMAX_F32 = math.sqrt(2 * 33 * math.log(2))     # 6.7637...

LOG_SEAM = 0x3fe6a09e      # high word of sqrt(1/2): where neg2log_unit_tab splits exponent and mantissa
LOG_SLOTS, ANGLE_SLOTS = 128, 256
LOG_EXPONENTS = (0, -1, -2, -26, -51)


def host_constant(pattern):
    """a constant of csrc/mc_api.hip, read from the source (every occurrence must agree)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = set(re.findall(pattern, open(os.path.join(root, "montecarlocuda_amd", "csrc", "mc_api.hip")).read()))
    assert len(found) == 1, (pattern, found)
    return float(found.pop())


def host_zmax_f32():
    return host_constant(r"const double zmax = ([0-9.]+);")


def host_zmax_f64():
    return host_constant(r"constexpr double Z_MAX_F64 = ([0-9.]+);")


def available():
    return np.finfo(LD).nmant >= 63


def u64(a):
    return np.asarray(a, dtype=U64)


# ---- bits ------------------------------------------------------------------------------------------------------------
def dbl_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(U64)


def bits_dbl(b):
    return np.ascontiguousarray(b, dtype=U64).view(np.float64)


def hilo(hi, lo):
    """the double with the given high and low words"""
    return bits_dbl((u64(hi) << U64(32)) | u64(lo))


def J_of(lo, hi):
    """J = hi:lo >> 12, the 52-bit integer of u01_f64(lo, hi)"""
    return ((u64(hi) << U64(32)) | u64(lo)) >> U64(12)


def u_of_J(J):
    """u = (J + 1/2) 2^-52 = (2 J + 1) 2^-53: an odd integer below 2^53 times a power of two, exact in a double"""
    return (u64(J) * U64(2) + U64(1)).astype(np.float64) * 2.0 ** -53


def pair_J(a, m, c):
    """Stream version 2: (J of the radius uniform, J of the angle uniform) of the words (a, m, c)."""
    a, m, c = u64(a), u64(m), u64(c)
    radius = (a << U64(20)) | (m >> U64(12))
    angle = ((c << U64(12)) | (m & U64(0xfff))) << U64(8)
    return radius, angle


def u01_f32(x):
    """fmaf((float) x, 2^-32, 2^-33), the definition include/mc_mi355x.h gives: the conversion of the word rounds to 24 bits
    (nearest even), then the fma rounds once -- fl(x) 2^-32 + 2^-33 is exact in a double, the cast is that rounding"""
    xf = np.asarray(u64(x), dtype=np.uint32).astype(np.float32)
    return (xf.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def angle_f32_bits(x):
    """angle_f32 returns 1 + (x >> 9) 2^-23 as a float in [1, 2): its bit pattern"""
    return (u64(x) >> U64(9)) | U64(0x3f800000)


def angle_f32_N(x):
    """the fp32 angle (x >> 9) 2^-23 revolutions as N 2^-53"""
    return (u64(x) >> U64(9)) << U64(30)


# ---- functions in long double ----------------------------------------------------------------------------------------------
def neg2log(u):
    return LD(-2) * np.log(np.asarray(u, dtype=np.float64).astype(LD))


def sincos_N(N):
    """(sin, cos) of 2 pi N 2^-53, integer N in [0, 2^53)"""
    N = u64(N)
    assert np.all(N < U64(1 << 53))
    q = (N >> U64(50)).astype(np.int64)
    f = N & U64((1 << 50) - 1)
    odd = (q & 1) == 1
    f = np.where(odd, U64(1 << 50) - f, f)            # odd octants measure the angle back from their upper end
    th = TWO_PI * (f.astype(LD) * LD(2.0 ** -53))     # <= pi / 4; f < 2^51 is exact in a long double
    s, c = np.sin(th), np.cos(th)
    #            q:   0   1   2   3   4   5   6   7
    sin = np.choose(q, [s, c, c, s, -s, -c, -c, -s])
    cos = np.choose(q, [c, s, -s, -c, -c, -s, s, c])
    return sin, cos


def sincos_J(J):
    """(sin, cos) of 2 pi u, u = (J + 1/2) 2^-52"""
    return sincos_N(u64(J) * U64(2) + U64(1))


def exp(x):
    with np.errstate(over="ignore", under="ignore"):      # |x| up to 5e6 is in the lists: inf and 0 are the right answers there
        return np.exp(np.asarray(x, dtype=np.float64).astype(LD))


def sqrt(x):
    return np.sqrt(np.asarray(x, dtype=np.float64).astype(LD))


def recip(x):
    return LD(1) / np.asarray(x, dtype=np.float64).astype(LD)


def normals_J(Jr, Ja):
    """Box-Muller (z_cos, z_sin) of the radius uniform J = Jr and the angle uniform J = Ja"""
    r = np.sqrt(neg2log(u_of_J(Jr)))
    s, c = sincos_J(Ja)
    return r * c, r * s


def normals_f32(xa, xb):
    """Box-Muller (z_cos, z_sin) on the fp32 path's own uniforms: radius from u01_f32(xa), angle (xb >> 9) 2^-23 revolutions"""
    r = np.sqrt(neg2log(u01_f32(xa).astype(np.float64)))
    s, c = sincos_N(angle_f32_N(xb))
    return r * c, r * s


def ulp(ref):
    """the spacing of doubles at a long-double value"""
    return np.spacing(np.abs(np.asarray(ref, dtype=LD)).astype(np.float64)).astype(LD)


def log_slot(u):
    """(exponent k, slot) that neg2log_unit_tab's reduction assigns to the double u -- from the definition: u = 2^k m with
    m in [sqrt(1/2), sqrt 2) cut at the high word of sqrt(1/2), slot = the top 7 bits of the 20-bit offset from the cut"""
    h = (dbl_bits(u) >> U64(32)).astype(np.int64) - LOG_SEAM
    return h >> 20, (h >> 13) & 0x7f


def check_neg2log(u, got):
    """The bound on -2 ln u that the GPU test and the host twin's test share; returns the observed maxima.

    u <= 1 + 2^-13 -- the generator's range (0, 1) and the whole slot that holds m = 1 (c = 1, t = 0): 4e-16 RELATIVE, the host
    twin's bound.  u = 1 exactly: 0.
    Above that slot (exponent 0, slots 75 ... 127: arguments no generator produces, in the list because every slot is) the
    result is t_i + S with t_i != 0 and the two cancel towards u -> 1: at u = 1.00015, the first mantissa of slot 75,
    t = -0.0081 and S = +0.0078 leave -3.0e-4 with the half ulp of t in it, 2.3e-15 relative on the host twin and on the
    device alike.  No relative bound exists there by construction of the table; what the arithmetic gives is
        |error| <= 2^-53 (|t_i| + |S| + |t_i + S|) + the series' 1e-17 |S|,  |S| <= 2^-7 (1 + 2^-7),  |t_i| <= |ref| + |S|
                <= 4e-16 |ref| + 2^-58,
    and that is asserted for them."""
    u = np.asarray(u, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).astype(LD)
    ref = neg2log(u)
    err = np.abs(got - ref)
    assert np.all(np.isfinite(got))
    assert np.all(got[u == 1.0] == 0)
    inside = (u <= 1 + 2.0 ** -13) & (u != 1.0)
    above = u > 1 + 2.0 ** -13
    rel = err[inside] / np.abs(ref[inside])
    assert rel.max() <= 4e-16, (float(rel.max()), float(u[inside][rel.argmax()]))
    assert np.all(err[above] <= LD(4e-16) * np.abs(ref[above]) + LD(2.0 ** -58)), float((err[above] / np.abs(ref[above])).max())
    return {"inside": float(rel.max()), "above_rel": float((err[above] / np.abs(ref[above])).max()) if above.any() else 0.0}


# ---- input lists -------------------------------------------------------------------------------------------------------
RANDOM = 4096


def rng(tag):
    return np.random.default_rng([20261020, tag])


def rand_words(g, n):
    return g.integers(0, 1 << 32, size=n, dtype=np.uint64)


def neg2log_inputs():
    """doubles u"""
    one, top = 1, (1 << 52) - 1
    parts = [u_of_J([0, 1, 2, top - 1, top])]
    k = np.arange(-1, -53, -1).astype(np.float64)
    parts += [2.0 ** k, 2.0 ** k * (1 + 2.0 ** -52), 2.0 ** k * (1 - 2.0 ** -52)]
    hi, lo = [], []
    for e in LOG_EXPONENTS:
        for i in range(LOG_SLOTS):
            base = LOG_SEAM + (e << 20) + (i << 13)
            hi += [base, base + 0x1000, base + 0x1fff]       # first, centre, last mantissa of the slot
            lo += [0, 0, 0xffffffff]
    for h in (LOG_SEAM - 1, LOG_SEAM, LOG_SEAM + 1):          # the seam of the reduction, both sides
        hi += [h, h]
        lo += [0, 0xffffffff]
    parts.append(hilo(hi, lo))
    parts.append(np.array([1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, 1.0 + 2.0 ** -51]))   # the slot that holds m = 1
    g = rng(1)
    parts.append(u_of_J(J_of(rand_words(g, RANDOM), rand_words(g, RANDOM))))
    return np.concatenate(parts)


def quarter_turn_words():
    """64-bit words hi:lo around the four quarter turns J = q 2^50: the word itself, its neighbours by one J and by one bit"""
    out = []
    for q in range(4):
        for d in (0, 1, -1, 4096, -4096, 4095, -4097, 8192, -8192):
            out.append(((q << 62) + d) % (1 << 64))
    return out


def sincos_inputs(v2=False):
    """(lo, hi) word pairs; v2: lo restricted to its top 12 bits, which is all that stream version 2 supplies"""
    lo, hi = [], []
    for i in range(ANGLE_SLOTS):
        hi += [i << 24, (i << 24) | 0x800000, (i << 24) | 0xffffff]
        lo += [0, 0, 0xffffffff]
    for w in quarter_turn_words():
        hi.append(w >> 32)
        lo.append(w & 0xffffffff)
    g = rng(2)
    lo = np.concatenate([u64(lo), rand_words(g, RANDOM)])
    hi = np.concatenate([u64(hi), rand_words(g, RANDOM)])
    if v2:
        lo = lo & U64(0xfff00000)
    return lo, hi


EXP_TIES = (0, 127, 254, 255, 256, -1, -256)


def exp_inputs():
    """doubles x, all inside the precondition |x| < 5e6 of exp_f64"""
    xs = [0.0, 1e-300, -1e-300]
    for j in EXP_TIES:
        t = float((LD(j) + LD(0.5)) * LN2 / LD(256))     # where n = rint(256 x / ln 2) is a tie
        xs += [t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), np.nextafter(np.nextafter(t, np.inf), np.inf),
               np.nextafter(np.nextafter(t, -np.inf), -np.inf)]
    xs += [700.0, -700.0, 709.7, -708.3, -745.0, -800.0, -1e4, 4.99e6, -4.99e6]
    g = rng(3)
    return np.concatenate([np.array(xs, dtype=np.float64), g.uniform(-750.0, 709.7, RANDOM // 2), g.uniform(-40.0, 40.0, RANDOM // 2)])


def sqrt_inputs():
    """positive normal doubles"""
    xs = [2.0 ** -52, 73.47, 1e-24, 1e-16, 1e3]
    g = rng(4)
    roots = np.concatenate([np.arange(1, 65, dtype=np.float64), g.uniform(0.01, 31.0, 64)])
    sq = roots * roots
    parts = [np.array(xs), sq, np.nextafter(sq, np.inf), np.nextafter(sq, 0.0), 2.0 ** np.arange(-80, 11).astype(np.float64),
             2.0 ** g.uniform(-53.0, 10.0, RANDOM)]
    return np.concatenate(parts)


def recip_inputs():
    """(n, 4) doubles in [1, 3], the Hastings denominators' range"""
    edges = [1.0, 3.0, 1.0 + 2.0 ** -52, float(np.nextafter(3.0, 0.0))]
    rows = [[a, b, c, d] for a in edges for b in edges for c in edges for d in edges]
    g = rng(5)
    return np.concatenate([np.array(rows), g.uniform(1.0, 3.0, (RANDOM, 4))])


def u01_inputs():
    """(lo, hi) word pairs"""
    edge = [0, 1, 0xfff, 0x1000, 0x1001, 0x7fffffff, 0x80000000, 0xfffff000, 0xffffefff, 0xffffffff]
    lo = [a for a in edge for _ in edge]
    hi = [b for _ in edge for b in edge]
    g = rng(6)
    return np.concatenate([u64(lo), rand_words(g, RANDOM)]), np.concatenate([u64(hi), rand_words(g, RANDOM)])


def pair_extreme_inputs():
    """(a, m, c): the radius uniform at J = 0 and at J = 2^52 - 1 while the angle sits at each quarter turn (and one step
    of the 44-bit angle on either side of it)"""
    rows = []
    for a, m_top in ((0, 0), (0xffffffff, 0xfffff)):
        for q in range(4):
            for d in (0, 1, -1):
                ja = ((q << 42) + d) % (1 << 44)              # the 44-bit angle integer
                rows.append([a, (m_top << 12) | (ja & 0xfff), ja >> 12])
    return u64(rows)


def pair_split_inputs():
    """(base, top, low): word triples (n, 3) where `top` differs from `base` only in the top 20 bits of m and `low` only in its
    low 12 bits"""
    g = rng(7)
    n = 512
    base = np.stack([rand_words(g, n), rand_words(g, n), rand_words(g, n)], axis=1)
    top, low = base.copy(), base.copy()
    flip_top = U64((1 << 31) | (1 << 12))     # the highest and the lowest of the top 20 bits: the radius uniform moves by ~2^-33
    flip_low = g.integers(1, 1 << 12, size=n, dtype=np.uint64)
    top[:, 1] ^= flip_top
    low[:, 1] ^= flip_low
    return base, top, low


def pair_random_inputs():
    g = rng(8)
    return np.stack([rand_words(g, RANDOM), rand_words(g, RANDOM), rand_words(g, RANDOM)], axis=1)


F32_XA = (0, 1, 2, 0x7fffffff, 0x80000000, 0xffffff7f, 0xffffff80, 0xffffffff)
F32_XB = tuple(dict.fromkeys([0, 1 << 9] + [((q << 30) + d) % (1 << 32) for q in range(4) for d in (-(1 << 9), 0, 1 << 9)] + [0xffffffff]))


def f32_block_inputs():
    """(n, 4) words (x, y, z, w): pair A = (x, y), pair B = (z, w); every (xa, xb) of the two lists appears in both positions"""
    grid = [(a, b) for a in F32_XA for b in F32_XB]
    rows = [[a, b, a2, b2] for (a, b), (a2, b2) in zip(grid, reversed(grid))]
    g = rng(9)
    return np.concatenate([u64(rows), np.stack([rand_words(g, RANDOM) for _ in range(4)], axis=1)])


# ---- the vanilla call at forced extremes (tests/test_gpu_vanilla_extremes.py) -----------------------------------------------------
LOG2E = 1.4426950408889634074
BASE = dict(s=105.0, k=95.0, r=0.02, v=0.35, t=2.5)
# v sqrt(t) = 2.531 puts (r - v^2/2) t + 6.73 v sqrt(t) at 20 binary orders: the fp32 rescale exponent is 21, and a clamp sized for
# normals up to 6.7 only (one order less) saturates at the generator's 6.7637
WIDE = dict(s=100.0, k=100.0, r=0.03, v=2.531, t=1.0)
MARKETS = {"itm": BASE, "deep_otm": dict(s=80.0, k=140.0, r=-0.01, v=0.15, t=0.25), "zero_strike": dict(BASE, k=0.0),
           "negative_strike": dict(BASE, k=-20.0), "wide": WIDE}
NEAR_MAX = {"f32": 6.76, "f64": 8.57}          # just inside the host's bounds 6.77 / 8.58
DEVICE_MAX = {"f32": ZMAX_F32, "f64": ZMAX_F64}
NP = {"f32": np.float32, "f64": np.float64}


def as_given(o, X):
    """the market as the kernels of precision X receive it: mc_option_f32 holds floats"""
    return {c: float(NP[X](o[c])) for c in "skrvt"}


def drift_vol(o):
    return (o["r"] - 0.5 * o["v"] * o["v"]) * o["t"], o["v"] * math.sqrt(o["t"])


def f32_rescale_exponent(o, zmax):
    """k of the fp32 kernels' power-of-two rescale as VanillaTraits<float>::prepare states it: the smallest integer with
    2^((drift + vol zmax) log2 e) + max(-K/S, 0) <= 2^k"""
    drift, vol = drift_vol(as_given(o, "f32"))
    return math.ceil(math.log2(2.0 ** ((drift + vol * zmax) * LOG2E) + max(-o["k"] / o["s"], 0.0)))


def vanilla_payoff(o, z, X):
    """max(S exp((r - v^2/2) t + v sqrt(t) z) - K, 0) in long double on the market as precision X receives it; returns
    (payoff, S_T)"""
    o = as_given(o, X)
    z = np.asarray(z, dtype=np.float64).astype(LD)
    drift = (LD(o["r"]) - LD(0.5) * LD(o["v"]) * LD(o["v"])) * LD(o["t"])
    st = LD(o["s"]) * np.exp(drift + LD(o["v"]) * np.sqrt(LD(o["t"])) * z)
    return np.maximum(st - LD(o["k"]), LD(0)), st


def extreme_normals(o, X):
    """The per-path list: +- the device's largest |z|, +- the host bound's neighbour, +-0, and -- where K > 0 -- the normals
    around the one that puts S_T on K (two representable steps to either side)."""
    ty = NP[X]
    zs = [DEVICE_MAX[X], -DEVICE_MAX[X], NEAR_MAX[X], -NEAR_MAX[X], 0.0, -0.0]
    if o["k"] > 0:
        drift, vol = drift_vol(as_given(o, X))
        z0 = ty((math.log(o["k"] / o["s"]) - drift) / vol)
        up = dn = z0
        zs.append(z0)
        for _ in range(2):
            up, dn = np.nextafter(up, ty(np.inf)), np.nextafter(dn, ty(-np.inf))
            zs += [up, dn]
    return np.array(zs, dtype=ty)
