"""Independent float64 reference of the arithmetic-average (Asian) call and its geometric control variate (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_dates equally spaced dates t_j = j T / m,
    dt = T / m,  a = (r - v^2/2) dt,  bx = v sqrt(dt),  W_j = z_1 + ... + z_j,  ln S_j = ln S0 + j a + bx W_j,
    A = (1/m) sum_j S_j,   G = exp(ln S0 + a (m + 1)/2 + (bx/m) sum_j W_j),
    plain (A - K)^+,  control (A - K)^+ - (G - K)^+,  antithetic: the mean of the value at z and at -z,
evaluated with numpy on a given array of normals.  `asian` returns a greeks_ref.Paths (value, scale, jump, edge), each of shape
(1, n_paths) like a one-plane product of greeks_ref, so that greeks_ref.bound applies: a kernel computing the same formulas
in a precision of unit roundoff u is within a small multiple of u * scale of value.  (x)^+ is continuous: no jump, no edge.

The forward-error scale, in units of roundoff:
  - S_j carries the relative error of its exponent, el_j = 1 + |ln S0| + j |a| + bx (|W_j| + sum_{i<=j} |W_i|) (the rounded
    per-date constant, and the running sum W_j whose every partial sum is rounded): what greeks_ref.cva charges for ln S_j;
  - the running sum over the dates adds one rounding of every partial sum: sum_j (S_1 + ... + S_j);
  - the division by m one rounding of A, the subtraction |K|;
  - the control the same for G: its exponent's el = 1 + |ln S0| + |a| (m + 1)/2 + (bx/m) (|sum_j W_j| + sum_j sum_{i<=j} |W_i|
    + sum_j |W_1 + ... + W_j|) (every W_j's own error, and the running sum of the W_j), and |K| once more.
"""
import math

import numpy as np

from greeks_ref import NPB, Paths, basket_normals, random_vanilla   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_ASIAN = 4


def asian_normals(draw, first, n, n_dates, npb):
    """Path p is unit p of domain 4; date j (1-based) draws entry (j - 1) % npb of block (j - 1) // npb.  Shape (n, n_dates)."""
    return basket_normals(lambda _, u, c, b: draw(DOMAIN_ASIAN, u, c, b), first, n, n_dates, npb)


def _one_side(s0, k, a, bx, m, W, control):
    """value and scale of one path direction, from its Brownian sums W (n, m)."""
    j = np.arange(1, m + 1)
    W_abs = np.cumsum(np.abs(W), axis=1)
    S = np.exp(math.log(s0) + j * a + bx * W)
    el = 1.0 + abs(math.log(s0)) + j * abs(a) + bx * (np.abs(W) + W_abs)
    A = S.sum(axis=1) / m
    value = np.maximum(A - k, 0.0)
    scale = ((S * el).sum(axis=1) + np.cumsum(S, axis=1).sum(axis=1)) / m + A + abs(k)
    if control:
        sw = W.sum(axis=1)
        G = np.exp(math.log(s0) + a * (m + 1) / 2.0 + (bx / m) * sw)
        eg = (1.0 + abs(math.log(s0)) + abs(a) * (m + 1) / 2.0
              + (bx / m) * (np.abs(sw) + W_abs.sum(axis=1) + np.abs(np.cumsum(W, axis=1)).sum(axis=1)))
        value = value - np.maximum(G - k, 0.0)
        scale = scale + G * eg + abs(k)
    return value, scale


def asian(o, n_dates, z, control=False, anti=False):
    """Per-path values of the Asian call on the normals z (n_paths, >= n_dates), and their forward-error scales."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    m = int(n_dates)
    z = np.asarray(z, dtype=np.float64)[:, :m]
    n = z.shape[0]
    dt = t / m
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    W = np.cumsum(z, axis=1)
    value, scale = _one_side(s0, k, a, bx, m, W, control)
    if anti:
        vm, sm = _one_side(s0, k, a, bx, m, -W, control)
        value, scale = 0.5 * (value + vm), 0.5 * (scale + sm)
    return Paths(value.reshape(1, n), scale.reshape(1, n), np.zeros((1, n)), np.full(n, np.inf))


def geometric_mean_closed_form(o, n_dates):
    """E[(G - K)^+] from first principles: the moments of ln G by the explicit sums over the dates
    (mu = ln S0 + (r - v^2/2) sum_j t_j / m,  var = v^2 sum_i sum_j min(t_i, t_j) / m^2), the lognormal call with erfc."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    m = int(n_dates)
    tj = np.arange(1, m + 1, dtype=np.float64) * (t / m)
    mu = math.log(s0) + (r - 0.5 * v * v) * float(tj.sum()) / m
    # sum_i sum_j min(t_i, t_j) row by row (bounded memory at m = 4096)
    var = v * v * float(sum(float(np.minimum(ti, tj).sum()) for ti in tj)) / (m * m)
    sd = math.sqrt(var)
    d1 = (mu - math.log(k) + var) / sd
    d2 = d1 - sd
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    return math.exp(mu + 0.5 * var) * Phi(d1) - k * Phi(d2)


def black_scholes_call(o):
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    sd = v * math.sqrt(t)
    d1 = (math.log(s0 / k) + (r + 0.5 * v * v) * t) / sd
    Phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))
    return s0 * Phi(d1) - k * math.exp(-r * t) * Phi(d1 - sd)


# ---- the shapes of the many-trip GPU test (tests/test_gpu_walk_trips.py) --------------------------------------------------------
TRIP_DATES = [3, 8, 17]        # per path against the model: the ends of the date loops (fp32 4 dates per trip; fp64 8, then 2)
TRIP_BITS_DATES = [5, 9, 257]  # the same bits on every grid, ranges B and C
CASES = [random_vanilla(np.random.default_rng(7100 + i)) for i in range(3)]   # asymmetric markets, as the one-trip test draws them
