"""Independent float64 reference of the calls and puts under a local-volatility surface (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_steps = n_dates * steps_per_date equal steps,
dt = T / m, sdt = sqrt(dt), y = ln(S / S0), y_0 = 0, and for step j = 1 ... m with the step's normal z_j
    sigma_j = surface(slice(j), y_{j-1}),      slice(j) = (j - 1) // (m // n_times),
    y_j     = y_{j-1} + (r - sigma_j^2 / 2) dt + sigma_j sdt z_j,
the surface on n_nodes equally spaced nodes of y in [y_lo, y_hi], h = (y_hi - y_lo) / (n_nodes - 1):
    u = clamp((y - y_lo) / h, 0, n_nodes - 1),  i = min(floor(u), n_nodes - 2),  sigma = a_i + (u - i) b_i,  b_i = a_{i+1} - a_i,
a_i the caller's volatilities as rounded for the precision, b_i their difference in float64 rounded once to it.  Date d falls after
step d * steps_per_date; with S_d = S0 exp(y_d), phi = +1 (call) or -1 (put):
    European (phi (S_m - K))^+      Asian (phi ((1/n_dates) sum_d S_d - K))^+
    barrier  d_d = sgn (ln(B / S0) - y_d),  P = [min_d d_d > 0],  knock-out P (phi (S_m - K))^+,  knock-in (1 - P)(phi (S_m - K))^+
    antithetic: the mean of the value at z and at -z, each direction with its own y and its own lookups.
`walk` returns one dict per path direction; `european` / `asian` / `barrier` turn them into per-path values.

The forward error, at EVERY date, to first order, for a kernel of unit roundoff tol that evaluates the same formulas in any
association.  With w = sdt z - sigma dt (the step's derivative in sigma) and sigma' = b_i / h (0 where clamped) the step's Jacobian is
J_j = 1 + sigma' w, signed; an error committed at step i reaches date d multiplied by the product of the later J, and with absolute
values taken at the end the bound is sum_i |prod_{i<k<=j} J_k| l_i = the forward pass
    E_j = |J_j| E_{j-1} + tol l_j,      E_0 = 0,
    l_j = |w| ls_j + 3 |sigma sdt z| + 2 sigma^2 dt + 2 |r| dt + |y_{j-1}| + |c_j| + |y_j|     (c_j = (r - sigma^2/2) dt)
        (sdt, dt/2 and r dt rounded once each; the products, the square, the partial sum and the final fma),
    ls_j = |sigma'| (|y| + |y_lo| + h |u|) + |(u - i) b_i| + 2 sigma
        (u = fma(y, 1/h, -y_lo/h): the two rounded constants and the fma, carried into sigma through the slope; b_i rounded once;
         the rounded a_i and the interpolation's fma).
At a node the two one-sided slopes differ (beyond the first and the last node one of them is 0): a step whose y_{j-1} lies within
E_{j-1} + tol (|y| + |y_lo| + h |u|) of a node is charged the slope of larger magnitude in J and in ls -- the interpolant is
continuous, so landing in the neighbouring interval moves sigma by no more than that slope times the error.  Every path has a bound.
At date d (step j):
    bx_d = E_j + tol (1 + 2 |ln S0| + 3 |y_d| + |ln S0 + y_d|)       on the exponent of S_d (the conversion to the exponential's units),
    bd_d = E_j + tol (1 + |ln(B / S0)| + 2 |y_d| + 2 |d_d|)           on the distance to the barrier,
    European error <= S_m expm1(bx_m) + tol (2 S_m + |K| + value)
    Asian error    <= (1/n_dates) sum_d S_d expm1(bx_d) + tol ((2 sum_d S_d + sum_d (S_1 + ... + S_d)) / n_dates + A + |K| + value)
    barrier: a direction with |d_d| > bd_d at every date has its P decided and is checked within the European bound.  A NEAR direction
        (some |d_d| <= bd_d) may take either of its two values; `barrier_errors` accepts the nearest combination.  No path is left out.

`displaced_surface` samples sigma(t, S) = sd (S + a e^{-r (T - t)}) / S at slice midpoints: under it S + a e^{-r (T - t)} is a geometric
Brownian motion of volatility sd, and `displaced_price` is the exact price of the continuous model.

BIAS[strike] = (b, h): the model's mean minus displaced_price (discounted) on BIAS_CASE, and its 95 % half-width, from this module's
own walk in float64 on numpy normals, 4 194 304 antithetic pairs, seed 2024:
    python tests/localvol_ref.py bias
"""
import math
import sys

import numpy as np

from barrier_ref import black_scholes_call   # noqa: F401  (re-exported for the tests)
from greeks_ref import NPB, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_LOCALVOL = 16
KINDS = ["up-and-out", "up-and-in", "down-and-out", "down-and-in"]
MUTATIONS = ("slice_late", "round_nearest", "no_half", "clamp_n", "date_late", "one_more", "put_as_call")
NEAR_CAP = 0.05
MUTATION_SHARE = 0.40   # tests/test_heston_ref.py's

MKT = dict(s=87.0, k=91.0, r=0.02, t=0.75)
UP, DOWN = 110.0, 70.0


def localvol_normals(draw, first, n, m, npb):
    """Path p is unit p of domain 16; step j (1-based) draws entry (j - 1) % npb of block (j - 1) // npb.  Shape (n, m)."""
    return basket_normals(lambda _, u, c, b: draw(DOMAIN_LOCALVOL, u, c, b), first, n, m, npb)


# ---- surfaces -------------------------------------------------------------------------------------------------------
def make_surface(sigma, y_lo, y_hi):
    return dict(sigma=np.atleast_2d(np.asarray(sigma, dtype=np.float64)), y_lo=float(y_lo), y_hi=float(y_hi))


def displaced_surface(sd, a, r, T, n_times, n_nodes, y_lo, y_hi, s0=100.0):
    """sigma(t, S) = sd (S + a e^{-r (T - t)}) / S at the slice midpoints and the nodes of y = ln(S / s0)."""
    t = (np.arange(n_times) + 0.5) * T / n_times
    S = s0 * np.exp(np.linspace(y_lo, y_hi, n_nodes))
    return make_surface(sd * (S[None, :] + a * np.exp(-r * (T - t))[:, None]) / S[None, :], y_lo, y_hi)


def _phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def displaced_price(s0, k, r, T, sd, a, right="call"):
    """Discounted exact price under the continuous displaced diffusion: e^{-rT} [(F + a) Phi(d1) - (K + a) Phi(d2)]; the put by parity."""
    F = s0 * math.exp(r * T)
    sq = sd * math.sqrt(T)
    d1 = math.log((F + a) / (k + a)) / sq + 0.5 * sq
    call = math.exp(-r * T) * ((F + a) * _phi(d1) - (k + a) * _phi(d1 - sq))
    return call if right == "call" else call - s0 + k * math.exp(-r * T)


def wavy_surface(n_times, n_nodes, y_lo, y_hi):
    """A skewed smile in y that rises with the slice, plus a wiggle per node in proportion to the node spacing: rows and intervals all
    differ (an exchanged row or interval changes the paths through it) while the slope in y stays of order 1 on any grid -- a slope of
    order 1 / h would make the walk itself chaotic, and no bound could follow it."""
    q, i = np.arange(n_times)[:, None], np.arange(n_nodes)[None, :]
    y = np.linspace(y_lo, y_hi, n_nodes)[None, :]
    h = (y_hi - y_lo) / (n_nodes - 1)
    return make_surface(0.22 + 0.04 * q / n_times - 0.25 * y + 0.3 * y * y + 0.05 * h * np.cos(2.3 * i + 0.7 * q), y_lo, y_hi)


def rounded(d, dtype):
    """The scalar inputs as the precision's struct holds them."""
    return {c: float(dtype(x)) for c, x in d.items() if np.ndim(x) == 0}


def tables(surface, dtype):
    """(a, b) as the engine holds them for `dtype`, as float64 arrays of shape (n_times, n_nodes) and (n_times, n_nodes - 1)."""
    a = np.asarray(surface["sigma"], dtype=dtype).astype(np.float64)
    b = (a[:, 1:] - a[:, :-1]).astype(dtype).astype(np.float64)
    return a, b


def sigma_at(surface, m, step, y, dtype=np.float64):
    """The header's lookup in float64 on the table as rounded for dtype: what mc_localvol_sigma_* returns."""
    a, b = tables(surface, dtype)
    nt, nn = a.shape
    q = (step - 1) // (m // nt)
    g = rounded(surface, dtype)
    h = (g["y_hi"] - g["y_lo"]) / (nn - 1)
    u = min(max((y - g["y_lo"]) / h, 0.0), nn - 1.0)
    i = min(int(math.floor(u)), nn - 2)
    return a[q, i] + (u - i) * b[q, i]


# ---- the walk -------------------------------------------------------------------------------------------------------
def walk(o, surface, n_dates, spd, z, anti=False, tol=None, dtype=np.float64, mutation=None, table=None):
    """One dict per path direction: `y` (n_dates, n_paths) at the dates, as float64 whatever dtype the walk ran in, and with tol the
    forward bound `E` (n_dates, n_paths) of the docstring.  z: (n_paths, m).  table: the dtype the surface's (a, b) are rounded for
    (default: dtype) -- the model of a float32 kernel is dtype float64 on the float32 table."""
    n_dates, spd = int(n_dates), int(spd)
    m = n_dates * spd
    R = dtype
    table = R if table is None else table
    o, g = rounded(o, table), rounded(surface, table)
    s0, r, t = (o[c] for c in "srt")
    a64, b64 = tables(surface, table)
    nt, nn = a64.shape
    assert m % nt == 0 and z.shape[1] == m
    a, b = a64.astype(R), b64.astype(R)
    y_lo, h = g["y_lo"], (g["y_hi"] - g["y_lo"]) / (nn - 1)
    dt = t / m
    sdt = math.sqrt(dt)
    inv_h, u0, u_max = R(1.0 / h), R(-y_lo / h), R(nn if mutation == "clamp_n" else nn - 1)
    rdt, hdt, sdt_r = R(r * dt), R(0.0 if mutation == "no_half" else 0.5 * dt), R(sdt)
    per = m // nt
    # the one-sided slopes at node k: left = interval k - 1 (0 at k = 0), right = interval k (0 at k = nn - 1)
    slope = np.concatenate([np.zeros((nt, 1)), b64 / h, np.zeros((nt, 1))], axis=1)   # slope[:, i + 1] = interval i; 0 beyond both ends
    sides = []
    for sign in ((1.0, -1.0) if anti else (1.0,)):
        n = z.shape[0]
        y = np.zeros(n, dtype=R)
        E = np.zeros(n)
        ys, Es = np.empty((n_dates, n)), np.empty((n_dates, n))
        clamped = np.zeros((2, n), dtype=bool)
        # date d falls after step d spd; the mutation reads every date but the last one step late
        at = {}
        for d in range(1, n_dates + 1):
            at.setdefault(min(d * spd + 1, m) if mutation == "date_late" and d < n_dates else d * spd, []).append(d - 1)
        for j in range(1, m + 1):
            q = (j - 2 if mutation == "slice_late" else j - 1) // per
            q = min(max(q, 0), nt - 1)
            zj = (sign * z[:, j - 1]).astype(R)
            u_raw = y * inv_h + u0
            u = np.minimum(np.maximum(u_raw, R(0)), u_max)
            fl = np.rint(u) if mutation == "round_nearest" else np.floor(u)
            i = np.minimum(fl, R(nn - 2)).astype(np.int64)
            f = u - i.astype(R)
            sig = a[q, i] + f * b[q, i]
            c = rdt - sig * sig * hdt
            zs = sdt_r * zj
            y_new = y + c + sig * zs
            if tol is not None:
                y8, u8, sig8 = y.astype(np.float64), u.astype(np.float64), sig.astype(np.float64)
                clamped[0] |= u_raw <= 0
                clamped[1] |= u_raw >= nn - 1
                du = tol * (np.abs(y8) + abs(y_lo) + h * np.abs(u8))
                own = np.where((u_raw <= 0) | (u_raw >= nn - 1), 0.0, slope[q, i + 1])
                k = np.rint(np.minimum(np.maximum(u_raw.astype(np.float64), -1.0), float(nn))).astype(np.int64)   # the nearest node, or just beyond an end
                k = np.minimum(np.maximum(k, 0), nn - 1)
                near = np.abs(y8 - (y_lo + k * h)) <= E + du
                left, right = slope[q, k], slope[q, k + 1]
                big = np.where(np.abs(left) >= np.abs(right), left, right)
                sl = np.where(near & (np.abs(big) > np.abs(own)), big, own)
                w = (zs - sig * R(dt)).astype(np.float64)
                ls = np.abs(sl) * (np.abs(y8) + abs(y_lo) + h * np.abs(u8)) + np.abs(f.astype(np.float64) * b64[q, i]) + 2.0 * sig8
                loc = (np.abs(w) * ls + 3.0 * np.abs(sig8 * zs.astype(np.float64)) + 2.0 * sig8 * sig8 * dt + 2.0 * abs(r) * dt + np.abs(y8) +
                       np.abs(c.astype(np.float64)) + np.abs(y_new.astype(np.float64)))
                # J at the own slope and, near a node, at the other one-sided slope too: the larger magnitude
                J = np.maximum(np.abs(1.0 + own * w), np.where(near, np.maximum(np.abs(1.0 + left * w), np.abs(1.0 + right * w)), 0.0))
                E = J * E + tol * loc
            y = y_new
            for d in at.get(j, ()):
                ys[d], Es[d] = y, E
        sides.append(dict(y=ys, E=Es if tol is not None else None, o=o, n_dates=n_dates, spd=spd, tol=tol, clamped=clamped, ln_s0=math.log(s0)))
    return sides


def _sign(right, mutation=None):
    return 1.0 if right == "call" or mutation == "put_as_call" else -1.0


def _pay(s, right, mutation=None):
    return np.maximum(_sign(right, mutation) * (float(s["o"]["s"]) * np.exp(s["y"][-1]) - float(s["o"]["k"])), 0.0)


def european(sides, right="call", mutation=None):
    return sum(_pay(s, right, mutation) for s in sides) / len(sides)


def asian(sides, right="call", mutation=None):
    out = 0.0
    for s in sides:
        A = float(s["o"]["s"]) * np.exp(s["y"]).sum(axis=0) / (s["n_dates"] + (1 if mutation == "one_more" else 0))
        out = out + np.maximum(_sign(right, mutation) * (A - float(s["o"]["k"])), 0.0)
    return out / len(sides)


def _bx(s):
    tol, y = s["tol"], s["y"]
    return s["E"] + tol * (1.0 + 2.0 * abs(s["ln_s0"]) + 3.0 * np.abs(y) + np.abs(s["ln_s0"] + y))


def _pay_bound(s, right):
    tol, k = s["tol"], float(s["o"]["k"])
    S = float(s["o"]["s"]) * np.exp(s["y"][-1])
    with np.errstate(over="ignore"):
        return S * np.expm1(_bx(s)[-1]) + tol * (2.0 * S + abs(k) + _pay(s, right))


def european_bound(sides, right="call"):
    return sum(_pay_bound(s, right) for s in sides) / len(sides) + sides[0]["tol"] * np.abs(european(sides, right))


def asian_bound(sides, right="call"):
    total = 0.0
    for s in sides:
        tol, nd, k = s["tol"], s["n_dates"], float(s["o"]["k"])
        S = float(s["o"]["s"]) * np.exp(s["y"])
        A = S.sum(axis=0) / nd
        with np.errstate(over="ignore"):
            b = (S * np.expm1(_bx(s))).sum(axis=0) / nd
        total = total + b + tol * ((2.0 * S.sum(axis=0) + np.cumsum(S, axis=0).sum(axis=0)) / nd + A + abs(k) + np.abs(A - k))
    return total / len(sides) + sides[0]["tol"] * np.abs(asian(sides, right))


def _barrier_side(s, B, up, right, bounded):
    sgn = 1.0 if up else -1.0
    g = math.log(float(B) / float(s["o"]["s"]))
    d = sgn * (g - s["y"])
    live = d.min(axis=0) > 0
    pay = _pay(s, right)
    if not bounded:
        return live, None, pay, None
    bd = s["E"] + s["tol"] * (1.0 + abs(g) + 2.0 * np.abs(s["y"]) + 2.0 * np.abs(d))
    return live, (np.abs(d) <= bd).any(axis=0), pay, _pay_bound(s, right)


def barrier(sides, B, kind="up-and-out", right="call", mutation=None):
    up, knock_in = kind.startswith("up"), kind.endswith("in")
    c0, c1 = (1.0, -1.0) if knock_in else (0.0, 1.0)
    out = 0.0
    for s in sides:
        live = _barrier_side(s, B, up, right, False)[0]
        out = out + (c0 + c1 * live) * _pay(s, right, mutation)
    return out / len(sides)


def barrier_errors(got, sides, B, kind, right="call"):
    """(|got - nearest admissible value| / bound per path, near mask): a decided direction has one admissible value, a near direction
    two (knocked, not knocked); the admissible values of the path are the means over the directions."""
    up, knock_in = kind.startswith("up"), kind.endswith("in")
    c0, c1 = (1.0, -1.0) if knock_in else (0.0, 1.0)
    n = sides[0]["y"].shape[1]
    cands, bound, near_any = [np.zeros(n)], np.zeros(n), np.zeros(n, dtype=bool)
    for s in sides:
        live, near, pay, bpay = _barrier_side(s, B, up, right, True)
        own = (c0 + c1 * live) * pay
        other = np.where(near, (c0 + c1 * ~live) * pay, own)
        cands = [c + v for c in cands for v in (own, other)]
        bound, near_any = bound + bpay, near_any | near
    w = 1.0 / len(sides)
    got = np.asarray(got, dtype=np.float64)
    err = np.minimum.reduce([np.abs(got - w * c) for c in cands])
    return err / (w * bound + sides[0]["tol"] * np.abs(barrier(sides, B, kind, right))), near_any


def check(got, want, bound, what):
    """The per-path rule: every value finite, >= 0 and within the bound of the model's.  Returns the worst error / bound; asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    r = np.abs(got - want) / bound
    assert np.all(r <= 1.0), (what, int(np.argmax(r)), float(r.max()))
    return float(r.max())


def check_barrier(got, sides, B, kind, right, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    r, near = barrier_errors(got, sides, B, kind, right)
    assert np.all(r <= 1.0), (what, kind, int(np.argmax(r)), float(r.max()))
    assert near.sum() <= NEAR_CAP * got.size, (what, kind, int(near.sum()))
    return float(r.max()), int(near.sum())


# ---- the shapes of the per-path GPU test (tests/test_gpu_localvol.py) ------------------------------------------------------------
# (n_steps, n_times, steps_per_date, n_nodes): the step counts 1 ... 64 are the trip boundaries of both precisions (fp32: four steps per
# Philox block; fp64: eight per trip, then two); n_steps / n_times odd, even, 1 and n_times = n_steps; steps_per_date 1, 2, 3, n_steps.
SHAPES = [(1, 1, 1, 2), (2, 1, 1, 3), (2, 2, 2, 2), (3, 1, 3, 65), (3, 3, 1, 3), (4, 2, 2, 65), (4, 1, 1, 2), (5, 1, 5, 3), (7, 1, 1, 65),
          (8, 2, 2, 3), (8, 1, 8, 2), (9, 3, 3, 65), (9, 1, 1, 3), (15, 3, 3, 2), (15, 1, 1, 65), (16, 2, 2, 3), (16, 16, 1, 65), (17, 1, 1, 3),
          (33, 3, 3, 65), (33, 1, 1, 2), (64, 2, 2, 65), (64, 1, 1, 3), (64, 64, 1, 2), (64, 32, 2, 64)]
BIG_SHAPE = (4096, 2, 2, 65)
F32_BARRIER_MAX_STEPS = 64   # the fp32 barrier payoff runs up to here (the near paths of BIG_SHAPE pass NEAR_CAP in fp32)
WIDE, NARROW = (-1.5, 1.5), (-0.05, 0.05)
FIRSTS = [4242, (1 << 32) - 2000]
N_PATHS = 4096 + 37


def surface_for(shape, grid):
    m, nt, spd, nn = shape
    return wavy_surface(nt, nn, *grid)


# ---- the scheme's bias against the continuous displaced diffusion -----------------------------------------------------------------
BIAS_CASE = dict(s=100.0, sd=0.2, a=50.0, r=0.03, t=1.0, n_times=8, n_nodes=65, y_lo=-1.5, y_hi=1.5, n_steps=64)
BIAS = {   # strike: (b, h); printed by `python tests/localvol_ref.py bias`
    80.0: (0.004449, 0.008666),
    100.0: (0.012338, 0.010605),
    120.0: (0.014226, 0.008782),
}


def bias_surface():
    c = BIAS_CASE
    return displaced_surface(c["sd"], c["a"], c["r"], c["t"], c["n_times"], c["n_nodes"], c["y_lo"], c["y_hi"], c["s"])


def _fast_levels(o, surface, m, z):
    """S_m of both directions without the bookkeeping of the bound (same formulas)."""
    a, b = tables(surface, np.float64)
    nt, nn = a.shape
    y_lo, h = surface["y_lo"], (surface["y_hi"] - surface["y_lo"]) / (nn - 1)
    s0, r, t = (float(o[c]) for c in "srt")
    dt = t / m
    sdt = math.sqrt(dt)
    out = []
    for sign in (1.0, -1.0):
        y = np.zeros(z.shape[0])
        for j in range(m):
            q = j // (m // nt)
            u = np.clip((y - y_lo) / h, 0.0, nn - 1.0)
            i = np.minimum(np.floor(u), nn - 2).astype(np.int64)
            sig = a[q, i] + (u - i) * b[q, i]
            y = y + (r - 0.5 * sig * sig) * dt + sig * sdt * (sign * z[:, j])
        out.append(s0 * np.exp(y))
    return out


def _measure_bias(pairs=1 << 22, chunk=1 << 18, seed=2024):
    c = BIAS_CASE
    rng = np.random.default_rng(seed)
    surf = bias_surface()
    o = dict(s=c["s"], r=c["r"], t=c["t"])
    strikes = (80.0, 100.0, 120.0)
    tot, tot2 = np.zeros(3), np.zeros(3)
    for _ in range(pairs // chunk):
        up, dn = _fast_levels(o, surf, c["n_steps"], rng.standard_normal((chunk, c["n_steps"])))
        for q, k in enumerate(strikes):
            v = 0.5 * (np.maximum(up - k, 0.0) + np.maximum(dn - k, 0.0))
            tot[q], tot2[q] = tot[q] + v.sum(), tot2[q] + (v * v).sum()
    disc = math.exp(-c["r"] * c["t"])
    for q, k in enumerate(strikes):
        mean = tot[q] / pairs
        sd = math.sqrt((tot2[q] / pairs - mean * mean) * pairs / (pairs - 1))
        print(f"    {k}: ({disc * mean - displaced_price(c['s'], k, c['r'], c['t'], c['sd'], c['a']):.6f}, {1.96 * disc * sd / math.sqrt(pairs):.6f}),")


if __name__ == "__main__" and sys.argv[1:] == ["bias"]:
    _measure_bias()
