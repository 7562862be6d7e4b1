"""Independent float64 reference of the Asian and the discretely monitored barrier call on the Heston walk (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel.  The walk is heston_ref's: m = n_dates * steps_per_date
full-truncation Euler steps, two normals per step; heston_ref.walk gives the variance path, the local-error terms of every step and
the value at maturity.  The contract's dates are t_d = d T / n_dates, d = 1 ... n_dates; date d falls after step j = d * steps_per_date,
where
    x_d = ln S0 + r t_d - (dt/2) A_j + sdt B_j,      A_j = sum_{i<=j} V+_{i-1},  B_j = sum_{i<=j} s_{i-1} z1_i,
    Asian     ((1/n_dates) sum_d exp(x_d) - K)^+
    barrier   d_d = sgn (ln B - x_d),  P = [min_d d_d > 0],  knock-out P (exp(x_m) - K)^+,  knock-in (1 - P)(exp(x_m) - K)^+
    antithetic: the mean of the value at (z1, z2) and at (-z1, -z2).
`walk` returns one dict per path direction; `asian` / `barrier` turn them into per-path values.

The forward error, at EVERY date.  heston_ref bounds x_m by a signed backward recursion from maturity; a bound at every date by that
route costs O(dates * steps * paths).  Here ONE forward pass carries, in absolute values, the size of the error in V and in x:
    E_j  = |J_j| E_{j-1} + tol lV_j,           E_0 = tol v0,
    Ex_j = Ex_{j-1} + |g_j| E_{j-1} + tol ((dt/2) |A_j| + sdt (2 s |z1_j| + |B_j|)),          Ex_0 = 0,
J_j, g_j, lV_j and the kink branch (|V_{j-1}| < E_{j-1}: J = 1, g = 0, the step charged kappa dt E + |zv_j| sqrt(E) into V and
(dt/2) E + sdt |z1_j| sqrt(E) into x) exactly as heston_ref states them.  At date d (step j) the bound on |dx_d| is
    bx_d = Ex_j + tol (1 + |ln S0 + r t_d| + 3 (dt/2) A_j + 3 sdt |B_j| + 2 |x_d|)
(the rounded per-date constant, the two fmas, the exponent's conversion), and on the distance
    bd_d = Ex_j + tol (1 + |sgn (ln B - ln S0 - r t_d)| + 3 (dt/2) A_j + 3 sdt |B_j| + 2 |d_d|).
It is looser than the backward recursion (no damping by the sign of J) but O(steps * paths).  From it:
    Asian error <= (1/n_dates) sum_d S_d expm1(bx_d) + tol ((2 sum_d S_d + sum_d (S_1 + ... + S_d)) / n_dates + A + |K| + value)
        (every exponential's own rounding, every partial sum of the running sum, the division, the subtraction);
    barrier: a path direction with |d_d| > bd_d at every date has its P decided; it is then checked within heston_ref's bound of the
        value at maturity.  A NEAR direction (some |d_d| <= bd_d) may take either of its two values; `barrier_errors` accepts the
        nearest combination.  No path is left out.
A path with a kink step in the forward pass is a KINK PATH (heston_ref); every path has a bound.

Shares measured with this bound on numpy normals, S0 = 100, B = 125 and B = 80, heston_ref.CASES (tests/test_heston_path_ref.py asserts
the caps on every shape of the GPU test and prints the shares): see NEAR_CAP and `barrier_runs` below.
"""
import math

import numpy as np

import heston_ref as hr
from greeks_ref import NPB, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_HESTON_PATH = 7
KINDS = ["up-and-out", "up-and-in", "down-and-out", "down-and-in"]
PAYOFF_MUTATIONS = ("late", "one_more", "up_as_down")

# (n_dates, steps_per_date) of the per-path GPU test: date boundaries against every loop boundary (fp32: two steps per Philox block,
# an odd steps_per_date splits a block; fp64: four pairs per trip, then one); the last three are at MC_MAX_HESTON_STEPS
SHAPES = [(1, 1), (1, 2), (1, 5), (2, 1), (3, 1), (3, 3), (4, 1), (5, 2), (7, 3), (8, 1), (9, 1), (16, 1), (16, 16), (17, 1), (12, 21), (63, 1),
          (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (5, 51), (1, 4096), (256, 16), (4096, 1)]
# the many-trip GPU test (tests/test_gpu_walk_trips.py): per path against the model on the path counts of greeks_ref.TRIP_RANGES "A" and
# "C"; the same bits on every grid on "B" and "C"
TRIP_SHAPES = [(3, 1), (5, 2), (16, 1)]
TRIP_BITS_SHAPES = [(3, 3), (9, 1), (257, 1)]
FOUR_KIND_SHAPES = [(7, 3), (16, 1)]   # all four barrier types; elsewhere up-and-out at UP and down-and-in at DOWN
UP, DOWN = 125.0, 80.0
NEAR_CAP = 0.05
F32_BARRIER_MAX_STEPS = 64   # beyond it the fp32 near paths pass NEAR_CAP, except at (16, 16) without VIOLATED


def barrier_runs(name, X, n_dates, spd):
    """Whether the per-path GPU test runs the barrier payoff on this (case, precision, shape): fp64 everywhere heston_ref.runs admits,
    fp32 up to 64 total steps, plus 16 x 16 without VIOLATED."""
    m = n_dates * spd
    if not hr.runs(name, X, m):
        return False
    return X == "f64" or m <= F32_BARRIER_MAX_STEPS or ((n_dates, spd) == (16, 16) and name != "VIOLATED")


def heston_path_normals(draw, first, n, m, npb):
    """Path p is unit p of domain 7; step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of block 2(j-1) // npb as z1 and
    z2: the Heston layout.  Returns (z1, z2), each of shape (n, m)."""
    z = basket_normals(lambda _, u, c, b: draw(DOMAIN_HESTON_PATH, u, c, b), first, n, 2 * m, npb)
    return z[:, 0::2], z[:, 1::2]


def _dates(s, o, n_dates, spd, dtype, late, mutation=None):
    """x at the dates of one path direction of heston_ref.walk, evaluated in dtype from the variance path.  late: the mutation that
    reads every date but the last one step late; mutation: heston_ref's, where it touches the log price."""
    s0, r, t = (float(o[c]) for c in "srt")
    m = n_dates * spd
    R = dtype
    V = np.asarray(s["V"], dtype=R)                      # V_0 ... V_{m-1}, exactly representable in R (computed there)
    Vp = np.maximum(V, R(0))
    S = np.sqrt(np.abs(V)) if mutation == "abs_root" else np.sqrt(Vp)
    A, B = np.cumsum(Vp, axis=0, dtype=R), np.cumsum(S * np.asarray(s["Z1"], dtype=R), axis=0, dtype=R)
    idx = np.arange(1, n_dates + 1) * spd - 1            # row of step j = d spd in the cumulative sums
    if late:
        idx = np.minimum(idx + 1, m - 1)
    x0 = np.array([math.log(s0) + r * (t * d / n_dates) for d in range(1, n_dates + 1)]).astype(R)
    x = x0[:, None] - R(0.0 if mutation == "no_half" else 0.5 * s["dt"]) * A[idx] + R(s["sdt"]) * B[idx]
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    return dict(x=f8(x), x0=f8(x0), A=f8(A), B=f8(B), S=f8(S), idx=idx)


def walk(o, model, n_dates, spd, z1, z2, anti=False, mutation=None, dtype=np.float64, late=False):
    """One dict per path direction: heston_ref's side (`base`: variance path, local errors, value at maturity) and the log prices
    at the dates, `x` of shape (n_dates, n_paths)."""
    n_dates, spd = int(n_dates), int(spd)
    m = n_dates * spd
    base = hr.walk(o, model, m, z1, z2, anti, mutation, dtype)
    sides = []
    for s in base.sides:
        d = _dates(s, o, n_dates, spd, dtype, late, mutation)
        sides.append(dict(d, base=s, n_dates=n_dates, spd=spd, o=o, xb={}))
    return sides


def european(sides):
    """The value at maturity, heston_ref's."""
    return sum(s["base"]["value"] for s in sides) / len(sides)


def asian(sides, one_more=False):
    """Per-path values of the Asian call.  one_more: the mutation that divides by n_dates + 1."""
    out = 0.0
    for s in sides:
        a = np.exp(s["x"]).sum(axis=0) / (s["n_dates"] + (1 if one_more else 0))
        out = out + np.maximum(a - float(s["o"]["k"]), 0.0)
    return out / len(sides)


def x_bounds(s, tol):
    """(Ex at the dates (n_dates, n_paths) before the date's own terms, bx (n_dates, n_paths), kink mask) of one direction."""
    if tol in s["xb"]:
        return s["xb"][tol]
    b = s["base"]
    V, ZV, Z1, locV = b["V"], b["ZV"], b["Z1"], b["locV"]
    m, n = V.shape
    kdt, dt, sdt = b["kdt"], b["dt"], b["sdt"]
    pos = V > 0
    inv = np.where(pos, 0.5 / np.sqrt(np.where(pos, V, 1.0)), 0.0)
    absJ = np.abs(1.0 - kdt * pos + ZV * inv)
    absg = np.abs(-0.5 * dt * pos + sdt * Z1 * inv)
    absV, absZV, absZ1 = np.abs(V), np.abs(ZV), np.abs(Z1)
    step_direct = 0.5 * dt * np.abs(s["A"]) + sdt * (2.0 * s["S"] * absZ1 + np.abs(s["B"]))
    E = np.full(n, tol * b["v0"])
    Ex = np.zeros(n)
    kink = np.zeros(n, dtype=bool)
    at = {int(j): d for d, j in enumerate(s["idx"])}
    ex = np.empty((s["n_dates"], n))
    for j in range(m):
        kj = absV[j] < E
        if kj.any():
            rootE = np.sqrt(E)
            dV = kdt * E + absZV[j] * rootE
            Ex = Ex + np.where(kj, 0.5 * dt * E + sdt * absZ1[j] * rootE, absg[j] * E)
            E = np.where(kj, E + dV, absJ[j] * E) + tol * locV[j]
            kink |= kj
        else:
            Ex = Ex + absg[j] * E
            E = absJ[j] * E + tol * locV[j]
        Ex = Ex + tol * step_direct[j]
        if j in at:
            ex[at[j]] = Ex
    i = s["idx"]
    common = 1.0 + 3.0 * 0.5 * dt * np.abs(s["A"][i]) + 3.0 * sdt * np.abs(s["B"][i])
    bx = ex + tol * (common + np.abs(s["x0"])[:, None] + 2.0 * np.abs(s["x"]))
    s["xb"][tol] = (ex, bx, kink, common)
    return s["xb"][tol]


def asian_bound(sides, tol):
    """Per-path bound on |kernel value - asian(sides)| for a kernel of unit roundoff tol, and the mask of the kink paths."""
    total, kink = 0.0, False
    for s in sides:
        _, bx, kk, _ = x_bounds(s, tol)
        S = np.exp(s["x"])
        nd, k = s["n_dates"], float(s["o"]["k"])
        A = S.sum(axis=0) / nd
        with np.errstate(over="ignore"):
            b = (S * np.expm1(bx)).sum(axis=0) / nd
        b = b + tol * ((2.0 * S.sum(axis=0) + np.cumsum(S, axis=0).sum(axis=0)) / nd + A + abs(k) + np.maximum(A - k, 0.0))
        total, kink = total + b, np.logical_or(kink, kk)
    value = asian(sides)
    return total / len(sides) + tol * np.abs(value), kink


def _barrier_side(s, B, up, tol):
    """Of one direction: P of the model, the mask of the near dates' paths, the payoff at maturity and its bound."""
    sgn = 1.0 if up else -1.0
    h = math.log(float(B))
    d = sgn * (h - s["x"])
    live = d.min(axis=0) > 0
    pay = s["base"]["value"]
    if tol is None:
        return live, None, pay, None, None
    ex, _, kink, common = x_bounds(s, tol)
    bd = ex + tol * (common + np.abs(h - s["x0"])[:, None] + 2.0 * np.abs(d))
    near = (np.abs(d) <= bd).any(axis=0)
    bpay, kink_m = hr._side_bound(s["base"], tol)
    return live, near, pay, bpay + 2.0 * tol * np.abs(pay), np.logical_or(kink, kink_m)


def barrier(sides, B, kind="up-and-out", up_as_down=False):
    """Per-path values of the barrier call monitored on the dates.  up_as_down: the mutation that reads the barrier's direction wrong."""
    up, knock_in = kind.startswith("up") != up_as_down, kind.endswith("in")
    c0, c1 = (1.0, -1.0) if knock_in else (0.0, 1.0)
    out = 0.0
    for s in sides:
        live, _, pay, _, _ = _barrier_side(s, B, up, None)
        out = out + (c0 + c1 * live) * pay
    return out / len(sides)


def barrier_errors(got, sides, B, kind, tol):
    """(|got - nearest admissible value| / bound per path, near mask, kink mask): a decided direction has one admissible value, a
    near direction two (knocked, not knocked); the admissible values of the path are the means over the directions."""
    up, knock_in = kind.startswith("up"), kind.endswith("in")
    c0, c1 = (1.0, -1.0) if knock_in else (0.0, 1.0)
    n = sides[0]["x"].shape[1]
    cands = [np.zeros(n)]
    bound, near_any, kink_any = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for s in sides:
        live, near, pay, bpay, kink = _barrier_side(s, B, up, tol)
        own = (c0 + c1 * live) * pay
        other = np.where(near, (c0 + c1 * ~live) * pay, own)
        cands = [c + v for c in cands for v in (own, other)]
        bound, near_any, kink_any = bound + bpay, near_any | near, kink_any | kink
    w = 1.0 / len(sides)
    got = np.asarray(got, dtype=np.float64)
    err = np.minimum.reduce([np.abs(got - w * c) for c in cands])
    value = barrier(sides, B, kind)
    return err / (w * bound + tol * np.abs(value)), near_any, kink_any


def barrier_bound(sides, B, kind, tol):
    """Per-path bound on |kernel value - barrier(sides)| that charges a near direction the whole jump between its two values (for
    sums, where `barrier_errors` does not apply), the near mask and the kink mask."""
    up = kind.startswith("up")
    n = sides[0]["x"].shape[1]
    bound, near_any, kink_any = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for s in sides:
        _, near, pay, bpay, kink = _barrier_side(s, B, up, tol)
        bound, near_any, kink_any = bound + bpay + near * pay, near_any | near, kink_any | kink
    return bound / len(sides) + tol * np.abs(barrier(sides, B, kind)), near_any, kink_any


def check_asian(got, sides, tol, what):
    """The per-path rule of the Asian payoff: every value finite, >= 0 and within asian_bound of the model's; the kink paths under
    heston_ref.KINK_CAP.  Returns (worst error / bound, number of kink paths); asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    b, kink = asian_bound(sides, tol)
    r = np.abs(got - asian(sides)) / b
    assert np.all(r <= 1.0), (what, int(np.argmax(r)), float(r.max()))
    assert kink.sum() <= hr.KINK_CAP * got.size, what
    return float(r.max()), int(kink.sum())


def check_barrier(got, sides, B, kind, tol, what):
    """The per-path rule of the barrier payoff: every value finite, >= 0 and within its bound of the nearest value the path can take
    (barrier_errors); the near paths under NEAR_CAP, the kink paths under heston_ref.KINK_CAP.  Returns (worst error / bound, number
    of near paths, number of kink paths); asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    r, near, kink = barrier_errors(got, sides, B, kind, tol)
    assert np.all(r <= 1.0), (what, kind, int(np.argmax(r)), float(r.max()))
    assert near.sum() <= NEAR_CAP * got.size and kink.sum() <= hr.KINK_CAP * got.size, (what, kind)
    return float(r.max()), int(near.sum()), int(kink.sum())


def european_bound(sides, tol):
    """heston_ref's bound of the value at maturity (n_dates = 1 Asian, knock-in + knock-out, a barrier out of reach)."""
    return hr.bound(hr.HestonPaths(european(sides).reshape(1, -1), [s["base"] for s in sides]), tol)
