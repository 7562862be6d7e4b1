"""Independent float64 reference of the single-barrier call, discrete and Brownian-bridge continuous monitoring (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_dates equally spaced dates t_j = j T / m,
    dt = T / m,  a = (r - v^2/2) dt,  bx = v sqrt(dt),  W_j = z_1 + ... + z_j,  x_j = ln S_j = ln S0 + j a + bx W_j,  x_0 = ln S0,
    d_j = sgn (ln B - x_j)  (sgn = +1 up, -1 down; natural-log units),
    discrete    P = [min_{j>=1} d_j > 0],
    continuous  P = [min_{j>=1} d_j > 0] prod_{j=1..m} (1 - exp(-2 d_{j-1} d_j / bx^2)),
    knock-out P (S_T - K)^+,  knock-in (1 - P)(S_T - K)^+,  antithetic: the mean of the value at z and at -z,
evaluated with numpy on a given array of normals.  `barrier` returns a greeks_ref.Paths (value, scale, jump, edge), each of
shape (1, n_paths) like a one-plane product of greeks_ref, so that greeks_ref.bound applies: a kernel computing the same
formulas in a precision of unit roundoff u is within a small multiple of u * scale of value.

The forward-error scale, in units of roundoff:
  - d_j carries dd_j = 1 + |sgn (ln B - ln S0 - j a)| + bx (|W_j| + sum_{i<=j} |W_i|) + |d_j| (the rounded per-date constant, the
    running sum W_j whose every partial sum is rounded -- what asian_ref charges for ln S_j -- and its own rounding); dd_0 = |d_0|;
  - S_T the relative error of its exponent, el = 1 + |ln S0| + m |a| + bx (|W_m| + sum_{i<=m} |W_i|); the subtraction |K|;
  - continuous: factor f_j = 1 - e_j, e_j = exp(-u_j), u_j = 2 d_{j-1} d_j / bx^2, has the absolute error
    df_j = e_j (2 (|d_{j-1}| dd_j + |d_j| dd_{j-1}) / bx^2 + 3 u_j) + 1   (the propagated errors of the two distances, the roundings
    of the rounded constant 2 / bx^2 and of the two products, and one rounding of the factor), and P the error
    sum_j df_j prod_{i != j} f_i + m P (one rounding per multiplication), the products of the other factors taken as prefix times
    suffix products so that a near-zero factor does not divide; the factor of a crossed interval counts as 0 there, so that a
    path just beyond the barrier still carries the error of the factor that a kernel just inside it would have;
  - value = (c0 + c1 P) payoff:  payoff dP + |c0 + c1 P| (S_T el + S_T + |K|) + |value|.
The discrete form has an indicator: `jump` is the payoff, `edge` = min_j |d_j| / dd_j, the distance of the path to the step in
units of the error of d_j.  The continuous form goes to zero continuously at the barrier (d_j -> 0 makes f_j -> 0): no jump.
`value(..., full=True)` also returns, for the discrete form's near paths, the two values a path can take: knocked or not.

Closed forms, each from first principles (the reflection principle: under the measure where ln S has drift nu = r - v^2/2, the
density of x_T on paths that stayed on the live side of h is phi(x; x0) - exp(2 nu (h - x0) / v^2) phi(x; 2h - x0), i.e. the
free price minus (B/S)^(2 nu / v^2) times the free price started at B^2/S): `reiner_rubinstein`, the one-date discrete
form `one_date_discrete`, and `black_scholes_call`.
"""
import math

import numpy as np

from greeks_ref import NPB, Paths, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_BARRIER = 5
KINDS = ["up-and-out", "up-and-in", "down-and-out", "down-and-in"]
MONITORINGS = ["discrete", "continuous"]


def barrier_normals(draw, first, n, n_dates, npb):
    """Path p is unit p of domain 5; date j (1-based) draws entry (j - 1) % npb of block (j - 1) // npb.  Shape (n, n_dates)."""
    return basket_normals(lambda _, u, c, b: draw(DOMAIN_BARRIER, u, c, b), first, n, n_dates, npb)


def _one_side(s0, k, a, bx, m, gap, sgn, continuous, W, exponent=2.0, lagged=True):
    """One path direction, from its Brownian sums W (n, m): the payoff and its error, the survival weight P and its error, the
    jump and the edge.  exponent and lagged are the mutation switches of the tests: the bridge exponent's 2, and d_{j-1} (True)
    or d_j (False)."""
    n = W.shape[0]
    j = np.arange(1, m + 1)
    W_abs = np.cumsum(np.abs(W), axis=1)
    dk = sgn * (gap - j * a)
    d = dk - sgn * bx * W
    dd = 1.0 + np.abs(dk) + bx * (np.abs(W) + W_abs) + np.abs(d)
    xT = math.log(s0) + m * a + bx * W[:, -1]
    ST = np.exp(xT)
    el = 1.0 + abs(math.log(s0)) + m * abs(a) + bx * (np.abs(W[:, -1]) + W_abs[:, -1])
    pay = np.maximum(ST - k, 0.0)
    dpay = ST * el + ST + abs(k)
    live = d.min(axis=1) > 0
    if continuous:
        d_prev = np.concatenate([np.full((n, 1), sgn * gap), d[:, :-1]], axis=1) if lagged else d
        dd_prev = np.concatenate([np.full((n, 1), abs(gap)), dd[:, :-1]], axis=1) if lagged else dd
        u = exponent * d_prev * d / (bx * bx)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-np.maximum(u, -700.0))
            # the error scale extends P continuously beyond the barrier: a factor of a crossed interval (u <= 0) is 0, with the
            # slope it has at u = 0, so a path that the model sees just beyond the barrier and the kernel just inside it (where
            # its factor is tiny, not 0) is charged that factor's error; P itself is the select
            df = np.minimum(e, 1.0) * (2.0 * (np.abs(d_prev) * dd + np.abs(d) * dd_prev) / (bx * bx) + 3.0 * np.abs(u)) + 1.0
            fl = np.clip(1.0 - e, 0.0, 1.0)
            pre = np.cumprod(fl, axis=1)
            suf = np.cumprod(fl[:, ::-1], axis=1)[:, ::-1]
            others = np.concatenate([np.ones((n, 1)), pre[:, :-1]], axis=1) * np.concatenate([suf[:, 1:], np.ones((n, 1))], axis=1)
            P = np.where(live, pre[:, -1], 0.0)
            dP = (df * others).sum(axis=1) + m * P
        jump, edge = np.zeros(n), np.full(n, np.inf)
    else:
        P = live.astype(np.float64)
        dP = np.zeros(n)
        jump, edge = pay, (np.abs(d) / dd).min(axis=1)
    return dict(pay=pay, dpay=dpay, P=P, dP=dP, jump=jump, edge=edge)


def walk(o, B, n_dates, z, up, monitoring="discrete", anti=False, exponent=2.0, lagged=True):
    """Everything about the paths on the normals z (n_paths, >= n_dates) that does not depend on knock-in or knock-out: one
    _one_side per path direction.  `value` turns it into the Paths of a barrier type."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    m = int(n_dates)
    z = np.asarray(z, dtype=np.float64)[:, :m]
    dt = t / m
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    gap = math.log(float(B)) - math.log(s0)
    W = np.cumsum(z, axis=1)
    args = (s0, k, a, bx, m, gap, 1.0 if up else -1.0, monitoring == "continuous")
    return [_one_side(*args, W, exponent, lagged)] + ([_one_side(*args, -W, exponent, lagged)] if anti else [])


def value(sides, knock_in, full=False):
    """Paths of the knock-in or knock-out call from `walk`.  full=True also returns the candidates of the discrete form: per
    path direction the two values a path can take (knocked, not knocked) and their scales, each of shape (2, n_paths)."""
    c0, c1 = (1.0, -1.0) if knock_in else (0.0, 1.0)
    w = 1.0 / len(sides)
    n = sides[0]["pay"].size
    val, scale, jump, cands = np.zeros(n), np.zeros(n), np.zeros(n), []
    for s in sides:
        v1 = (c0 + c1 * s["P"]) * s["pay"]
        val += w * v1
        scale += w * (s["pay"] * s["dP"] + np.abs(c0 + c1 * s["P"]) * s["dpay"] + np.abs(v1))
        jump += w * s["jump"]
        both = np.stack([c0 * s["pay"], (c0 + c1) * s["pay"]])
        cands.append((both, np.stack([abs(c0) * s["dpay"], abs(c0 + c1) * s["dpay"]]) + np.abs(both)))
    p = Paths(val.reshape(1, n), scale.reshape(1, n), jump.reshape(1, n), np.minimum.reduce([s["edge"] for s in sides]))
    return (p, cands) if full else p


def barrier(o, B, n_dates, z, kind="up-and-out", monitoring="discrete", anti=False, exponent=2.0, lagged=True):
    """Per-path values of the barrier call on the normals z (n_paths, >= n_dates), and their forward-error scales."""
    return value(walk(o, B, n_dates, z, kind.startswith("up"), monitoring, anti, exponent, lagged), kind.endswith("in"))


# ---- closed forms -------------------------------------------------------------------------------------------------------
def _Phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _call_above(s, k, r, v, t, lo):
    """e^{-rT} E[(S_T - K) 1{S_T > lo}] for GBM started at s (lo >= K makes it a call with a gap; lo = K the vanilla call)."""
    sd = v * math.sqrt(t)
    d1 = (math.log(s / lo) + (r + 0.5 * v * v) * t) / sd
    return s * _Phi(d1) - k * math.exp(-r * t) * _Phi(d1 - sd)


def black_scholes_call(o):
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    return _call_above(s0, k, r, v, t, k)


def _live_call(s, k, r, v, t, B, up):
    """e^{-rT} E[(S_T - K)^+ 1{S_T on the live side of B}] for GBM started at s: the terminal condition alone."""
    if up:
        return _call_above(s, k, r, v, t, k) - _call_above(s, k, r, v, t, B) if k < B else 0.0
    return _call_above(s, k, r, v, t, max(k, B))


def one_date_discrete(o, B, kind):
    """Discounted price of the call monitored at maturity only."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    out = _live_call(s0, k, r, v, t, float(B), kind.startswith("up"))
    return black_scholes_call(o) - out if kind.endswith("in") else out


def reiner_rubinstein(o, B, kind):
    """Discounted price of the continuously monitored call: the image solution.  The knock-out price is the live-side terminal
    expectation started at S0 minus (B/S0)^(2 r / v^2 - 1) times the same expectation started at the mirror point B^2/S0."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    B = float(B)
    up = kind.startswith("up")
    out = _live_call(s0, k, r, v, t, B, up) - (B / s0) ** (2.0 * r / (v * v) - 1.0) * _live_call(B * B / s0, k, r, v, t, B, up)
    return black_scholes_call(o) - out if kind.endswith("in") else out


# ---- the shapes of the GPU tests (tests/test_gpu_barrier.py), shared with the checks on the reference alone --------------------
ATM = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
# (option, barrier): up with K below B, down with K above B, down with K below B
CASES = [(ATM, 120.0), (dict(s=100.0, k=95.0, r=0.02, v=0.2, t=1.0), 85.0), (dict(s=100.0, k=80.0, r=0.03, v=0.25, t=0.5), 88.0)]
DATES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 255, 256, 257, 1000, 4096]   # the last one is MC_MAX_BARRIER_DATES
N_PATHS = 2121   # eight workgroups and a partial wave
# the many-trip GPU test (tests/test_gpu_walk_trips.py): per path against the model at the ends of the date loops (fp32 4 dates per
# trip; fp64 8, then 2), on the path counts of greeks_ref.TRIP_RANGES "A" and "C"; the same bits on every grid on "B" and "C"
TRIP_DATES = [3, 8, 17]
TRIP_BITS_DATES = [5, 9, 257]


def kinds_of(o, B):
    """The two barrier types that are valid for this spot and barrier."""
    return KINDS[:2] if B > o["s"] else KINDS[2:]
