"""Independent float64 reference of the six Greeks estimators (not a test module).

Written from the model, not from the oracle twins (oracle/mc_oracle_impl.h): the estimators are the ones stated above
vanilla_greeks_kernel, basket_greeks_kernel and cva_greeks_kernel (csrc/mc_kernels.hpp) and in basket_greeks_run /
cva_greeks_run (csrc/mc_api.hip), evaluated in float64 with numpy on a given array of normals.

Every function returns a `Paths`: per path (rows price, delta, vega; basket: price, delta_0..n-1, vega_0..n-1)
  value  the estimator's value,
  scale  the size of the terms in play: a kernel computing the same formulas in a precision of unit roundoff u is within
         a small multiple of u * scale of `value` (forward error of the products, sums and exponentials involved),
  jump   the value's step where the estimator has an indicator (pathwise Greeks at the strike, the CVA's intrinsic date),
  edge   the distance of the path to that step in units of its own `scale` (inf where there is no step).
`bound(p, eps)` turns these into per-path bounds: eps * scale, plus the jump on paths within eps of the step, where two
correct implementations may land on opposite sides of it.

The normal-stream layout is the kernels': `vanilla_normals`, `basket_normals` and `cva_normals` build the per-product
normal arrays from a `draw(domain, first_unit, n_units, block) -> (n_units, npb)` callable (Engine.normals on the GPU,
the oracle's dev_normals on the CPU).
"""
import math
from collections import namedtuple

import numpy as np

DOMAIN_VANILLA, DOMAIN_BASKET, DOMAIN_CVA = 1, 2, 3
NPB = {"f32": 4, "f64": 8}   # normals per Philox block

Paths = namedtuple("Paths", "value scale jump edge")

INV_SQRT_2PI = 0.39894228040143267793994605993438


# ---- the normal streams ---------------------------------------------------------------------------------------------
def vanilla_normals(draw, first, n, npb):
    """Path p's normal is entry p % npb of Philox unit p // npb, block 0."""
    u0, u1 = first // npb, (first + n + npb - 1) // npb
    z = np.asarray(draw(DOMAIN_VANILLA, u0, u1 - u0, 0), dtype=np.float64).reshape(-1)
    return z[first - u0 * npb:first - u0 * npb + n]


def basket_normals(draw, first, n, n_assets, npb):
    """Path p is unit p; asset a's normal is entry a % npb of block a // npb.  Shape (n, n_assets)."""
    blocks = [np.asarray(draw(DOMAIN_BASKET, first, n, b), dtype=np.float64).reshape(n, npb) for b in range((n_assets + npb - 1) // npb)]
    return np.concatenate(blocks, axis=1)[:, :n_assets]


def cva_normals(draw, first, n, n_dates, npb):
    """Path p is unit p; date j (1-based) draws entry (j - 1) % npb of block (j - 1) // npb.  Shape (n, n_dates)."""
    return basket_normals(lambda _, u, c, b: draw(DOMAIN_CVA, u, c, b), first, n, n_dates, npb)


def bound(p, eps):
    """Per-path bounds (same shape as p.value) for a kernel of unit roundoff eps."""
    near = p.edge <= eps
    return eps * p.scale + np.where(near, p.jump, 0.0)


def kink_free(p, eps):
    """True when no path lies within eps of an indicator step (the bounds then carry no jump term)."""
    return not bool(np.any(p.edge <= eps))


def check_sums(est, got, n, what):
    """{sum, sum2, n} of a run-form call against the same call's per-path dump `got`: the kernels add (double) p and
    fma((double) p, (double) p, acc) in fp64 in some order, so |sum - S p| <= n 2^-53 S |p| and |sum2 - S p^2| <= (n + 1) 2^-53 S p^2
    (p^2 is exact inside the device's fma, rounded once on the host), with S taken exactly (math.fsum)."""
    u = 2.0 ** -53
    p = [float(x) for x in got]
    assert est.n == n, what
    assert abs(est.sum - math.fsum(p)) <= n * u * math.fsum(abs(x) for x in p), (what, est.sum, math.fsum(p))
    q = math.fsum(x * x for x in p)
    assert abs(est.sum2 - q) <= (n + 1) * u * q, (what, est.sum2, q)


# ---- path ranges on which a lane of a small engine takes several grid-stride trips (tests/test_gpu_walk_trips.py) ------------------
# A dated product launches min(ceil(n / 256), blocks * 3 / 2) workgroups of 256 lanes per segment of its range:
#   A  16 blocks (6144 lanes): three full trips, 2125 lanes take a fourth, the last wave is partial (2125 mod 64 = 13)
#   B  16 blocks, two segments around 2^32 units: the second is written at out + 7000 and runs more than two trips
#   C  1 block (256 lanes): nine full trips and a partial tenth
TripRange = namedtuple("TripRange", "blocks first n")
TRIP_RANGES = {"A": TripRange(16, 4242, 16 * 256 * 5 + 77), "B": TripRange(16, (1 << 32) - 7000, 20_000), "C": TripRange(1, 11, 256 * 9 + 77)}
TRIP_GROUP = 256


def trip_pick(cases, i, name):
    """The market of the i-th count of a family's TRIP list on range `name`: the family's cases, rotated over counts and ranges."""
    return cases[(i + "ABC".index(name)) % len(cases)]


def trip_lanes(blocks):
    """The lanes a dated product's launch is capped at on an engine of `blocks` blocks."""
    return blocks * 3 // 2 * TRIP_GROUP


def trip_guard(e, blocks, n_last):
    """After a dated product's call whose last launch priced n_last paths on the engine e of `blocks` blocks: the launch was capped
    at the engine's lanes and every lane ran at least two full trips (Engine.last_launch), so that a changed grid rule fails the test
    instead of turning it back into a one-trip test.  Returns the number of full trips."""
    grid, group = e.last_launch()
    assert e.blocks == blocks and grid * group == trip_lanes(blocks) and grid * group * 2 <= n_last, (blocks, grid, group, n_last)
    return n_last // (grid * group)


def trip_last_segment(r):
    """Paths of the last launch of range r: the part of it beyond the next multiple of 2^32 units, or all of it."""
    room = (1 << 32) - (r.first & ((1 << 32) - 1))
    return r.n if r.n <= room else r.n - room


# ---- vanilla call -----------------------------------------------------------------------------------------------------
def vanilla(o, z, lr=False):
    """S_T = S exp((r - v^2/2) T + v sqrt(T) z), payoff (S_T - K)^+.
    Pathwise: delta = I S_T / S, vega = I S_T (sqrt(T) z - v T).
    Likelihood ratio: delta = payoff z / (S v sqrt T), vega = payoff ((z^2 - 1) / v - z sqrt T)."""
    s, k, r, v, t = (float(o[c]) for c in "skrvt")
    z = np.asarray(z, dtype=np.float64)
    sqt = math.sqrt(t)
    x = (r - 0.5 * v * v) * t + v * sqt * z
    st = s * np.exp(x)
    itm = st > k
    pay = np.where(itm, st - k, 0.0)
    ex = 1.0 + np.abs(x) + abs((r - 0.5 * v * v) * t) + v * sqt * np.abs(z)   # relative error of S_T, in units of eps
    s_pay = st * ex + abs(k)
    n = z.size
    value, scale = np.zeros((3, n)), np.zeros((3, n))
    jump, edge = np.zeros((3, n)), np.full(n, np.inf)
    value[0], scale[0] = pay, s_pay
    if lr:
        sc_d = z / (s * v * sqt)
        sc_v = (z * z - 1.0) / v - z * sqt
        value[1], value[2] = pay * sc_d, pay * sc_v
        scale[1] = s_pay * np.abs(sc_d)
        scale[2] = s_pay * ((z * z + 1.0) / v + np.abs(z) * sqt)
    else:
        dl = st / s
        vg = st * (sqt * z - v * t)
        value[1], value[2] = np.where(itm, dl, 0.0), np.where(itm, vg, 0.0)
        scale[1] = dl * ex
        scale[2] = st * ex * (sqt * np.abs(z) + v * t)
        jump[1], jump[2] = np.abs(dl), np.abs(vg)
        edge = np.abs(st - k) / s_pay
    return Paths(value, scale, jump, edge)


# ---- basket call ------------------------------------------------------------------------------------------------------
def basket(b, g, lr=False):
    """bt = L g + d,  s_a = S_a exp((r - v_a^2/2) T + v_a sqrt(T) bt_a),  B = sum_a w_a s_a,  payoff (B - K)^+.
    Pathwise: delta_a = I w_a s_a / S_a,  vega_a = I w_a s_a (bt_a sqrt T - v_a T).
    Likelihood ratio (x = ln S(T) ~ N(m, T D L L' D), D = diag(v), y = L^-T g):
        delta_a = payoff y_a / (S_a v_a sqrt T),
        vega_a  = payoff [ (y_a (L g)_a - 1) / v_a + (sqrt T d_a - v_a T) y_a / (v_a sqrt T) ].
    g has shape (n_paths, n_assets); only the lower triangle of the factor is used (as the kernels do)."""
    S, v, d, w = (np.asarray(b[c], dtype=np.float64) for c in "svdw")
    L = np.tril(np.asarray(b["p"], dtype=np.float64).reshape(len(S), len(S)))
    k, t, r = float(b["k"]), float(b["t"]), float(b["r"])
    g = np.asarray(g, dtype=np.float64)
    n, na = g.shape
    sqt = math.sqrt(t)
    lg = g @ L.T                                    # (L g)_a per path
    lg_abs = np.abs(g) @ np.abs(L).T                # its rounding scale
    bt = lg + d
    mu = (r - 0.5 * v * v) * t
    x = mu + v * sqt * bt
    term = w * S * np.exp(x)
    ex = 1.0 + np.abs(x) + np.abs(mu) + v * sqt * (lg_abs + np.abs(d))  # relative error of each term, in units of eps
    B = term.sum(axis=1)
    itm = B > k
    pay = np.where(itm, B - k, 0.0)
    s_pay = (np.abs(term) * ex).sum(axis=1) + abs(k)
    value, scale = np.zeros((1 + 2 * na, n)), np.zeros((1 + 2 * na, n))
    jump, edge = np.zeros((1 + 2 * na, n)), np.full(n, np.inf)
    value[0], scale[0] = pay, s_pay
    if lr:
        Lt_inv = np.linalg.inv(L).T                   # L^-T (upper triangular)
        y = np.linalg.solve(L.T, g.T).T               # y = L^-T g per path
        y_abs = np.abs(g) @ np.abs(Lt_inv).T
        sd = y / (S * v * sqt)
        mcoef = (sqt * d - v * t) / (v * sqt)
        sv = (y * lg - 1.0) / v + mcoef * y
        value[1:1 + na] = (pay[:, None] * sd).T
        value[1 + na:] = (pay[:, None] * sv).T
        scale[1:1 + na] = (s_pay[:, None] * np.abs(sd) + pay[:, None] * y_abs / (S * v * sqt)).T
        sv_abs = (np.abs(y * lg) + 1.0) / v + np.abs(mcoef * y)
        sv_err = (y_abs * np.abs(lg) + np.abs(y) * lg_abs) / v + np.abs(mcoef) * y_abs
        scale[1 + na:] = (s_pay[:, None] * sv_abs + pay[:, None] * sv_err).T
    else:
        dl = term / S
        vg = term * (bt * sqt - v * t)
        value[1:1 + na] = np.where(itm[:, None], dl, 0.0).T
        value[1 + na:] = np.where(itm[:, None], vg, 0.0).T
        scale[1:1 + na] = (dl * ex).T
        scale[1 + na:] = (np.abs(term) * ex * (np.abs(bt) * sqt + v * t) + np.abs(term) * (lg_abs + np.abs(d)) * sqt).T
        jump[1:1 + na], jump[1 + na:] = np.abs(dl).T, np.abs(vg).T
        edge = np.abs(B - k) / s_pay
    return Paths(value, scale, jump, edge)


# ---- CVA of one call --------------------------------------------------------------------------------------------------
def cnd(d):
    """The reference's Hastings approximation of the normal CDF (double_precision/MonteCarloKernel.cu, cnd)."""
    d = np.asarray(d, dtype=np.float64)
    K = 1.0 / (1.0 + 0.2316419 * np.abs(d))
    c = INV_SQRT_2PI * np.exp(-0.5 * d * d) * (K * (0.31938153 + K * (-0.356563782 + K * (1.781477937 + K * (-1.821255978 + K * 1.330274429)))))
    return np.where(d > 0, 1.0 - c, c)


def cva_dates(c, X="f64"):
    """The exposure dates of a CVA call: (t_j, tau_j, dp_j) for j = 1, 2, ..., with the reference's rule for the residual
    maturity (tau -= dt in the simulation type; a date with tau < 0 ends the schedule, one with tau == 0 is the last and is
    priced at intrinsic value).  dt = T / n_grid in the simulation type."""
    R = np.float32 if X == "f32" else np.float64
    dt = R(c["t"]) / R(c["n_grid"])
    tau = R(c["t"])
    lam = float(c["defint"])
    ts, taus, dps = [], [], []
    for j in range(1, int(c["n_grid"]) + 1):
        tau = R(tau - dt)
        if not tau >= 0:
            break
        t_prev, t_now = float(dt) * (j - 1), float(dt) * j
        ts.append(t_now)
        taus.append(float(tau))
        dps.append(math.exp(-lam * t_prev) - math.exp(-lam * t_now))
        if tau == 0:
            break
    return float(dt), np.array(ts), np.array(taus), np.array(dps)


def cva(c, z, X="f64", lr=False):
    """CVA = LGD sum_j dp_j C_j,  S_j = S_0 exp(j (r - v^2/2) dt + v sqrt(dt) W_j),  W_j = z_1 + ... + z_j,
    C_j = S_j cnd(d1_j) - K e^{-r tau_j} cnd(d2_j) with the Hastings cnd, (S_j - K)^+ on a date with tau_j = 0.
    Pathwise:  delta = LGD sum_j dp_j Delta_j S_j / S_0,  Delta_j = cnd(d1_j)  (I[S_j > K] at tau_j = 0),
               vega  = LGD sum_j dp_j [ S_j phi(d1_j) sqrt(tau_j) + S_j Delta_j (W_j sqrt(dt) - v t_j) ].
    Likelihood ratio:  delta = CVA z_1 / (S_0 v sqrt(dt)),
               vega  = LGD sum_j dp_j S_j phi(d1_j) sqrt(tau_j) + CVA sum_j ((z_j^2 - 1) / v - z_j sqrt(dt)).
    z has shape (n_paths, >= number of dates); X picks the date schedule's arithmetic (cva_dates)."""
    s0, k, r, v = (float(c[q]) for q in "skrv")
    lgd = float(c["lgd"])
    dt, tj, tau, dp = cva_dates(c, X)
    nd = tj.size
    z = np.asarray(z, dtype=np.float64)[:, :nd]
    n = z.shape[0]
    sdt = math.sqrt(dt)
    a = (r - 0.5 * v * v) * dt
    W = np.cumsum(z, axis=1)
    W_abs = np.cumsum(np.abs(W), axis=1)           # rounding scale of the running sum
    j = np.arange(1, nd + 1)
    lns = math.log(s0) + j * a + v * sdt * W
    S = np.exp(lns)
    bs = tau > 0
    sig = v * np.sqrt(np.where(bs, tau, 1.0))
    d1 = (lns - math.log(k) + (r + 0.5 * v * v) * np.where(bs, tau, 0.0)) / sig
    d2 = d1 - sig
    disc = k * np.exp(-r * tau)
    A = INV_SQRT_2PI * np.exp(lns - 0.5 * d1 * d1)   # S_j phi(d1_j)
    itm = S > k
    ee = np.where(bs, S * cnd(d1) - disc * cnd(d2), np.where(itm, S - k, 0.0))
    delta_j = np.where(bs, cnd(d1), np.where(itm, 1.0, 0.0))
    A = np.where(bs, A, 0.0)
    # forward-error scales in units of eps: el of ln S_j (the rounded table row plus the running sum's rounding), ed of d1
    # and d2, eA of A = S_j phi(d1_j) (the one exponential both Hastings terms share, as K e^{-r tau} phi(d2) = S phi(d1))
    el = 1.0 + abs(math.log(s0)) + j * abs(a) + v * sdt * (np.abs(W) + W_abs)
    ed = np.where(bs, 1.0 + np.abs(d1) + v * sdt * (np.abs(W) + W_abs) / sig, 0.0)
    eA = el + d1 * d1 + np.abs(d1) * ed
    s_ee = S * el + disc + np.where(bs, 3.0 * A * (1.0 + eA), k)
    cva_p = lgd * (ee * dp).sum(axis=1)
    s_cva = abs(lgd) * ((s_ee * dp).sum(axis=1) + np.cumsum(np.abs(ee * dp), axis=1).sum(axis=1))   # + the running sum's rounding
    value, scale = np.zeros((3, n)), np.zeros((3, n))
    jump, edge = np.zeros((3, n)), np.full(n, np.inf)
    value[0], scale[0] = cva_p, s_cva
    sqrt_tau = np.sqrt(tau)
    vega_cf = lgd * (dp * A * sqrt_tau).sum(axis=1)
    s_vega_cf = abs(lgd) * ((dp * A * sqrt_tau * (1.0 + eA)).sum(axis=1) + np.cumsum(dp * A * sqrt_tau, axis=1).sum(axis=1))
    if lr:
        score = ((z * z - 1.0) / v - z * sdt).sum(axis=1)
        score_abs = ((z * z + 1.0) / v + np.abs(z) * sdt).sum(axis=1) + np.abs(np.cumsum((z * z - 1.0) / v - z * sdt, axis=1)).sum(axis=1)
        value[1] = cva_p * z[:, 0] / (s0 * v * sdt)
        scale[1] = s_cva * np.abs(z[:, 0]) / (s0 * v * sdt)
        value[2] = vega_cf + cva_p * score
        scale[2] = s_vega_cf + s_cva * score_abs
    else:
        path = W * sdt - v * tj
        value[1] = lgd * (dp * delta_j * S).sum(axis=1) / s0
        scale[1] = abs(lgd) * ((dp * (S * el + A * ed)).sum(axis=1) + np.cumsum(dp * S * delta_j, axis=1).sum(axis=1)) / s0
        value[2] = vega_cf + lgd * (dp * S * delta_j * path).sum(axis=1)
        dv = dp * S * delta_j * path
        scale[2] = s_vega_cf + abs(lgd) * ((dp * (S * el + A * ed) * (np.abs(W) * sdt + v * tj + W_abs * sdt)).sum(axis=1)
                                           + np.abs(np.cumsum(dv, axis=1)).sum(axis=1))
        if nd and not bs[-1]:   # the intrinsic date's indicator
            jump[1] = abs(lgd) * dp[-1] * S[:, -1] / s0
            jump[2] = abs(lgd) * dp[-1] * S[:, -1] * np.abs(path[:, -1])
            edge = np.abs(S[:, -1] - k) / (S[:, -1] * el[:, -1] + k)
    return Paths(value, scale, jump, edge)


def cnd_slope_ratio(d):
    """cnd'(d) / phi(d) of the Hastings cnd, in closed form (1 for the true normal CDF).  cnd is symmetric about its step at
    0, so cnd'(d) = -c'(|d|) with c the tail term phi(x) P(k), k = 1 / (1 + 0.2316419 x)."""
    x = np.abs(np.asarray(d, dtype=np.float64))
    K = 1.0 / (1.0 + 0.2316419 * x)
    P = K * (0.31938153 + K * (-0.356563782 + K * (1.781477937 + K * (-1.821255978 + K * 1.330274429))))
    dP = 0.31938153 + K * (2 * -0.356563782 + K * (3 * 1.781477937 + K * (4 * -1.821255978 + K * 5 * 1.330274429)))
    return x * P + 0.2316419 * K * K * dP


def cnd_prime(d):
    d = np.asarray(d, dtype=np.float64)
    return INV_SQRT_2PI * np.exp(-0.5 * d * d) * cnd_slope_ratio(d)


# sup_d |cnd'(d) - phi(d)|: the Hastings cnd is not the integral of phi, so its call price's derivatives are not the
# Black-Scholes ones the pathwise CVA estimator uses (test_greeks_ref.py checks this constant on a grid).  The cnd itself
# also steps by |1 - 2 c(0)| ~ 1e-9 at d = 0: a difference quotient whose step moves a d1 or d2 across 0 is not a slope.
HASTINGS_SLOPE_GAP = 2.6e-6   # 2.563e-6, at d = 0


def cva_hastings_gap(c, z, X="f64"):
    """Per-path bounds on |d CVA_H / d S_0 - pathwise delta| and |d CVA_H / d sigma - pathwise vega|, CVA_H being this
    module's own price (value[0] of `cva`).  On a closed-form date, with rho = cnd' / phi (cnd_slope_ratio), s = v sqrt(tau_j)
    and K e^{-r tau} phi(d2) = S phi(d1) = A:
        d C / d S     - cnd(d1)              = phi(d1) (rho(d1) - rho(d2)) / s
        d C / d sigma - S phi(d1) sqrt(tau)  = A sqrt(tau) ((rho(d2) - 1) d1 - (rho(d1) - 1) d2) / s
    (both vanish for the true normal CDF, rho = 1; |rho - 1| phi <= HASTINGS_SLOPE_GAP).  The intrinsic date has no gap.
    Returns (delta_gap, vega_gap): LGD sum_j dp_j |...| with the chain factors S_j / S_0 and d S_j / d sigma."""
    s0, k, r, v = (float(c[q]) for q in "skrv")
    lgd = abs(float(c["lgd"]))
    dt, tj, tau, dp = cva_dates(c, X)
    nd = tj.size
    z = np.asarray(z, dtype=np.float64)[:, :nd]
    sdt = math.sqrt(dt)
    W = np.cumsum(z, axis=1)
    lns = math.log(s0) + np.arange(1, nd + 1) * (r - 0.5 * v * v) * dt + v * sdt * W
    bs = tau > 0
    sig = v * np.sqrt(np.where(bs, tau, 1.0))
    d1 = (lns - math.log(k) + (r + 0.5 * v * v) * np.where(bs, tau, 0.0)) / sig
    d2 = d1 - sig
    A = np.where(bs, INV_SQRT_2PI * np.exp(lns - 0.5 * d1 * d1), 0.0)
    r1, r2 = cnd_slope_ratio(d1), cnd_slope_ratio(d2)
    gd = A * np.abs(r1 - r2) / sig                               # S_j times the delta gap
    gv = A * np.sqrt(tau) * np.abs((r2 - 1.0) * d1 - (r1 - 1.0) * d2) / sig
    path = np.abs(W * sdt - v * tj)
    return lgd * (dp * gd).sum(axis=1) / s0, lgd * (dp * (gv + gd * path)).sum(axis=1)


def cva_sides(c, z, X="f64"):
    """Per path and date: which side of 0 d1 (bit 0) and d2 (bit 1) lie on, and on the intrinsic date which side of K the
    spot (bit 2).  A difference quotient is a slope only on paths whose pattern the step does not change."""
    s0, k, r, v = (float(c[q]) for q in "skrv")
    dt, tj, tau, _ = cva_dates(c, X)
    nd = tj.size
    W = np.cumsum(np.asarray(z, dtype=np.float64)[:, :nd], axis=1)
    lns = math.log(s0) + np.arange(1, nd + 1) * (r - 0.5 * v * v) * dt + v * math.sqrt(dt) * W
    bs = tau > 0
    sig = v * np.sqrt(np.where(bs, tau, 1.0))
    d1 = (lns - math.log(k) + (r + 0.5 * v * v) * np.where(bs, tau, 0.0)) / sig
    return np.where(bs, (d1 > 0) * 1 + (d1 - sig > 0) * 2, (lns > math.log(k)) * 4)


# ---- random asymmetric markets (the tests' inputs) --------------------------------------------------------------------
def random_vanilla(rng):
    s = float(rng.uniform(20, 300))
    return dict(s=s, k=s * float(rng.choice([0.2, 0.6, 0.9, 1.0, 1.15, 1.6])), r=float(rng.uniform(-0.02, 0.08)),
                v=float(rng.uniform(0.05, 0.8)), t=float(rng.uniform(0.05, 2.0)))


def random_basket(rng, n_assets, chol):
    """Distinct spots 20..300, vols 0.05..0.8, d in +-0.05, unequal weights with one zero, a random correlation factored by
    `chol` (the product's mc.chol), a strike from deep in to deep out of the money."""
    S = rng.uniform(20, 300, n_assets)
    v = rng.uniform(0.05, 0.8, n_assets)
    d = rng.uniform(-0.05, 0.05, n_assets)
    w = rng.uniform(0.2, 1.5, n_assets)
    if n_assets > 1:
        w[rng.integers(n_assets)] = 0.0
    w /= w.sum()
    A = rng.normal(size=(n_assets, n_assets + 2))
    C = A @ A.T
    C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
    L, bad = chol(C)
    assert bad == 0
    return dict(s=S.tolist(), v=v.tolist(), p=np.asarray(L, dtype=np.float64).tolist(), d=d.tolist(), w=w.tolist(),
                k=float(w @ S) * float(rng.choice([0.3, 0.8, 1.0, 1.1, 1.5])), t=float(rng.uniform(0.1, 1.5)), r=float(rng.uniform(-0.01, 0.06)))


def random_cva(rng, n_grid=None):
    s = float(rng.uniform(20, 300))
    return dict(s=s, k=s * float(rng.choice([0.3, 0.9, 1.0, 1.2, 2.0])), r=float(rng.uniform(-0.01, 0.08)), v=float(rng.uniform(0.05, 0.8)),
                t=float(rng.uniform(0.1, 3.0)), defint=float(rng.uniform(0.0, 0.1)), lgd=float(rng.uniform(0.1, 1.0)),
                n_grid=int(rng.integers(1, 301)) if n_grid is None else n_grid)
