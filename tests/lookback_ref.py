"""Independent float64 reference of the lookback options, discrete and Brownian-bridge continuous extrema (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_dates equally spaced dates t_j = j T / m,
    dt = T / m,  a = (r - v^2/2) dt,  bx = v sqrt(dt),  W_j = z_1 + ... + z_j,  x_j = ln S_j = ln S0 + j a + bx W_j,  x_0 = ln S0,
    y_j = sgn (x_j - x_0) = sgn (j a + bx W_j),  y_0 = 0   (sgn = +1: the payoff is on the maximum, -1: on the minimum),
    discrete    Y = max_{1<=j<=m} y_j,
    continuous  Y = max_{1<=j<=m} M_j,  M_j = (y_{j-1} + y_j + sqrt((y_j - y_{j-1})^2 + bx^2 E_j)) / 2,  E_j = -2 ln u_j,
    ext = S0 exp(sgn Y),  S_T = S0 exp(sgn y_m)  (= exp(x_m)),
    floating call (sgn -1) max(S_T - ext, 0),  floating put (sgn +1) max(ext - S_T, 0),
    fixed call (sgn +1) max(ext - K, 0),  fixed put (sgn -1) max(K - ext, 0),
    antithetic: the mean of the value at z and at -z, both on the same E_j,
evaluated with numpy on given arrays of normals and uniforms.  `value` returns a greeks_ref.Paths (value, scale, jump, edge),
each of shape (1, n_paths) like a one-plane product of greeks_ref, so that greeks_ref.bound applies: a kernel computing the same
formulas in a precision of unit roundoff eps is within eps * scale of value.  There is no indicator anywhere: jump = 0 and
edge = inf on every path, no path is left out and none has two admissible values.

The forward-error scale, in units of roundoff (absolute errors unless said otherwise):
  - y_j carries dy_j = |sgn j a| + bx (|W_j| + sum_{i<=j} |W_i|) + |y_j|: the rounded table value, the running sum W_j whose
    every partial sum is rounded (what asian_ref charges for ln S_j, and it covers the rounded bx), and its own rounding; dy_0 = 0;
  - the bridge term: d = y_j - y_{j-1} carries dd = dy_j + dy_{j-1} + |d|; the radicand x = d^2 + bx^2 E_j carries
    ex = 2 |d| dd + d^2 + REL_E bx^2 E_j + x  (the propagated error of d, the square's rounding, the relative error of E_j --
    the logarithm, the rounded constant in front of it and their product: REL_E = 3 -- and the fma's rounding).  The square root
    is not Lipschitz at 0 (u next to 1 in fp32, where E_j is next to 0): an absolute error e under the root moves it by at most
    min(e / (2 sqrt x), sqrt e), heston_ref's treatment of its kink.  sqrt e is not linear in the roundoff, so the scale is built
    for a GIVEN roundoff `eps` (the tolerance it will be multiplied with): in units of eps the charge is
    er = min(ex / (2 sqrt x), sqrt(ex / eps)), plus sqrt x for the root's own rounding.
    M_j carries dM_j = (dy_{j-1} + dy_j + er + sqrt x + |y_{j-1} + y_j|) / 2 + |M_j|  (the two additions' roundings);
  - Y: the maximum is 1-Lipschitz in the sup norm, so dY = max over its candidates' errors;
  - ext and S_T: the relative error of their exponents ln S0 + sgn Y and ln S0 + sgn y_m -- the exponent's terms, the rounded
    constants of the exponent's units, the propagated dY or dy_m, and the exponential itself:
    d_ext = ext (2 + 2 |ln S0| + 2 |Y| + |ln ext| + dY), d_ST likewise;
  - value = max(q (ext - R), 0), R = S_T or K: d_ext + (d_ST or |K|) + |ext - R|; max(., 0) is 1-Lipschitz; the antithetic mean
    adds its own rounding |value|.

Closed forms from first principles, for the tests: the law of the maximum of X_t = nu t + sigma W_t on [0, T], nu = r - v^2/2,
    P(max X <= y) = Phi((y - nu T)/(sigma sqrt T)) - exp(2 nu y / sigma^2) Phi((-y - nu T)/(sigma sqrt T)),  y >= 0
(the minimum is the maximum of -X), and each price D (f(0) + int f'(y) P(max > y) dy) by Gauss-Legendre panels that start at
the payoff's kink: `quadrature_price`.
"""
import math

import numpy as np

from greeks_ref import NPB, Paths, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_LOOKBACK, DOMAIN_LOOKBACK_BRIDGE = 8, 9
KINDS = ["floating-call", "floating-put", "fixed-call", "fixed-put"]
ON_MAX = {"floating-call": False, "floating-put": True, "fixed-call": True, "fixed-put": False}
MONITORINGS = ["discrete", "continuous"]
REL_E = 3.0
EPS = {"f32": 2e-6, "f64": 1e-14}   # TOL[X]["pay"] of tests/test_gpu_parity.py: the roundoff the scales are built for


# ---- the streams ----------------------------------------------------------------------------------------------------------
def u01_f32(words):
    """mc_rng.hpp u01_f32 exactly: fma((float) x, 2^-32, 2^-33) in float32.  The conversion rounds to nearest even; the product
    and the sum are exact in float64 (34 significant bits at most) and round once to float32, as the fma does.  In (0, 1]."""
    xf = np.asarray(words, dtype=np.uint32).astype(np.float32)
    return (xf.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)


def u01_f64(lo, hi):
    """mc_rng.hpp u01_f64 exactly: (((hi:lo) >> 12) + 1/2) 2^-52, 53 significant bits, strictly inside (0, 1)."""
    j = (np.asarray(hi, dtype=np.uint64) << np.uint64(20)) | (np.asarray(lo, dtype=np.uint64) >> np.uint64(12))
    return (j.astype(np.float64) + 0.5) * 2.0 ** -52


def bridge_uniforms(words, n_dates, X):
    """The dates' uniforms (n, n_dates) float64 from the raw words (n, n_blocks, 4) of domain 9, blocks 0 ... : fp32 date j
    (1-based) takes word (j-1) % 4 of block (j-1) // 4; fp64 takes words 2((j-1) % 2) and 2((j-1) % 2) + 1 of block (j-1) // 2
    as (lo, hi)."""
    w = np.asarray(words, dtype=np.uint32)
    n = w.shape[0]
    if X == "f32":
        return u01_f32(w.reshape(n, -1)[:, :n_dates]).astype(np.float64)
    p = w.reshape(n, -1, 2)
    return u01_f64(p[:, :, 0], p[:, :, 1])[:, :n_dates]


def bridge_blocks(n_dates, X):
    """How many raw blocks of domain 9 a path's n_dates uniforms take."""
    per = 4 if X == "f32" else 2
    return (n_dates + per - 1) // per


def lookback_draws(draw_normals, draw_words, first, n, n_dates, X):
    """(normals (n, n_dates), uniforms (n, n_dates)), float64.  Path p is unit p; date j (1-based) draws the normal entry
    (j - 1) % npb of block (j - 1) // npb of domain 8 and its uniform from the raw words of domain 9 (bridge_uniforms).
    draw_normals(domain, first_unit, n_units, block) -> (n_units, npb); draw_words(domain, first_unit, n_units, first_block,
    n_blocks) -> (n_units, n_blocks, 4) uint32."""
    z = basket_normals(lambda _, u, c, b: draw_normals(DOMAIN_LOOKBACK, u, c, b), first, n, n_dates, NPB[X])
    words = draw_words(DOMAIN_LOOKBACK_BRIDGE, first, n, 0, bridge_blocks(n_dates, X))
    return z, bridge_uniforms(words, n_dates, X)


# ---- the model ------------------------------------------------------------------------------------------------------------
def _one_side(s0, a, bx, m, sgn, continuous, W, W_abs, E, eps, mutation=None):
    """One path direction from its Brownian sums W (n, m), their running sums of magnitudes W_abs and the dates' E (n, m): the
    extremum, the terminal spot and their errors.  mutation: the tests' switches ("half_e", "next_bridge", "min_for_max")."""
    n = W.shape[0]
    j = np.arange(1, m + 1)
    yk = sgn * j * a
    y = yk + sgn * bx * W
    dy = np.abs(yk) + bx * (np.abs(W) + W_abs) + np.abs(y)
    pick = np.min if mutation == "min_for_max" else np.max
    if continuous:
        zero = np.zeros((n, 1))
        yp, dyp = np.concatenate([zero, y[:, :-1]], axis=1), np.concatenate([zero, dy[:, :-1]], axis=1)
        yc, dyc = y, dy
        if mutation == "next_bridge":   # the bridge between y_j and y_{j+1} (the last date's degenerates to a point)
            yp, dyp = y, dy
            yc, dyc = np.concatenate([y[:, 1:], y[:, -1:]], axis=1), np.concatenate([dy[:, 1:], dy[:, -1:]], axis=1)
        d = yc - yp
        dd = dyc + dyp + np.abs(d)
        be = bx * bx * E * (0.5 if mutation == "half_e" else 1.0)
        x = d * d + be
        root = np.sqrt(x)
        ex = 2.0 * np.abs(d) * dd + d * d + REL_E * be + x
        with np.errstate(divide="ignore", invalid="ignore"):
            er = np.minimum(np.where(x > 0, ex / (2.0 * np.where(x > 0, root, 1.0)), np.inf), np.sqrt(ex / eps))
        M = 0.5 * (yp + yc + root)
        dM = 0.5 * (dyp + dyc + er + root + np.abs(yp + yc)) + np.abs(M)
        Y, dY = pick(M, axis=1), dM.max(axis=1)
    else:
        Y, dY = pick(y, axis=1), dy.max(axis=1)
    ln0 = math.log(s0)
    yT, dyT = y[:, -1], dy[:, -1]
    ext, ST = s0 * np.exp(sgn * Y), s0 * np.exp(sgn * yT)
    d_ext = ext * (2.0 + 2.0 * abs(ln0) + 2.0 * np.abs(Y) + np.abs(ln0 + sgn * Y) + dY)
    d_ST = ST * (2.0 + 2.0 * abs(ln0) + 2.0 * np.abs(yT) + np.abs(ln0 + sgn * yT) + dyT)
    return dict(ext=ext, d_ext=d_ext, ST=ST, d_ST=d_ST, Y=Y)


def walk(o, n_dates, z, u, on_max, monitoring="discrete", anti=False, eps=EPS["f32"], mutation=None):
    """Everything about the paths on the normals z and uniforms u (n_paths, >= n_dates; u may be None for the discrete form) that
    does not depend on floating or fixed: one _one_side per path direction.  `value` turns it into the Paths of a type; the two
    types on the maximum share a walk, and so do the two on the minimum."""
    s0, r, v, t = (float(o[c]) for c in "srvt")
    m = int(n_dates)
    dt = t / m
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    continuous = monitoring == "continuous"
    args = (s0, a, bx, m, 1.0 if on_max else -1.0, continuous)
    n = np.shape(z)[0]
    rows = max(1, (1 << 17) // m)   # a block of paths at a time: the (rows, m) temporaries stay in the cache
    parts = []
    for i in range(0, n, rows):
        W = np.cumsum(np.asarray(z[i:i + rows, :m], dtype=np.float64), axis=1)
        W_abs = np.cumsum(np.abs(W), axis=1)
        E = -2.0 * np.log(np.asarray(u[i:i + rows, :m], dtype=np.float64)) if continuous else None
        parts.append([_one_side(*args, W, W_abs, E, eps, mutation)] + ([_one_side(*args, -W, W_abs, E, eps, mutation)] if anti else []))
    return [{key: np.concatenate([p[d][key] for p in parts]) for key in parts[0][d]} for d in range(len(parts[0]))]


def value(sides, kind, k):
    """Paths of one lookback type from `walk` (whose on_max must be ON_MAX[kind])."""
    q = 1.0 if ON_MAX[kind] else -1.0
    floating = kind.startswith("floating")
    n = sides[0]["ext"].size
    val, scale = np.zeros(n), np.zeros(n)
    for s in sides:
        R, dR = (s["ST"], s["d_ST"]) if floating else (float(k), abs(float(k)))
        diff = q * (s["ext"] - R)
        val += np.maximum(diff, 0.0) / len(sides)
        scale += (s["d_ext"] + dR + np.abs(diff)) / len(sides)
    if len(sides) > 1:
        scale = scale + np.abs(val)
    return Paths(val.reshape(1, n), scale.reshape(1, n), np.zeros((1, n)), np.full(n, np.inf))


def lookback(o, n_dates, z, u, kind="floating-call", monitoring="discrete", anti=False, eps=EPS["f32"], mutation=None):
    """Per-path values of the lookback option on the normals z and uniforms u, and their forward-error scales."""
    return value(walk(o, n_dates, z, u, ON_MAX[kind], monitoring, anti, eps, mutation), kind, o["k"])


def lookback_f32(o, n_dates, z, u, kind, monitoring="discrete", anti=False):
    """The same formulas in float32 numpy, operation by operation (the soundness check of the scale: a float32 evaluation must stay
    inside the bound).  z and u are float32 arrays (n, n_dates)."""
    f = np.float32
    m = int(n_dates)
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    dt = t / m
    sgn = 1.0 if ON_MAX[kind] else -1.0
    a, bx = (r - 0.5 * v * v) * dt, v * math.sqrt(dt)
    yk = (sgn * np.arange(1, m + 1) * a).astype(f)
    W = np.cumsum(np.asarray(z, dtype=f)[:, :m], axis=1, dtype=f)
    E = None
    if monitoring == "continuous":
        E = (f(-2.0) * np.log(np.asarray(u, dtype=f)[:, :m])) * f(bx * bx)
    vals = []
    for Wd in ([W, -W] if anti else [W]):
        y = (Wd * f(sgn * bx) + yk).astype(f)
        if E is not None:
            yp = np.concatenate([np.zeros((y.shape[0], 1), dtype=f), y[:, :-1]], axis=1)
            d = y - yp
            Y = (f(0.5) * ((y + yp) + np.sqrt(d * d + E))).max(axis=1)
        else:
            Y = y.max(axis=1)
        ext = f(s0) * np.exp(f(sgn) * Y)
        R = f(s0) * np.exp(f(sgn) * y[:, -1]) if kind.startswith("floating") else f(k)
        vals.append(np.maximum(f(sgn) * (ext - R), f(0)))
    return (sum(vals) / f(len(vals))).astype(f)


# ---- closed forms from first principles -----------------------------------------------------------------------------------
def _Phi(x):
    return 0.5 * np.vectorize(math.erfc)(-np.asarray(x, dtype=np.float64) / math.sqrt(2.0))


def _tail(y, nu, sig, T):
    """P(max_{[0,T]} (nu t + sig W_t) > y), y >= 0."""
    sd = sig * math.sqrt(T)
    return 1.0 - (_Phi((y - nu * T) / sd) - np.exp(2.0 * nu * y / (sig * sig)) * _Phi((-y - nu * T) / sd))


def _integral(g, lo, hi, panels=400, order=32):
    x, w = np.polynomial.legendre.leggauss(order)
    edges = np.linspace(lo, hi, panels + 1)
    half = 0.5 * (edges[1:] - edges[:-1])
    mid = 0.5 * (edges[1:] + edges[:-1])
    pts = mid[:, None] + half[:, None] * x[None, :]
    return float((g(pts) * w[None, :] * half[:, None]).sum())


def quadrature_price(o, kind):
    """Discounted price at inception of the continuously monitored lookback: D (f(0) + int f'(y) P(max > y) dy) with y the
    maximum of sgn (ln S - ln S0), the integral started at the payoff's kink."""
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    D = math.exp(-r * t)
    sgn = 1.0 if ON_MAX[kind] else -1.0
    nu = sgn * (r - 0.5 * v * v)   # the drift of sgn (ln S - ln S0)
    span = abs(nu) * t + 14.0 * v * math.sqrt(t)
    if kind.startswith("floating"):
        # E[ext] = S0 + sgn S0 int_0^inf e^{sgn y} P(max > y) dy;  E[S_T] = S0 e^{rT}
        e_ext = s0 + sgn * s0 * _integral(lambda y: np.exp(sgn * y) * _tail(y, nu, v, t), 0.0, span)
        return sgn * (D * e_ext - s0)
    y0 = max(0.0, sgn * math.log(k / s0))   # the payoff q (S0 e^{sgn y} - K) is positive beyond y0
    f0 = max(sgn * (s0 - k), 0.0)
    return D * (f0 + s0 * _integral(lambda y: np.exp(sgn * y) * _tail(y, nu, v, t), y0, y0 + span))


# ---- the shapes of the GPU tests (tests/test_gpu_lookback.py), shared with the checks on the reference alone ------------------
ATM = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
# k at, below and above the spot; one r small; one t != 1
CASES = [ATM, dict(s=100.0, k=90.0, r=0.002, v=0.3, t=1.0), dict(s=80.0, k=95.0, r=0.03, v=0.25, t=0.5)]
DATES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 255, 256, 257, 1000, 4096]   # the last one is MC_MAX_LOOKBACK_DATES
N_PATHS = 2121   # eight workgroups and a partial wave
# the many-trip GPU test (tests/test_gpu_walk_trips.py): per path against the model at the ends of the date loops (fp32 4 dates per
# trip; fp64 8, then 2), on the path counts of greeks_ref.TRIP_RANGES "A" and "C"; the same bits on every grid on "B" and "C"
TRIP_DATES = [3, 8, 17]
TRIP_BITS_DATES = [5, 9, 257]
