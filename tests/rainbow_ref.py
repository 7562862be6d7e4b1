"""Independent float64 reference of the worst-of / best-of options on a correlated basket walked over dates (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: n assets, m = n_dates equally spaced dates,
    dt = t/m,  a_i = (r - v_i^2/2) dt,  M = diag(v_i sqrt(dt)) L (lower triangle),  W_k(j) = z_{1,k} + ... + z_{j,k},
    y_i(j) = ln(w_i s_i) + j a_i + sum_{k<=i} M_ik W_k(j),
    e = -1 (min types) or +1 (max types):  Y(j) = max_i e y_i(j),  X_j = exp(e Y(j)),  payoff = max(q (X_m - K), 0), q = +1 call, -1 put,
    barrier on the same extremum, dates 1 ... m:  d_j = b (ln B - e Y(j)), b = +1 up, -1 down,  P = [min_j d_j > 0],
    value = (c0 + c1 P) payoff, (c0, c1) = (0, 1) knock-out, (1, -1) knock-in, (1, 0) no barrier;  antithetic: the mean at z and -z,
evaluated with numpy on a given array of normals z of shape (n_paths, n_dates, n_assets).  `rainbow` returns a greeks_ref.Paths
(value, scale, jump, edge), each of shape (1, n_paths), so that greeks_ref.bound applies.

Stream: path p is unit p of domain 14; the normal of date j (1-based) and factor k (0-based) is FLAT entry (j - 1) n + k of the
Asian layout: entry % npb of block entry // npb (`rainbow_normals`).

The forward-error scale, in units of roundoff:
  - y_i(j) carries dy = 1 + |ln(w_i s_i) + j a_i| + sum_k |M_ik| (|W_k(j)| + sum_{l<=j} |W_k(l)|) + |y_i(j)|  (the rounded per-date
    constant, the running sums whose every partial sum is rounded, and its own rounding);
  - the extremum takes the charge of the asset that attains it, or the largest among the assets within their bounds of it (at the
    weaker, fp32 tolerance `NEAR`);
  - d_j carries dd_j = 1 + |ln B| + dY(j) + |d_j|;  `edge` = min_j |d_j| / dd_j,  `jump` = the payoff;
  - X_m the relative error dY(m) of its exponent; the subtraction |K|:  dpay = X_m dY(m) + X_m + |K|;
  - value = (c0 + c1 P) payoff:  |c0 + c1 P| dpay + |value|.
`value(..., full=True)` also returns per path direction the two values a near path may take: knocked or not.

Closed checks, each from first principles: `binorm` (the bivariate normal distribution function as a one-dimensional integral),
`stulz` and `margrabe` on top of it, `black_scholes`, and `one_factor`: the exact European price at any n under a one-factor
correlation rho_ij = beta_i beta_j, by conditioning on the common factor (the assets are then independent lognormals with
distribution functions F_i(x | y)) and integrating int_K^inf (1 - prod_i F_i) dx for the call on the maximum,
int_K^inf prod_i (1 - F_i) dx for the call on the minimum, the puts over (0, K): Gauss-Legendre inside, Gauss-Hermite outside.
"""
import math

import numpy as np

from greeks_ref import NPB, Paths   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_RAINBOW = 14
KINDS = ["call-on-min", "call-on-max", "put-on-min", "put-on-max"]
BARRIER_KINDS = ["up-and-out", "up-and-in", "down-and-out", "down-and-in"]
NEAR = 2e-6   # TOL["f32"]["pay"] of tests/test_gpu_parity.py: which assets count as tied for the extremum


def rainbow_normals(draw, first, n, n_assets, n_dates, npb):
    """Path p is unit p of domain 14; date j (1-based), factor k draws flat entry (j - 1) n_assets + k.  Shape (n, n_dates, n_assets)."""
    total = n_assets * n_dates
    blocks = [np.asarray(draw(DOMAIN_RAINBOW, first, n, b), dtype=np.float64).reshape(n, npb) for b in range((total + npb - 1) // npb)]
    return np.concatenate(blocks, axis=1)[:, :total].reshape(n, n_dates, n_assets)


def fold(b, n_dates):
    """(ln(w_i s_i), a_i, M) of the basket b on n_dates dates."""
    s, v, w = (np.asarray(b[c], dtype=np.float64) for c in "svw")
    n = s.size
    L = np.tril(np.asarray(b["p"], dtype=np.float64).reshape(n, n))
    dt = float(b["t"]) / n_dates
    return np.log(w * s), (float(b["r"]) - 0.5 * v * v) * dt, (v * math.sqrt(dt))[:, None] * L


def _one_side(b, m, e, q, W, W_abs, ln_b, up, mutate):
    """One path direction from its running sums W (N, m, n): payoff and its error, P, the jump and the edge."""
    ln_s, a, M = fold(b, m)
    if mutate == "transpose":
        M = M.T
    j = np.arange(0 if mutate == "zero-based" else 1, m + (0 if mutate == "zero-based" else 1), dtype=np.float64)
    c = ln_s[None, :] + j[:, None] * a[None, :]                     # (m, n)
    y = c[None] + W @ M.T                                           # (N, m, n)
    dy = 1.0 + np.abs(c)[None] + (np.abs(W) + W_abs) @ np.abs(M).T + np.abs(y)
    u = e * y
    Y = u.max(axis=2)
    d_top = np.take_along_axis(dy, u.argmax(axis=2)[..., None], axis=2)
    dY = np.where(u >= Y[..., None] - NEAR * (dy + d_top), dy, 0.0).max(axis=2)   # (N, m)
    X = np.exp(e * Y[:, -1])
    pay = np.maximum(q * (X - float(b["k"])), 0.0)
    dpay = X * dY[:, -1] + X + abs(float(b["k"]))
    N = W.shape[0]
    if ln_b is None:
        return dict(pay=pay, dpay=dpay, P=np.zeros(N), jump=np.zeros(N), edge=np.full(N, np.inf))
    sgn = 1.0 if up else -1.0
    d = sgn * (ln_b - e * Y)
    dd = 1.0 + abs(ln_b) + dY + np.abs(d)
    if mutate == "late":   # the barrier tested one date late: date j sees the level of date j - 1, the first one the initial level
        d0 = sgn * (ln_b - (e * ln_s).max())
        d, dd = np.concatenate([np.full((N, 1), d0), d[:, :-1]], axis=1), np.concatenate([np.full((N, 1), 1.0), dd[:, :-1]], axis=1)
    return dict(pay=pay, dpay=dpay, P=(d.min(axis=1) > 0).astype(np.float64), jump=pay, edge=(np.abs(d) / dd).min(axis=1))


def walk(b, n_dates, z, kind, barrier=None, up=None, anti=False, mutate=None):
    """Everything about the paths on the normals z (n_paths, >= n_dates, n_assets) that does not depend on knock-in or knock-out:
    one _one_side per path direction.  `value` turns it into the Paths of a barrier choice."""
    m = int(n_dates)
    z = np.asarray(z, dtype=np.float64)[:, :m, :]
    e, q = (1.0 if kind.endswith("max") else -1.0), (1.0 if kind.startswith("call") else -1.0)
    W = np.cumsum(z, axis=1)
    W_abs = np.cumsum(np.abs(W), axis=1)
    ln_b = None if barrier is None else math.log(float(barrier))
    return [_one_side(b, m, e, q, sign * W, W_abs, ln_b, up, mutate) for sign in ((1.0, -1.0) if anti else (1.0,))]


def value(sides, barrier_kind=None, full=False):
    """Paths of the contract from `walk`: barrier_kind None, or one of BARRIER_KINDS (its direction was given to `walk`).
    full=True also returns per path direction the two values a path can take (knocked, not knocked) and their scales, (2, n_paths)."""
    c0, c1 = (1.0, 0.0) if barrier_kind is None else (1.0, -1.0) if barrier_kind.endswith("in") else (0.0, 1.0)
    w = 1.0 / len(sides)
    n = sides[0]["pay"].size
    val, scale, jump, cands = np.zeros(n), np.zeros(n), np.zeros(n), []
    for s in sides:
        v1 = (c0 + c1 * s["P"]) * s["pay"]
        val += w * v1
        scale += w * (np.abs(c0 + c1 * s["P"]) * s["dpay"] + np.abs(v1))
        jump += w * (s["jump"] if c1 else 0.0)
        both = np.stack([c0 * s["pay"], (c0 + c1) * s["pay"]])
        cands.append((both, np.stack([abs(c0) * s["dpay"], abs(c0 + c1) * s["dpay"]]) + np.abs(both)))
    edge = np.minimum.reduce([s["edge"] for s in sides]) if c1 else np.full(n, np.inf)
    p = Paths(val.reshape(1, n), scale.reshape(1, n), jump.reshape(1, n), edge)
    return (p, cands) if full else p


def rainbow(b, n_dates, z, kind="put-on-min", barrier=None, barrier_kind=None, anti=False, mutate=None, full=False):
    """Per-path values of the contract on the normals z (n_paths, >= n_dates, n_assets), and their forward-error scales."""
    up = None if barrier_kind is None else barrier_kind.startswith("up")
    return value(walk(b, n_dates, z, kind, barrier, up, anti, mutate), barrier_kind, full)


# ---- closed forms -------------------------------------------------------------------------------------------------------
_GL16 = np.polynomial.legendre.leggauss(16)


def _Phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


_vPhi = np.vectorize(_Phi)


def binorm(a, b, rho, panels=600):
    """P(X <= a, Y <= b), corr rho, |rho| < 1:  int_{-inf}^{a} phi(x) Phi((b - rho x) / sqrt(1 - rho^2)) dx, composite Gauss-Legendre."""
    lo = min(a, -12.0) - 1.0
    edges = np.linspace(lo, a, panels + 1)
    mid, half = 0.5 * (edges[1:] + edges[:-1]), 0.5 * (edges[1:] - edges[:-1])
    x = mid[:, None] + half[:, None] * _GL16[0][None, :]
    f = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) * _vPhi((b - rho * x) / math.sqrt(1.0 - rho * rho))
    return float((f * _GL16[1][None, :] * half[:, None]).sum())


def levels(b):
    """(S_i = w_i s_i, v_i, K, r, t, correlation matrix) of the basket."""
    s, v, w = (np.asarray(b[c], dtype=np.float64) for c in "svw")
    L = np.tril(np.asarray(b["p"], dtype=np.float64).reshape(s.size, s.size))
    return w * s, v, float(b["k"]), float(b["r"]), float(b["t"]), L @ L.T


def black_scholes(S, k, r, v, t, call=True):
    sd = v * math.sqrt(t)
    d1 = (math.log(S / k) + (r + 0.5 * v * v) * t) / sd
    c = S * _Phi(d1) - k * math.exp(-r * t) * _Phi(d1 - sd)
    return c if call else c - S + k * math.exp(-r * t)


def margrabe(S1, S2, v1, v2, rho, t):
    """PV of max(S_1(T) - S_2(T), 0), no dividends."""
    sg = math.sqrt(v1 * v1 + v2 * v2 - 2.0 * rho * v1 * v2) * math.sqrt(t)
    d = (math.log(S1 / S2) + 0.5 * sg * sg) / sg
    return S1 * _Phi(d) - S2 * _Phi(d - sg)


def stulz(b, kind, M2=binorm):
    """Discounted price of the two-asset contract without a barrier; M2 the bivariate normal distribution function."""
    S, v, k, r, t, corr = levels(b)
    rho, st = corr[1, 0] / math.sqrt(corr[0, 0] * corr[1, 1]), math.sqrt(t)
    sg = math.sqrt(v[0] ** 2 + v[1] ** 2 - 2.0 * rho * v[0] * v[1])
    y = [(math.log(S[i] / k) + (r + 0.5 * v[i] ** 2) * t) / (v[i] * st) for i in range(2)]
    d = (math.log(S[0] / S[1]) + 0.5 * sg * sg * t) / (sg * st)
    rho1, rho2 = (v[0] - rho * v[1]) / sg, (v[1] - rho * v[0]) / sg
    kd = k * math.exp(-r * t)
    cmin = S[0] * M2(y[0], -d, -rho1) + S[1] * M2(y[1], d - sg * st, -rho2) - kd * M2(y[0] - v[0] * st, y[1] - v[1] * st, rho)
    ex = margrabe(S[0], S[1], v[0], v[1], rho, t)
    if kind.endswith("max"):
        c, pv = black_scholes(S[0], k, r, v[0], t) + black_scholes(S[1], k, r, v[1], t) - cmin, S[1] + ex
    else:
        c, pv = cmin, S[0] - ex
    return c if kind.startswith("call") else c - pv + kd


def one_factor(b, beta, kind, hermite=96, panels=96):
    """Exact discounted European price (no barrier) of the basket whose correlation is rho_ij = beta_i beta_j (unit diagonal)."""
    S, v, k, r, t, _ = levels(b)
    beta = np.asarray(beta, dtype=np.float64)
    yy, wy = np.polynomial.hermite_e.hermegauss(hermite)
    wy = wy / math.sqrt(2.0 * math.pi)
    sd = v * math.sqrt(t)
    mu = np.log(S)[None, :] + (r - 0.5 * v * v)[None, :] * t + (sd * beta)[None, :] * yy[:, None]   # (H, n)
    sig = sd * np.sqrt(1.0 - beta * beta)
    lk = math.log(k)
    lo, hi = (lk, max(lk, float((mu + 12.0 * sig[None, :]).max())) + 1.0) if kind.startswith("call") else (min(lk, float((mu - 12.0 * sig[None, :]).min())) - 1.0, lk)
    edges = np.linspace(lo, hi, panels + 1)
    mid, half = 0.5 * (edges[1:] + edges[:-1]), 0.5 * (edges[1:] - edges[:-1])
    u = (mid[:, None] + half[:, None] * _GL16[0][None, :]).reshape(-1)                  # ln x
    wu = (half[:, None] * _GL16[1][None, :]).reshape(-1) * np.exp(u)                   # dx = e^u du
    F = _vPhi((u[None, :, None] - mu[:, None, :]) / sig[None, None, :])                 # (H, U, n)
    all_below, all_above = F.prod(axis=2), (1.0 - F).prod(axis=2)
    g = {"call-on-max": 1.0 - all_below, "call-on-min": all_above, "put-on-max": all_below, "put-on-min": 1.0 - all_above}[kind]
    return math.exp(-r * t) * float(wy @ (g @ wu))


# ---- the shapes of the GPU tests (tests/test_gpu_rainbow.py), shared with the checks on the reference alone --------------------
ASSETS = [1, 2, 3, 4, 5, 8]   # every phase class of the flat layout in both precisions, and the cap
N_PATHS = 2121   # eight workgroups and a partial wave
MAX_TABLE = 4096   # MC_MAX_RAINBOW_TABLE


def DATES(n):
    return [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 255, 256, 257, MAX_TABLE // n]


def betas(n):
    return np.linspace(0.6, 0.8, n) if n > 1 else np.array([0.7])


def one_factor_corr(beta):
    c = np.outer(beta, beta)
    np.fill_diagonal(c, 1.0)
    return c


def market(n, k=1.0, r=0.03, t=1.0, performance=True):
    """n assets with volatilities spread over 0.15 ... 0.35 and the one-factor correlation beta_i beta_j (0.36 ... 0.64)."""
    v = np.linspace(0.15, 0.35, n) if n > 1 else np.array([0.25])
    s = 100.0 * (1.0 + 0.1 * np.arange(n))
    w = 1.0 / s if performance else np.ones(n)
    return dict(s=s, v=v, p=np.linalg.cholesky(one_factor_corr(betas(n))), d=np.zeros(n), w=w, k=k, t=t, r=r)


def cases(n):
    """(basket, kind, barrier, up): both barrier kinds of the direction are valid for each."""
    b = market(n)
    return [(b, "put-on-min", 0.7, False), (b, "call-on-max", 1.5, True)]


ABSOLUTE = (dict(s=np.array([80.0, 100.0, 125.0]), v=np.array([0.3, 0.2, 0.25]), p=np.linalg.cholesky(one_factor_corr(betas(3))), d=np.zeros(3),
                 w=np.ones(3), k=90.0, t=1.5, r=0.01), "put-on-min", 60.0, False)


def kinds_of(up):
    return BARRIER_KINDS[:2] if up else BARRIER_KINDS[2:]
