"""Independent float64 reference of the worst-of autocallable notes (not a test module).

Written from the model stated in include/mc_mi355x.h (mc_autocall_run_*), not from the kernel, on top of rainbow_ref.fold and
rainbow_ref.rainbow_normals with domain 15: n assets, m = n_dates dates, n_obs observation dates, E = m / n_obs,
    y(j) = min_i y_i(j),  y_i(j) = ln(w_i s_i) + j a_i + sum_{k<=i} M_ik W_k(j)          (rainbow_ref's model, the minimum)
and per path direction, with alive = 1, miss = 0, V = 0, at observation k on date j = k E
    called = [y(j) >= ln A_k],  paid = [y(j) >= ln min(A_k, C_k)],  cash = c (1 + memory miss) paid,  miss = paid ? 0 : miss + 1
    k < n_obs:  V += alive D_k (cash + called),  alive &= !called
    k = n_obs:  V += alive D_k (cash + 1 - g KI max(K - exp(y(m)), 0)),   D_k = exp(-r t k / n_obs)
    KI = 1 without a knock-in condition, else [min over the monitored dates of y(j) <= ln B]
    antithetic: the mean of V at z and at -z.
A contract is a dict: autocall (n_obs,), coupon_barrier (n_obs,), coupon, memory, barrier (None: no knock-in condition), ki ("dates",
"maturity" or None), gearing; the strike, rate and maturity are the basket's.

`autocall` returns a greeks_ref.Paths (value, scale, jump, edge), each of shape (1, n_paths).  The forward-error scale, in units
of roundoff:
  - y(j) carries rainbow_ref's dY(j): the rounded per-date constant, the running sums, the tie among the assets;
  - a decision y >= L has the distance |y - L| / (1 + |L| + dY + |y - L|) (an infinite L: no decision, the distance is infinite);
  - a cash flow alive D_k f is charged the rounding of D_k, of c (1 + miss), of the sum f and of the product (3 D_k f + D_k cash),
    and the running sum |V| after it;
  - the put is charged g D (X dY + X + K), X = exp(y(m)): the error of its exponent, its own rounding and the subtraction's.
A decision is NEAR when its distance is <= tol; only the decisions a path reaches while alive count.  The knock-in counts as ONE
near decision, and only if no monitored date is clearly hit.  `edge` is the smallest such distance of the path, over both
directions.  With full=True the values a near path can take are enumerated by flipping each near decision and re-walking the path
from there: per path direction a list of (value, scale), for the paths whose edge is <= tol.

`exact_single` is the price of the one-asset note by density propagation (no sampling), `single_two_obs` and `single_one_obs`
closed forms it is checked against.
"""
import math

import numpy as np

import rainbow_ref as rr
from greeks_ref import NPB, Paths   # noqa: F401

DOMAIN_AUTOCALL = 15
INF = math.inf
MUTANTS = ["late", "no-reset", "dead-coupon", "discount-maturity", "ki-obs", "paid-not-forced"]


def autocall_normals(draw, first, n, n_assets, n_dates, npb):
    """Path p is unit p of domain 15; the rainbow's flat layout.  Shape (n, n_dates, n_assets)."""
    total = n_assets * n_dates
    blocks = [np.asarray(draw(DOMAIN_AUTOCALL, first, n, b), dtype=np.float64).reshape(n, npb) for b in range((total + npb - 1) // npb)]
    return np.concatenate(blocks, axis=1)[:, :total].reshape(n, n_dates, n_assets)


def contract(autocall, coupon_barrier, coupon, barrier=None, ki="dates", gearing=None, memory=True, n_obs=None, k=1.0):
    A = np.full(n_obs, float(autocall)) if np.ndim(autocall) == 0 else np.asarray(autocall, dtype=np.float64)
    C = np.full(A.size, float(coupon_barrier)) if np.ndim(coupon_barrier) == 0 else np.asarray(coupon_barrier, dtype=np.float64)
    assert A.size == C.size and (barrier is None) == (ki is None)
    return dict(autocall=A, coupon_barrier=C, coupon=float(coupon), memory=bool(memory), barrier=barrier, ki=ki,
                gearing=1.0 / k if gearing is None else float(gearing))


def worst(b, m, W, W_abs):
    """(y, dY), each (N, m): the log of the worst level on every date and its error scale, as rainbow_ref._one_side forms them."""
    ln_s, a, M = rr.fold(b, m)
    j = np.arange(1, m + 1, dtype=np.float64)
    c = ln_s[None, :] + j[:, None] * a[None, :]
    y = c[None] + W @ M.T
    dy = 1.0 + np.abs(c)[None] + (np.abs(W) + W_abs) @ np.abs(M).T + np.abs(y)
    Y = y.min(axis=2)
    d_low = np.take_along_axis(dy, y.argmin(axis=2)[..., None], axis=2)
    dY = np.where(y <= Y[..., None] + rr.NEAR * (dy + d_low), dy, 0.0).max(axis=2)
    return Y, dY


def _dist(y, L, dY):
    if math.isinf(L):
        return np.full(np.shape(y), INF)
    d = np.abs(y - L)
    return d / (1.0 + abs(L) + dY + d)


def _log(x):
    return -INF if x == 0 else math.log(x)


def _schedule(b, m, con, mutate):
    """Per observation (index of its date, ln A_k, ln of the coupon level, D_k)."""
    n_obs = con["autocall"].size
    assert m % n_obs == 0
    E, r, t = m // n_obs, float(b["r"]), float(b["t"])
    rows = []
    for k in range(1, n_obs + 1):
        A, C = float(con["autocall"][k - 1]), float(con["coupon_barrier"][k - 1])
        j = k * E - 1
        if mutate == "late":
            j = min(j + 1, m - 1)
        D = math.exp(-r * (t * (n_obs if mutate == "discount-maturity" else k) / n_obs))
        rows.append((j, _log(A), _log(C) if mutate == "paid-not-forced" else _log(min(A, C)), D))
    return rows


def _knock_in(b, m, con, y, dY, mutate):
    """(KI as 0 / 1, the distance of the knock-in decision), each (N,)."""
    N = y.shape[0]
    if con["ki"] is None:
        return np.ones(N), np.full(N, INF)
    lb = math.log(float(con["barrier"]))
    n_obs = con["autocall"].size
    if con["ki"] == "maturity":
        cols = [m - 1]
    elif mutate == "ki-obs":
        cols = [k * (m // n_obs) - 1 for k in range(1, n_obs + 1)]
    else:
        cols = list(range(m))
    yy, dd = y[:, cols], _dist(y[:, cols], lb, dY[:, cols])
    hit = yy <= lb
    # clearly hit: some monitored date is below the level by more than any tolerance in use -- its distance is the decision's;
    # otherwise the decision is as far as its nearest date
    far_hit = np.where(hit, dd, 0.0).max(axis=1)
    return hit.any(axis=1).astype(np.float64), np.where(hit.any(axis=1), far_hit, dd.min(axis=1))


def _one_side(b, m, con, y, dY, mutate=None):
    """One path direction, vectorised: value, scale, the distance of every decision (N, 2 n_obs + 1; inf where not reached)."""
    N = y.shape[0]
    rows = _schedule(b, m, con, mutate)
    n_obs, c, mem, g, K = len(rows), con["coupon"], float(con["memory"]), con["gearing"], float(b["k"])
    alive, miss, V, S = np.ones(N), np.zeros(N), np.zeros(N), np.zeros(N)
    dist = np.full((N, 2 * n_obs + 1), INF)
    KI, d_ki = _knock_in(b, m, con, y, dY, mutate)
    for k, (j, LA, LP, D) in enumerate(rows):
        yk, dk = y[:, j], dY[:, j]
        last = k == n_obs - 1
        called, paid = yk >= LA, yk >= LP
        live = alive > 0
        dist[:, 2 * k] = np.where(live, _dist(yk, LP, dk), INF)
        if not last:
            dist[:, 2 * k + 1] = np.where(live, _dist(yk, LA, dk), INF)
        cash = np.where(paid, c * (1.0 + mem * miss), 0.0)
        if mutate != "no-reset":
            miss = np.where(paid, 0.0, miss + 1.0)
        else:
            miss = miss + np.where(paid, 0.0, 1.0)
        if not last:
            f = cash + called
            extra = 0.0
        else:
            X = np.exp(yk)
            put = np.maximum(K - X, 0.0)
            f = cash + 1.0 - g * KI * put
            extra = g * D * (X * dk + X + K)
            dist[:, 2 * n_obs] = np.where(live & (g > 0) & (put > 0), d_ki, INF)
        pays = np.ones(N) if mutate == "dead-coupon" else alive
        V = V + alive * D * (f - cash) + pays * D * cash
        S = S + alive * (D * (3.0 * np.abs(f) + cash) + extra) + np.abs(V)
        if not last:
            alive = np.where(called, 0.0, alive)
    return V, S, dist


def _enumerate(b, m, con, y, dY, tol):
    """Every (value, scale) ONE path direction can take when each decision within tol may fall either way (scalar re-walk)."""
    rows = _schedule(b, m, con, None)
    n_obs, c, mem, g, K = len(rows), con["coupon"], float(con["memory"]), con["gearing"], float(b["k"])
    KI, d_ki = _knock_in(b, m, con, y[None], dY[None], None)
    KI, d_ki = float(KI[0]), float(d_ki[0])
    out = []

    def options(yk, L, dk):
        v = bool(yk >= L)
        return [v, not v] if float(_dist(yk, L, dk)) <= tol else [v]

    stack = [(0, 0.0, 0.0, 0.0)]   # (observation, miss, V, scale) of the branches still to walk: no recursion, n_obs may be large
    while stack:
        k, miss, V, S = stack.pop()
        j, LA, LP, D = rows[k]
        yk, dk = float(y[j]), float(dY[j])
        last = k == n_obs - 1
        for paid in options(yk, LP, dk):
            cash = c * (1.0 + mem * miss) if paid else 0.0
            miss2 = 0.0 if paid else miss + 1.0
            if last:
                X = math.exp(yk)
                put = max(K - X, 0.0)
                for ki in ([KI, 1.0 - KI] if d_ki <= tol and g > 0 and put > 0 else [KI]):
                    f = cash + 1.0 - g * ki * put
                    V2 = V + D * f
                    out.append((V2, S + D * (3.0 * abs(f) + cash) + g * D * (X * dk + X + K) + abs(V2)))
                continue
            for called in options(yk, LA, dk):
                if called and not paid:   # ln min(A, C) <= ln A: a called note always pays
                    continue
                f = cash + called
                V2 = V + D * f
                S2 = S + D * (3.0 * abs(f) + cash) + abs(V2)
                if called:
                    # the running sum is still charged at the later observations of the vectorised walk: do the same
                    out.append((V2, S2 + (n_obs - 1 - k) * abs(V2)))
                else:
                    stack.append((k + 1, miss2, V2, S2))
    return out


def walk(b, n_dates, z, anti=False):
    """(y, dY) per path direction on the normals z (n_paths, >= n_dates, n_assets)."""
    m = int(n_dates)
    z = np.asarray(z, dtype=np.float64)[:, :m, :]
    W = np.cumsum(z, axis=1)
    W_abs = np.cumsum(np.abs(W), axis=1)
    return [worst(b, m, sign * W, W_abs) for sign in ((1.0, -1.0) if anti else (1.0,))]


def value(b, n_dates, con, sides, tol=0.0, mutate=None, full=False):
    """Paths of the contract from `walk`.  full=True also returns {path: [per direction, a list of (value, scale)]} for the paths with
    a decision within tol."""
    m = int(n_dates)
    w = 1.0 / len(sides)
    n = sides[0][0].shape[0]
    val, scale, edge = np.zeros(n), np.zeros(n), np.full(n, INF)
    for y, dY in sides:
        V, S, dist = _one_side(b, m, con, y, dY, mutate)
        val += w * V
        scale += w * S
        edge = np.minimum(edge, dist.min(axis=1))
    p = Paths(val.reshape(1, n), scale.reshape(1, n), np.zeros((1, n)), edge)
    if not full:
        return p
    cands = {int(i): [_enumerate(b, m, con, y[i], dY[i], tol) for y, dY in sides] for i in np.flatnonzero(edge <= tol)}
    return p, cands


def autocall(b, n_dates, z, con, anti=False, tol=0.0, mutate=None, full=False):
    return value(b, n_dates, con, walk(b, n_dates, z, anti), tol, mutate, full)


def shares(b, n_dates, z, con):
    """(share of paths called before maturity, share knocked in) of the plain direction: which branches a shape exercises."""
    (y, dY), = walk(b, n_dates, z)
    rows = _schedule(b, n_dates, con, None)
    called = np.zeros(y.shape[0], dtype=bool)
    for j, LA, _, _ in rows[:-1]:
        called |= y[:, j] >= LA
    return float(called.mean()), float(_knock_in(b, n_dates, con, y, dY, None)[0].mean())


def check(got, p, cands, tol):
    """The per-path rule: a path whose decisions are all farther than tol must lie within tol * scale of the model's value; a near
    path must match one of the values it can take.  Returns (worst error / bound, number of near paths); asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got))
    err = np.abs(got - p.value[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (tol * p.scale[0]))
    near = p.edge <= tol
    worst_r = float(r[~near].max()) if (~near).any() else 0.0
    assert worst_r <= 1.0, (int(np.argmax(np.where(near, 0.0, r))), worst_r)
    for i, sides in cands.items():
        w = 1.0 / len(sides)
        combos = [(0.0, 0.0)]
        for side in sides:
            combos = [(v0 + w * v, s0 + w * s) for v0, s0 in combos for v, s in side]
        best = min(abs(got[i] - v) / (tol * s) if got[i] != v else 0.0 for v, s in combos)
        assert best <= 1.0, (i, best, float(got[i]), combos)
        worst_r = max(worst_r, best)
    return worst_r, int(near.sum())


def rejects(mutant_value, p, cands, tol):
    """Per path: does the rule of `check` refuse the value mutant_value[i]?"""
    bad = np.abs(mutant_value - p.value[0]) > tol * p.scale[0]
    for i, sides in cands.items():
        if not bad[i]:
            continue
        w = 1.0 / len(sides)
        combos = [(0.0, 0.0)]
        for side in sides:
            combos = [(v0 + w * v, s0 + w * s) for v0, s0 in combos for v, s in side]
        bad[i] = all(abs(mutant_value[i] - v) > tol * s for v, s in combos)
    return bad


# ---- the fp32 walk in the header's order --------------------------------------------------------------------------------
def walk_f32(b, n_dates, z, con, anti=False):
    """The header's arithmetic in float32 with numpy (no fma: a product and a sum round separately), per path."""
    f = np.float32
    m = int(n_dates)
    ln_s, a, M = rr.fold(b, m)
    n = ln_s.size
    tab = (ln_s[None, :] + np.arange(1, m + 1, dtype=np.float64)[:, None] * a[None, :]).astype(f)
    M = M.astype(f)
    rows = [(j, f(LA), f(LP), f(D)) for j, LA, LP, D in _schedule(b, m, con, None)]
    n_obs, c, g, K = len(rows), f(con["coupon"]), f(con["gearing"]), f(b["k"])
    cm = c if con["memory"] else f(0)
    lb = f(INF) if con["ki"] is None else f(math.log(float(con["barrier"])))
    W = np.cumsum(np.asarray(z, dtype=np.float64)[:, :m, :].astype(f), axis=1, dtype=f)
    total = np.zeros(W.shape[0], dtype=f)
    for sign in ((1, -1) if anti else (1,)):
        y = np.full((W.shape[0], m), np.inf, dtype=f)
        for i in range(n):
            cs = M[i, 0] * W[:, :, 0]
            for k in range(1, i + 1):
                cs = (M[i, k] * W[:, :, k] + cs).astype(f)
            y = np.minimum(y, tab[None, :, i] + f(sign) * cs)
        alive, miss, V = np.ones(W.shape[0], dtype=f), np.zeros(W.shape[0], dtype=f), np.zeros(W.shape[0], dtype=f)
        for k, (j, LA, LP, D) in enumerate(rows):
            yk = y[:, j]
            paid = yk >= LP
            cash = np.where(paid, cm * miss + c, f(0)).astype(f)
            miss = np.where(paid, f(0), miss + f(1)).astype(f)
            if k < n_obs - 1:
                called = yk >= LA
                V = ((alive * D) * (cash + called.astype(f)) + V).astype(f)
                alive = np.where(called, f(0), alive)
            else:
                mn = y.min(axis=1) if con["ki"] == "dates" else yk
                gk = np.where(mn <= lb, g, f(0)).astype(f)
                put = np.maximum(K - np.exp(yk, dtype=f), f(0))
                V = ((alive * D) * ((cash + f(1)) - gk * put) + V).astype(f)
        total = total + V
    return (total * f(0.5) if anti else total).astype(np.float64)


# ---- the exact single-asset price ---------------------------------------------------------------------------------------
_GL = np.polynomial.legendre.leggauss(16)


def exact_single(b, n_dates, con, panels_per_sd=2.0, width=9.0):
    """Present value of the one-asset note by propagating the density of x = ln(w s S_t / s) over the walk dates: Gauss-Legendre
    panels split at every ln A_k, ln C_k, ln B and ln K (the densities jump there), one density per (knocked in or not, number
    of missed coupons); an observation every E-th date moves the mass: called mass is paid and leaves, paid mass resets miss."""
    assert len(b["s"]) == 1
    m = int(n_dates)
    ln_s, a, M = rr.fold(b, m)
    x0, a, sd = float(ln_s[0]), float(a[0]), abs(float(M[0, 0]))
    rows = _schedule(b, m, con, None)
    n_obs, c, mem, g, K = len(rows), con["coupon"], float(con["memory"]), con["gearing"], float(b["k"])
    lb = None if con["ki"] is None else math.log(float(con["barrier"]))
    lo, hi = x0 + min(0.0, m * a) - width * sd * math.sqrt(m), x0 + max(0.0, m * a) + width * sd * math.sqrt(m)
    cuts = {lo, hi, math.log(K)} | ({lb} if lb is not None else set())
    for _, LA, LP, _ in rows:
        cuts |= {L for L in (LA, LP) if not math.isinf(L)}
    cuts = sorted(x for x in cuts if lo <= x <= hi)
    edges = np.concatenate([np.linspace(p, q, max(1, int(math.ceil((q - p) * panels_per_sd / sd))) + 1)[:-1] for p, q in zip(cuts[:-1], cuts[1:])] + [[hi]])
    mid, half = 0.5 * (edges[1:] + edges[:-1]), 0.5 * (edges[1:] - edges[:-1])
    x = (mid[:, None] + half[:, None] * _GL[0][None, :]).reshape(-1)
    wx = (half[:, None] * _GL[1][None, :]).reshape(-1)
    T = np.exp(-0.5 * ((x[:, None] - x[None, :] - a) / sd) ** 2) / (sd * math.sqrt(2.0 * math.pi)) * wx[None, :]   # to x[:, None] from x[None, :]
    first = np.exp(-0.5 * ((x - x0 - a) / sd) ** 2) / (sd * math.sqrt(2.0 * math.pi))
    f = np.zeros((2, n_obs + 1, x.size))   # [knocked in][missed coupons]
    V, k = 0.0, 0
    for j in range(m):
        f = f @ T.T if j else f
        if j == 0:
            f[0, 0] = first
        if lb is not None and con["ki"] == "dates":
            below = x <= lb
            f[1] += f[0] * below
            f[0] = f[0] * ~below
        if j != rows[k][0]:
            continue
        _, LA, LP, D = rows[k]
        last = k == n_obs - 1
        called, paid = x >= LA, x >= LP
        new = np.zeros_like(f)
        for ki in (0, 1):
            for miss in range(n_obs):
                d = f[ki, miss] * wx
                cash = c * (1.0 + mem * miss)
                if last:
                    KI = 1.0 if lb is None else (x <= lb).astype(np.float64) if con["ki"] == "maturity" else float(ki)
                    V += D * float((d * (np.where(paid, cash, 0.0) + 1.0 - g * KI * np.maximum(K - np.exp(x), 0.0))).sum())
                    continue
                V += D * float((d * (np.where(paid, cash, 0.0) + called)).sum())
                stay = f[ki, miss] * ~called
                new[ki, 0] += stay * paid
                new[ki, miss + 1] += stay * ~paid
        f = new
        k += 1
    return V


def _Phi(v):
    return 0.5 * math.erfc(-v / math.sqrt(2.0))


def single_one_obs(b, con):
    """n = 1, one date, one observation: Black-Scholes digitals and the gap put (KI at maturity or none)."""
    ln_s, a, M = rr.fold(b, 1)
    x0, sd = float(ln_s[0]) + float(a[0]), abs(float(M[0, 0]))
    K, g, c = float(b["k"]), con["gearing"], con["coupon"]
    D = math.exp(-float(b["r"]) * float(b["t"]))
    LP = _log(min(float(con["autocall"][0]), float(con["coupon_barrier"][0])))
    p_paid = 1.0 if math.isinf(LP) else _Phi((x0 - LP) / sd)
    L = math.log(K) if con["ki"] is None else min(math.log(K), math.log(float(con["barrier"])))   # the put pays below min(K, B)
    z = (L - x0) / sd
    put = K * _Phi(z) - math.exp(x0 + 0.5 * sd * sd) * _Phi(z - sd)   # E[(K - e^x) 1{x <= L}]: the gap put
    return D * (c * p_paid + 1.0 - g * put)


def single_two_obs(b, con):
    """n = 1, two dates, two observations, the put always live (ki None): bivariate normal probabilities (rainbow_ref.binorm)."""
    assert con["ki"] is None
    ln_s, a, M = rr.fold(b, 2)
    x0, a, sd = float(ln_s[0]), float(a[0]), abs(float(M[0, 0]))
    K, g, c, mem = float(b["k"]), con["gearing"], con["coupon"], float(con["memory"])
    r, t = float(b["r"]), float(b["t"])
    D1, D2 = math.exp(-r * t / 2.0), math.exp(-r * t)
    (LA1, LP1), (_, LP2) = [(_log(float(A)), _log(min(float(A), float(C)))) for A, C in zip(con["autocall"], con["coupon_barrier"])]
    rho = math.sqrt(0.5)

    def P1(L, shift=0.0):   # P(y1 < L) with the drift of both dates shifted by `shift` variances
        return 1.0 if L == INF else 0.0 if L == -INF else _Phi((L - x0 - a - shift * sd * sd) / sd)

    def P12(L1, L2, shift=0.0):   # P(y1 < L1, y2 < L2)
        if L1 == -INF or L2 == -INF:
            return 0.0
        s2 = sd * math.sqrt(2.0)
        b2 = (L2 - x0 - 2.0 * a - 2.0 * shift * sd * sd) / s2
        if L1 == INF:
            return _Phi(b2)
        return rr.binorm((L1 - x0 - a - shift * sd * sd) / sd, b2, rho)

    V = D1 * ((c + 1.0) * (1.0 - P1(LA1)) + c * (P1(LA1) - P1(LP1)))
    alive = P1(LA1)
    coupon2 = c * (alive - P12(LA1, LP2)) + c * mem * (P1(LP1) - P12(LP1, LP2))
    lk = math.log(K)
    put = K * P12(LA1, lk) - math.exp(x0 + 2.0 * a + sd * sd) * P12(LA1, lk, shift=1.0)
    return V + D2 * (coupon2 + alive - g * put)


# ---- the shapes shared by the CPU and GPU tests -------------------------------------------------------------------------
ASSETS = rr.ASSETS
N_PATHS = rr.N_PATHS
MAX_TABLE = 4096   # MC_MAX_AUTOCALL_TABLE


def SHAPES(n):
    K = MAX_TABLE // (n + 3)
    return [(1, 1), (4, 4), (5, 5), (8, 4), (12, 4), (16, 4), (17, 17), (63, 3), (64, 4), (255, 51), (256, 4), (257, 1), ((MAX_TABLE - 3) // n, 1), (K, K)]


def contract_a(n_obs):
    A = 1.0 - 0.05 * np.arange(n_obs) if n_obs <= 8 else np.ones(n_obs)
    return contract(A, 0.8, 0.02, barrier=0.6, ki="dates", gearing=1.0, memory=True, n_obs=n_obs)


def contract_b(n_obs):
    """On rainbow_ref.ABSOLUTE's basket (absolute levels): the first observation not callable, unconditional coupons, no memory,
    the knock-in looked at on the last date only."""
    b, _, B, _ = rr.ABSOLUTE
    A = np.full(n_obs, 85.0)
    A[0] = INF
    return contract(A, 0.0, 0.02, barrier=B, ki="maturity", gearing=1.0 / b["k"], memory=False, n_obs=n_obs)
