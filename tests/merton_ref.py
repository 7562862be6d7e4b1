"""Independent float64 reference of the calls under Merton's jump-diffusion: European, Asian, discretely monitored barrier (not a
test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_dates equally spaced dates t_j = j T / m,
    dt = T / m,  kappa = exp(mu_j + delta^2/2) - 1,  a = (r - lambda kappa - v^2/2) dt,  bx = v sqrt(dt),
    s_n = sqrt(bx^2 + n delta^2),  C_j = N_1 + ... + N_j,  A_j = sum_{i<=j} s_{N_i} z_i,  x_j = ln S_j = ln S0 + j a + mu_j C_j + A_j,
    european (S_m - K)^+,   asian ((1/m) sum_j S_j - K)^+,
    barrier  d_j = sgn (ln B - x_j), P = [min_j d_j > 0], knock-out P (S_m - K)^+, knock-in (1 - P)(S_m - K)^+,
    antithetic: the mean of the value at z and at -z on the SAME counts,
evaluated with numpy on given normals z and counts N.  `merton` returns a greeks_ref.Paths (value, scale, jump, edge), each of
shape (1, n_paths) like a one-plane product of greeks_ref, so that greeks_ref.bound applies: a kernel computing the same formulas
in a precision of unit roundoff u is within a small multiple of u * scale of value.

The forward-error scale, in units of roundoff, follows barrier_ref's scheme.  The log price of date j carries
    ex_j = 1 + 2 |c_j| + 3 |mu_j| C_j + 2 sum_{i<=j} |s_{N_i} z_i| + sum_{i<=j} |A_i| + 2 |A_j| + |x_j|
(c_j = ln S0 + j a the rounded per-date constant and the rounding of the sum it enters; mu_j C_j the rounded mu_j, the product and
the sum it enters; the rounded s_n and the product s_n z; the running sum A_j whose every partial sum is rounded; a rounded unit
factor on A_j where the exponent is taken in another unit; the rounding of x_j itself; the exponential's own error).  The distance
d_j carries the same with c_j replaced by sgn (ln B - ln S0 - j a) and x_j by d_j.
  - S_j has the relative error el_j = ex_j; the subtraction charges |K|;
  - the Asian sum adds one rounding of every partial sum, sum_j (S_1 + ... + S_j), the division by m one rounding of the average:
    asian_ref's terms;
  - the barrier has an indicator: `jump` is the payoff, `edge` = min_j |d_j| / dd_j, the distance of the path to the step in units of
    the error of d_j; `value(..., full=True)` also returns the two values a near path can take, knocked or not (barrier_ref.value).

`merton_counts` inverts raw words against the library's integer thresholds with integer compares: N = #{k : w >= T_k};
`merton_draws` rebuilds the device's normals and counts from Engine.normals and Engine.words.

The mutation switches of the tests: "delta_plain" (s_n = sqrt(bx^2 + n delta)), "no_compensator" (a without -lambda kappa),
"late" (N_j applied one date late); the fourth, the compare turned into w > T_k, is merton_counts' `strict`.
"""
import math

import numpy as np

import barrier_ref as br
from greeks_ref import NPB, Paths, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_MERTON, DOMAIN_MERTON_JUMPS = 10, 11
PAYOFFS = ["european", "asian", "barrier"]
KINDS = br.KINDS


def merton_normals(draw, first, n, n_dates, npb):
    """Path p is unit p of domain 10; date j (1-based) draws entry (j - 1) % npb of block (j - 1) // npb.  Shape (n, n_dates)."""
    return basket_normals(lambda _, u, c, b: draw(DOMAIN_MERTON, u, c, b), first, n, n_dates, npb)


def jump_blocks(n_dates, X):
    """Raw Philox blocks per path: four dates per block in f32, two in f64."""
    per = 4 if X == "f32" else 2
    return (int(n_dates) + per - 1) // per


def jump_words(words, n_dates, X):
    """The dates' raw words from the blocks (n, n_blocks, 4) uint32 of domain 11: f32 date j (1-based) takes word (j - 1) % 4 of block
    (j - 1) // 4; f64 date j takes words 2 ((j - 1) % 2) and 2 ((j - 1) % 2) + 1 of block (j - 1) // 2 as (lo, hi).  uint64, (n, n_dates)."""
    w = np.asarray(words, dtype=np.uint32)
    n = w.shape[0]
    if X == "f32":
        return w.reshape(n, -1)[:, :n_dates].astype(np.uint64)
    lo, hi = w[:, :, 0::2].astype(np.uint64), w[:, :, 1::2].astype(np.uint64)
    return ((hi << np.uint64(32)) | lo).reshape(n, -1)[:, :n_dates]


def merton_counts(w, thresholds, strict=False):
    """N = #{k : w >= T_k} by integer compares (strict: the mutation w > T_k)."""
    T = np.asarray(thresholds, dtype=np.uint64)
    w = np.asarray(w, dtype=np.uint64)
    return np.searchsorted(T, w, side="left" if strict else "right").astype(np.int64)


def merton_draws(eng, seed, X, first, n, n_dates, thresholds):
    """The device's own draws of paths first ... first + n - 1: the normals (n, n_dates) and the counts (n, n_dates)."""
    z = merton_normals(lambda domain, u0, c, block: eng.normals(seed, domain, u0, c, block, X), first, n, n_dates, NPB[X])
    words = eng.words(seed, DOMAIN_MERTON_JUMPS, first, n, 0, jump_blocks(n_dates, X))
    return z, merton_counts(jump_words(words, n_dates, X), thresholds)


def constants(o, jumps, n_dates, mutation=None):
    s0, k, r, v, t = (float(o[c]) for c in "skrvt")
    lam, mu, delta = float(jumps["lambda"]), float(jumps["mu_j"]), float(jumps["delta"])
    m = int(n_dates)
    dt = t / m
    kappa = math.expm1(mu + 0.5 * delta * delta)
    comp = 0.0 if mutation == "no_compensator" else lam * kappa
    return dict(s0=s0, k=k, m=m, a=(r - comp - 0.5 * v * v) * dt, bx=v * math.sqrt(dt), mu=mu, d2=delta if mutation == "delta_plain" else delta * delta)


def _one_side(c, A, S_abs, A_abs, C, gap, sgn):
    """One path direction from its running sums A (n, m): the payoffs, the distances and their errors."""
    m, mu = c["m"], c["mu"]
    j = np.arange(1, m + 1)
    ck = math.log(c["s0"]) + j * c["a"]
    x = ck + mu * C + A
    common = 3.0 * abs(mu) * C + 2.0 * S_abs + A_abs + 2.0 * np.abs(A)
    el = 1.0 + 2.0 * np.abs(ck) + common + np.abs(x)
    S = np.exp(x)
    ST, elT = S[:, -1], el[:, -1]
    out = dict(S=S, el=el, pay=np.maximum(ST - c["k"], 0.0), dpay=ST * elT + ST + abs(c["k"]))
    if gap is not None:
        dk = sgn * (gap - j * c["a"])
        d = dk - sgn * (mu * C + A)
        dd = 1.0 + 2.0 * np.abs(dk) + common + np.abs(d)
        n = A.shape[0]
        out.update(P=(d.min(axis=1) > 0).astype(np.float64), dP=np.zeros(n), jump=out["pay"], edge=(np.abs(d) / dd).min(axis=1))
    return out


def walk(o, jumps, n_dates, z, N, B=None, up=True, anti=False, mutation=None):
    """Everything about the paths on the normals z and counts N (n_paths, >= n_dates) that does not depend on the payoff: one
    _one_side per path direction.  With a barrier B the sides carry barrier_ref's fields, so that barrier_ref.value applies."""
    c = constants(o, jumps, n_dates, mutation)
    m = c["m"]
    z = np.asarray(z, dtype=np.float64)[:, :m]
    N = np.asarray(N, dtype=np.int64)[:, :m]
    if mutation == "late":
        N = np.concatenate([np.zeros((N.shape[0], 1), dtype=np.int64), N[:, :-1]], axis=1)
    sN = np.sqrt(c["bx"] ** 2 + N * c["d2"])
    inc = sN * z
    A = np.cumsum(inc, axis=1)
    S_abs = np.cumsum(np.abs(inc), axis=1)
    A_abs = np.cumsum(np.abs(A), axis=1)
    C = np.cumsum(N, axis=1).astype(np.float64)
    gap = None if B is None else math.log(float(B)) - math.log(c["s0"])
    sgn = 1.0 if up else -1.0
    sides = [_one_side(c, A, S_abs, A_abs, C, gap, sgn)] + ([_one_side(c, -A, S_abs, A_abs, C, gap, sgn)] if anti else [])
    return c, sides


def value(c, sides, payoff, knock_in=False, full=False):
    """Paths of one payoff from `walk`.  The barrier goes through barrier_ref.value (full=True: with the candidates of a near path)."""
    if payoff == "barrier":
        return br.value(sides, knock_in, full)
    m, k = c["m"], c["k"]
    n = sides[0]["pay"].size
    val, scale = np.zeros(n), np.zeros(n)
    for s in sides:
        if payoff == "european":
            v1, s1 = s["pay"], s["dpay"]
        else:
            S, el = s["S"], s["el"]
            avg = S.sum(axis=1) / m
            v1 = np.maximum(avg - k, 0.0)
            s1 = ((S * el).sum(axis=1) + np.cumsum(S, axis=1).sum(axis=1)) / m + avg + abs(k)
        val += v1 / len(sides)
        scale += s1 / len(sides)
    return Paths(val.reshape(1, n), scale.reshape(1, n), np.zeros((1, n)), np.full(n, np.inf))


def merton(o, jumps, n_dates, z, N, payoff="european", B=None, kind="up-and-out", anti=False, mutation=None):
    """Per-path values of one payoff on the normals z and the counts N, and their forward-error scales."""
    barrier = payoff == "barrier"
    c, sides = walk(o, jumps, n_dates, z, N, B if barrier else None, kind.startswith("up"), anti, mutation)
    return value(c, sides, payoff, kind.endswith("in"))


def ratio(err, b):
    """err / b per path, with 0 / 0 = 0: a knocked-out path has value 0 and bound 0, and the kernel must return exactly 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / b)


def check_paths(got, c, sides, payoff, knock_in, tol):
    """The per-path rule: a path farther from the barrier's step than tol (in units of the error of its distance; every path of the
    other payoffs) must match the model's value within tol * scale; a nearer one must match one of the two values each of its
    directions can take, knocked or not -- no path is left out.  Returns (worst error / bound, number of near paths)."""
    import itertools
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got))
    if payoff != "barrier":
        p = value(c, sides, payoff)
        r = ratio(np.abs(got - p.value[0]), tol * p.scale[0])
        assert np.all(r <= 1.0), (int(np.argmax(r)), float(r.max()))
        return float(r.max()), 0
    p, cands = value(c, sides, payoff, knock_in, full=True)
    r = ratio(np.abs(got - p.value[0]), tol * p.scale[0])
    near = p.edge <= tol
    worst = float(r[~near].max()) if (~near).any() else 0.0
    assert worst <= 1.0, (int(np.argmax(np.where(near, 0.0, r))), worst)
    if near.any():
        w = 1.0 / len(cands)
        best = np.full(int(near.sum()), np.inf)
        for pick in itertools.product((0, 1), repeat=len(cands)):
            v = w * sum(cd[0][i][near] for cd, i in zip(cands, pick))
            sc = w * sum(cd[1][i][near] for cd, i in zip(cands, pick))
            best = np.minimum(best, ratio(np.abs(got[near] - v), tol * sc))
        assert np.all(best <= 1.0), float(best.max())
        worst = max(worst, float(best.max()))
    return worst, int(near.sum())


# ---- the same formulas in float32, the way a kernel of that precision may evaluate them ------------------------------------------
def merton_f32(o, jumps, n_dates, z, N, payoff="european", B=None, kind="up-and-out", anti=False):
    """Every constant folded in float64 and rounded once, every operation in float32, the running sums sequential, the exponent in
    units of log2: one admissible float32 evaluation of the model (not the kernel's code)."""
    f = np.float32
    c = constants(o, jumps, n_dates)
    m = c["m"]
    z = np.asarray(z, dtype=np.float32)[:, :m]
    N = np.asarray(N, dtype=np.int64)[:, :m]
    L2E = 1.4426950408889634
    j = np.arange(1, m + 1)
    unit = 1.0 if payoff == "barrier" else L2E
    sN = (np.sqrt(c["bx"] ** 2 + np.arange(int(N.max()) + 1) * c["d2"]) * unit).astype(f)[N]
    A = np.cumsum(sN * z, axis=1, dtype=f)
    C = np.cumsum(N, axis=1).astype(f)
    k = f(c["k"])
    ln_s0 = math.log(c["s0"])
    vals = []
    for sg in ((1.0, -1.0) if anti else (1.0,)):
        As = f(sg) * A
        if payoff == "barrier":
            up = kind.startswith("up")
            sgn = 1.0 if up else -1.0
            dk = (sgn * (math.log(float(B)) - ln_s0 - j * c["a"])).astype(f)
            d = (C * f(-sgn * c["mu"]) + dk) + f(-sgn) * As
            P = (d.min(axis=1) > 0).astype(f)
            xT = (C[:, -1] * f(c["mu"] * L2E) + f((ln_s0 + m * c["a"]) * L2E)) + As[:, -1] * f(L2E)
            pay = np.maximum(np.exp2(xT) - k, f(0))
            vals.append((f(1) - P if kind.endswith("in") else P) * pay)
        else:
            x = (C * f(c["mu"] * L2E) + ((ln_s0 + j * c["a"]) * L2E).astype(f)) + As
            if payoff == "european":
                vals.append(np.maximum(np.exp2(x[:, -1]) - k, f(0)))
            else:
                avg = np.cumsum(np.exp2(x), axis=1, dtype=f)[:, -1] * f(1.0 / m)
                vals.append(np.maximum(avg - k, f(0)))
    return vals[0] if not anti else f(0.5) * (vals[0] + vals[1])


# ---- the exact price, from first principles ---------------------------------------------------------------------------------
def lewis_price(o, jumps, digits=30):
    """Discounted price of the European call by Lewis's single integral of the characteristic function, with mpmath:
        C = S - sqrt(S K) e^{-rT/2} / pi  int_0^inf Re[ e^{i u kk} phi(u - i/2) ] / (u^2 + 1/4) du,   kk = ln(S / K) + r T,
    (the forward form F - sqrt(F K) / pi int ..., F = S e^{rT}, discounted),  phi(u) = E exp(i u (ln S_T - ln S0 - r T)) = exp(T psi(u)),
        psi(u) = -i u (v^2/2 + lambda kappa) - v^2 u^2 / 2 + lambda (exp(i u mu_j - delta^2 u^2 / 2) - 1)."""
    import mpmath as mp
    with mp.workdps(digits + 10):
        s, k, r, v, t = (mp.mpf(float(o[c])) for c in "skrvt")
        lam, mu, delta = (mp.mpf(float(jumps[c])) for c in ("lambda", "mu_j", "delta"))
        kappa = mp.expm1(mu + delta * delta / 2)
        kk = mp.log(s / k) + r * t

        def psi(u):
            return -1j * u * (v * v / 2 + lam * kappa) - v * v * u * u / 2 + lam * (mp.exp(1j * u * mu - delta * delta * u * u / 2) - 1)

        def f(u):
            w = u - 0.5j
            return mp.re(mp.exp(1j * u * kk + t * psi(w))) / (u * u + mp.mpf(1) / 4)

        width = 1 / mp.sqrt((v * v + lam * (mu * mu + delta * delta)) * t)
        cuts = [0] + [width * i for i in (1, 2, 4, 8, 16, 32, 64)]
        integral = mp.quad(f, cuts) + mp.quad(f, [cuts[-1], mp.inf])
        return float(s - mp.sqrt(s * k) * mp.exp(-r * t / 2) / mp.pi * integral)


def poisson_cdf(p, kmax, digits=50):
    """F_0 ... F_kmax and the tails P(N > k) of Poisson(p), mpmath numbers."""
    import mpmath as mp
    with mp.workdps(digits):
        p = mp.mpf(float(p))
        f = [mp.exp(-p)]
        for n in range(1, kmax + 400):
            f.append(f[-1] * p / n)
        F, acc = [], mp.mpf(0)
        for n in range(kmax + 1):
            acc += f[n]
            F.append(acc)
        tails = [mp.fsum(f[n + 1:]) for n in range(kmax + 1)]
        return F, tails


# ---- the shapes of the GPU tests (tests/test_gpu_merton.py), shared with the checks on the reference alone ------------------------
JUMPS = [dict([("lambda", 1.0), ("mu_j", -0.1), ("delta", 0.15)]),    # about 64 % of the paths jump
         dict([("lambda", 3.0), ("mu_j", 0.02), ("delta", 0.08)]),    # about 95 %
         dict([("lambda", 0.5), ("mu_j", -0.2), ("delta", 0.25)])]    # about 22 % (t = 0.5)
CASES = [(o, B, jp) for (o, B), jp in zip(br.CASES, JUMPS)]
# the count loop near its cap: lambda dt up to 4.5, one to four dates only
HEAVY = (br.ATM, 120.0, dict([("lambda", 4.5), ("mu_j", -0.05), ("delta", 0.1)]))
HEAVY_DATES = [1, 2, 3, 4]
DATES = br.DATES
N_PATHS = br.N_PATHS
TRIP_DATES, TRIP_BITS_DATES = br.TRIP_DATES, br.TRIP_BITS_DATES   # the many-trip GPU test (tests/test_gpu_walk_trips.py)
TRIP_HEAVY_DATES = 4                                               # ... and its one case on HEAVY
kinds_of = br.kinds_of
