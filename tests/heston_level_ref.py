"""Independent float64 reference of one multilevel correction on the Heston walk, Y = P_fine - P_coarse, of the path counts of a
multilevel plan and of the multilevel driver (not a test module).

Written from include/mc_mi355x.h (mc_heston_level_*, mc_mlmc_plan, mc_heston_mlmc_run_*), not from the kernel.  The FINE walk is
heston_path_ref.walk on m = n_dates * steps_per_date steps of dt, P its Asian value (one date: the European call).  The COARSE walk
takes m / 2 steps of 2 dt on the same Brownian increments: coarse step i stands on the fine steps a = 2i - 1 and b = 2i,
    t_j = c1 z1_j + c2 z2_j,   W1_i = z1_a + z1_b,   T_i = t_a + t_b,
    V+ = max(V, 0),  s = sqrt(V+),   x_c += (r - V+/2) 2 dt + s sdt W1_i,   V += kappa (theta - V+) 2 dt + s T_i,
date d after coarse step d * steps_per_date / 2 with the fine walk's per-date constant.  The header rounds W1_i and T_i once, in the
precision of the call.  W1 is a sum of two of the device's own normals, so the model forms it in that precision (`prec`) and holds
the very number the kernel holds; T is formed here in float64 and the bound charges the kernel's three roundings (below).

The coarse leg is returned in the shape of a heston_ref side -- the variance path V_0 ... V_{m/2-1}, `Z1` = W1, `ZV` = T, `dt` = 2 dt
for the drift, `sdt` = the FINE sdt for the noise (sqrt(2 dt) z_c = sdt W), `kdt` = 2 kappa dt -- so that heston_ref._side_bound and
heston_path_ref.x_bounds / asian_bound apply to it line by line.  What differs is the local error of the variance increment: where a
fine step has lz = 2 (|c1 z1| + |c2 z2|) + |t|, a coarse step has lz_a + lz_b + |T| (the two fine increments' own errors and the
rounded sum), and the log price is charged one more roundoff s sdt |W1| per step for W1's own rounding (spare when `prec` is the
kernel's precision).  bound(level, tol) = the fine walk's Asian bound + the coarse walk's + tol (sum over the directions of
|P_fine - P_coarse| / directions + |Y|) for the subtractions and the mean; the kink mask is the union of the two legs'.

MUTATIONS of the coarse leg: `first_only` (only the first fine step of each pair: W1 = z1_a, T = t_a), `dt_once` (2 dt not doubled:
kdt, ktdt and dt/2 the fine walk's), `date_late` (every date but the last read one coarse step late), `half_twice` (W scaled by
1/sqrt 2 once more: W1 / sqrt 2, T / sqrt 2).
"""
import math
from collections import namedtuple

import numpy as np

import heston_path_ref as hp
import heston_ref as hr
from greeks_ref import NPB, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_HESTON_LEVEL = 17
MUTATIONS = ("first_only", "dt_once", "date_late", "half_twice")
# (n_dates, steps_per_date) of the per-path GPU test, the smallest shapes that reach every branch: one fine pair (the fp64 remainder
# alone); m = 2 (mod 4); a date inside an fp64 trip; a date in the remainder; whole trips only (twice); many trips
SHAPES = [(1, 2), (1, 6), (3, 2), (2, 10), (1, 64), (4, 16), (1, 256)]
VIOLATED_F32_MAX_STEPS = 32   # at 64 fine steps 2 - 5 % of VIOLATED's fp32 paths are kink paths (either leg): too close to KINK_CAP; far beyond it at 256
MLMC_CASE = dict(mkt=hr.OTM, model=hr.VIOLATED, n_dates=1, steps_per_date=4, eps=0.05, min_levels=2, max_levels=8, n_pilot=10_000)
MLMC_SEED = 20081   # numpy's in the model-only test, the stream's in the GPU test

Level = namedtuple("Level", "fine coarse")


def runs(name, X, m):
    """Whether the per-path GPU test runs this (case, precision, fine step count)."""
    return not (name == "VIOLATED" and X == "f32" and m > VIOLATED_F32_MAX_STEPS)


def level_normals(draw, first, n, m, npb):
    """Path p is unit p of domain 17; FINE step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of block 2(j-1) // npb as z1
    and z2: the Heston layout.  Returns (z1, z2), each of shape (n, m)."""
    z = basket_normals(lambda _, u, c, b: draw(DOMAIN_HESTON_LEVEL, u, c, b), first, n, 2 * m, npb)
    return z[:, 0::2], z[:, 1::2]


def _coarse_side(o, model, m, z1, z2, mutation, dtype, prec):
    """The coarse walk of one direction on the fine normals z1, z2 of shape (n, m), m even, as a heston_ref side (module docstring)."""
    s0, k, r, t = (float(o[c]) for c in "skrt")
    v0, kappa, theta, xi, rho = (float(model[f]) for f in hr.MODEL_FIELDS)
    n, mc = z1.shape[0], m // 2
    dt = t / m
    sdt = math.sqrt(dt)
    dtc = dt if mutation == "dt_once" else 2.0 * dt
    R = dtype
    kdt, ktdt = R(kappa * dtc), R(kappa * theta * dtc)
    c1, c2 = R(xi * sdt * rho), R(xi * sdt * math.sqrt(1.0 - rho * rho))
    Z1, Z2 = np.ascontiguousarray(z1.T, dtype=R), np.ascontiguousarray(z2.T, dtype=R)   # (m, n)
    tf = c1 * Z1 + c2 * Z2
    W1 = (Z1[0::2].astype(prec) + Z1[1::2].astype(prec)).astype(R)     # rounded once, in the precision of the call
    T = tf[0::2] + tf[1::2]
    if mutation == "first_only":
        W1, T = Z1[0::2].copy(), tf[0::2].copy()
    if mutation == "half_twice":
        W1, T = W1 * R(math.sqrt(0.5)), T * R(math.sqrt(0.5))
    V = np.empty((mc + 1, n), dtype=R)
    V[0] = v0
    zero = R(0)
    for i in range(mc):
        v = V[i]
        vp = np.maximum(v, zero)
        V[i + 1] = (v + ktdt) - kdt * vp + np.sqrt(vp) * T[i]
    Vprev = V[:mc]
    Vp = np.maximum(Vprev, zero)
    S = np.sqrt(Vp)
    A, B = np.cumsum(Vp, axis=0, dtype=R), np.cumsum(S * W1, axis=0, dtype=R)
    x = R(math.log(s0) + r * t) - R(0.5 * dtc) * A[-1] + R(sdt) * B[-1]
    ST = np.exp(x)
    value = np.maximum(ST - R(k), zero)
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    Vprev, Vp, S, T, W1, Z1, Z2, tf = f8(Vprev), f8(Vp), f8(S), f8(T), f8(W1), f8(Z1), f8(Z2), f8(tf)
    lzf = 2.0 * (np.abs(f8(c1) * Z1) + np.abs(f8(c2) * Z2)) + np.abs(tf)      # a fine increment's own error, heston_ref's lz
    lz = lzf[0::2] + lzf[1::2] + np.abs(T)                                     # ... of both, and the rounded sum
    kd, kt = float(kdt), float(ktdt)
    locV = 2.0 * (np.abs(Vprev) + kt + kd * Vp) + 2.0 * kt + 2.0 * kd * Vp + S * lz + 3.0 * np.abs(S * T) + np.abs(f8(V[1:]))
    direct = (0.5 * dtc * np.abs(f8(A)) + sdt * (3.0 * S * np.abs(W1) + np.abs(f8(B)))).sum(axis=0)   # 3 = heston_ref's 2 + W1's rounding
    direct += 1.0 + abs(math.log(s0) + r * t) + 3.0 * 0.5 * dtc * np.abs(f8(A[-1])) + 3.0 * sdt * np.abs(f8(B[-1])) + 2.0 * np.abs(f8(x))
    return dict(value=f8(value), ST=f8(ST), V=Vprev, ZV=T, Z1=W1, locV=locV, direct=direct, k=k, v0=v0, kdt=kappa * dtc, dt=dtc, sdt=sdt,
                truncated=(Vprev < 0).any(axis=0), bounds={})


def walk(o, model, n_dates, spd, z1, z2, anti=False, mutation=None, dtype=np.float64, prec=np.float64):
    """Level(fine, coarse): per leg one heston_path_ref side per path direction.  spd even.  prec: the precision in which the device
    forms W1 (np.float32 for the _f32 calls); dtype = np.float32 evaluates every formula of both legs in float32."""
    n_dates, spd = int(n_dates), int(spd)
    assert spd % 2 == 0
    m = n_dates * spd
    if dtype != np.float64:
        prec = dtype
    z1, z2 = np.asarray(z1, dtype=np.float64)[:, :m], np.asarray(z2, dtype=np.float64)[:, :m]
    fine = hp.walk(o, model, n_dates, spd, z1, z2, anti, None, dtype)
    coarse = []
    for sign in (1.0, -1.0)[:2 if anti else 1]:
        s = _coarse_side(o, model, m, sign * z1, sign * z2, mutation, dtype, prec)
        d = hp._dates(s, o, n_dates, spd // 2, dtype, mutation == "date_late")
        coarse.append(dict(d, base=s, n_dates=n_dates, spd=spd // 2, o=o, xb={}))
    return Level(fine, coarse)


def value(lv):
    """Per-path Y = P_fine - P_coarse; antithetic: the mean over the two directions."""
    return hp.asian(lv.fine) - hp.asian(lv.coarse)


def bound(lv, tol):
    """Per-path bound on |kernel value - value(lv)| for a kernel of unit roundoff tol, and the mask of the kink paths (either leg)."""
    bf, kf = hp.asian_bound(lv.fine, tol)
    bc, kc = hp.asian_bound(lv.coarse, tol)
    sub = sum(np.abs(hp.asian([f]) - hp.asian([c])) for f, c in zip(lv.fine, lv.coarse)) / len(lv.fine)
    return bf + bc + tol * (sub + np.abs(value(lv))), np.logical_or(kf, kc)


def plain_of(lv):
    """The plain estimator's level from an antithetic walk: the first direction of both legs."""
    return Level(lv.fine[:1], lv.coarse[:1])


def check(got, lv, tol, what):
    """The per-path rule: every value finite and within bound of the model's; the kink paths under heston_ref.KINK_CAP.  Returns
    (worst error / bound, number of kink paths); asserts."""
    got = np.asarray(got, dtype=np.float64)
    assert np.all(np.isfinite(got)), what
    b, kink = bound(lv, tol)
    r = np.abs(got - value(lv)) / b
    assert np.all(r <= 1.0), (what, int(np.argmax(r)), float(r.max()))
    assert kink.sum() <= hr.KINK_CAP * got.size, what
    return float(r.max()), int(kink.sum())


# ---- the same values without the bookkeeping of the bound (variances, the driver) ------------------------------------------------
def fast_values(o, model, n_dates, spd, z1, z2, coarse=True):
    """(P_fine, P_coarse) per path in float64, plain, step by step as the header states the two walks (x_j itself is walked).
    coarse = False: P_fine alone (level 0), any spd."""
    s0, k, r, t = (float(o[c]) for c in "skrt")
    v0, kappa, theta, xi, rho = (float(model[f]) for f in hr.MODEL_FIELDS)
    m = n_dates * spd
    dt = t / m
    sdt, rp = math.sqrt(dt), math.sqrt(1.0 - rho * rho)
    n = z1.shape[0]
    V, x, Vc, xc = (np.full(n, v) for v in (v0, math.log(s0), v0, math.log(s0)))
    acc, accc = np.zeros(n), np.zeros(n)
    W1 = T = 0.0
    for j in range(m):
        a = z1[:, j]
        tj = xi * sdt * (rho * a + rp * z2[:, j])
        Vp = np.maximum(V, 0.0)
        s = np.sqrt(Vp)
        x = x + (r - 0.5 * Vp) * dt + s * sdt * a
        V = V + kappa * (theta - Vp) * dt + s * tj
        if coarse:
            W1, T = (a, tj) if j % 2 == 0 else (W1 + a, T + tj)
            if j % 2 == 1:
                Vp = np.maximum(Vc, 0.0)
                s = np.sqrt(Vp)
                xc = xc + (r - 0.5 * Vp) * 2.0 * dt + s * sdt * W1
                Vc = Vc + kappa * (theta - Vp) * 2.0 * dt + s * T
        if (j + 1) % spd == 0:
            acc = acc + np.exp(x)
            accc = accc + np.exp(xc)
    pf = np.maximum(acc / n_dates - k, 0.0)
    return (pf, np.maximum(accc / n_dates - k, 0.0)) if coarse else (pf, None)


# ---- mc_mlmc_plan and mc_heston_mlmc_run_*, restated -----------------------------------------------------------------------------
def mlmc_plan(var, cost, eps):
    """n_l = ceil(2 eps^-2 sqrt(V_l / C_l) sum_k sqrt(V_k C_k)); ValueError where the C function returns MC_ERR_INVALID."""
    var, cost = [float(v) for v in var], [float(c) for c in cost]
    if not var or len(var) != len(cost) or not (eps > 0 and math.isfinite(eps)):
        raise ValueError("levels or eps")
    if any(not (v >= 0 and math.isfinite(v)) for v in var) or any(not (c > 0 and math.isfinite(c)) for c in cost):
        raise ValueError("variance or cost")
    total = sum(math.sqrt(v * c) for v, c in zip(var, cost))
    return [int(math.ceil(2.0 / (eps * eps) * math.sqrt(v / c) * total)) for v, c in zip(var, cost)]


def level_cost(n_steps, l):
    return (1.0 if l == 0 else 1.5) * n_steps * 2 ** l


def mlmc(sample, n_steps, eps, min_levels, max_levels, n_pilot, plan=mlmc_plan):
    """The header's algorithm on sample(l, first, n) -> (sum, sum2) of the DISCOUNTED values of level l's paths [first, first + n) of
    its own range.  Returns dict(price, stderr, bias, converged, levels=[dict(sum, sum2, n, mean, var)])."""
    lv = []

    def extend(l, more):
        s, s2 = sample(l, lv[l]["n"], more)
        e = lv[l]
        e["sum"], e["sum2"], e["n"] = e["sum"] + s, e["sum2"] + s2, e["n"] + more
        n = float(e["n"])
        e["mean"], e["var"] = e["sum"] / n, max(n * e["sum2"] - e["sum"] ** 2, 0.0) / (n * (n - 1.0))

    def open_level():
        lv.append(dict(sum=0.0, sum2=0.0, n=0, cost=level_cost(n_steps, len(lv))))
        extend(len(lv) - 1, n_pilot)

    for _ in range(max(min_levels, 2) + 1):
        open_level()
    while True:
        grew = True
        while grew:
            want = plan([e["var"] for e in lv], [e["cost"] for e in lv], eps)
            grew = False
            for l, w in enumerate(want):
                if w > lv[l]["n"]:
                    extend(l, w - lv[l]["n"])
                    grew = True
        bias = max(abs(lv[-1]["mean"]), 0.5 * abs(lv[-2]["mean"]))
        converged = bias <= eps / math.sqrt(2.0)
        if converged or len(lv) - 1 == max_levels:
            break
        open_level()
    return dict(price=sum(e["mean"] for e in lv), stderr=math.sqrt(sum(e["var"] / e["n"] for e in lv)), bias=bias, converged=converged, levels=lv)
