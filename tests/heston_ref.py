"""Independent float64 reference of the European call under the Heston model, full-truncation Euler (not a test module).

Written from the model stated in include/mc_mi355x.h, not from the kernel: m = n_steps equal steps, dt = T / m, sdt = sqrt(dt),
rho' = sqrt(1 - rho^2), x_0 = ln S0, V_0 = v0, and for j = 1 ... m with the step's normals (z1_j, z2_j)
    V+ = max(V_{j-1}, 0),  s = sqrt(V+),
    x_j = x_{j-1} + (r - V+/2) dt + s sdt z1_j,
    V_j = V_{j-1} + kappa (theta - V+) dt + xi sdt s (rho z1_j + rho' z2_j),
value (exp(x_m) - K)^+, antithetic: the mean of the value at (z1, z2) and at (-z1, -z2); evaluated with numpy on given arrays
of normals.  The variance is walked step by step as written; the log price is NOT: `walk` forms x_m = ln S0 + r T - (dt/2) sum V+
+ sdt sum s z1 from the two cumulative sums, the same real number in another association (the bound below charges every
partial sum of both).  The header's own recurrence for x_j is `_fast_values`, which tests/test_heston_ref.py ties to `walk` at 1e-12.  `walk` returns a HestonPaths: `value` of shape (1, n_paths) like a one-plane product of greeks_ref,
and per path direction what `bound` needs.

The forward error.  The step is non-linear in V, so greeks_ref's "roundoff times a scale" does not apply as it stands.  A kernel
that evaluates the same formulas in a precision of unit roundoff u -- in any association: it may keep the running sums
A = sum V+ and B = sum s z1 and form x_m = ln S0 + r T - (dt/2) A + sdt B at the end -- commits at every step LOCAL errors,
in units of u:
  - zv = xi sdt (rho z1 + rho' z2):  lz = 2 (|c1 z1| + |c2 z2|) + |zv|   (c1 = xi sdt rho, c2 = xi sdt rho': two rounded constants,
    two products, one sum);
  - into V_j:  lV = 2 (|V_{j-1}| + kappa theta dt + kappa dt V+) + 2 kappa theta dt + 2 kappa dt V+ + s lz + 3 |s zv| + |V_j|
    (the rounded constants kappa dt and kappa theta dt, every product and partial sum, the root's own rounding 2 s carried into
    s zv); V_0 = v0 itself is rounded once: lV_0 = v0;
  - into x_m:  (dt/2) |A_j| + sdt (2 s |z1_j| + |B_j|)   (every partial sum of the two running sums is rounded -- what asian_ref
    charges for ln S_j -- and the root's own rounding and the product s z1), and at maturity
    1 + |ln S0 + r T| + 3 (dt/2) A + 3 sdt |B| + 2 |x_m|   (the rounded constants, the final two fmas, the exponent's conversion).
An error dV in V_i reaches x_m through the later steps.  To first order it is multiplied by
    G_i = g_{i+1} + J_{i+1} G_{i+1},  G_m = 0,   g_j = -dt/2 [V>0] + sdt z1_j / (2 sqrt V+),
    J_j = dV_j/dV_{j-1} = 1 - kappa dt [V>0] + zv_j / (2 sqrt V+)      (V = V_{j-1}; both sqrt terms absent where V <= 0)
with the SIGNS kept, so that mean reversion damps it; absolute values are taken only at the end: |dx_m| <= sum_i lV_i |G_i| + the
direct terms, and the value's error is S_T (exp(|dx_m|) - 1) + 2 S_T + |K| + |value| roundoffs.
The square root is not Lipschitz at 0.  An absolute error e in V moves s by at most min(e / sqrt V+, sqrt e), valid at every
V+ >= 0.  The running size of the error in V, E_j = |J_j| E_{j-1} + tol lV_j, says which branch is the smaller: a step with
|V_{j-1}| < E_{j-1} is on the sqrt(e) branch (for V_{j-1} <= -E_{j-1} both the model and the kernel truncate, and the step passes
the error on unchanged).  There J_j and g_j lose their root terms, and the step is charged LOCALLY
    into V_j: kappa dt E + |zv_j| sqrt(E),    into x_m: (dt/2) E + sdt |z1_j| sqrt(E),      E = E_{j-1},
with E_j = (1 + kappa dt) E + |zv_j| sqrt(E) + tol lV_j.  A path with at least one such step is a KINK PATH; its bound is no
longer linear in the tolerance, which is why this module exposes bound(paths, tol) and not a scale.  Every path has a bound.

Closed forms: `closed_form` is the price of the continuous model by Lewis's single integral (the C library integrates
Heston's P1 / P2), `black_scholes_call` is barrier_ref's, `euler_variance_path` the deterministic variance walk at xi = 0.

BIAS[case] = (b, h): the bias of the scheme at 64 steps, model mean minus closed form (discounted), and its 95 % half-width,
from this module's own walk in float64 on numpy normals, 4 194 304 antithetic pairs, seed 2024:
    python tests/heston_ref.py bias
"""
import math
import sys
from collections import namedtuple

import numpy as np

from barrier_ref import black_scholes_call   # noqa: F401  (re-exported for the tests)
from greeks_ref import NPB, basket_normals   # noqa: F401  (NPB re-exported for the tests)

DOMAIN_HESTON = 6
MODEL_FIELDS = ("v0", "kappa", "theta", "xi", "rho")
MUTATIONS = ("drift_V", "rho1", "no_half", "abs_root")

HestonPaths = namedtuple("HestonPaths", "value sides")


def heston_normals(draw, first, n, m, npb):
    """Path p is unit p of domain 6; step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of block 2(j-1) // npb as
    z1 and z2.  Returns (z1, z2), each of shape (n, m)."""
    z = basket_normals(lambda _, u, c, b: draw(DOMAIN_HESTON, u, c, b), first, n, 2 * m, npb)
    return z[:, 0::2], z[:, 1::2]


def _one_side(o, model, m, z1, z2, mutation=None, dtype=np.float64):
    """One path direction, step by step.  dtype = float32 evaluates the same formulas in float32 (tests of the bound)."""
    s0, k, r, t = (float(o[c]) for c in "skrt")
    v0, kappa, theta, xi, rho = (float(model[f]) for f in MODEL_FIELDS)
    n = z1.shape[0]
    dt = t / m
    sdt = math.sqrt(dt)
    rp = 1.0 if mutation == "rho1" else math.sqrt(1.0 - rho * rho)
    R = dtype
    kdt, ktdt, c1, c2 = R(kappa * dt), R(kappa * theta * dt), R(xi * sdt * rho), R(xi * sdt * rp)
    Z1, Z2 = np.ascontiguousarray(z1.T, dtype=R), np.ascontiguousarray(z2.T, dtype=R)   # (m, n)
    ZV = c1 * Z1 + c2 * Z2
    V = np.empty((m + 1, n), dtype=R)
    V[0] = v0
    zero = R(0)
    for j in range(m):   # the recurrence itself; everything else is taken from V afterwards
        v = V[j]
        vp = np.maximum(v, zero)
        root = np.sqrt(np.abs(v)) if mutation == "abs_root" else np.sqrt(vp)
        V[j + 1] = (v + ktdt) - kdt * (v if mutation == "drift_V" else vp) + root * ZV[j]
    Vprev = V[:m]
    Vp = np.maximum(Vprev, zero)
    S = np.sqrt(np.abs(Vprev)) if mutation == "abs_root" else np.sqrt(Vp)
    A, B = np.cumsum(Vp, axis=0, dtype=R), np.cumsum(S * Z1, axis=0, dtype=R)   # every partial sum, rounded in R
    half = R(0.0) if mutation == "no_half" else R(0.5 * dt)
    x = R(math.log(s0) + r * t) - half * A[-1] + R(sdt) * B[-1]
    ST = np.exp(x)
    value = np.maximum(ST - R(k), zero)
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    Vprev, Vp, S, ZV, Z1 = f8(Vprev), f8(Vp), f8(S), f8(ZV), f8(Z1)
    lz = 2.0 * (np.abs(f8(c1) * Z1) + np.abs(f8(c2) * f8(Z2))) + np.abs(ZV)
    kd, kt = float(kdt), float(ktdt)
    locV = 2.0 * (np.abs(Vprev) + kt + kd * Vp) + 2.0 * kt + 2.0 * kd * Vp + S * lz + 3.0 * np.abs(S * ZV) + np.abs(f8(V[1:]))
    # the local errors that go straight into x_m, in roundoffs
    direct = (0.5 * dt * np.abs(f8(A)) + sdt * (2.0 * S * np.abs(Z1) + np.abs(f8(B)))).sum(axis=0)
    direct += 1.0 + abs(math.log(s0) + r * t) + 3.0 * 0.5 * dt * np.abs(f8(A[-1])) + 3.0 * sdt * np.abs(f8(B[-1])) + 2.0 * np.abs(f8(x))
    return dict(value=f8(value), ST=f8(ST), V=Vprev, ZV=ZV, Z1=Z1, locV=locV, direct=direct, k=k, v0=v0, kdt=kappa * dt, dt=dt, sdt=sdt,
                truncated=(Vprev < 0).any(axis=0), bounds={})


def walk(o, model, m, z1, z2, anti=False, mutation=None, dtype=np.float64):
    """Per-path values of the Heston call on the normals z1, z2 (n_paths, >= m) and what `bound` needs."""
    m = int(m)
    z1, z2 = np.asarray(z1, dtype=np.float64)[:, :m], np.asarray(z2, dtype=np.float64)[:, :m]
    sides = [_one_side(o, model, m, z1, z2, mutation, dtype)]
    if anti:
        sides.append(_one_side(o, model, m, -z1, -z2, mutation, dtype))
    value = sum(s["value"] for s in sides) / len(sides)
    return HestonPaths(value.reshape(1, -1), sides)


def _side_bound(s, tol):
    """(bound on the value's error, kink mask) of one path direction: the module docstring, step by step."""
    if tol in s["bounds"]:
        return s["bounds"][tol]
    V, ZV, Z1, locV = s["V"], s["ZV"], s["Z1"], s["locV"]
    m, n = V.shape
    kdt, dt, sdt = s["kdt"], s["dt"], s["sdt"]
    pos = V > 0
    inv = np.where(pos, 0.5 / np.sqrt(np.where(pos, V, 1.0)), 0.0)
    J = 1.0 - kdt * pos + ZV * inv          # the linear branch; a kink step overwrites its row entries below
    g = -0.5 * dt * pos + sdt * Z1 * inv
    absV, absJ, absZV, absZ1 = np.abs(V), np.abs(J), np.abs(ZV), np.abs(Z1)
    charge = tol * locV                      # the error committed into V_{j+1} by step j, plus the kink charges
    # forward: the running size of the error in V decides the branch of the root at each step
    E = np.full(n, tol * s["v0"])
    extra_x = np.zeros(n)
    kink = np.zeros(n, dtype=bool)
    for j in range(m):
        kj = absV[j] < E
        if kj.any():
            rootE = np.sqrt(E)
            J[j][kj], g[j][kj] = 1.0, 0.0
            dV = kdt * E + absZV[j] * rootE
            charge[j] += np.where(kj, dV, 0.0)
            extra_x += np.where(kj, 0.5 * dt * E + sdt * absZ1[j] * rootE, 0.0)
            E = np.where(kj, E + dV, absJ[j] * E) + tol * locV[j]
            kink |= kj
        else:
            E = absJ[j] * E + tol * locV[j]
    # backward: the signed sensitivity G_i of x_m to an error in V_i; at the top of trip j, G = G_{j+1}
    G = np.zeros(n)
    dx = extra_x + tol * s["direct"]
    for j in range(m - 1, -1, -1):
        dx += charge[j] * np.abs(G)
        G = g[j] + J[j] * G
    dx += tol * s["v0"] * np.abs(G)
    with np.errstate(over="ignore"):
        b = s["ST"] * np.expm1(dx) + tol * (2.0 * s["ST"] + abs(s["k"]) + s["value"])
    s["bounds"][tol] = (b, kink)
    return b, kink


def bound(p, tol):
    """Per-path bound on |kernel value - p.value| for a kernel of unit roundoff tol, and the mask of the kink paths."""
    parts = [_side_bound(s, tol) for s in p.sides]
    b = sum(x[0] for x in parts) / len(parts) + tol * np.abs(p.value[0])
    kink = np.logical_or.reduce([x[1] for x in parts])
    return b, kink


def plain_of(p):
    """The plain estimator's paths from an antithetic walk: its first direction (the same normals, nothing else shared)."""
    return HestonPaths(p.sides[0]["value"].reshape(1, -1), p.sides[:1])


def truncated(p):
    """Mask of the paths on which some V_j (j < m) fell below zero, in any direction."""
    return np.logical_or.reduce([s["truncated"] for s in p.sides])


def euler_variance_path(model, m, T):
    """The deterministic variance of the scheme at xi = 0: the array V_0 ... V_{m-1} that the steps use, and the variance of the
    Euler log-price sum_j V+_{j-1} dt."""
    v0, kappa, theta = (float(model[f]) for f in ("v0", "kappa", "theta"))
    dt = float(T) / m
    V = np.empty(m)
    v = v0
    for j in range(m):
        V[j] = v
        v = v + kappa * (theta - max(v, 0.0)) * dt
    return V, float(np.maximum(V, 0.0).sum() * dt)


def closed_form(o, model, panels=None, upper=None):
    """Discounted price of the call in the continuous model by Lewis's single integral
        C = S - sqrt(S K) e^{-rT/2} / pi  int_0^inf Re[ e^{i u kk} phi(u - i/2) ] du / (u^2 + 1/4),   kk = ln(S/K) + r T,
    phi the characteristic function of ln S_T - ln S0 - r T (Schoutens' form of the exponent), numpy complex arithmetic,
    32-point Gauss-Legendre on `panels` equal panels (default: at most 0.05 wide, at least 4000) up to `upper` (default: where the
    integrand is far below 1e-20; |rho| = 1 decays slowly and takes a long range)."""
    s0, k, r, t = (float(o[c]) for c in "skrt")
    v0, kappa, theta, xi, rho = (float(model[f]) for f in MODEL_FIELDS)
    if xi == 0:
        kt = kappa * t
        w = theta + (v0 - theta) * (1.0 - math.exp(-kt)) / kt if kt > 0 else v0
        return black_scholes_call(dict(s=s0, k=k, r=r, v=math.sqrt(w), t=t))
    kk = math.log(s0 / k) + r * t

    def integrand(u):
        w = u - 0.5j
        d = np.sqrt((rho * xi * 1j * w - kappa) ** 2 + xi * xi * (1j * w + w * w))
        bm = kappa - rho * xi * 1j * w - d
        gg = bm / (kappa - rho * xi * 1j * w + d)
        e = np.exp(-d * t)
        ln_phi = kappa * theta / (xi * xi) * (bm * t - 2.0 * np.log((1.0 - gg * e) / (1.0 - gg))) + v0 / (xi * xi) * bm * (1.0 - e) / (1.0 - gg * e)
        return (np.exp(1j * u * kk + ln_phi)).real / (u * u + 0.25)

    if upper is None:
        upper = 50.0
        while abs(integrand(np.array([upper]))[0]) > 1e-22 and upper < 1e6:
            upper *= 1.5
    if panels is None:
        panels = max(4000, int(upper / 0.05))
    x, wgt = np.polynomial.legendre.leggauss(32)
    h = upper / panels
    u = (np.arange(panels)[:, None] + 0.5 * (x[None, :] + 1.0)) * h
    total = float((integrand(u) * wgt[None, :]).sum() * 0.5 * h)
    return s0 - math.sqrt(s0 * k) * math.exp(-0.5 * r * t) / math.pi * total


# ---- the shapes of the GPU tests (tests/test_gpu_heston.py), shared with the checks on the reference alone --------------------
STRONG = dict(v0=0.09, kappa=3.0, theta=0.09, xi=0.2, rho=-0.7)
FELLER = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
VIOLATED = dict(v0=0.02, kappa=1.5, theta=0.04, xi=0.6, rho=-0.7)
POSRHO = dict(v0=0.05, kappa=2.5, theta=0.06, xi=0.25, rho=0.4)
MODELS = dict(STRONG=STRONG, FELLER=FELLER, VIOLATED=VIOLATED, POSRHO=POSRHO)
ATM = dict(s=100.0, k=100.0, r=0.05, t=1.0)
ITM = dict(s=100.0, k=90.0, r=0.05, t=1.0)
OTM = dict(s=100.0, k=110.0, r=0.05, t=1.0)
# (name, market, model): every model at the money, the three named ones also on an asymmetric strike
CASES = [("STRONG", ATM, STRONG), ("FELLER", ITM, FELLER), ("VIOLATED", OTM, VIOLATED), ("POSRHO", ATM, POSRHO)]
STEPS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024, 4096]   # the last one is MC_MAX_HESTON_STEPS
VIOLATED_F32_MAX_STEPS = 64   # beyond it more than 5 % of VIOLATED's fp32 paths are kink paths
KINK_CAP = 0.05
N_PATHS = 2121   # eight workgroups and a partial wave
N_PATHS_LONG = 329   # one workgroup and a partial wave, from 1024 steps on (the model walks step by step in Python)


# the many-trip GPU test (tests/test_gpu_walk_trips.py): per path against the model at the ends of the step loops, on the path counts of
# greeks_ref.TRIP_RANGES "A" and "C"; the same bits on every grid on "B" and "C"
TRIP_STEPS = [3, 8, 17]
TRIP_BITS_STEPS = [5, 9, 257]


def n_paths_for(m):
    return N_PATHS if m < 1024 else N_PATHS_LONG


def runs(name, X, m):
    """Whether the per-path GPU test runs this (case, precision, step count)."""
    return not (name == "VIOLATED" and X == "f32" and m > VIOLATED_F32_MAX_STEPS)


FIRSTS = (0, 12345, (1 << 32) - 100)   # the last range crosses the 2^32-unit seam


def cases_for(m):
    """(name, market, model) of the per-path GPU test at m steps, each of which runs on every first path of FIRSTS: the three
    named cases at every step count, the rho > 0 case below 1024 steps."""
    return CASES[:3] + (CASES[3:] if m < 1024 else [])


BIAS_STEPS = 64
BIAS = {   # at the money (ATM); printed by `python tests/heston_ref.py bias`
    "STRONG": (0.010081, 0.010330),
    "FELLER": (0.004682, 0.004974),
}


def _measure_bias(pairs=1 << 22, chunk=1 << 18, seed=2024):
    rng = np.random.default_rng(seed)
    for name, mkt, model in (("STRONG", ATM, STRONG), ("FELLER", ATM, FELLER)):
        tot, tot2 = 0.0, 0.0
        for _ in range(pairs // chunk):
            z1, z2 = rng.standard_normal((chunk, BIAS_STEPS)), rng.standard_normal((chunk, BIAS_STEPS))
            v = _fast_values(mkt, model, BIAS_STEPS, z1, z2)
            tot, tot2 = tot + v.sum(), tot2 + (v * v).sum()
        disc = math.exp(-mkt["r"] * mkt["t"])
        mean = tot / pairs
        sd = math.sqrt((tot2 / pairs - mean * mean) * pairs / (pairs - 1))
        print(f'    "{name}": ({disc * mean - closed_form(mkt, model):.6f}, {1.96 * disc * sd / math.sqrt(pairs):.6f}),')


def _fast_values(o, model, m, z1, z2):
    """The antithetic values of `walk` without the bookkeeping of the bound (same formulas)."""
    s0, k, r, t = (float(o[c]) for c in "skrt")
    v0, kappa, theta, xi, rho = (float(model[f]) for f in MODEL_FIELDS)
    dt = t / m
    sdt, rp = math.sqrt(dt), math.sqrt(1.0 - rho * rho)
    out = 0.0
    for sign in (1.0, -1.0):
        V, x = np.full(z1.shape[0], v0), np.full(z1.shape[0], math.log(s0))
        for j in range(m):
            a, b = sign * z1[:, j], sign * z2[:, j]
            Vp = np.maximum(V, 0.0)
            s = np.sqrt(Vp)
            x = x + (r - 0.5 * Vp) * dt + s * sdt * a
            V = V + kappa * (theta - Vp) * dt + xi * sdt * s * (rho * a + rp * b)
        out = out + 0.5 * np.maximum(np.exp(x) - k, 0.0)
    return out


if __name__ == "__main__" and sys.argv[1:] == ["bias"]:
    _measure_bias()
