"""Independent float64 model of the basket pricing sample (not a test module).

Written from the model statement in include/mc_mi355x.h (mc_basket_*, mc_context_set_antithetic, mc_context_set_control_variate),
not from the kernels or the oracle.  With bt = L g + d and s_a(T) = S_a exp((r - v_a^2/2) T + v_a sqrt(T) bt_a):
  plain       max(B - K, 0),  B = sum_a w_a s_a(T)                              (row 0 of greeks_ref.basket, with its scale)
  control     max(B - K, 0) - max(G - K, 0),  G = W prod_a s_a(T)^(w_a/W),  W = sum_a w_a
  antithetic  the mean of the value at g and at -g
`value` returns a greeks_ref.Paths of one row: the payoff is continuous, so jump = 0 and edge = inf -- no path is ever left out of
a comparison; scale is the forward-error scale a kernel of unit roundoff u stays within a small multiple of u of.

The second half states what the kernels do with the model -- constants folded on the host into (m, base, coef, wg), the path
evaluated as coef . exp(base + m g) -- only so that INDEX ERRORS can be written down: MUTATIONS are named mistakes in how the folded
constants are laid out or read, `value_folded` the plain payoff through (possibly mutated) constants.  test_basket_ref.py shows that
the suite's symmetric market (test_gpu_parity.basket_inputs) cannot see any of them and that the markets of `random_market` reject
every one on almost every path; test_gpu_basket_ref.py then holds the kernels to `value` on those markets.
"""
import math

import numpy as np

import greeks_ref as gr

ESTIMATORS = [(False, False), (True, False), (False, True), (True, True)]   # (antithetic, control)
LOG2E = 1.4426950408889634074


def _arrays(b):
    S, v, d, w = (np.asarray(b[c], dtype=np.float64) for c in "svdw")
    L = np.tril(np.asarray(b["p"], dtype=np.float64).reshape(len(S), len(S)))
    return S, v, d, w, L, float(b["k"]), float(b["t"]), float(b["r"])


def geometric(b, g):
    """(G, scale of max(G - K, 0)) per path: ln G = ln W + sum_a (w_a/W) ln s_a(T); the scale is the geometric side's own forward
    error, G (1 + sum_a (w_a/W) ex_a) + |K|, ex_a the relative error of s_a(T) in units of eps as in greeks_ref.basket."""
    S, v, d, w, L, k, t, r = _arrays(b)
    g = np.asarray(g, dtype=np.float64)
    sqt = math.sqrt(t)
    W = w.sum()
    q = w / W
    lg = g @ L.T
    lg_abs = np.abs(g) @ np.abs(L).T
    mu = (r - 0.5 * v * v) * t
    x = mu + v * sqt * (lg + d)
    ex = 1.0 + np.abs(x) + np.abs(mu) + v * sqt * (lg_abs + np.abs(d))
    G = np.exp(math.log(W) + (q * (np.log(S) + x)).sum(axis=1))
    return G, G * (1.0 + (q * ex).sum(axis=1)) + abs(k)


def _side(b, g, control):
    p = gr.basket(b, g)
    value, scale = p.value[0], p.scale[0]
    if control:
        G, s_geo = geometric(b, g)
        value = value - np.maximum(G - float(b["k"]), 0.0)
        scale = scale + s_geo
    return value, scale


def value(b, g, anti=False, control=False):
    """Per-path values of the basket call on the normals g (n_paths, n_assets), as a one-row greeks_ref.Paths."""
    g = np.asarray(g, dtype=np.float64)
    val, scale = _side(b, g, control)
    if anti:
        v2, s2 = _side(b, -g, control)
        val, scale = 0.5 * (val + v2), 0.5 * (scale + s2)
    n = g.shape[0]
    return gr.Paths(val[None, :], scale[None, :], np.zeros((1, n)), np.full(n, np.inf))


def control_mean(b):
    """E[max(G - K, 0)], undiscounted: G is lognormal, ln G ~ N(m, s2) with
         m  = ln W + sum_a (w_a/W) (ln S_a + (r - v_a^2/2) T + v_a sqrt(T) d_a),    s2 = T sum_b (sum_a (w_a/W) v_a L_ab)^2,
       so the mean is exp(m + s2/2) Phi(d1) - K Phi(d2), d1 = (m - ln K + s2) / sqrt(s2), d2 = d1 - sqrt(s2)."""
    S, v, d, w, L, k, t, r = _arrays(b)
    W = float(w.sum())
    q = w / W
    m = math.log(W) + float((q * (np.log(S) + (r - 0.5 * v * v) * t + v * math.sqrt(t) * d)).sum())
    c = (q * v) @ L
    s2 = t * float(c @ c)
    if s2 == 0.0:
        return max(math.exp(m) - k, 0.0)
    sd = math.sqrt(s2)
    d1 = (m - math.log(k) + s2) / sd
    phi = lambda x: 0.5 * math.erfc(-x / math.sqrt(2.0))  # noqa: E731
    return math.exp(m + 0.5 * s2) * phi(d1) - k * phi(d1 - sd)


def as_seen(b, X):
    """The market as the entry points of precision X read it: every input rounded to that type (fp64: unchanged)."""
    R = np.float32 if X == "f32" else np.float64
    out = {c: np.asarray(b[c], dtype=R).astype(np.float64).tolist() for c in "svpdw"}
    out.update({c: float(R(b[c])) for c in "ktr"})
    return out


# ---- random asymmetric markets ----------------------------------------------------------------------------------------
MONEYNESS = [0.3, 0.8, 1.0, 1.1, 1.5]


def random_market(rng, n, chol, positive_weights=False):
    """greeks_ref.random_basket's recipe: distinct spots 20..300, vols 0.05..0.8, d in +-0.05, unequal weights (one of them zero
    unless positive_weights -- the control variate needs w[a] > 0), a random correlation factored by `chol` (the product's
    mc.chol), a strike from deep in (0.3 of the forward basket) to deep out of the money (1.5)."""
    S = rng.uniform(20, 300, n)
    v = rng.uniform(0.05, 0.8, n)
    d = rng.uniform(-0.05, 0.05, n)
    w = rng.uniform(0.2, 1.5, n)
    if n > 1 and not positive_weights:
        w[rng.integers(n)] = 0.0
    w /= w.sum()
    A = rng.normal(size=(n, n + 2))
    C = A @ A.T
    C /= np.sqrt(np.outer(np.diag(C), np.diag(C)))
    L, bad = chol(C)
    assert bad == 0
    return dict(s=S.tolist(), v=v.tolist(), p=np.asarray(L, dtype=np.float64).tolist(), d=d.tolist(), w=w.tolist(),
                k=float(w @ S) * float(rng.choice(MONEYNESS)), t=float(rng.uniform(0.1, 1.5)), r=float(rng.uniform(-0.01, 0.06)))


def in_the_money(b):
    """The same market struck deep in the money (0.3 of the spot basket).  An out-of-the-money path is worth 0 whatever the
    constants are; here (almost) every path pays, so a wrong constant shows on (almost) every path."""
    return dict(b, k=MONEYNESS[0] * float(np.dot(b["w"], b["s"])))


# ---- the folded form and its index errors -------------------------------------------------------------------------------
def folded(b):
    """(m, base, coef, wg) in fp64, natural-log units, zero-padded to whole 4 x 4 tiles (np = 4 ceil(n / 4)):
    m[a][c] = v_a sqrt(T) L[a][c] (lower triangle), base[a] = (r - v_a^2/2) T + v_a sqrt(T) d_a, coef[a] = w_a S_a, wg[a] = w_a / W.
    Padded rows carry coef = 0, padded columns multiply by 0: they add exact zeros."""
    S, v, d, w, L, k, t, r = _arrays(b)
    n = len(S)
    npad = 4 * ((n + 3) // 4)
    sqt = math.sqrt(t)
    m, base, coef, wg = np.zeros((npad, npad)), np.zeros(npad), np.zeros(npad), np.zeros(npad)
    m[:n, :n] = (v * sqt)[:, None] * L
    base[:n] = (r - 0.5 * v * v) * t + v * sqt * d
    coef[:n] = w * S
    wg[:n] = w / w.sum()
    return m, base, coef, wg


def _swap_tiles(n, m, base, coef, wg):
    m = m.copy()
    m[8:12, 0:4], m[12:16, 0:4] = m[12:16, 0:4].copy(), m[8:12, 0:4].copy()
    return m, base, coef, wg


def _stale_half_tile(n, m, base, coef, wg):
    m = m.copy()
    m[12:16, 2:4] = m[8:12, 2:4]
    return m, base, coef, wg


def _swap_vectors(a, c, with_wg):
    def f(n, m, base, coef, wg):
        base, coef, wg = base.copy(), coef.copy(), wg.copy()
        for x in (base, coef) + ((wg,) if with_wg else ()):
            x[a], x[c] = x[c], x[a]
        return m, base, coef, wg
    return f


def _swap_entry(n, m, base, coef, wg):
    a = n - 3                     # rows a and a + 2 = n - 1, the column next to row a's diagonal
    m = m.copy()
    m[a, a - 1], m[a + 2, a - 1] = m[a + 2, a - 1], m[a, a - 1]
    return m, base, coef, wg


def _swap_assets(n, m, base, coef, wg):
    return _swap_vectors(n - 3, n - 1, True)(n, m, base, coef, wg)


# name -> (smallest n it applies to, f(n, m, base, coef, wg) -> the constants a kernel with that index error would see)
MUTATIONS = {
    "tiles (2,0) and (3,0) exchanged": (16, _swap_tiles),                # block rows 2 and 3 exchange their tile in block column 0
    "half tile (3,1) read from (2,1)": (16, _stale_half_tile),           # a prefetch index one block row behind
    "base/coef of assets 5 and 7 exchanged": (16, _swap_vectors(5, 7, False)),
    "m[a][b] and m[a+2][b] exchanged": (4, _swap_entry),
    "base/coef/wg of assets a and a+2 exchanged": (4, _swap_assets),
}


def mutations(n):
    """The named index errors that apply to a basket of n assets."""
    return {name: f for name, (n_min, f) in MUTATIONS.items() if n >= n_min}


def value_folded(b, g, mutate=None):
    """The plain payoff max(coef . exp(base + m g) - K, 0) per path, in fp64, through the folded constants (after `mutate`)."""
    n = len(b["s"])
    m, base, coef, wg = folded(b)
    if mutate is not None:
        m, base, coef, wg = mutate(n, m, base, coef, wg)
    gp = np.zeros((np.shape(g)[0], len(base)))
    gp[:, :n] = np.asarray(g, dtype=np.float64)
    B = (coef * np.exp(base + gp @ m.T)).sum(axis=1)
    return np.maximum(B - float(b["k"]), 0.0)


def value_folded_f32(b, g):
    """An fp32 emulation of the same formula, the way an fp32 kernel may run it: constants folded in fp64, times log2(e), rounded
    once; per asset an fma chain over the columns in float32; exp2 in float32; the basket as an fma chain; the plain max.  (numpy
    has no fma: the product of two floats is exact in a double, the sum is rounded to double and then to float -- one rounding,
    except on a tie of the second.)"""
    f32 = np.float32
    n = len(b["s"])
    m, base, coef, wg = folded(b)
    m32, base32, coef32 = (m * LOG2E).astype(f32), (base * LOG2E).astype(f32), coef.astype(f32)
    fma = lambda a, c, s: (a.astype(np.float64) * c.astype(np.float64) + s.astype(np.float64)).astype(f32)  # noqa: E731
    g32 = np.zeros((np.shape(g)[0], len(base)), dtype=f32)
    g32[:, :n] = np.asarray(g, dtype=f32)
    x = np.broadcast_to(base32, g32.shape).copy()
    for c in range(n):
        x = fma(np.broadcast_to(m32[:, c], x.shape), np.broadcast_to(g32[:, c:c + 1], x.shape), x)
    E = np.exp2(x)
    assert E.dtype == f32
    B = np.zeros(g32.shape[0], dtype=f32)
    for a in range(n):
        B = fma(np.broadcast_to(coef32[a], B.shape), E[:, a], B)
    return np.maximum(B - f32(b["k"]), f32(0)).astype(np.float64)
