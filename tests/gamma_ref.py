"""Independent float64 reference of the second-order Greeks estimators (not a test module).

Written from the model: the mixed estimator (Glasserman 7.3, the likelihood-ratio derivative of the pathwise delta) stated
above vanilla_greeks_kernel (its SECOND_ORDER form) and basket_gamma_kernel (csrc/mc_kernels.hpp) and in include/mc_mi355x.h,
evaluated in float64 with numpy on a given array of normals (greeks_ref's normal streams: vanilla_normals, basket_normals).

Every function returns a greeks_ref `Paths` (value, scale, jump, edge), so that greeks_ref.bound turns it into per-path bounds:
  vanilla_greeks2  rows price, delta, vega, gamma, vanna
  basket_gamma     rows price, then the entries gamma[a][b], a <= b, in row-major order (the kernel's planes)
"""
import math

import numpy as np

from greeks_ref import Paths, INV_SQRT_2PI


def _ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def black_scholes(o):
    """Closed forms of the call: (price, delta, vega, gamma, vanna)."""
    s, k, r, v, t = (float(o[c]) for c in "skrvt")
    sqt = math.sqrt(t)
    d1 = (math.log(s / k) + (r + 0.5 * v * v) * t) / (v * sqt)
    d2 = d1 - v * sqt
    phi = INV_SQRT_2PI * math.exp(-0.5 * d1 * d1)
    price = s * _ncdf(d1) - k * math.exp(-r * t) * _ncdf(d2)
    return price, _ncdf(d1), s * phi * sqt, phi / (s * v * sqt), -phi * d2 / v


# ---- vanilla call -----------------------------------------------------------------------------------------------------
def vanilla_greeks2(o, z):
    """S_T = S exp((r - v^2/2) T + v sqrt(T) z), I = [S_T > K]:
    price I (S_T - K), delta I S_T / S, vega I S_T (sqrt(T) z - v T),
    gamma I S_T / S^2 (z / (v sqrt T) - 1),  vanna I S_T / S ((z^2 - 1) / v - z sqrt T)."""
    s, k, r, v, t = (float(o[c]) for c in "skrvt")
    z = np.asarray(z, dtype=np.float64)
    sqt = math.sqrt(t)
    x = (r - 0.5 * v * v) * t + v * sqt * z
    st = s * np.exp(x)
    itm = st > k
    ex = 1.0 + np.abs(x) + abs((r - 0.5 * v * v) * t) + v * sqt * np.abs(z)   # relative error of S_T, in units of eps
    s_pay = st * ex + abs(k)
    dl = st / s
    vg = st * (sqt * z - v * t)
    fg = z / (s * v * sqt) - 1.0 / s            # the gamma score
    fv = (z * z - 1.0) / v - z * sqt            # the vanna score
    n = z.size
    value, scale, jump = np.zeros((5, n)), np.zeros((5, n)), np.zeros((5, n))
    value[0], scale[0] = np.where(itm, st - k, 0.0), s_pay
    rows = [(dl, dl * ex),
            (vg, st * ex * (sqt * np.abs(z) + v * t)),
            (dl * fg, dl * ex * np.abs(fg) + 2.0 * dl * (np.abs(z) / (s * v * sqt) + 1.0 / s)),
            (dl * fv, dl * ex * np.abs(fv) + 2.0 * dl * ((z * z + 1.0) / v + np.abs(z) * sqt))]
    for q, (val, sc) in enumerate(rows, start=1):
        value[q], scale[q], jump[q] = np.where(itm, val, 0.0), sc, np.abs(val)
    return Paths(value, scale, jump, np.abs(st - k) / s_pay)


# ---- basket call ------------------------------------------------------------------------------------------------------
def upper_index(n):
    """(a, b) of the planes 1.. of basket_gamma, a <= b in row-major order."""
    return [(a, b) for a in range(n) for b in range(a, n)]


def basket_gamma(bk, g):
    """bt = L g + d,  s_a = S_a exp((r - v_a^2/2) T + v_a sqrt(T) bt_a),  B = sum_a w_a s_a,  I = [B > K],
    p_a = I w_a s_a / S_a,  y = L^-T g,  c_a = 1 / (S_a v_a sqrt T):
        gamma[a][b] = 1/2 (p_a y_b c_b + p_b y_a c_a) - [a == b] p_a / S_a.
    g has shape (n_paths, n_assets); only the lower triangle of the factor is used."""
    S, v, d, w = (np.asarray(bk[c], dtype=np.float64) for c in "svdw")
    na = len(S)
    L = np.tril(np.asarray(bk["p"], dtype=np.float64).reshape(na, na))
    k, t, r = float(bk["k"]), float(bk["t"]), float(bk["r"])
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[0]
    sqt = math.sqrt(t)
    lg = g @ L.T
    lg_abs = np.abs(g) @ np.abs(L).T
    mu = (r - 0.5 * v * v) * t
    x = mu + v * sqt * (lg + d)
    term = w * S * np.exp(x)
    ex = 1.0 + np.abs(x) + np.abs(mu) + v * sqt * (lg_abs + np.abs(d))
    B = term.sum(axis=1)
    itm = B > k
    s_pay = (np.abs(term) * ex).sum(axis=1) + abs(k)
    y = np.linalg.solve(L.T, g.T).T                      # y = L^-T g per path
    y_abs = np.abs(g) @ np.abs(np.linalg.inv(L).T).T     # its rounding scale
    c = 1.0 / (S * v * sqt)
    p = term / S                                         # the pathwise delta term with I = 1
    qs = y * c
    sp = np.abs(p) * ex                                  # rounding scales of p and of q = y c
    sq = (np.abs(y) + y_abs) * c
    ent = upper_index(na)
    value, scale, jump = np.zeros((1 + len(ent), n)), np.zeros((1 + len(ent), n)), np.zeros((1 + len(ent), n))
    value[0], scale[0] = np.where(itm, B - k, 0.0), s_pay
    for u, (a, b) in enumerate(ent, start=1):
        val = 0.5 * (p[:, a] * qs[:, b] + p[:, b] * qs[:, a])
        sc = (0.5 * (sp[:, a] * np.abs(qs[:, b]) + np.abs(p[:, a]) * sq[:, b] + sp[:, b] * np.abs(qs[:, a]) + np.abs(p[:, b]) * sq[:, a])
              + np.abs(p[:, a] * qs[:, b]) + np.abs(p[:, b] * qs[:, a]))
        if a == b:
            val = val - p[:, a] / S[a]
            sc = sc + 2.0 * (sp[:, a] + np.abs(p[:, a])) / S[a]
        value[u], scale[u], jump[u] = np.where(itm, val, 0.0), sc, np.abs(val)
    return Paths(value, scale, jump, np.abs(B - k) / s_pay)


def gamma_matrix(p):
    """The per-path n x n matrices of a basket_gamma Paths' values: shape (n_paths, n, n), both triangles."""
    m = p.value.shape[0] - 1
    na = int(round((math.sqrt(8 * m + 1) - 1) / 2))
    out = np.zeros((p.value.shape[1], na, na))
    for u, (a, b) in enumerate(upper_index(na), start=1):
        out[:, a, b] = out[:, b, a] = p.value[u]
    return out
