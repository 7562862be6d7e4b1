"""Merton's jump-diffusion without a GPU: the closed form (mc_merton_closed_form_*, plain C in mc_hostmath_impl.h) against an
independent 30-digit quadrature of the characteristic function (merton_ref.lewis_price); the integer Poisson thresholds
(mc_merton_thresholds_*) against mpmath's Poisson law; the float64 reference model merton_ref.py on numpy's own normals and counts
-- its identities per path and its price against the closed form at 1 and 16 dates, which is the guard on the walk itself; the
soundness of the model's forward-error scale (a float32 evaluation of the same formulas stays inside the bound on every path of
every shape of tests/test_gpu_merton.py) and its power (four mutations fall outside it); the cap on near-barrier paths; the refusals
that need no device; the structs' layout.

The Monte Carlo check uses ONE fixed seed and 3 half-widths (1.96 sigma / sqrt(n) each, so 5.9 sigma): the margin is for nothing
but sampling noise."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import asian_ref as ar
import barrier_ref as br
import greeks_ref as gr
import merton_ref as mr
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def J(lam, mu, delta):
    return {"lambda": lam, "mu_j": mu, "delta": delta}


# four markets: the issue's example, r < 0, lambda t = 4, a short one with rare large jumps
MARKETS = [(br.ATM, J(1.0, -0.1, 0.15)),
           (dict(s=100.0, k=100.0, r=-0.015, v=0.17, t=1.3), J(0.8, 0.05, 0.2)),
           (dict(s=100.0, k=100.0, r=0.03, v=0.25, t=2.0), J(2.0, -0.03, 0.1)),
           (dict(s=100.0, k=100.0, r=0.04, v=0.1, t=0.25), J(0.5, -0.3, 0.4))]
STRIKES = [80.0, 100.0, 125.0]
CLOSED_FORM_BOUND = 1e-10   # the header's, at s = 100
MC_PATHS, MC_CHUNK = 1 << 20, 1 << 17
INVALID = "mc error 1"


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def rounded(o, X):
    """The inputs as the precision's struct holds them."""
    f = (lambda x: float(np.float32(x))) if X == "f32" else float
    return {c: f(x) for c, x in o.items()}


# ---- the closed form --------------------------------------------------------------------------------------------------------
def test_closed_form_matches_the_quadrature_of_the_characteristic_function(mc):
    assert abs(MARKETS[2][1]["lambda"] * MARKETS[2][0]["t"] - 4.0) < 1e-12 and MARKETS[1][0]["r"] < 0
    worst = 0.0
    for o, jp in MARKETS:
        for k in STRIKES:
            q = dict(o, k=k)
            got, want = mc.merton_closed_form(q, jp), mr.lewis_price(q, jp)
            print(f"{q} {jp}: closed form {got:.12f} quadrature {want:.12f} difference {got - want:.3g}")
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= CLOSED_FORM_BOUND, (q, jp, got, want)
    print(f"worst difference {worst:.3g}: the stated bound is {CLOSED_FORM_BOUND / worst:.3g} times that")
    assert CLOSED_FORM_BOUND <= 1e-8 and CLOSED_FORM_BOUND >= 10 * worst   # the header's bound is neither empty nor tight by accident
    # the struct of the other precision rounds the inputs, nothing else
    o, jp = (rounded(x, "f32") for x in MARKETS[0])
    assert abs(mc.merton_closed_form(o, jp, "f32") - mr.lewis_price(o, jp)) <= CLOSED_FORM_BOUND
    assert round(mc.merton_closed_form(*MARKETS[0]), 4) == 12.7613   # the issue's digits


def test_closed_form_without_jumps_is_black_scholes(mc):
    for o, jp in MARKETS:
        for k in STRIKES:
            q = dict(o, k=k)
            bs = br.black_scholes_call(q)
            assert abs(mc.merton_closed_form(q, dict(jp, **{"lambda": 0.0})) - bs) <= 1e-12
            assert abs(mc.merton_closed_form(q, J(jp["lambda"], 0.0, 0.0)) - bs) <= 1e-12   # jumps of size 1
    # n_dates, payoff and the barrier are ignored by the formula
    L = mc._lib
    price = C.c_double()
    f = L.lib().mc_merton_closed_form_f64
    opt = L.OPTION["f64"](100.0, 100.0, 0.05, 0.2, 1.0)
    assert f(C.byref(L.MERTON["f64"](opt, 1.0, -0.1, 0.15, 1, 0, 0, 0.0)), C.byref(price)) == 0
    a = price.value
    for n_dates, payoff, kind, B in ((4096, 1, 0, 0.0), (0, 2, 7, -1.0), (-3, 9, 0, 50.0)):
        assert f(C.byref(L.MERTON["f64"](opt, 1.0, -0.1, 0.15, n_dates, payoff, kind, B)), C.byref(price)) == 0 and price.value == a
    assert f(None, C.byref(price)) == 1


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_host_refusals(mc, X):
    o, jp = MARKETS[0]
    for bad in (dict(o, s=0.0), dict(o, t=0.0), dict(o, v=-0.1), dict(o, r=float("inf")), dict(o, k=float("nan")), dict(o, k=0.0)):
        with pytest.raises(mc.McError, match=INVALID):
            mc.merton_closed_form(bad, jp, X)
    for bad in (dict(jp, **{"lambda": -1.0}), dict(jp, delta=-0.1), dict(jp, mu_j=float("nan")), dict(jp, **{"lambda": float("inf")})):
        with pytest.raises(mc.McError, match=INVALID):
            mc.merton_closed_form(o, bad, X)
        with pytest.raises(mc.McError, match=INVALID):
            mc.merton_thresholds(o, bad, 4, X)
    for bad_m in (0, -1, mc._lib.MAX_MERTON_DATES + 1):
        with pytest.raises(mc.McError, match=INVALID):
            mc.merton_thresholds(o, jp, bad_m, X)
    assert mc.merton_closed_form(dict(o, v=0.0), jp, X) > 0 and mc.merton_closed_form(dict(o, v=0.0), J(1.0, 0.0, 0.0), X) > 0
    assert len(mc.merton_thresholds(o, jp, mc._lib.MAX_MERTON_DATES, X)) >= 1   # and the next call is served


# ---- the thresholds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X,W", [("f32", 32), ("f64", 64)])
def test_thresholds_against_the_poisson_law(mc, X, W):
    import mpmath as mp
    o = dict(br.ATM, t=1.0)
    for p in (2.0 ** -12, 0.01, 0.5, 1.0, 3.0, 5.0):
        lam = rounded({"lambda": p}, X)["lambda"]   # lambda dt as the library forms it: the struct's lambda, t = 1, one date
        T = [int(t) for t in mc.merton_thresholds(o, J(p, 0.0, 0.0), 1, X)]
        K = len(T)
        F, tails = mr.poisson_cdf(lam, K)
        with mp.workdps(50):
            assert all(a <= b for a, b in zip(T, T[1:])) and all(0 <= t < (1 << W) for t in T)                # monotone, in range
            err = max(abs(mp.mpf(t) / mp.mpf(2) ** W - f) for t, f in zip(T, F))
            assert err <= mp.mpf(2) ** -W + 4 * mp.mpf(2) ** -53, (p, float(err))
            assert tails[K] < mp.mpf(2) ** -W                                                                  # what the cut-off folds into N = K
            assert tails[K] < mp.mpf(2) ** -(W + 1) and (K == 0 or tails[K - 1] >= mp.mpf(2) ** -(W + 1))     # the header's rule for K
            print(f"{X} lambda dt = {p:g}: K = {K}, worst |T_k / 2^W - F_k| = {float(err * mp.mpf(2) ** W):.3f} 2^-{W}, tail {float(tails[K]):.3g}")
        assert K <= mc._lib.MAX_MERTON_JUMPS
    assert len(mc.merton_thresholds(o, J(0.0, 0.0, 0.0), 1, X)) == 0   # no jumps, no thresholds: N = 0 whatever the word
    # the same lambda dt over several dates
    assert list(mc.merton_thresholds(dict(o, t=2.0), J(2.0, 0.0, 0.0), 4, X)) == list(mc.merton_thresholds(o, J(1.0, 0.0, 0.0), 1, X))


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_the_cap_refuses_just_above_its_limit(mc, X):
    o = dict(br.ATM, t=1.0)

    def count(p):
        try:
            return len(mc.merton_thresholds(o, J(p, 0.0, 0.0), 1, X))
        except mc.McError as e:
            assert INVALID in str(e)
            return None

    assert count(5.0) is not None and count(41.0) is None
    lo, hi = 5.0, 41.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if count(mid) is not None else (lo, mid)
    print(f"{X}: the cap of {mc._lib.MAX_MERTON_JUMPS} thresholds is reached at lambda dt = {lo:.6f}")
    assert count(lo) == mc._lib.MAX_MERTON_JUMPS and count(hi) is None and hi - lo < 1e-6
    with pytest.raises(mc.McError, match="Poisson thresholds"):
        mc.merton_thresholds(o, J(hi, 0.0, 0.0), 1, X)


def test_counts_are_integer_compares():
    T = np.array([10, 10, 20, (1 << 64) - 1], dtype=np.uint64)
    w = np.array([0, 9, 10, 11, 19, 20, (1 << 64) - 2, (1 << 64) - 1], dtype=np.uint64)
    assert list(mr.merton_counts(w, T)) == [0, 0, 2, 2, 2, 3, 3, 4]
    assert list(mr.merton_counts(w, T, strict=True)) == [0, 0, 0, 2, 2, 2, 3, 3]
    assert list(mr.merton_counts(w, np.array([], dtype=np.uint64))) == [0] * 8
    # the stream rule: which words make which date's count
    words = np.arange(2 * 3 * 4, dtype=np.uint32).reshape(2, 3, 4)
    w32 = mr.jump_words(words, 9, "f32")
    assert w32.shape == (2, 9) and w32[1, 5] == words[1, 1, 1]
    w64 = mr.jump_words(words, 5, "f64")
    assert w64.shape == (2, 5) and int(w64[1, 3]) == (int(words[1, 1, 3]) << 32) | int(words[1, 1, 2]) and int(w64[0, 4]) == (int(words[0, 2, 1]) << 32) | int(words[0, 2, 0])
    assert [mr.jump_blocks(m, "f32") for m in (1, 4, 5)] == [1, 1, 2] and [mr.jump_blocks(m, "f64") for m in (1, 2, 3)] == [1, 1, 2]


# ---- the model on numpy draws -----------------------------------------------------------------------------------------------
def numpy_counts(rng, jp, t, m, shape):
    return rng.poisson(jp["lambda"] * t / m, size=shape)


@pytest.fixture(scope="module")
def shape_draws():
    """numpy normals (float32 values) for the shapes of the GPU test: N_PATHS paths of the largest date count, shared and left
    unchanged; the counts are drawn per shape from a generator seeded by the shape."""
    rng = np.random.default_rng(12)
    z = rng.standard_normal((mr.N_PATHS, max(mr.DATES))).astype(np.float32)
    z.setflags(write=False)
    return z


def counts_for(o, jp, m, n=mr.N_PATHS):
    return numpy_counts(np.random.default_rng(1000 + m), jp, o["t"], m, (n, m))


@pytest.mark.parametrize("m", [1, 2, 7, 64, 257])
def test_identities_per_path(shape_draws, m):
    z = shape_draws
    for o, B, jp in mr.CASES:
        N = counts_for(o, jp, m)
        up = B > o["s"]
        for anti in (False, True):
            # without jumps, or with jumps of size exactly 1, the walk is the constant-volatility walk
            for jq, Nq in ((dict(jp, **{"lambda": 0.0}), np.zeros_like(N)), (J(jp["lambda"], 0.0, 0.0), N)):
                a = ar.asian(o, m, z, False, anti)
                assert np.allclose(mr.merton(o, jq, m, z, Nq, "asian", anti=anti).value[0], a.value[0], rtol=1e-12, atol=1e-12 * o["s"])
                for kind in mr.kinds_of(o, B):
                    b = br.barrier(o, B, m, z, kind, "discrete", anti)
                    assert np.allclose(mr.merton(o, jq, m, z, Nq, "barrier", B, kind, anti).value[0], b.value[0], rtol=1e-12, atol=1e-12 * o["s"])
            c, sides = mr.walk(o, jp, m, z, N, B, up, anti)
            eu = mr.value(c, sides, "european").value[0]
            k_out, k_in = mr.kinds_of(o, B)
            assert np.allclose(mr.value(c, sides, "barrier", False).value[0] + mr.value(c, sides, "barrier", True).value[0], eu, rtol=1e-15, atol=0)
            if m == 1:
                assert np.array_equal(mr.value(c, sides, "asian").value[0], eu)   # one date: the average is the terminal spot
            one, other = (mr.merton(o, jp, m, zz, N, "asian").value[0] for zz in (z, -z.astype(np.float64)))
            if anti:
                assert np.allclose(mr.value(c, sides, "asian").value[0], 0.5 * (one + other), rtol=1e-15, atol=0)


@pytest.mark.parametrize("m", [1, 16])
def test_reference_model_prices_the_closed_form_at_any_date_count(mc, m):
    """2^20 numpy paths with numpy's Poisson counts, one seed: within 3 half-widths of the series.  The walk is exact in law."""
    for i, (o, jp) in enumerate(MARKETS[:3]):
        rng = np.random.default_rng(20261019 + 100 * i + m)
        acc = [0.0, 0.0]
        for _ in range(MC_PATHS // MC_CHUNK):
            z, N = rng.standard_normal((MC_CHUNK, m)), numpy_counts(rng, jp, o["t"], m, (MC_CHUNK, m))
            v = mr.merton(o, jp, m, z, N, "european").value[0]
            acc[0] += v.sum()
            acc[1] += (v * v).sum()
        disc, n = math.exp(-o["r"] * o["t"]), MC_PATHS
        mean = acc[0] / n
        price, half = disc * mean, 1.96 * disc * math.sqrt(max(acc[1] / n - mean * mean, 0.0) / (n - 1))
        exact = mc.merton_closed_form(o, jp)
        print(f"m={m} {o} {jp}: model {price:.5f} +- {half:.2g}, series {exact:.5f} ({abs(price - exact) / half:.2f} half-widths)")
        assert abs(price - exact) <= 3 * half, (o, jp, price, exact, half)


# ---- the scale: sound and sharp ---------------------------------------------------------------------------------------------
def shapes(m):
    """(market, barrier, jumps) of the GPU test at m dates."""
    return ([*mr.CASES] if m in mr.DATES else []) + ([mr.HEAVY] if m in mr.HEAVY_DATES else [])


@pytest.mark.parametrize("m", mr.DATES)
def test_a_float32_evaluation_stays_inside_the_bound(shape_draws, m):
    z = shape_draws
    tol = TOL["f32"]["pay"]
    worst, near_total = 0.0, 0
    for o, B, jp in shapes(m):
        q, jq = rounded(o, "f32"), rounded(jp, "f32")
        N = counts_for(o, jp, m)
        for anti in (False, True):
            c, sides = mr.walk(q, jq, m, z, N, B, B > o["s"], anti)
            for payoff, kind in [("european", None), ("asian", None)] + [("barrier", kind) for kind in mr.kinds_of(o, B)]:
                got = mr.merton_f32(q, jq, m, z, N, payoff, B, kind or "up-and-out", anti)
                w, near = mr.check_paths(got, c, sides, payoff, bool(kind) and kind.endswith("in"), tol)
                worst, near_total = max(worst, w), near_total + near
    print(f"m={m}: worst float32 error / bound {worst:.3g}, {near_total} near paths")


@pytest.mark.parametrize("m", [2, 16, 257])
def test_the_bound_rejects_the_mutations_of_the_walk(shape_draws, m):
    """At the weaker (fp32) tolerance, on more than 0.40 of the paths a mutation can touch, on the lambda = 3 case where 95 % of the
    paths jump.  A mutation of the jumps touches the paths that jump; the dropped compensator touches every path.  Measured on the
    Asian payoff, which is positive on most paths (a path out of the money under both walks shows nothing)."""
    z = shape_draws
    tol = TOL["f32"]["pay"]
    o, B, jp = mr.CASES[1]
    assert jp["lambda"] == 3.0
    N = counts_for(o, jp, m)
    jumped = N.sum(axis=1) > 0
    if m >= 16:
        assert 0.90 < jumped.mean() < 0.99
    q = o
    p = mr.merton(q, jp, m, z, N, "asian")
    b = tol * p.scale[0]
    for mutation, touched in (("delta_plain", jumped), ("no_compensator", np.ones_like(jumped)), ("late", jumped)):
        mutant = mr.merton(q, jp, m, z, N, "asian", mutation=mutation).value[0]
        share = float((np.abs(mutant - p.value[0]) > b)[touched].mean())
        print(f"m={m} {mutation}: outside the bound on {share:.3f} of the {int(touched.sum())} paths it can touch")
        assert share > 0.40, (m, mutation, share)


@pytest.mark.parametrize("X,W", [("f32", 32), ("f64", 64)])
@pytest.mark.parametrize("m", [2, 16, 257])
def test_the_bound_rejects_a_strict_compare(mc, shape_draws, X, W, m):
    """w > T_k for w >= T_k changes a count only where a word EQUALS a threshold, which no random word does: the paths it can touch
    are made here, every path with one date whose word is exactly a threshold (T_0 on even paths, the last one on odd paths)."""
    z = shape_draws
    tol = TOL["f32"]["pay"]
    o, B, jp = mr.CASES[1]
    T = mc.merton_thresholds(rounded(o, X), rounded(jp, X), m, X)
    rng = np.random.default_rng(77 + m)
    n = mr.N_PATHS
    w = rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64) << np.uint64(W - 32) | rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64) >> np.uint64(64 - W)
    at = rng.integers(0, m, size=n)
    w[np.arange(n), at] = np.where(np.arange(n) % 2 == 0, T[0], T[-1])
    N, Ns = mr.merton_counts(w, T), mr.merton_counts(w, T, strict=True)
    assert np.all((N - Ns).sum(axis=1) >= 1) and np.all(N >= Ns)
    q = o
    p = mr.merton(q, jp, m, z, N, "asian")
    mutant = mr.merton(q, jp, m, z, Ns, "asian").value[0]
    share = float((np.abs(mutant - p.value[0]) > tol * p.scale[0]).mean())
    print(f"{X} m={m} strict compare: outside the bound on {share:.3f} of the paths it can touch")
    assert share > 0.40, (X, m, share)


# ---- the barrier's step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", mr.DATES)
def test_few_paths_are_near_the_barrier(shape_draws, m):
    """Per path direction, the share of paths within the fp32 tolerance of the step (in units of the error of their distance): at
    most 0.05 up to 257 dates and 0.5 at 1000 and 4096; none at the fp64 tolerance."""
    cap = 0.05 if m <= 257 else 0.5
    cases = [(case, shape_draws) for case in shapes(m)]
    # the shapes of tests/test_gpu_walk_trips.py: the path counts of its ranges, each on the market it rotates to, and HEAVY
    for name in ("A", "C"):
        n = gr.TRIP_RANGES[name].n
        trip = ([gr.trip_pick(mr.CASES, mr.TRIP_DATES.index(m), name)] if m in mr.TRIP_DATES else []) + ([mr.HEAVY] if m == mr.TRIP_HEAVY_DATES else [])
        cases += [(case, np.random.default_rng(60 + m).standard_normal((n, m))) for case in trip]
    for (o, B, jp), z in cases:
        N = counts_for(o, jp, m, len(z))
        _, sides = mr.walk(o, jp, m, z, N, B, B > o["s"], True)
        for s in sides:
            share = float((s["edge"] <= TOL["f32"]["pay"]).mean())
            print(f"m={m} {jp}: {share:.4f} of the paths within the fp32 tolerance of the barrier")
            assert share <= cap, (m, jp, share)
            assert not np.any(s["edge"] <= TOL["f64"]["pay"])


# ---- the header -------------------------------------------------------------------------------------------------------------
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
#define ROW(T) sizeof(T), offsetof(T, lambda), offsetof(T, mu_j), offsetof(T, delta), offsetof(T, n_dates), offsetof(T, payoff), offsetof(T, barrier_type), offsetof(T, barrier)
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %u %u %d %d %d %d\n", ROW(mc_merton_f32), ROW(mc_merton_f64),
         MC_MAX_MERTON_DATES, MC_MAX_MERTON_JUMPS, MC_DOMAIN_MERTON, MC_DOMAIN_MERTON_JUMPS, MC_MERTON_EUROPEAN, MC_MERTON_ASIAN,
         MC_MERTON_BARRIER, MC_STREAM_VERSION);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    row = lambda T: [C.sizeof(T), T.lambda_.offset, T.mu_j.offset, T.delta.offset, T.n_dates.offset, T.payoff.offset, T.barrier_type.offset, T.barrier.offset]
    assert got == row(L.MertonF32) + row(L.MertonF64) + [L.MAX_MERTON_DATES, L.MAX_MERTON_JUMPS, L.DOMAIN_MERTON, L.DOMAIN_MERTON_JUMPS] + \
        [L.MERTON_PAYOFFS[k] for k in mr.PAYOFFS] + [2]
    assert L.MAX_MERTON_DATES == max(mr.DATES) and (L.DOMAIN_MERTON, L.DOMAIN_MERTON_JUMPS) == (mr.DOMAIN_MERTON, mr.DOMAIN_MERTON_JUMPS)
    assert "merton_closed_form" in mc.__all__ and "merton_thresholds" in mc.__all__
