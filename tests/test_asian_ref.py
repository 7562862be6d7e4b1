"""The Asian call without a GPU: the closed-form mean of its geometric control (mc_asian_control_mean_*, plain C in
mc_hostmath_impl.h) against an independent derivation, the one-date case against Black-Scholes, the float64 reference model
asian_ref.py on numpy's own normals (the variance reduction the control is there for), the refusals that need no device,
and the structs' layout against the header."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import asian_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

MARKETS = [dict(s=100.0, k=110.0, r=0.03, v=0.4, t=2.0), dict(s=50.0, k=40.0, r=0.01, v=0.6, t=0.5),
           dict(s=237.5, k=213.75, r=-0.015, v=0.07, t=1.3)]
DATES = [1, 2, 3, 12, 64, 255, 4096]


@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


def rounded(o, X):
    """The market as the precision's struct holds it."""
    return {c: float(np.float32(x)) if X == "f32" else float(x) for c, x in o.items()}


@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("m", DATES)
def test_control_mean_matches_an_independent_derivation(mc, X, m):
    for o in MARKETS:
        q = rounded(o, X)
        got, want = mc.asian_control_mean(q, m, X), ar.geometric_mean_closed_form(q, m)
        assert abs(got - want) <= 1e-12 * abs(want), (o, m, got, want)


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_one_date_is_black_scholes(mc, X):
    for o in MARKETS + [dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)]:
        q = rounded(o, X)
        got = math.exp(-q["r"] * q["t"]) * mc.asian_control_mean(q, 1, X)
        want = ar.black_scholes_call(q)
        assert abs(got - want) <= 1e-12 * abs(want), (o, got, want)
    o = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
    assert abs(mc.asian_control_mean(o, 1, "f64") - 10.98639645) < 5e-9   # undiscounted Black-Scholes call


def test_reference_model_control_variate():
    """Only claimed for the model here: the controlled estimator agrees with the plain one, has more than 100 times less
    variance (538 measured), and is non-negative path by path (arithmetic mean >= geometric mean)."""
    o, m, n = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0), 64, 200_000
    rng = np.random.default_rng(20240607)
    plain, ctrl = [], []
    for _ in range(n // 20_000):
        z = rng.standard_normal((20_000, m))
        plain.append(ar.asian(o, m, z).value[0])
        ctrl.append(ar.asian(o, m, z, control=True).value[0])
    plain, ctrl = np.concatenate(plain), np.concatenate(ctrl)
    disc = math.exp(-o["r"] * o["t"])
    mean = ar.geometric_mean_closed_form(o, m)
    e_p, e_c = disc * plain.mean(), disc * (ctrl.mean() + mean)
    h_p, h_c = (1.96 * disc * x.std(ddof=1) / math.sqrt(n) for x in (plain, ctrl))
    assert abs(e_p - e_c) <= h_p + h_c, (e_p, e_c, h_p, h_c)
    ratio = plain.var(ddof=1) / ctrl.var(ddof=1)
    assert ratio > 100, ratio
    assert ctrl.min() >= 0.0
    # the antithetic forms are means of two such values
    z = rng.standard_normal((1000, m))
    both = ar.asian(o, m, z, control=True, anti=True).value[0]
    assert np.array_equal(both, 0.5 * (ar.asian(o, m, z, control=True).value[0] + ar.asian(o, m, -z, control=True).value[0]))


@pytest.mark.parametrize("X", ["f32", "f64"])
def test_control_mean_refusals(mc, X):
    ok = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
    assert mc.asian_control_mean(ok, 12, X) > 0
    for bad, m in ((ok, 0), (ok, -3), (ok, mc._lib.MAX_ASIAN_DATES + 1), (dict(ok, k=0.0), 12), (dict(ok, k=-1.0), 12), (dict(ok, v=0.0), 12),
                   (dict(ok, s=0.0), 12), (dict(ok, t=0.0), 12), (dict(ok, r=float("nan")), 12)):
        with pytest.raises(mc.McError):
            mc.asian_control_mean(bad, m, X)
    with pytest.raises(mc.McError, match="k > 0"):
        mc.asian_control_mean(dict(ok, k=0.0), 12, X)
    with pytest.raises(mc.McError, match="v != 0"):
        mc.asian_control_mean(dict(ok, v=0.0), 12, X)
    assert mc.asian_control_mean(ok, 12, X) > 0   # and the next call is served


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "mc_mi355x.h"
int main(void)
{
  printf("%zu %zu %zu %zu %d %u\n", sizeof(mc_asian_f32), offsetof(mc_asian_f32, n_dates), sizeof(mc_asian_f64),
         offsetof(mc_asian_f64, n_dates), MC_MAX_ASIAN_DATES, MC_DOMAIN_ASIAN);
  return 0;
}
"""


def test_struct_layout_matches_the_header(mc, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c11", f"-I{INC}", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    L = mc._lib
    assert got == [C.sizeof(L.AsianF32), L.AsianF32.n_dates.offset, C.sizeof(L.AsianF64), L.AsianF64.n_dates.offset,
                   L.MAX_ASIAN_DATES, L.DOMAIN_ASIAN]
    assert L.MAX_ASIAN_DATES >= 4096
