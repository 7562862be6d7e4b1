"""The basket PRICING kernels -- every size 1..64, the four estimators, every kernel family, the fp32-normals mode and the
launch-geometry mode -- per path against the float64 model basket_ref.py, on random ASYMMETRIC markets and on the device's own
normals (Engine.normals).

Why: on the market of test_gpu_parity.basket_inputs (equal spots and weights, two vols, one correlation) the folded matrix has a
handful of distinct values, so an index error in packed rows, the LDS copy, the 4 x 4 tiles, the half-tile prefetch, the zero
padding or the second path of a lane leaves every path bit-identical (test_basket_ref.py shows it, and shows that on these markets
the same errors move almost every path beyond the bound used here).  Every market is priced at its drawn strike (deep in to deep
out of the money) and once more struck deep in the money (basket_ref.in_the_money), where every path shows every constant.

Tolerances: the per-path bound greeks_ref.bound(p, TOL[X]["pay"]) with the project's TOL of test_gpu_parity.py (per unit of the
model's forward-error scale); the bound on a sum is the sum of the per-path bounds.  The model is evaluated on the inputs as the
entry point of that precision reads them (basket_ref.as_seen).  Every case prints its worst err/bound.
"""
import contextlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import basket_ref as br
import greeks_ref as gr
from test_gpu_parity import SEED, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 1 << 32
PLAIN, ANTI, CONTROL, BOTH = br.ESTIMATORS

# ---- the cases (test_basket_ref.py shows the power of the bound on exactly these markets) ---------------------------
N_PATHS = 2121                 # eight workgroups and a partial wave; odd: a pair kernel's last trip has no second path
SEAM_FIRST = U32 - 1000        # crosses the 2^32-unit seam: two segments
SIZES_ALL = list(range(1, 65))
SIZES_TRIPS = [4, 12, 13, 16, 20, 28, 32, 33, 64]     # one per kernel, and the two tiled sizes nothing else launches
N_TRIPS = 6007
SIZES_GENERIC = [1, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 28, 29, 32, 33, 47, 64]
FAMILIES = {   # name -> (X, environment, (static_max f32, f64, tiled_min) that describe() must name, sizes)
    "f64-arguments": ("f64", dict(MC_BASKET_STATIC_MAX_F64="16"), (12, 16, 9), list(range(1, 17))),
    "f64-tiled": ("f64", dict(), (12, 8, 9), list(range(9, 33))),
    "f64-generic": ("f64", dict(MC_BASKET_STATIC_MAX_F64="0", MC_BASKET_TILED_MIN="1000"), (12, 0, 1000), SIZES_GENERIC),
    "f32-arguments": ("f32", dict(MC_BASKET_STATIC_MAX_F32="16"), (16, 8, 9), list(range(1, 17))),
    "f32-generic": ("f32", dict(MC_BASKET_STATIC_MAX_F32="0", MC_BASKET_TILED_MIN="1000"), (0, 8, 1000), SIZES_GENERIC),
}
SIZES_F32N = [1, 3, 4, 8, 9, 12, 16, 17, 20, 28, 32, 33, 64]
SIZES_GRID = [1, 3, 4, 5, 7, 8, 9, 13, 16]            # sizes below a compiled size (4, 8, 16) run it zero-padded
GEOMS_GRID = [(3, 64, 200), (2, 64, 4100)]
# fp32 normals in the fp64 kernels: the combinations mc_api.hip refuses (MC_ERR_UNSUPPORTED, "mc error 4"), by its three
# mechanisms.  Under the default limits there are none among SIZES_F32N x the four estimators: (1) with_anti_gen only takes the
# external-normals policy away under antithetic variates; (2) static_max capped at 8 sends 9..16 assets to the tiled kernels,
# which are compiled for the mode; (3) where tiled_ok fails (beyond 32 assets) the generic kernel is, for both estimators.
REFUSED_F32N = {}   # (n_assets, antithetic, control) -> why


# markets whose first seed drew two nearly equal matrix entries where the one-entry exchange of basket_ref.MUTATIONS acts, so
# that it moved fewer than 90 % of the paths (test_basket_ref.py): the seed moves on by 100 000 per step, the condition stays
RESEEDED = {("a", 38): 2, ("a", 47): 1, ("a", 61): 1, ("a0", 39): 1, ("a0", 52): 1, ("a0", 63): 1, ("c", 32): 1}


def seed_of(test, n_assets):
    return {"a": 2000, "a0": 3000, "b": 4000, "c": 5000, "d": 6000, "e": 7000}[test] + n_assets + 100_000 * RESEEDED.get((test, n_assets), 0)


def market(mc, test, n_assets):
    """(market, a first path drawn below 2^34) of a test's size.  "a0" is (a)'s second market, with one zero weight.  The
    correlation is factored in fp64 for both precisions: one market per size, which the fp32 entry points round on entry."""
    rng = np.random.default_rng(seed_of(test, n_assets))
    b = br.random_market(rng, n_assets, lambda c: mc.chol(c, "f64"), positive_weights=test != "a0")
    return b, int(rng.integers(0, 1 << 34))


def power_cases():
    """Every (test, size) market above at which an index error of basket_ref.MUTATIONS applies."""
    sizes = {"a": SIZES_ALL, "a0": SIZES_ALL, "b": SIZES_TRIPS, "c": sorted({n for f in FAMILIES.values() for n in f[3]}),
             "d": SIZES_F32N, "e": SIZES_GRID}
    return [(t, n) for t, ns in sizes.items() for n in ns if br.mutations(n)]


# ---- plumbing -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc():
    import montecarlocuda_amd as mc
    return mc


@pytest.fixture(scope="module")
def eng(mc):
    e = mc.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def estimator(e, anti, cv):
    e.set_antithetic(anti), e.set_control_variate(cv)
    try:
        yield
    finally:
        e.set_antithetic(False), e.set_control_variate(False)


def device_normals(e, X, first, n, n_assets):
    """The device's own basket normals of paths first .. first + n - 1, (n, n_assets) in fp64.  Blocks of 4 in fp32 and under
    set_normals("f32"), of 8 in native fp64."""
    npb = 4 if (X == "f32" or e._normals_f32) else 8
    return gr.basket_normals(lambda domain, u0, c, block: e.normals(SEED, domain, u0, c, block, X), first, n, n_assets, npb)


def check_paths(got, p, X, what):
    """Per path within the bound; returns the worst err/bound."""
    bnd, v = gr.bound(p, TOL[X]["pay"])[0], p.value[0]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == v.shape
    err = np.abs(got - v)
    i = int(np.argmax(err / bnd))
    assert np.all(err <= bnd), (what, i, got[i], v[i], err[i], bnd[i], int((err > bnd).sum()))
    return float(err[i] / bnd[i])


def check_call(e, b, g, n, first, X, anti, cv, what):
    """basket_paths per path, basket's (sum, sum2) within the summed bounds, expected closed from the call's own sum."""
    seen = br.as_seen(b, X)
    p = br.value(seen, g, anti, cv)
    with estimator(e, anti, cv):
        got = e.basket_paths(b, n, SEED, first, X)
        est = e.basket(b, n, SEED, first, X)
    ratio = check_paths(got, p, X, what)
    bnd, v = gr.bound(p, TOL[X]["pay"])[0], p.value[0]
    assert est.n == n
    assert abs(est.sum - v.sum()) <= bnd.sum(), (what, est.sum, v.sum(), bnd.sum())
    assert abs(est.sum2 - (v * v).sum()) <= (2 * np.abs(v) * bnd + bnd * bnd).sum(), (what, est.sum2, (v * v).sum())
    mean = br.control_mean(seen) if cv else 0.0      # plain and antithetic: nothing is added back
    assert est.expected == pytest.approx(math.exp(-seen["r"] * seen["t"]) * (est.sum / n + mean), rel=1e-12), what
    return ratio


def report(test, X, n_assets, worst):
    print(f"basket_ref {test} {X} n_assets={n_assets}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- a. every size, every estimator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", SIZES_ALL)
def test_every_size_every_estimator(mc, eng, X, n_assets):
    b, drawn = market(mc, "a", n_assets)
    b0, _ = market(mc, "a0", n_assets)       # one weight zero: no control variate
    worst = {}
    for first in (SEAM_FIRST, drawn):
        g = device_normals(eng, X, first, N_PATHS, n_assets)
        cases = [(b, est, "") for est in br.ESTIMATORS] + [(br.in_the_money(b), PLAIN, " itm"), (br.in_the_money(b), BOTH, " itm")]
        cases += [(b0, PLAIN, " w0"), (b0, ANTI, " w0"), (br.in_the_money(b0), PLAIN, " w0 itm")]
        for m, (anti, cv), tag in cases:
            key = f"{'anti' if anti else 'plain'}{'+cv' if cv else ''}{tag}"
            r = check_call(eng, m, g, N_PATHS, first, X, anti, cv, (n_assets, X, first, key))
            worst[key] = max(worst.get(key, 0.0), r)
    report("a", X, n_assets, worst)


# ---- b. many trips ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", SIZES_TRIPS)
def test_many_trips(mc, X, n_assets):
    """Two workgroups: every lane runs several grid-stride trips, the fp32 kernels reach their flush to fp64."""
    b, first = market(mc, "b", n_assets)
    worst = {}
    with mc.Engine(0, blocks=2) as e:
        g = device_normals(e, X, first, N_TRIPS, n_assets)
        for m, (anti, cv), key in ((b, PLAIN, "plain"), (b, BOTH, "anti+cv"), (br.in_the_money(b), PLAIN, "plain itm")):
            worst[key] = check_call(e, m, g, N_TRIPS, first, X, anti, cv, (n_assets, X, first, key))
    report("b", X, n_assets, worst)


# ---- c. families, in child processes ------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import montecarlocuda_amd as mc
job = json.load(open(sys.argv[2]))
out = {}
with mc.Engine(0) as e:
    text = e.describe()
    assert job["describe"] in text, (job["describe"], text)
    for n_assets, variants in job["markets"].items():
        for tag, b in variants.items():
            for anti, cv in ((0, 0), (1, 1)):
                e.set_antithetic(bool(anti)), e.set_control_variate(bool(cv))
                out[f"{n_assets}|{tag}|{anti}{cv}"] = e.basket_paths(b, job["n"], job["seed"], job["first"], job["X"])
np.savez(sys.argv[3], **out)
"""
_family_cache = {}


def family_paths(mc, name, tmp):
    """The per-path values of one family: one child process (the limits are read once per process) runs all of the family's
    sizes, both strikes, plain and antithetic+control, and saves one .npz.  Run once per session, one child after the other."""
    if name not in _family_cache:
        import json
        X, env, (s32, s64, tmin), sizes = FAMILIES[name]
        job = dict(X=X, n=N_PATHS, seed=SEED, first=SEAM_FIRST, describe=f"basket_static_max=f32:{s32},f64:{s64} basket_tiled_min={tmin} ",
                   markets={str(n): {"drawn": market(mc, "c", n)[0], "itm": br.in_the_money(market(mc, "c", n)[0])} for n in sizes})
        jpath, opath = os.path.join(tmp, name + ".json"), os.path.join(tmp, name + ".npz")
        with open(jpath, "w") as f:
            json.dump(job, f)
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MC_BASKET_")}
        run = subprocess.run([sys.executable, "-c", CHILD, ROOT, jpath, opath], env=dict(clean, **env), timeout=300, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        with np.load(opath) as z:
            _family_cache[name] = {k: z[k] for k in z.files}
    return _family_cache[name]


@pytest.fixture(scope="module")
def family_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("basket_families"))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_meets_the_model(mc, eng, family_dir, name):
    X, _, _, sizes = FAMILIES[name]
    got = family_paths(mc, name, family_dir)
    assert len(got) == 4 * len(sizes)
    worst = {}
    for n_assets in sizes:
        b, _ = market(mc, "c", n_assets)
        g = device_normals(eng, X, SEAM_FIRST, N_PATHS, n_assets)
        for tag, m in (("drawn", b), ("itm", br.in_the_money(b))):
            for anti, cv in (PLAIN, BOTH):
                vals = got[f"{n_assets}|{tag}|{int(anti)}{int(cv)}"]
                assert vals.dtype == (np.float32 if X == "f32" else np.float64)
                r = check_paths(vals, br.value(br.as_seen(m, X), g, anti, cv), X, (name, n_assets, tag, anti, cv))
                worst[n_assets] = max(worst.get(n_assets, 0.0), r)
    print(f"basket_ref c {name}: worst err/bound by size " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))
    print(f"basket_ref c {name}: worst err/bound {max(worst.values()):.3f}")


def test_f64_families_agree_bitwise(mc, family_dir):
    """The three fp64 families run the same fma chains in the same order (padding adds exact zeros): identical bits, now on markets
    where a misplaced constant changes them."""
    fam = {name: family_paths(mc, name, family_dir) for name in ("f64-arguments", "f64-tiled", "f64-generic")}
    compared = 0
    for a, c in (("f64-arguments", "f64-tiled"), ("f64-arguments", "f64-generic"), ("f64-tiled", "f64-generic")):
        common = sorted(set(fam[a]) & set(fam[c]))
        assert common
        for key in common:
            assert np.array_equal(fam[a][key].view(np.uint64), fam[c][key].view(np.uint64)), (a, c, key)
            compared += 1
    assert compared == 4 * (8 + 9 + 10)      # sizes 9..16; 1, 3, 4, 5, 8, 9, 12, 13, 16; the generic list's ten sizes from 9 to 32


# ---- d. fp32 normals in the fp64 kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_assets", SIZES_F32N)
def test_fp32_normals_mode_is_fp64_downstream(mc, n_assets):
    """set_normals("f32"): the normal is a widened float, everything downstream of it fp64 -- antithetic and the control
    included -- so on the mode's own normals the fp64 bound holds per path."""
    b, first = market(mc, "d", n_assets)
    worst = {}
    with mc.Engine(0) as e:
        e.set_normals("f32")
        g = device_normals(e, "f64", first, N_PATHS, n_assets)
        assert np.array_equal(g, g.astype(np.float32).astype(np.float64)) and np.abs(g).max() < 6.77
        for m, tag in ((b, ""), (br.in_the_money(b), " itm")):
            for anti, cv in br.ESTIMATORS:
                key = f"{'anti' if anti else 'plain'}{'+cv' if cv else ''}{tag}"
                try:
                    worst[key] = check_call(e, m, g, N_PATHS, first, "f64", anti, cv, (n_assets, first, key))
                except mc.McError as ex:
                    assert (n_assets, anti, cv) in REFUSED_F32N and str(ex).startswith("mc error 4"), (n_assets, key, str(ex))
                else:
                    assert (n_assets, anti, cv) not in REFUSED_F32N, (n_assets, key)
    report("d", "f64 on fp32 normals", n_assets, worst)


# ---- e. launch-geometry mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", ["f32", "f64"])
@pytest.mark.parametrize("n_assets", SIZES_GRID)
def test_launch_geometry_forms(mc, eng, po, X, n_assets):
    """The fused kernels (4, 8 and 16 assets compiled, smaller sizes zero-padded) give the staged form's bits, and the staged form's
    per-path values meet the model on the normals rebuilt from the threads' streams."""
    from test_gpu_grid import both_forms
    b, _ = market(mc, "e", n_assets)
    worst = {}
    for G, T, per_block in GEOMS_GRID:
        streams = eng.grid_normals(G, T, po.grid_draws_per_thread(T, per_block, n_assets))
        g = po.grid_path_normals(streams, per_block, n_assets).astype(np.float64)
        for m, tag in ((b, "drawn"), (br.in_the_money(b), "itm")):
            both_forms(eng, "basket", m, G, T, per_block, X)
            try:
                eng.set_grid_form("staged")
                vals = eng.paths_grid("basket", m, G, T, per_block, X)
            finally:
                eng.set_grid_form("auto")
            r = check_paths(vals.reshape(-1), br.value(br.as_seen(m, X), g, False, False), X, (n_assets, X, G, T, per_block, tag))
            worst[tag] = max(worst.get(tag, 0.0), r)
    report("e", X, n_assets, worst)
