"""Multilevel Monte Carlo on the Heston walk: what one level costs, and what the multilevel run buys, in one process.

(a) Kernel time of ONE level launch (mc_heston_level_run_*, a fine walk on m steps and a coarse walk on m / 2 on the same normals) beside
    the two launches it replaces, mc_heston_path_run_* (one date) at m and at m / 2 steps on the same path count; m in {16, 256, 4096},
    fp32 and fp64, plain and antithetic.  kernel_ms (HIP events, timing on) as the median of REPS calls after WARM warm-ups, the three
    forms called in alternation, with the spread (max - min) / median of each form's calls, and level / (fine + coarse).
(b) Time to a given root-mean-square error eps in {0.05, 0.01, 0.002} on the VIOLATED model out of the money: mc_heston_mlmc_run_*
    (level 0 at 4 steps) against ONE level, mc_heston_path_run_* at the smallest step count 4 * 2^l whose MEASURED bias is at most
    eps / sqrt 2 (the bias is measured first, on the walk itself: its price at every step count 4 ... 4096 on BIAS_PATHS antithetic pairs
    against the closed form; a bias inside two standard errors of that measurement counts as its two standard errors) with
    N = 2 Var / eps^2 paths.  Both sides report the sum of their kernels' time and the wall time of the call(s), the median of REPS_B
    runs after one warm-up, alternated, and the ratio single / mlmc.
No figure is fixed in advance: the tool prints what it measured.
    python tools/heston_mlmc_speed.py [--quick]      (--quick: a tenth of the paths of (a), the two larger eps of (b))
"""
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=110.0, r=0.05, v=0.0, t=1.0)
MODEL = dict(v0=0.02, kappa=1.5, theta=0.04, xi=0.6, rho=-0.7)
SEED = mc.MC_DEFAULT_SEED
WARM, REPS, REPS_B = 2, 7, 5
STEPS_PATHS = {16: 1 << 26, 256: 1 << 24, 4096: 1 << 21}
EPS = (0.05, 0.01, 0.002)
BIAS_PATHS = 1 << 28
N_PILOT = 10_000


def median_spread(x):
    m = statistics.median(x)
    return m, (max(x) - min(x)) / m


def part_a(eng, scale):
    print(f"(a) kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    for X in ("f32", "f64"):
        for anti in (False, True):
            eng.set_antithetic(anti)
            for m, paths in STEPS_PATHS.items():
                paths //= scale
                forms = [lambda: eng.heston_level(OPT, MODEL, 1, m, paths, SEED, 0, X).kernel_ms,
                         lambda: eng.heston_asian(OPT, MODEL, 1, m, paths, SEED, 0, X).kernel_ms,
                         lambda: eng.heston_asian(OPT, MODEL, 1, m // 2, paths, SEED, 0, X).kernel_ms]
                ms = [[] for _ in forms]
                for rep in range(WARM + REPS):
                    for k, f in enumerate(forms):
                        t = f()
                        if rep >= WARM:
                            ms[k].append(t)
                (lv, sl), (fi, sf), (co, sc) = (median_spread(x) for x in ms)
                print(f"{X} {'antithetic' if anti else 'plain':10s} m={m:5d} paths={paths:9d}: level {lv:9.3f} ms ({sl:6.2%})  fine {fi:9.3f} ms ({sf:6.2%})  "
                      f"coarse {co:9.3f} ms ({sc:6.2%})  level / (fine + coarse) = {lv / (fi + co):5.3f}", flush=True)
    eng.set_antithetic(False)


def measured_bias(eng, X, exact):
    """[(steps, bias, its standard error)] of the walk itself at 4 ... 4096 steps: antithetic pairs, discounted, against the closed form."""
    rows = []
    disc = math.exp(-OPT["r"] * OPT["t"])
    eng.set_antithetic(True)
    for l in range(11):
        g = eng.heston_asian(OPT, MODEL, 1, 4 << l, BIAS_PATHS, SEED, 1 << 44, X)
        rows.append((4 << l, g.expected - exact, disc * g.confidence / 1.96))
    eng.set_antithetic(False)
    return rows


def part_b(eng, eps_list):
    exact = mc.heston_closed_form(OPT, MODEL)
    disc = math.exp(-OPT["r"] * OPT["t"])
    print(f"(b) VIOLATED out of the money, closed form {exact:.6f}; times: median of {REPS_B} runs after 1 warm-up, the two sides alternated")
    for X in ("f32", "f64"):
        bias = measured_bias(eng, X, exact)
        print(f"{X} measured bias of the walk ({BIAS_PATHS} antithetic pairs): " + ", ".join(f"{m}: {b:+.5f} +- {s:.5f}" for m, b, s in bias), flush=True)
        for eps in eps_list:
            fit = [m for m, b, s in bias if max(abs(b), 2.0 * s) <= eps / math.sqrt(2.0)]
            if not fit:
                print(f"{X} eps={eps}: no step count up to 4096 has a measured bias of at most eps / sqrt 2: single level not run")
                continue
            steps = fit[0]
            pilot = eng.heston_asian(OPT, MODEL, 1, steps, 1 << 20, SEED, 1 << 45, X)
            n = float(pilot.n)
            var = disc * disc * (n * pilot.sum2 - pilot.sum ** 2) / (n * (n - 1.0))
            n_single = int(math.ceil(2.0 * var / (eps * eps)))
            ml_k, ml_w, sg_k, sg_w = [], [], [], []
            for rep in range(1 + REPS_B):
                t0 = time.perf_counter()
                r = eng.heston_mlmc(OPT, MODEL, 1, 4, eps, SEED, X, 2, 10, N_PILOT)
                t1 = time.perf_counter()
                g = eng.heston_asian(OPT, MODEL, 1, steps, n_single, SEED, 0, X)
                t2 = time.perf_counter()
                if rep:
                    ml_k.append(sum(v.estimate.kernel_ms for v in r.levels)), ml_w.append((t1 - t0) * 1e3)
                    sg_k.append(g.kernel_ms), sg_w.append((t2 - t1) * 1e3)
            (mk, smk), (mw, _), (sk, ssk), (sw, _) = (median_spread(x) for x in (ml_k, ml_w, sg_k, sg_w))
            se_single = disc * g.confidence / 1.96
            print(f"{X} eps={eps}: mlmc {len(r.levels)} levels, paths {[v.n_paths for v in r.levels]}, price {r.price:.5f} +- {r.stderr:.5f} "
                  f"(err {r.price - exact:+.5f}), converged {r.converged}, kernels {mk:.3f} ms ({smk:.2%}), call {mw:.3f} ms | single {steps} steps x {n_single} paths, "
                  f"price {g.expected:.5f} +- {se_single:.5f} (err {g.expected - exact:+.5f}), kernel {sk:.3f} ms ({ssk:.2%}), call {sw:.3f} ms | "
                  f"single / mlmc: kernels {sk / mk:.3f}, calls {sw / mw:.3f}", flush=True)


def main(quick):
    eng = mc.Engine(0)
    print(eng.describe())
    part_a(eng, 10 if quick else 1)
    part_b(eng, EPS[:2] if quick else EPS)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main("--quick" in sys.argv))
