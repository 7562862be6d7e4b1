"""Kernel time of the worst-of / best-of options (mc_rainbow_run_*) against two yardsticks.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), for n = 1, 2, 4, 8 assets: kernel_ms (HIP events, timing
on) of the worst-of put
    without a barrier | with a down-and-in barrier | the two with antithetic variates
and, at the same (dates, paths), of (a) mc_barrier_run_* discrete (to compare with n = 1 + barrier) and (b) mc_asian_run_* plain, as
the median of REPS calls after WARM warm-ups, all forms of a row called in alternation in one process, with the spread
(max - min) / median of each form's calls.  Per size the table also gives the time per normal drawn (n * dates * paths) and the time
relative to n = 1: whether the times scale with the normals drawn per path.  Each (precision, dates, paths) row is measured in a
child process of its own under a time limit; the first child that fails ends the run.
    python tools/rainbow_speed.py [--quick] [--sizes 3,5,6,7]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]
SIZES = [1, 2, 4, 8]
ROW_TIMEOUT_S = 240


def market(n):
    """Performance levels, volatilities 0.15 ... 0.35, the one-factor correlation beta_i beta_j with beta from 0.6 to 0.8."""
    import numpy as np
    beta = np.linspace(0.6, 0.8, n) if n > 1 else np.array([0.7])
    corr = np.outer(beta, beta)
    np.fill_diagonal(corr, 1.0)
    s = 100.0 * (1.0 + 0.1 * np.arange(n))
    return dict(s=s, v=np.linspace(0.15, 0.35, n) if n > 1 else np.array([0.25]), p=np.linalg.cholesky(corr), d=np.zeros(n), w=1.0 / s, k=1.0, t=1.0, r=0.03)


def row(X, dates, paths):
    import montecarlocuda_amd as mc
    seed = mc.MC_DEFAULT_SEED
    opt = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
    eng = mc.Engine(0)

    def rainbow(b, barrier, anti):
        eng.set_antithetic(anti)
        r = eng.rainbow(b, dates, paths, "put-on-min", 0.7 if barrier else None, "down-and-in" if barrier else None, seed, 0, X)
        eng.set_antithetic(False)
        return r.kernel_ms

    names, forms = [], []
    for n in SIZES:
        b = market(n)
        for label, barrier, anti in (("free", False, False), ("barrier", True, False), ("free anti", False, True), ("barrier anti", True, True)):
            names.append(f"n={n} {label}")
            forms.append(lambda b=b, barrier=barrier, anti=anti: rainbow(b, barrier, anti))
    names += ["(a) barrier discrete", "(b) asian plain"]
    forms += [lambda: eng.barrier(opt, 120.0, dates, paths, seed, 0, X, "up-and-out", "discrete").kernel_ms,
              lambda: eng.asian(opt, dates, paths, seed, 0, X).kernel_ms]
    ms = [[] for _ in forms]
    for rep in range(WARM + REPS):
        for k, f in enumerate(forms):
            t = f()
            if rep >= WARM:
                ms[k].append(t)
    eng.close()
    med = [statistics.median(x) for x in ms]
    spread = [(max(x) - min(x)) / m for m, x in zip(med, ms)]
    ya, yb = med[-2], med[-1]
    print(f"{X} {dates} dates x {paths} paths: (a) mc_barrier_run discrete {ya:.3f} ms ({spread[-2]:.2%}), (b) mc_asian_run plain {yb:.3f} ms ({spread[-1]:.2%})")
    print(f"  {'form':>16s} {'kernel_ms':>10s} {'spread':>7s} {'/ n=1':>7s} {'/ n':>7s} {'ps/normal':>10s} {'/ (a)':>7s} {'/ (b)':>7s}")
    for k, name in enumerate(names[:-2]):
        n = SIZES[k // 4]
        base = med[k % 4] / SIZES[0]   # the same form at the first size (n = 1 by default), per asset
        print(f"  {name:>16s} {med[k]:10.3f} {spread[k]:7.2%} {med[k] / base:7.3f} {med[k] / base / n:7.3f} {med[k] * 1e9 / (n * dates * paths):10.3f} "
              f"{med[k] / ya:7.3f} {med[k] / yb:7.3f}", flush=True)
    print(f"  largest spread of a form in this row: {max(spread):.2%}", flush=True)


def main(scale):
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sizes", ",".join(map(str, SIZES)), "--row", X, str(dates), str(paths // scale)],
                               timeout=ROW_TIMEOUT_S)
            if r.returncode != 0:
                print(f"row {X} {dates} x {paths // scale} ended with status {r.returncode}: stopping")
                return 1
    return 0


if __name__ == "__main__":
    if "--sizes" in sys.argv:   # e.g. --sizes 3,5,6,7: the sizes between the default ones ("/ n=1" is then relative to the first)
        SIZES = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    if "--row" in sys.argv:
        i = sys.argv.index("--row")
        row(sys.argv[i + 1], int(sys.argv[i + 2]), int(sys.argv[i + 3]))
        sys.exit(0)
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, the forms of a row alternated in one process; spread = (max - min) / median", flush=True)
    sys.exit(main(10 if "--quick" in sys.argv else 1))
