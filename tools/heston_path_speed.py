"""Kernel time of the Asian and the barrier call on the Heston walk (mc_heston_path_run_*) beside the European call, in one process.

For fp32 and fp64, at 128 steps x 1e7 paths, kernel_ms (HIP events, timing on) of
    mc_heston_run_* at 128 steps | the Asian call at 1, 8 and 128 dates | the up-and-out call (B = 125) at 1, 8 and 128 dates
(n_dates x steps_per_date = 128 throughout, plain estimator) as the median of REPS calls after WARM warm-ups, the forms called in
alternation, with the spread (max - min) / median of each form's calls, and each form's ratio to mc_heston_run_*.  The one-date forms
walk the European call's steps and differ from it by the scalar countdown and one date; no ratio is fixed in advance, the tool prints
what it measured.
    python tools/heston_path_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
MODEL = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
STEPS, PATHS, DATES, BARRIER = 128, 10 ** 7, (1, 8, 128), 125.0


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    paths = PATHS // scale
    print(f"{STEPS} steps x {paths} paths, plain estimator; kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; "
          "(spread) = (max - min) / median; ratio = median / heston's median")
    names = ["heston"] + [f"asian {d} dates" for d in DATES] + [f"up-out {d} dates" for d in DATES]
    for X in ("f32", "f64"):
        forms = [lambda: eng.heston(OPT, MODEL, STEPS, paths, SEED, 0, X).kernel_ms]
        forms += [lambda d=d: eng.heston_asian(OPT, MODEL, d, STEPS // d, paths, SEED, 0, X).kernel_ms for d in DATES]
        forms += [lambda d=d: eng.heston_barrier(OPT, MODEL, BARRIER, d, STEPS // d, paths, SEED, 0, X).kernel_ms for d in DATES]
        ms = [[] for _ in forms]
        for rep in range(WARM + REPS):
            for k, f in enumerate(forms):
                t = f()
                if rep >= WARM:
                    ms[k].append(t)
        med = [statistics.median(x) for x in ms]
        for name, m, x in zip(names, med, ms):
            print(f"{X:4s} {name:18s} {m:10.3f} ms ({(max(x) - min(x)) / m:6.2%})  ratio {m / med[0]:6.3f}  ns/step {m * 1e6 / (STEPS * paths):8.5f}", flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
