"""Kernel time of the Heston call (mc_heston_run_*) against its yardstick, in one process.

For fp32 and fp64, at (128 steps x 1e7 paths) and (8 steps x 1e8 paths), kernel_ms (HIP events, timing on) of
    heston plain | heston antithetic | (a) mc_asian_run_* plain at TWICE the number of dates
as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread (max - min) / median of each
form's calls.  The Asian call at 2 m dates draws the same normals as the Heston call at m steps (two per step) and is the natural
yardstick: the step trades the two dates' exponentials for one square root and about six more fmas.  No ratio is fixed in
advance; the tool prints what it measured.
    python tools/heston_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
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
ROWS = [(128, 10 ** 7), (8, 10 ** 8)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    names = ["heston plain", "heston anti", "(a) asian 2m dates"]
    print(f"{'prec':4s} {'steps':>5s} {'paths':>10s} " + " ".join(f"{x:>20s}" for x in names) +
          f" {'plain/(a)':>9s} {'anti/plain':>10s} {'ns/step plain':>13s}")
    for X in ("f32", "f64"):
        for steps, paths in ROWS:
            paths //= scale

            def heston(anti):
                eng.set_antithetic(anti)
                r = eng.heston(OPT, MODEL, steps, paths, SEED, 0, X)
                eng.set_antithetic(False)
                return r.kernel_ms

            forms = [lambda: heston(False), lambda: heston(True), lambda: eng.asian(OPT, 2 * steps, paths, SEED, 0, X).kernel_ms]
            ms = [[] for _ in forms]
            for rep in range(WARM + REPS):
                for k, f in enumerate(forms):
                    t = f()
                    if rep >= WARM:
                        ms[k].append(t)
            med = [statistics.median(x) for x in ms]
            spread = [(max(x) - min(x)) / m for m, x in zip(med, ms)]
            cells = [f"{m:10.3f} ({s:6.2%})" for m, s in zip(med, spread)]
            print(f"{X:4s} {steps:5d} {paths:10d} " + " ".join(f"{c:>20s}" for c in cells) +
                  f" {med[0] / med[2]:9.3f} {med[1] / med[0]:10.3f} {med[0] * 1e6 / (steps * paths):13.5f}", flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
