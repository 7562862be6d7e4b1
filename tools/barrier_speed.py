"""Kernel time of the barrier call (mc_barrier_run_*) against two yardsticks, in one process.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), kernel_ms (HIP events, timing on) of
    barrier discrete | barrier continuous | the two with antithetic variates | (a) mc_asian_run_* plain | (b) mc_cva_run_*
at the same (dates, paths), as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread
(max - min) / median of each form's calls.  Two conditions follow from the instruction mix: the discrete form's date does
strictly less than the Asian call's (no exponential), the continuous form's strictly less than the CVA's -- neither may be
slower than its yardstick by more than the spread.  The continuous / Asian ratio and the antithetic cost are printed as findings.
    python tools/barrier_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
BARRIER = 120.0
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    names = ["discrete", "continuous", "discrete anti", "continuous anti", "(a) asian plain", "(b) cva"]
    print(f"{'prec':4s} {'dates':>5s} {'paths':>10s} " + " ".join(f"{x:>20s}" for x in names) +
          f" {'disc/(a)':>8s} {'cont/(b)':>8s} {'cont/(a)':>8s} {'anti/plain d':>12s} {'anti/plain c':>12s} {'ns/date disc':>12s}")
    slower = []
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            paths //= scale
            cva = dict(OPT, defint=0.03, lgd=0.4, n_grid=dates)

            def barrier(monitoring, anti):
                eng.set_antithetic(anti)
                r = eng.barrier(OPT, BARRIER, dates, paths, SEED, 0, X, "up-and-out", monitoring)
                eng.set_antithetic(False)
                return r.kernel_ms

            forms = [lambda: barrier("discrete", False), lambda: barrier("continuous", False), lambda: barrier("discrete", True),
                     lambda: barrier("continuous", True), lambda: eng.asian(OPT, dates, paths, SEED, 0, X).kernel_ms,
                     lambda: eng.cva(cva, paths, SEED, 0, X).kernel_ms]
            ms = [[] for _ in forms]
            for rep in range(WARM + REPS):
                for k, f in enumerate(forms):
                    t = f()
                    if rep >= WARM:
                        ms[k].append(t)
            med = [statistics.median(x) for x in ms]
            spread = [(max(x) - min(x)) / m for m, x in zip(med, ms)]
            cells = [f"{m:10.3f} ({s:6.2%})" for m, s in zip(med, spread)]
            print(f"{X:4s} {dates:5d} {paths:10d} " + " ".join(f"{c:>20s}" for c in cells) +
                  f" {med[0] / med[4]:8.3f} {med[1] / med[5]:8.3f} {med[1] / med[4]:8.3f} {med[2] / med[0]:12.3f} {med[3] / med[1]:12.3f}"
                  f" {med[0] * 1e6 / (dates * paths):12.5f}", flush=True)
            for name, k, ref in (("discrete", 0, 4), ("continuous", 1, 5)):
                if med[k] > med[ref] * (1.0 + max(spread[k], spread[ref])):
                    slower.append((X, dates, paths, name, med[k], med[ref]))
    eng.close()
    print("rows slower than their yardstick by more than the spread: " + (repr(slower) if slower else "none"))
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
