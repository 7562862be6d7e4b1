"""Kernel time of the lookback options (mc_lookback_run_*) against two yardsticks, in one process.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), kernel_ms (HIP events, timing on) of
    lookback discrete | lookback continuous | the two with antithetic variates | (a) mc_asian_run_* plain | (b) mc_barrier_run_* continuous
at the same (dates, paths), as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread
(max - min) / median of each form's calls.  The lookback is the floating-strike put (the four types run the same kernels).  One
condition follows from the instruction mix: the discrete form's date does strictly less than the Asian call's (no exponential),
so it may not be slower than (a) by more than the spread.  The continuous form draws two Philox blocks per four dates in fp32
where the Asian call draws one: its ratios to (a) and (b) and the antithetic costs are printed as findings.
    python tools/lookback_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
BARRIER = 120.0
KIND = "floating-put"
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    names = ["discrete", "continuous", "discrete anti", "continuous anti", "(a) asian plain", "(b) barrier cont"]
    print(f"{'prec':4s} {'dates':>5s} {'paths':>10s} " + " ".join(f"{x:>20s}" for x in names) +
          f" {'disc/(a)':>8s} {'cont/(a)':>8s} {'cont/(b)':>8s} {'cont/disc':>9s} {'anti/plain d':>12s} {'anti/plain c':>12s} {'ns/date disc':>12s}")
    slower = []
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            paths //= scale

            def lookback(monitoring, anti):
                eng.set_antithetic(anti)
                r = eng.lookback(OPT, dates, paths, SEED, 0, X, KIND, monitoring)
                eng.set_antithetic(False)
                return r.kernel_ms

            forms = [lambda: lookback("discrete", False), lambda: lookback("continuous", False), lambda: lookback("discrete", True),
                     lambda: lookback("continuous", True), lambda: eng.asian(OPT, dates, paths, SEED, 0, X).kernel_ms,
                     lambda: eng.barrier(OPT, BARRIER, dates, paths, SEED, 0, X, "up-and-out", "continuous").kernel_ms]
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
                  f" {med[0] / med[4]:8.3f} {med[1] / med[4]:8.3f} {med[1] / med[5]:8.3f} {med[1] / med[0]:9.3f} {med[2] / med[0]:12.3f} {med[3] / med[1]:12.3f}"
                  f" {med[0] * 1e6 / (dates * paths):12.5f}", flush=True)
            if med[0] > med[4] * (1.0 + max(spread[0], spread[4])):
                slower.append((X, dates, paths, "discrete", med[0], med[4]))
    eng.close()
    print("rows where the discrete form is slower than the Asian call by more than the spread: " + (repr(slower) if slower else "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
