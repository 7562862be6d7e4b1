"""Kernel time of the Asian call (mc_asian_run_*) against two yardsticks, in one process.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), kernel_ms (HIP events, timing on) of
    asian plain | asian control | (a) mc_cva_run_* at the same (dates, paths) | (b) mc_vanilla_run_* of dates x paths paths
as the median of REPS calls after WARM warm-ups, the four forms called in alternation.  (a): the Asian date step is a subset of
the CVA's -- the Asian call must not be slower in any row.  (b): the same number of normals and exponentials through the vanilla
loop, the rate of the generator-bound loop this kernel can approach; the ratio asian / (b) is printed, with the spread
(max - min) / median of each form's calls.  The control's extra cost is control / plain.
    python tools/asian_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    print(f"{'prec':4s} {'dates':>5s} {'paths':>10s} {'asian plain':>20s} {'asian control':>20s} {'(a) cva':>20s} {'(b) vanilla d x p':>20s}"
          f" {'ctrl/plain':>10s} {'plain/(a)':>9s} {'plain/(b)':>9s} {'ns/date plain':>13s}")
    slower = []
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            paths //= scale
            cva = dict(OPT, defint=0.03, lgd=0.4, n_grid=dates)

            def asian(control):
                eng.set_control_variate(control)
                r = eng.asian(OPT, dates, paths, SEED, 0, X)
                eng.set_control_variate(False)
                return r.kernel_ms

            forms = [lambda: asian(False), lambda: asian(True), lambda: eng.cva(cva, paths, SEED, 0, X).kernel_ms,
                     lambda: eng.vanilla(OPT, dates * paths, SEED, 0, X).kernel_ms]
            ms = [[] for _ in forms]
            for rep in range(WARM + REPS):
                for k, f in enumerate(forms):
                    t = f()
                    if rep >= WARM:
                        ms[k].append(t)
            med = [statistics.median(x) for x in ms]
            cells = [f"{m:10.3f} ({(max(x) - min(x)) / m:6.2%})" for m, x in zip(med, ms)]
            print(f"{X:4s} {dates:5d} {paths:10d} " + " ".join(f"{c:>20s}" for c in cells) +
                  f" {med[1] / med[0]:10.3f} {med[0] / med[2]:9.3f} {med[0] / med[3]:9.3f} {med[0] * 1e6 / (dates * paths):13.5f}", flush=True)
            for name, m in (("plain", med[0]), ("control", med[1])):
                if m > med[2]:
                    slower.append((X, dates, paths, name, m, med[2]))
    eng.close()
    print("rows slower than the CVA at the same size: " + (repr(slower) if slower else "none"))
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
