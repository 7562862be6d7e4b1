"""Kernel time of the Bermudan put's two stages (mc_american_run_*, mc_american_fit_*) against the Asian call, in one process.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), kernel_ms (HIP events, timing on) of
    the pricing pass, plain and with antithetic variates, under a rule fitted once on 2^16 paths,
    (a) mc_asian_run_* plain
at the same (dates, paths), as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread
(max - min) / median of each form's calls; then a fit at 50 dates x 2^20 paths in both precisions (kernel_ms spans its 101
launches).  What to read: the pricing pass's ratio to (a) says what the payoff, the cubic, the compares and the select cost on top
of the Asian call's date (one exponential either way), and the fit's time per date says what a launch and the round trip of the
per-path state through device memory cost.  Nothing is asserted: the ratios are printed as findings.
    python tools/american_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=36.0, k=40.0, r=0.06, v=0.2, t=1.0)
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]
FIT = (50, 1 << 20)


def measure(forms):
    ms = [[] for _ in forms]
    for rep in range(WARM + REPS):
        for k, f in enumerate(forms):
            t = f()
            if rep >= WARM:
                ms[k].append(t)
    med = [statistics.median(x) for x in ms]
    return med, [(max(x) - min(x)) / m for m, x in zip(med, ms)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            paths //= scale
            beta, _ = eng.american_fit(OPT, dates, 1 << 16, "put", 3, SEED, 0, X)

            def american(anti):
                eng.set_antithetic(anti)
                r = eng.american(OPT, dates, beta, paths, SEED, 0, X, "put")
                eng.set_antithetic(False)
                return r.kernel_ms

            labels = ["american plain", "american anti", "(a) asian plain"]
            med, spread = measure([lambda: american(False), lambda: american(True), lambda: eng.asian(OPT, dates, paths, SEED, 0, X).kernel_ms])
            print(f"{X} dates={dates} paths={paths}")
            for lab, m_, s_ in zip(labels, med, spread):
                print(f"  {lab:28s} {m_:10.3f} ms ({s_:6.2%})  /(a) {m_ / med[-1]:6.3f}  ns/date/path {m_ * 1e6 / (dates * paths):9.5f}", flush=True)
    dates, paths = FIT[0], FIT[1] // scale
    for X in ("f32", "f64"):
        med, spread = measure([lambda: eng.american_fit(OPT, dates, paths, "put", 3, SEED, 0, X)[1].kernel_ms])
        print(f"{X} fit dates={dates} paths={paths}")
        print(f"  {'american fit':28s} {med[0]:10.3f} ms ({spread[0]:6.2%})  us/date {med[0] * 1e3 / dates:8.3f}  ns/date/path {med[0] * 1e6 / (dates * paths):9.5f}", flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
