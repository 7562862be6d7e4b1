"""Kernel time of the calls under Merton's jump-diffusion (mc_merton_run_*) against two yardsticks, in one process.

For fp32 and fp64, at (256 dates x 1e7 paths) and (16 dates x 1e8 paths), kernel_ms (HIP events, timing on) of
    European | Asian | up-and-out, each plain and with antithetic variates, at lambda = 1 and at lambda = 0,
    (a) mc_asian_run_* plain | (b) mc_barrier_run_* discrete
at the same (dates, paths), as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread
(max - min) / median of each form's calls.  What to read: the Asian form's ratio to (a) and the up-and-out form's ratio to (b) say
what the jumps cost per date (a second Philox block per four fp32 or two fp64 dates, one compare and a branch, and on a date on
which some lane of the wave jumps the threshold loop); lambda = 0 has no thresholds and shows the walk alone.  Nothing is asserted:
the ratios are printed as findings.
    python tools/merton_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.05, v=0.2, t=1.0)
JUMPS = {"lambda": 1.0, "mu_j": -0.1, "delta": 0.15}
BARRIER = 120.0
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
ROWS = [(256, 10 ** 7), (16, 10 ** 8)]


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; (spread) = (max - min) / median")
    names = ["european", "asian", "up-and-out", "european anti", "asian anti", "up-and-out anti"]
    for X in ("f32", "f64"):
        for dates, paths in ROWS:
            paths //= scale

            def merton(payoff, anti, lam):
                jp = dict(JUMPS, **{"lambda": lam})
                eng.set_antithetic(anti)
                if payoff == 0:
                    r = eng.merton(OPT, jp, dates, paths, SEED, 0, X)
                elif payoff == 1:
                    r = eng.merton_asian(OPT, jp, dates, paths, SEED, 0, X)
                else:
                    r = eng.merton_barrier(OPT, jp, BARRIER, dates, paths, SEED, 0, X, "up-and-out")
                eng.set_antithetic(False)
                return r.kernel_ms

            forms, labels = [], []
            for lam in (1.0, 0.0):
                for anti in (False, True):
                    for payoff in (0, 1, 2):
                        forms.append(lambda payoff=payoff, anti=anti, lam=lam: merton(payoff, anti, lam))
                        labels.append(f"{names[payoff + 3 * anti]} lambda={lam:g}")
            forms += [lambda: eng.asian(OPT, dates, paths, SEED, 0, X).kernel_ms,
                      lambda: eng.barrier(OPT, BARRIER, dates, paths, SEED, 0, X, "up-and-out", "discrete").kernel_ms]
            labels += ["(a) asian plain", "(b) barrier discrete"]
            ms = [[] for _ in forms]
            for rep in range(WARM + REPS):
                for k, f in enumerate(forms):
                    t = f()
                    if rep >= WARM:
                        ms[k].append(t)
            med = [statistics.median(x) for x in ms]
            spread = [(max(x) - min(x)) / m for m, x in zip(med, ms)]
            a, b = med[-2], med[-1]
            print(f"{X} dates={dates} paths={paths}")
            for lab, m_, s_ in zip(labels, med, spread):
                print(f"  {lab:28s} {m_:10.3f} ms ({s_:6.2%})  /(a) {m_ / a:6.3f}  /(b) {m_ / b:6.3f}  ns/date/path {m_ * 1e6 / (dates * paths):9.5f}", flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
