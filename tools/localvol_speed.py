"""Kernel time of the local-volatility products (mc_localvol_run_*) beside the constant-volatility walks of the same commit, in one process.

For fp32 and fp64, at 128 steps x 1e7 paths, plain and antithetic, kernel_ms (HIP events, timing on) of
    mc_asian_run_* and mc_barrier_run_* (up-and-out, discrete) at 128 dates: the yardsticks |
    the Asian and the up-and-out call under a surface (128 dates x 1 step) on a flat 1 x 2, a displaced-diffusion 8 x 65 and a 32 x 64
    surface (the table cap), and the European call on the 8 x 65 surface
as the median of REPS calls after WARM warm-ups, the forms called in alternation, with the spread (max - min) / median of each form's
calls, and each local-volatility form's ratio to its yardstick (the European call's to mc_asian_run_*).  No ratio is fixed in advance:
the tool prints what it measured.
    python tools/localvol_speed.py [--quick]      (--quick: a tenth of the paths, to try the tool out)
"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import montecarlocuda_amd as mc  # noqa: E402

OPT = dict(s=100.0, k=100.0, r=0.03, v=0.2, t=1.0)
SEED = mc.MC_DEFAULT_SEED
WARM, REPS = 3, 10
STEPS, PATHS, BARRIER = 128, 10 ** 7, 130.0
Y_LO, Y_HI, SD, A = -1.5, 1.5, 0.2, 50.0


def displaced(n_times, n_nodes):
    """sigma(t, S) = SD (S + A e^{-r (T - t)}) / S at the slice midpoints and the nodes."""
    t = (np.arange(n_times) + 0.5) * OPT["t"] / n_times
    s = OPT["s"] * np.exp(np.linspace(Y_LO, Y_HI, n_nodes))
    return dict(sigma=SD * (s[None, :] + A * np.exp(-OPT["r"] * (OPT["t"] - t))[:, None]) / s[None, :], y_lo=Y_LO, y_hi=Y_HI)


SURFACES = {"flat 1x2": dict(sigma=np.full((1, 2), SD), y_lo=Y_LO, y_hi=Y_HI), "8x65": displaced(8, 65), "32x64": displaced(32, 64)}


def main(scale):
    eng = mc.Engine(0)
    print(eng.describe())
    paths = PATHS // scale
    print(f"{STEPS} steps x {paths} paths; kernel_ms: median of {REPS} calls after {WARM} warm-ups, forms alternated; "
          "(spread) = (max - min) / median; ratio = median / the yardstick's median")
    for X in ("f32", "f64"):
        for anti in (False, True):
            eng.set_antithetic(anti)
            names, forms, yard = ["mc_asian", "mc_barrier"], [], [0, 1]
            forms.append(lambda: eng.asian(OPT, STEPS, paths, SEED, 0, X).kernel_ms)
            forms.append(lambda: eng.barrier(OPT, BARRIER, STEPS, paths, SEED, 0, X, "up-and-out", "discrete").kernel_ms)
            for label, surf in SURFACES.items():
                names += [f"asian {label}", f"up-out {label}"]
                yard += [0, 1]
                forms.append(lambda s=surf: eng.localvol_asian(OPT, s, STEPS, 1, paths, "call", SEED, 0, X).kernel_ms)
                forms.append(lambda s=surf: eng.localvol_barrier(OPT, s, BARRIER, STEPS, 1, paths, "call", SEED, 0, X).kernel_ms)
            names.append("european 8x65")
            yard.append(0)
            forms.append(lambda: eng.localvol(OPT, SURFACES["8x65"], STEPS, paths, "call", SEED, 0, X).kernel_ms)
            ms = [[] for _ in forms]
            for rep in range(WARM + REPS):
                for k, f in enumerate(forms):
                    t = f()
                    if rep >= WARM:
                        ms[k].append(t)
            med = [statistics.median(x) for x in ms]
            for name, m, x, y in zip(names, med, ms, yard):
                print(f"{X:4s} {'anti ' if anti else 'plain'} {name:18s} {m:10.3f} ms ({(max(x) - min(x)) / m:6.2%})  ratio {m / med[y]:6.3f}  "
                      f"ns/step {m * 1e6 / (STEPS * paths):8.5f}", flush=True)
    eng.set_antithetic(False)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(10 if "--quick" in sys.argv else 1))
