"""Kernel time of the worst-of autocallable notes (mc_autocall_run_*): the early exit on and off, and the cost next to the rainbow walk.

Part 1, the early exit.  Two builds of the engine are loaded into ONE process: the library as built (MC_AUTOCALL_EARLY_EXIT as
committed: 0, no exit) and a second one built with the other setting,
    make -C montecarlocuda_amd/csrc ab AB_FLAGS=-DMC_AUTOCALL_EARLY_EXIT=1 AB_OUT=../../tools/ab/libmc_mi355x_exit.so
and both time, in alternation, two contracts for fp32 and fp64, plain and antithetic:
    driver    the contract of drivers/autocallOpt.c (3 assets, 5 years, 20 observations on 1260 dates, triggers stepping down from
              1.00, coupon level 0.70, memory, knock-in 0.60 on every date): most paths are called early
    never     the same with every trigger infinite: no path is ever called, the exit is pure overhead
    at once   the same with every trigger at 1e-6: every path is called at the first observation, the most the exit can gain
Part 2, the cost of a call relative to mc_rainbow_run_* (put on the minimum, down-and-in) at the same (n, n_dates), all triggers
infinite, n = 1, 3, 8.
kernel_ms (HIP events) as the median of REPS calls after WARM warm-ups, with the spread (max - min) / median of each form's calls.
    python tools/autocall_speed.py [--other PATH] [--paths N]
"""
import ctypes as C
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 10
N_OBS, N_DATES = 20, 1260


def driver_market():
    import numpy as np
    s = np.array([100.0, 50.0, 200.0])
    corr = np.array([[1.0, 0.5, 0.4], [0.5, 1.0, 0.6], [0.4, 0.6, 1.0]])
    return dict(s=s, v=np.array([0.2, 0.3, 0.25]), w=1.0 / s, p=np.linalg.cholesky(corr), d=np.zeros(3), k=1.0, t=5.0, r=0.03)


def timed(names, forms):
    ms = [[] for _ in forms]
    for rep in range(WARM + REPS):
        for k, f in enumerate(forms):
            t = f()
            if rep >= WARM:
                ms[k].append(t)
    med = [statistics.median(x) for x in ms]
    spread = [(max(x) - min(x)) / m for m, x in zip(med, ms)]
    return dict(zip(names, zip(med, spread)))


def main(other, paths):
    import numpy as np
    import montecarlocuda_amd as mc
    from montecarlocuda_amd import _lib
    from montecarlocuda_amd.engine import _AutocallHolder

    def market(n):   # tools/rainbow_speed.py's: performance levels, volatilities 0.15 ... 0.35, the one-factor correlation beta_i beta_j
        beta = np.linspace(0.6, 0.8, n) if n > 1 else np.array([0.7])
        corr = np.outer(beta, beta)
        np.fill_diagonal(corr, 1.0)
        s = 100.0 * (1.0 + 0.1 * np.arange(n))
        return dict(s=s, v=np.linspace(0.15, 0.35, n) if n > 1 else np.array([0.25]), p=np.linalg.cholesky(corr), d=np.zeros(n), w=1.0 / s, k=1.0, t=5.0, r=0.03)

    seed = mc.MC_DEFAULT_SEED
    libs = {"as built": _lib.lib(), "other": _lib._declare(C.CDLL(other))}
    ctx = {}
    for name, L in libs.items():
        ctx[name] = C.c_void_p()
        _lib.check(L.mc_context_create(0, 0, C.byref(ctx[name])))

    def call(name, X, h, anti):
        L, r = libs[name], _lib.Result()
        L.mc_context_set_antithetic(ctx[name], int(anti))
        rc = getattr(L, f"mc_autocall_run_{X}")(ctx[name], C.byref(h.struct), seed, 0, paths, C.byref(r))
        if rc != 0:
            raise RuntimeError(L.mc_last_error().decode())
        return r.kernel_ms, r.expected

    b = driver_market()
    A = np.where(np.arange(N_OBS) < 2, math.inf, 1.0 - 0.01 * np.arange(N_OBS))
    print(f"Part 1: {paths} paths, as built = the committed setting of MC_AUTOCALL_EARLY_EXIT (0: no exit), other = {os.path.relpath(other, ROOT)}")
    print(f"kernel_ms: median of {REPS} calls after {WARM} warm-ups, builds and forms alternated in one process; spread = (max - min) / median", flush=True)
    for X in ("f32", "f64"):
        hs = {"driver": _AutocallHolder(X, b, N_DATES, A, 0.7, 0.02, 0.6, "dates", 1.0, True, N_OBS),
              "never": _AutocallHolder(X, b, N_DATES, math.inf, 0.7, 0.02, 0.6, "dates", 1.0, True, N_OBS),
              "at once": _AutocallHolder(X, b, N_DATES, 1e-6, 0.7, 0.02, 0.6, "dates", 1.0, True, N_OBS)}
        names, forms = [], []
        for contract, h in hs.items():
            for anti in (False, True):
                prices = {name: call(name, X, h, anti)[1] for name in libs}
                assert prices["as built"] == prices["other"], prices   # the exit changes no value
                for name in libs:
                    names.append((contract, anti, name))
                    forms.append(lambda name=name, h=h, anti=anti: call(name, X, h, anti)[0])
        res = timed(names, forms)
        for contract in hs:
            for anti in (False, True):
                a, o = res[(contract, anti, "as built")], res[(contract, anti, "other")]
                print(f"  {X} {contract:>7s} {'antithetic' if anti else 'plain':>10s}: as built {a[0]:9.3f} ms ({a[1]:.2%})   other {o[0]:9.3f} ms ({o[1]:.2%})   "
                      f"other / as built {o[0] / a[0]:.3f}", flush=True)

    dates = N_DATES // 4
    print(f"Part 2: mc_autocall_run_* with every trigger infinite (as built) next to mc_rainbow_run_* put-on-min down-and-in, {dates} dates, {paths} paths", flush=True)
    eng = mc.Engine(0)
    for X in ("f32", "f64"):
        for n in (1, 3, 8):
            bn = market(n)
            h = _AutocallHolder(X, bn, dates, math.inf, 0.7, 0.02, 0.6, "dates", 1.0, True, 5)
            res = timed(["autocall", "rainbow"], [lambda: call("as built", X, h, False)[0],
                                                  lambda: eng.rainbow(bn, dates, paths, "put-on-min", 0.6, "down-and-in", seed, 0, X).kernel_ms])
            a, r = res["autocall"], res["rainbow"]
            print(f"  {X} n={n} {dates} dates: autocall {a[0]:9.3f} ms ({a[1]:.2%})   rainbow {r[0]:9.3f} ms ({r[1]:.2%})   autocall / rainbow {a[0] / r[0]:.3f}", flush=True)
    eng.close()
    for name, L in libs.items():
        L.mc_context_destroy(ctx[name])
    return 0


if __name__ == "__main__":
    other = os.path.join(ROOT, "tools", "ab", "libmc_mi355x_exit.so")
    if "--other" in sys.argv:
        other = sys.argv[sys.argv.index("--other") + 1]
    paths = int(sys.argv[sys.argv.index("--paths") + 1]) if "--paths" in sys.argv else 4_000_000
    sys.exit(main(other, paths))
