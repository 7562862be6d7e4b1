"""Host-side mirror of the reference's GPU interface on top of the C ABI (ctypes, no torch).

Names follow the reference (marcomatteo/MonteCarloCUDA): ``OptionData``, ``MultiOptionData``,
``CVA``, ``OptionValue`` (MonteCarlo.h:32-65) and ``dev_vanillaOpt`` / ``dev_basketOpt`` /
``dev_cvaEquityOption`` (MonteCarloKernel.cu:500,483,517).  ``Engine`` is the persistent
per-GPU context underneath, with the explicit-seed / path-range API the multi-GPU harness uses.
The simulation itself always runs in libmc_mi355x.so on the GPU; nothing here computes paths.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import MC_DEFAULT_SEED, check, lib

NP = {"f32": np.float32, "f64": np.float64}


# ---- reference-shaped inputs / outputs ----------------------------------------------------
@dataclass
class OptionData:           # MonteCarlo.h:32-38
    s: float
    k: float
    r: float
    v: float
    t: float


@dataclass
class MultiOptionData:      # MonteCarlo.h:41-50; p = Cholesky factor at call time
    s: Sequence[float]
    v: Sequence[float]
    p: Sequence[Sequence[float]]
    d: Sequence[float]
    w: Sequence[float]
    k: float
    t: float
    r: float


@dataclass
class CVA:                  # MonteCarlo.h:57-65
    defInt: float
    lgd: float
    option: OptionData
    n: int
    ns: int = 0


@dataclass
class OptionValue:          # MonteCarlo.h:52-55
    Expected: float
    Confidence: float


@dataclass
class Estimate:
    expected: float
    confidence: float
    sum: float
    sum2: float
    n: int
    kernel_ms: float = 0.0
    wall_ms: float = 0.0

    def value(self) -> OptionValue:
        return OptionValue(self.expected, self.confidence)


@dataclass
class MlmcLevel:
    estimate: Estimate      # the level's sums and their closing; kernel_ms and wall_ms summed over its calls
    n_paths: int
    first_path: int


@dataclass
class MlmcEstimate:         # mc_mlmc_result
    price: float
    stderr: float           # one standard error of the discounted price
    bias: float             # max(|m_L|, |m_{L-1}| / 2)
    converged: bool
    levels: list


def _as_option(X, o) -> C.Structure:
    if isinstance(o, dict):
        o = OptionData(**{k: o[k] for k in "skrvt"})
    return _lib.OPTION[X](o.s, o.k, o.r, o.v, o.t)


class _BasketHolder:
    """Keeps the numpy arrays alive for as long as the ctypes struct is in use."""

    def __init__(self, X, b):
        if isinstance(b, dict):
            b = MultiOptionData(**{k: b[k] for k in ("s", "v", "p", "d", "w", "k", "t", "r")})
        dt = NP[X]
        self.n = len(b.s)
        self.arrs = [np.ascontiguousarray(a, dtype=dt) for a in (b.s, b.v, np.asarray(b.p, dtype=dt).reshape(-1),
                                                                  b.d, b.w)]
        if self.arrs[2].size != self.n * self.n or any(a.size != self.n for a in (self.arrs[0], self.arrs[1],
                                                                               self.arrs[3], self.arrs[4])):
            raise ValueError("basket arrays disagree on n")
        P = C.POINTER(_lib.CT[X])
        self.struct = _lib.BASKET[X](self.n, *[a.ctypes.data_as(P) for a in self.arrs], b.k, b.t, b.r)


class _RainbowHolder(_BasketHolder):
    """mc_rainbow_*: a basket (MultiOptionData or dict; "d" may be left out of a dict: zeros) with the contract's fields, or a dict
    that carries "n_dates" and optionally "kind", "barrier", "barrier_kind" itself.  kind: a name of _lib.RAINBOW_TYPES or the
    header's integer; barrier_kind: a name of _lib.BARRIER_TYPES, its integer, or None with barrier=None for no barrier."""

    def __init__(self, X, b, n_dates=None, kind=None, barrier=None, barrier_kind=None):
        if isinstance(b, dict):
            if n_dates is None:
                n_dates, kind = b["n_dates"], b.get("kind", "put-on-min")
                barrier, barrier_kind = b.get("barrier"), b.get("barrier_kind")
            b = dict(b, d=b.get("d", np.zeros(len(b["s"]))))
        super().__init__(X, b)
        if (barrier is None) != (barrier_kind is None):
            raise ValueError("rainbow: barrier and barrier_kind go together")
        kind = _lib.RAINBOW_TYPES[kind] if isinstance(kind, str) else int(kind)
        if barrier_kind is None:
            barrier, barrier_kind = 0.0, _lib.RAINBOW_NO_BARRIER
        barrier_kind = _lib.BARRIER_TYPES[barrier_kind] if isinstance(barrier_kind, str) else int(barrier_kind)
        self.basket = self.struct
        self.struct = _lib.RAINBOW[X](self.basket, float(barrier), int(n_dates), kind, barrier_kind)


class _AutocallHolder(_BasketHolder):
    """mc_autocall_*: a basket (MultiOptionData or dict; "d" may be left out of a dict: zeros) with the note's fields, or a dict that
    carries "n_dates", "autocall", "coupon_barrier", "coupon" and optionally "barrier", "ki", "gearing", "memory", "n_obs" itself.
    autocall and coupon_barrier: a sequence of n_obs levels each, or a scalar with an explicit n_obs."""

    def __init__(self, X, b, n_dates=None, autocall=None, coupon_barrier=None, coupon=None, barrier=None, ki="dates", gearing=None, memory=True,
                 n_obs=None):
        if isinstance(b, dict):
            if n_dates is None:
                n_dates, autocall, coupon_barrier, coupon = b["n_dates"], b["autocall"], b["coupon_barrier"], b["coupon"]
                barrier, ki, gearing = b.get("barrier"), b.get("ki", "dates"), b.get("gearing")
                memory, n_obs = b.get("memory", True), b.get("n_obs")
            b = dict(b, d=b.get("d", np.zeros(len(b["s"]))))
        super().__init__(X, b)
        levels = []
        for name, a in (("autocall", autocall), ("coupon_barrier", coupon_barrier)):
            if np.ndim(a) == 0:
                if n_obs is None:
                    raise ValueError(f"autocall: a scalar {name} needs an explicit n_obs")
                a = np.full(max(int(n_obs), 0), a)
            a = np.ascontiguousarray(a, dtype=NP[X]).reshape(-1)
            n_obs = a.size if n_obs is None else int(n_obs)
            if a.size != max(n_obs, 0):
                raise ValueError(f"autocall: {name} has {a.size} levels for n_obs={n_obs}")
            levels.append(a)
        if ki not in _lib.AUTOCALL_KI:
            ki_code = int(ki)
        else:
            ki_code = _lib.AUTOCALL_KI[ki]
        if (barrier is None) != (ki_code == _lib.AUTOCALL_KI[None]):
            raise ValueError("autocall: a knock-in level goes with ki=\"dates\" or \"maturity\", none with ki=None")
        if gearing is None:
            gearing = 1.0 / self.struct.k if self.struct.k > 0 else 0.0   # k <= 0 is refused by the library
        self.levels = levels
        self.basket = self.struct
        P = C.POINTER(_lib.CT[X])
        self.struct = _lib.AUTOCALL[X](self.basket, levels[0].ctypes.data_as(P), levels[1].ctypes.data_as(P), float(coupon),
                                       0.0 if barrier is None else float(barrier), float(gearing), int(n_dates), n_obs, int(memory), ki_code)


def _as_cva(X, c) -> C.Structure:
    if isinstance(c, dict):
        c = CVA(c["defint"], c["lgd"], OptionData(*(c[k] for k in "skrvt")), c["n_grid"])
    return _lib.CVA[X](c.defInt, c.lgd, _as_option(X, c.option), c.n)


def _as_asian(X, a, n_dates=None) -> C.Structure:
    """mc_asian_*: an option (OptionData or dict) with n_dates, or a dict that carries "n_dates" itself."""
    if n_dates is None:
        n_dates = a["n_dates"]
    return _lib.ASIAN[X](_as_option(X, a), int(n_dates))


def _as_barrier(X, o, barrier=None, n_dates=None, kind=None, monitoring=None) -> C.Structure:
    """mc_barrier_*: an option (OptionData or dict) with the barrier's fields, or a dict that carries "barrier", "n_dates" and
    optionally "kind" / "monitoring" itself.  kind and monitoring: the names of _lib.BARRIER_TYPES / _lib.MONITORING, or the
    header's integers."""
    if barrier is None:
        barrier, n_dates = o["barrier"], o["n_dates"]
        kind, monitoring = o.get("kind", "up-and-out"), o.get("monitoring", "discrete")
    kind = _lib.BARRIER_TYPES[kind] if isinstance(kind, str) else int(kind)
    monitoring = _lib.MONITORING[monitoring] if isinstance(monitoring, str) else int(monitoring)
    return _lib.BARRIER[X](_as_option(X, o), float(barrier), int(n_dates), kind, monitoring)


def _as_lookback(X, o, n_dates=None, kind=None, monitoring=None) -> C.Structure:
    """mc_lookback_*: an option (OptionData or dict) with the contract's fields, or a dict that carries "n_dates" and optionally "kind" /
    "monitoring" itself.  kind and monitoring: the names of _lib.LOOKBACK_TYPES / _lib.MONITORING, or the header's integers."""
    if n_dates is None:
        n_dates, kind, monitoring = o["n_dates"], o.get("kind", "floating-call"), o.get("monitoring", "discrete")
    kind = _lib.LOOKBACK_TYPES[kind] if isinstance(kind, str) else int(kind)
    monitoring = _lib.MONITORING[monitoring] if isinstance(monitoring, str) else int(monitoring)
    return _lib.LOOKBACK[X](_as_option(X, o), int(n_dates), kind, monitoring)


def _as_heston(X, o, model=None, n_steps=None) -> C.Structure:
    """mc_heston_*: an option (OptionData or dict; its v is ignored) with the model {v0, kappa, theta, xi, rho} and n_steps, or a
    dict that carries the model's five fields and "n_steps" itself."""
    if model is None:
        model, n_steps = o, o["n_steps"]
    opt = _as_option(X, o if not isinstance(o, dict) else dict(o, v=o.get("v", 0.0)))
    return _lib.HESTON[X](opt, *(float(model[f]) for f in ("v0", "kappa", "theta", "xi", "rho")), int(n_steps))


def _as_heston_path(X, o, model=None, n_dates=None, steps_per_date=None, payoff=None, barrier=None, kind=None) -> C.Structure:
    """mc_heston_path_*: an option and a model as for _as_heston with the contract's n_dates, the Euler steps per date and the payoff
    ("asian" or "barrier", then with the barrier and its kind), or a dict that carries "n_dates", "steps_per_date", "payoff" and
    for the barrier "barrier" and optionally "kind" itself."""
    if model is None:
        model, n_dates, steps_per_date, payoff = o, o["n_dates"], o["steps_per_date"], o["payoff"]
        barrier, kind = o.get("barrier"), o.get("kind", "up-and-out")
    payoff = _lib.HESTON_PATH_PAYOFFS[payoff] if isinstance(payoff, str) else int(payoff)
    kind = 0 if kind is None else _lib.BARRIER_TYPES[kind] if isinstance(kind, str) else int(kind)
    h = _as_heston(X, o, model, int(n_dates) * int(steps_per_date))
    return _lib.HESTON_PATH[X](h, int(steps_per_date), payoff, kind, 0.0 if barrier is None else float(barrier))


class _LocalVolHolder:
    """mc_localvol_*: the struct with its surface, a contiguous (n_times, n_nodes) array kept alive for as long as the struct is in
    use.  An option (OptionData or dict; its v is ignored) with the surface {sigma, y_lo, y_hi}, the contract's n_dates, the Euler
    steps per date, the payoff ("european", "asian" or "barrier", then with the barrier and its kind) and the right ("call" or
    "put"), or a dict that carries "sigma", "y_lo", "y_hi", "n_dates", "steps_per_date" and optionally "payoff", "right", "barrier",
    "kind" itself."""

    def __init__(self, X, o, surface=None, n_dates=None, steps_per_date=None, payoff=None, right="call", barrier=None, kind=None):
        if surface is None:
            surface, n_dates, steps_per_date = o, o["n_dates"], o["steps_per_date"]
            payoff, right = o.get("payoff", "european"), o.get("right", "call")
            barrier, kind = o.get("barrier"), o.get("kind", "up-and-out")
        payoff = _lib.LOCALVOL_PAYOFFS[payoff] if isinstance(payoff, str) else int(payoff)
        right = _lib.LOCALVOL_RIGHTS[right] if isinstance(right, str) else int(right)
        kind = 0 if kind is None else _lib.BARRIER_TYPES[kind] if isinstance(kind, str) else int(kind)
        self.sigma = np.ascontiguousarray(surface["sigma"], dtype=NP[X])
        if self.sigma.ndim != 2:
            raise ValueError(f"localvol: sigma has shape {self.sigma.shape}, expected (n_times, n_nodes)")
        opt = _as_option(X, o if not isinstance(o, dict) else dict(o, v=o.get("v", 0.0)))
        self.struct = _lib.LOCALVOL[X](opt, self.sigma.ctypes.data_as(C.POINTER(_lib.CT[X])), self.sigma.shape[0], self.sigma.shape[1],
                                       float(surface["y_lo"]), float(surface["y_hi"]), int(n_dates) * int(steps_per_date), int(steps_per_date),
                                       payoff, right, kind, 0.0 if barrier is None else float(barrier))


def _as_merton(X, o, jumps=None, n_dates=None, payoff=None, barrier=None, kind=None) -> C.Structure:
    """mc_merton_*: an option (OptionData or dict) with the jumps {lambda, mu_j, delta}, the contract's n_dates and the payoff
    ("european", "asian" or "barrier", then with the barrier and its kind), or a dict that carries the jumps' three fields,
    "n_dates", optionally "payoff" and for the barrier "barrier" and optionally "kind" itself."""
    if jumps is None:
        jumps, n_dates, payoff = o, o["n_dates"], o.get("payoff", "european")
        barrier, kind = o.get("barrier"), o.get("kind", "up-and-out")
    payoff = _lib.MERTON_PAYOFFS[payoff] if isinstance(payoff, str) else int(payoff)
    kind = 0 if kind is None else _lib.BARRIER_TYPES[kind] if isinstance(kind, str) else int(kind)
    return _lib.MERTON[X](_as_option(X, o), float(jumps["lambda"]), float(jumps["mu_j"]), float(jumps["delta"]), int(n_dates), payoff, kind,
                          0.0 if barrier is None else float(barrier))


def _as_american(X, o, n_dates=None, kind=None, degree=None) -> C.Structure:
    """mc_american_*: an option (OptionData or dict) with n_dates, the kind ("put" or "call") and the degree of a fit's
    polynomial, or a dict that carries "n_dates" and optionally "kind" and "degree" itself."""
    if n_dates is None:
        n_dates, kind, degree = o["n_dates"], o.get("kind", "put"), o.get("degree", 3)
    kind = _lib.AMERICAN_TYPES[kind] if isinstance(kind, str) else int(kind)
    return _lib.AMERICAN[X](_as_option(X, o), int(n_dates), kind, 3 if degree is None else int(degree))


class _AmericanHolder:
    """The contract's struct with its exercise rule: an (n_dates, 4) float64 array kept alive for as long as the struct is in use."""

    def __init__(self, X, o, beta, n_dates=None, kind=None, degree=None):
        if beta is None:
            beta = o["beta"]
        self.struct = _as_american(X, o, n_dates, kind, degree)
        self.beta = np.ascontiguousarray(beta, dtype=np.float64)
        if self.beta.shape != (self.struct.n_dates, 4):
            raise ValueError(f"beta has shape {self.beta.shape}, expected ({self.struct.n_dates}, 4)")
        self.beta_ptr = self.beta.ctypes.data_as(C.POINTER(C.c_double))


def _estimate(r: _lib.Result) -> Estimate:
    return Estimate(r.expected, r.confidence, r.sum, r.sum2, int(r.n), float(r.kernel_ms), float(r.wall_ms))


class Engine:
    """One persistent context on one MI355X (mc_context_create / mc_context_destroy)."""

    def __init__(self, device: int = 0, blocks: int = 0):
        self._ctx = C.c_void_p()
        check(lib().mc_context_create(device, blocks, C.byref(self._ctx)))
        self.device = device
        self.blocks = lib().mc_context_blocks(self._ctx)
        self.stream = lib().mc_context_stream(self._ctx) or 0
        # the C context also enters the fp32-normals mode from the environment at creation (mc_api.hip: context_allocate)
        self._normals_f32 = os.environ.get("MC_F64_NORMALS") == "f32"

    def close(self):
        if self._ctx:
            lib().mc_context_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        name = C.create_string_buffer(128)
        cus, mhz = C.c_int(), C.c_int()
        check(lib().mc_context_info(self._ctx, name, 128, C.byref(cus), C.byref(mhz)))
        return {"name": name.value.decode(), "compute_units": cus.value, "clock_mhz": mhz.value,
                "blocks": self.blocks}

    def last_call_stats(self):
        """Stage breakdown (ms) of this context's last synchronous call: mc_context_last_call_stats."""
        from ._lib import CallStats
        k = CallStats()
        check(lib().mc_context_last_call_stats(self._ctx, C.byref(k)))
        return {f: getattr(k, f) for f, _ in CallStats._fields_}

    def describe(self):
        """The context's resolved configuration as one line (what MC_VERBOSE=2 prints at creation)."""
        buf = C.create_string_buffer(1024)
        check(lib().mc_context_describe(self._ctx, buf, 1024))
        return buf.value.decode()

    def last_launch(self):
        """(workgroups, lanes per workgroup) of the most recent simulation launch of this context."""
        g, t = C.c_int(), C.c_int()
        check(lib().mc_context_last_launch(self._ctx, C.byref(g), C.byref(t)))
        return g.value, t.value

    def set_antithetic(self, on: bool):
        """Plain Monte Carlo (the reference's estimator) or antithetic variates (pair means)."""
        check(lib().mc_context_set_antithetic(self._ctx, 1 if on else 0))

    def set_control_variate(self, on: bool):
        """Baskets and Asian calls: simulate payoff(arithmetic) - payoff(geometric) and add the geometric closed form back."""
        check(lib().mc_context_set_control_variate(self._ctx, 1 if on else 0))

    def order(self, stream: int):
        """Make `stream` (a hipStream_t handle) wait for everything this context has enqueued so far."""
        check(lib().mc_context_order(self._ctx, C.c_void_p(stream)))

    def idle(self) -> bool:
        """True when everything this context has enqueued has completed (a user-space poll, no sleeping)."""
        r = lib().mc_context_idle(self._ctx)
        if r < 0:
            raise _lib.McError("mc_context_idle failed")
        return r == 1

    def arm_direct(self):
        """The NEXT launch() also delivers its triple into a pinned host slot (mc_context_arm_direct).  Returns the slot
        (ctypes pointer to 3 doubles, word 2 preset to -1): poll with wait_slot()."""
        slot = C.POINTER(C.c_double)()
        check(lib().mc_context_arm_direct(self._ctx, C.byref(slot)))
        return slot

    def publish(self, d_src_ptr: int, stream: int):
        """Enqueue on `stream` the copy of the 3 doubles at device address d_src_ptr into a pinned host slot
        (mc_context_publish): how a triple that another kernel produced -- an all-reduce -- reaches a polling host."""
        slot = C.POINTER(C.c_double)()
        check(lib().mc_context_publish(self._ctx, C.c_void_p(d_src_ptr), C.c_void_p(stream), C.byref(slot)))
        return slot

    @staticmethod
    def wait_slot(slot, timeout_s: float = 30.0):
        """Poll a slot from user space until its n word is written; returns (sum, sum2, n)."""
        import time
        t0 = time.perf_counter()
        spins = 0
        while slot[2] == -1.0:
            spins += 1
            if (spins & 0xFFFF) == 0 and time.perf_counter() - t0 > timeout_s:
                raise _lib.McError("the device never delivered the result")
        return slot[0], slot[1], slot[2]

    def set_timing(self, on: bool):
        """Synchronous calls: HIP events + copy + synchronize (kernel_ms reported; default) or, off, the result written
        straight to pinned host memory and polled from user space (kernel_ms = 0, ~10 us less per call)."""
        check(lib().mc_context_set_timing(self._ctx, 1 if on else 0))

    def set_finish(self, fused: bool):
        """Final reduction inside the simulation kernel (default) or as a second launch (A/B baseline)."""
        check(lib().mc_context_set_finish(self._ctx, 1 if fused else 0))

    def set_generator(self, name: str, subsequence_base: int = 0):
        """'philox' (default; counter-based) or 'xorwow' (the reference's generator, one sequence per lane)."""
        check(lib().mc_context_set_generator(self._ctx, {"philox": 0, "xorwow": 1}[name], subsequence_base))

    def set_cva_date_lanes(self, lanes: int):
        """CVA: adjacent lanes sharing one path's dates (0 = by call size, 1 = never, 2 ... 64 = the whole call date-parallel)."""
        check(lib().mc_context_set_cva_date_lanes(self._ctx, int(lanes)))

    def set_normals(self, mode: str):
        """fp64 kernels: 'native' (default; true fp64 normals) or 'f32' (the reference's dp arithmetic: a float normal
        widened to double, four per Philox block)."""
        check(lib().mc_context_set_normals(self._ctx, {"native": 0, "f32": 1}[mode]))
        self._normals_f32 = mode == "f32"

    def xorwow_words(self, seed, first_subsequence, n_subsequences, words_each):
        out = np.empty((n_subsequences, words_each), dtype=np.uint32)
        check(lib().mc_xorwow_words(self._ctx, seed, first_subsequence, n_subsequences, words_each,
                                    out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def profile(self, every: int):
        """Sample the simulation kernel's device time on every `every`-th launch (0 = off)."""
        check(lib().mc_context_profile(self._ctx, every))

    def profile_read(self):
        """(samples, total_ms) of the sampled simulation-kernel launches since the last read."""
        n, ms = C.c_int(), C.c_double()
        check(lib().mc_context_profile_read(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # ---- synchronous estimators --------------------------------------------------------
    def _run(self, prod, X, struct, seed, first, n):
        r = _lib.Result()
        check(getattr(lib(), f"mc_{prod}_run_{X}")(self._ctx, C.byref(struct), seed, first, n, C.byref(r)))
        return _estimate(r)

    def vanilla(self, opt, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        return self._run("vanilla", precision, _as_option(precision, opt), seed, first_path, n_paths)

    @staticmethod
    def book_entries(options, n_paths, seeds=None, first_paths=None, precision="f64"):
        """The ctypes array of mc_book_entry_{f32,f64} for a book: n_paths, seeds and first_paths are one value for every
        option or one per option (seeds default to MC_DEFAULT_SEED, first paths to 0)."""
        B = len(options)

        def per(x, default):
            x = default if x is None else x
            xs = list(x) if isinstance(x, (list, tuple, np.ndarray)) else [x] * B
            if len(xs) != B:
                raise ValueError("vanilla_book: one value per option expected")
            return [int(v) for v in xs]
        ns, ss, fs = per(n_paths, None), per(seeds, MC_DEFAULT_SEED), per(first_paths, 0)
        arr = (_lib.BOOK_ENTRY[precision] * B)()
        for i, o in enumerate(options):
            arr[i].option = _as_option(precision, o)
            arr[i].seed, arr[i].first_path, arr[i].n_paths = ss[i], fs[i], ns[i]
        return arr

    def vanilla_book(self, options, n_paths, seeds=None, first_paths=None, precision="f64"):
        """A book of vanilla calls priced in one launch (mc_vanilla_book_run_*): one Estimate per option, each from the same
        per-path payoffs as vanilla(option, n, seed, first_path, precision)."""
        arr = self.book_entries(options, n_paths, seeds, first_paths, precision)
        res = (_lib.Result * len(arr))()
        check(getattr(lib(), f"mc_vanilla_book_run_{precision}")(self._ctx, arr, len(arr), res))
        return [_estimate(r) for r in res]

    def vanilla_book_launch(self, options, n_paths, d_triples_ptr: int, seeds=None, first_paths=None, precision="f64", stream: int = 0):
        """Enqueue a book (mc_vanilla_book_launch_*): entry i's undiscounted {sum, sum2, n} into the 3 doubles at
        d_triples_ptr + 24 i (device memory), on `stream` (0 = the HIP null stream)."""
        arr = self.book_entries(options, n_paths, seeds, first_paths, precision)
        check(getattr(lib(), f"mc_vanilla_book_launch_{precision}")(self._ctx, arr, len(arr), C.c_void_p(d_triples_ptr), C.c_void_p(stream)))

    def vanilla_greeks(self, opt, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """(price, delta, vega) Estimates from one pass (pathwise derivatives)."""
        g = _lib.Greeks()
        check(getattr(lib(), f"mc_vanilla_greeks_run_{precision}")(self._ctx, C.byref(_as_option(precision, opt)), seed,
                                                                    first_path, n_paths, C.byref(g)))
        return _estimate(g.price), _estimate(g.delta), _estimate(g.vega)

    def vanilla_greeks_lr(self, opt, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """(price, delta, vega) Estimates by the likelihood-ratio method (score of the density x payoff)."""
        g = _lib.Greeks()
        check(getattr(lib(), f"mc_vanilla_greeks_lr_run_{precision}")(self._ctx, C.byref(_as_option(precision, opt)), seed,
                                                                       first_path, n_paths, C.byref(g)))
        return _estimate(g.price), _estimate(g.delta), _estimate(g.vega)

    def basket_greeks(self, b, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", lr=False):
        """(price, [delta per asset], [vega per asset]) Estimates: pathwise derivatives, or (lr=True) likelihood-ratio forms."""
        h = _BasketHolder(precision, b)
        price = _lib.Result()
        delta, vega = (_lib.Result * h.n)(), (_lib.Result * h.n)()
        check(getattr(lib(), f"mc_basket_greeks{'_lr' if lr else ''}_run_{precision}")(self._ctx, C.byref(h.struct), seed, first_path, n_paths,
                                                                                        C.byref(price), delta, vega))
        return _estimate(price), [_estimate(x) for x in delta], [_estimate(x) for x in vega]

    def vanilla_greeks2(self, opt, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """(price, delta, vega, gamma, vanna) Estimates from one pass: delta and vega pathwise (the same bits as vanilla_greeks),
        gamma and vanna by the mixed estimator (likelihood ratio of the pathwise delta)."""
        g = _lib.Greeks2()
        check(getattr(lib(), f"mc_vanilla_greeks2_run_{precision}")(self._ctx, C.byref(_as_option(precision, opt)), seed,
                                                                     first_path, n_paths, C.byref(g)))
        return _estimate(g.price), _estimate(g.delta), _estimate(g.vega), _estimate(g.gamma), _estimate(g.vanna)

    def basket_gamma(self, b, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """(price, gamma) Estimates: gamma[a][b] = d2V / dS_a dS_b, an n x n list of lists (symmetric), by the mixed estimator."""
        h = _BasketHolder(precision, b)
        price = _lib.Result()
        gamma = (_lib.Result * (h.n * h.n))()
        check(getattr(lib(), f"mc_basket_gamma_run_{precision}")(self._ctx, C.byref(h.struct), seed, first_path, n_paths,
                                                                  C.byref(price), gamma))
        return _estimate(price), [[_estimate(gamma[a * h.n + c]) for c in range(h.n)] for a in range(h.n)]

    def cva_greeks(self, c, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", lr=False):
        """(cva, delta, vega) Estimates: the CVA and its derivatives with respect to spot and volatility, pathwise or (lr=True)
        by the likelihood ratio."""
        g = _lib.CvaGreeks()
        check(getattr(lib(), f"mc_cva_greeks{'_lr' if lr else ''}_run_{precision}")(self._ctx, C.byref(_as_cva(precision, c)), seed, first_path,
                                                                                     n_paths, C.byref(g)))
        return _estimate(g.cva), _estimate(g.delta), _estimate(g.vega)

    def basket(self, b, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        h = _BasketHolder(precision, b)
        return self._run("basket", precision, h.struct, seed, first_path, n_paths)

    def cva(self, c, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        return self._run("cva", precision, _as_cva(precision, c), seed, first_path, n_paths)

    def asian(self, opt, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """Arithmetic-average call over n_dates equally spaced dates (mc_asian_run_*); honours set_antithetic and
        set_control_variate (the geometric-average control's closed-form mean is added back)."""
        return self._run("asian", precision, _as_asian(precision, opt, n_dates), seed, first_path, n_paths)

    def barrier(self, opt, barrier, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="up-and-out",
                monitoring="discrete") -> Estimate:
        """Single-barrier call on n_dates equally spaced dates (mc_barrier_run_*).  kind: "up-and-out", "up-and-in", "down-and-out",
        "down-and-in"; monitoring: "discrete" (on the dates only) or "continuous" (Brownian-bridge survival probability between
        the dates: unbiased for the continuously monitored price, barrier_closed_form).  Honours set_antithetic."""
        return self._run("barrier", precision, _as_barrier(precision, opt, barrier, n_dates, kind, monitoring), seed, first_path, n_paths)

    def rainbow(self, basket, n_dates, n_paths, kind="put-on-min", barrier=None, barrier_kind=None, seed=MC_DEFAULT_SEED, first_path=0,
                precision="f64") -> Estimate:
        """Worst-of / best-of option on the basket's correlated assets walked over n_dates dates (mc_rainbow_run_*): kind is
        "call-on-min", "call-on-max", "put-on-min" or "put-on-max"; barrier and barrier_kind ("up-and-out" ... "down-and-in") put a
        barrier on the same extremum, monitored on the dates.  The basket's k, t, r are the strike, maturity and rate.  Honours
        set_antithetic."""
        h = _RainbowHolder(precision, basket, n_dates, kind, barrier, barrier_kind)
        return self._run("rainbow", precision, h.struct, seed, first_path, n_paths)

    def autocall(self, basket, n_dates, n_paths, autocall, coupon_barrier, coupon, barrier=None, ki="dates", gearing=None, memory=True,
                 seed=MC_DEFAULT_SEED, first_path=0, precision="f64", n_obs=None) -> Estimate:
        """Worst-of autocallable note on the basket's correlated assets walked over n_dates dates (mc_autocall_run_*).  autocall and
        coupon_barrier: the trigger and coupon levels per observation date, a sequence of n_obs values each (n_obs must divide
        n_dates) or a scalar with an explicit n_obs=; math.inf as a trigger: not callable there; 0 as a coupon level: unconditional.
        coupon: the amount per observation (notional 1), memory: missed coupons are paid with the next one.  barrier: the knock-in
        level of the put struck at the basket's k, monitored on all dates (ki="dates") or at maturity only (ki="maturity");
        ki=None with barrier=None: the put is always live.  gearing=None: 1 / k.  `expected` is the note's present value.  Honours
        set_antithetic."""
        h = _AutocallHolder(precision, basket, n_dates, autocall, coupon_barrier, coupon, barrier, ki, gearing, memory, n_obs)
        return self._run("autocall", precision, h.struct, seed, first_path, n_paths)

    def lookback(self, opt, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="floating-call",
                 monitoring="discrete") -> Estimate:
        """Lookback option on n_dates equally spaced dates (mc_lookback_run_*).  kind: "floating-call", "floating-put", "fixed-call",
        "fixed-put" (opt's k is ignored by the floating types); monitoring: "discrete" (the extremum over the dates) or "continuous"
        (Brownian-bridge maxima between the dates: unbiased for the continuously monitored price, lookback_closed_form).  Honours
        set_antithetic."""
        return self._run("lookback", precision, _as_lookback(precision, opt, n_dates, kind, monitoring), seed, first_path, n_paths)

    def heston(self, opt, model, n_steps, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """European call under the Heston model, full-truncation Euler on n_steps equal steps (mc_heston_run_*).  model: a dict
        with v0, kappa, theta, xi, rho; opt's v is ignored.  Honours set_antithetic; biased by the scheme against
        heston_closed_form, the price of the continuous model."""
        return self._run("heston", precision, _as_heston(precision, opt, model, n_steps), seed, first_path, n_paths)

    def heston_asian(self, opt, model, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """Arithmetic-average call over n_dates equally spaced dates under the Heston model, full-truncation Euler with
        steps_per_date steps between two dates (mc_heston_path_run_*).  Honours set_antithetic."""
        return self._run("heston_path", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "asian"), seed, first_path, n_paths)

    def heston_barrier(self, opt, model, barrier, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64",
                       kind="up-and-out") -> Estimate:
        """Single-barrier call monitored on n_dates equally spaced dates under the Heston model, steps_per_date Euler steps between
        two dates (mc_heston_path_run_*).  kind as for barrier(); there is no continuous monitoring.  Honours set_antithetic."""
        return self._run("heston_path", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "barrier", barrier, kind), seed,
                         first_path, n_paths)

    def heston_level(self, opt, model, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """One multilevel correction on the Heston walk (mc_heston_level_run_*): Y = P_fine - P_coarse of the Asian call (n_dates = 1:
        the European call), the fine walk on n_dates * steps_per_date steps (steps_per_date even), the coarse walk on half of them, on
        the same Brownian increments.  `expected` is the discounted mean of Y.  Honours set_antithetic."""
        return self._run("heston_level", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "asian"), seed, first_path, n_paths)

    def heston_mlmc(self, opt, model, n_dates, steps_per_date, eps, seed=MC_DEFAULT_SEED, precision="f64", min_levels=2, max_levels=8,
                    n_pilot=10_000) -> "MlmcEstimate":
        """The call of heston_asian(opt, model, n_dates, steps_per_date, ...) priced to a root-mean-square error eps by multilevel
        Monte Carlo (mc_heston_mlmc_run_*): level 0 on n_dates * steps_per_date steps, level l on 2^l times as many."""
        spec = _lib.MlmcSpec(float(eps), int(min_levels), int(max_levels), int(n_pilot))
        r = _lib.MlmcResult()
        struct = _as_heston_path(precision, opt, model, n_dates, steps_per_date, "asian")
        check(getattr(lib(), f"mc_heston_mlmc_run_{precision}")(self._ctx, C.byref(struct), C.byref(spec), seed, C.byref(r)))
        levels = [MlmcLevel(_estimate(r.level[l].result), int(r.level[l].n_paths), int(r.level[l].first_path)) for l in range(r.levels)]
        return MlmcEstimate(r.price, r.stderr_, r.bias, bool(r.converged), levels)

    def localvol(self, opt, surface, n_steps, n_paths, right="call", seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """European call or put under a local-volatility surface, log-Euler on n_steps equal steps (mc_localvol_run_*).  surface:
        a dict with sigma (an (n_times, n_nodes) array of volatilities over equal time slices and equally spaced nodes of
        ln(S / s)), y_lo and y_hi; opt's v is ignored.  Honours set_antithetic."""
        h = _LocalVolHolder(precision, opt, surface, 1, n_steps, "european", right)
        return self._run("localvol", precision, h.struct, seed, first_path, n_paths)

    def localvol_asian(self, opt, surface, n_dates, steps_per_date, n_paths, right="call", seed=MC_DEFAULT_SEED, first_path=0,
                       precision="f64") -> Estimate:
        """Arithmetic-average call or put over n_dates equally spaced dates under a local-volatility surface, steps_per_date Euler
        steps between two dates (mc_localvol_run_*).  Honours set_antithetic."""
        h = _LocalVolHolder(precision, opt, surface, n_dates, steps_per_date, "asian", right)
        return self._run("localvol", precision, h.struct, seed, first_path, n_paths)

    def localvol_barrier(self, opt, surface, barrier, n_dates, steps_per_date, n_paths, right="call", seed=MC_DEFAULT_SEED, first_path=0,
                         precision="f64", kind="up-and-out") -> Estimate:
        """Single-barrier call or put monitored on n_dates equally spaced dates under a local-volatility surface
        (mc_localvol_run_*).  kind as for barrier(); there is no continuous monitoring.  Honours set_antithetic."""
        h = _LocalVolHolder(precision, opt, surface, n_dates, steps_per_date, "barrier", right, barrier, kind)
        return self._run("localvol", precision, h.struct, seed, first_path, n_paths)

    def merton(self, opt, jumps, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """European call under Merton's jump-diffusion, walked over n_dates equally spaced dates (mc_merton_run_*; exact in law
        at any n_dates, merton_closed_form).  jumps: a dict with lambda, mu_j, delta.  Honours set_antithetic."""
        return self._run("merton", precision, _as_merton(precision, opt, jumps, n_dates, "european"), seed, first_path, n_paths)

    def merton_asian(self, opt, jumps, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64") -> Estimate:
        """Arithmetic-average call over n_dates equally spaced dates under Merton's jump-diffusion (mc_merton_run_*)."""
        return self._run("merton", precision, _as_merton(precision, opt, jumps, n_dates, "asian"), seed, first_path, n_paths)

    def merton_barrier(self, opt, jumps, barrier, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64",
                       kind="up-and-out") -> Estimate:
        """Single-barrier call under Merton's jump-diffusion, the barrier monitored on the n_dates dates only (mc_merton_run_*).
        kind as for barrier(); there is no continuous monitoring."""
        return self._run("merton", precision, _as_merton(precision, opt, jumps, n_dates, "barrier", barrier, kind), seed, first_path, n_paths)

    def american(self, opt, n_dates, beta, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="put") -> Estimate:
        """Bermudan put or call on n_dates equally spaced exercise dates under the exercise rule beta, an (n_dates, 4) table of
        cubics in the payoff (mc_american_run_*): a lower bound of the price when beta was not fitted on these paths.  Honours
        set_antithetic."""
        h = _AmericanHolder(precision, opt, beta, n_dates, kind)
        r = _lib.Result()
        check(getattr(lib(), f"mc_american_run_{precision}")(self._ctx, C.byref(h.struct), h.beta_ptr, seed, first_path, n_paths, C.byref(r)))
        return _estimate(r)

    def american_fit(self, opt, n_dates, n_paths, kind="put", degree=3, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """The exercise rule of a Bermudan put or call by Longstaff-Schwartz on n_paths (<= 2^24) paths of their own
        (mc_american_fit_*): (beta, Estimate), beta the (n_dates, 4) table american() prices, the Estimate the in-sample one
        (biased high)."""
        s = _as_american(precision, opt, n_dates, kind, degree)
        beta = np.zeros((min(max(int(n_dates), 1), _lib.MAX_AMERICAN_DATES), 4), dtype=np.float64)   # an n_dates out of range is refused before beta is written
        r = _lib.Result()
        check(getattr(lib(), f"mc_american_fit_{precision}")(self._ctx, C.byref(s), seed, first_path, n_paths,
                                                              beta.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return beta, _estimate(r)

    def american_fit_date(self, opt, n_dates, j, W, V, beta_next, kind="put", degree=3, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        """Test hook (mc_american_fit_date_*): one date launch of the fit on the state (W, V) of date j + 1; returns (W_j, V, sums)."""
        s = _as_american(precision, opt, n_dates, kind, degree)
        W, V = np.array(W, dtype=NP[precision]), np.array(V, dtype=NP[precision])
        b = np.ascontiguousarray(beta_next, dtype=np.float64)
        sums = np.zeros(12, dtype=np.float64)
        RP, DP = C.POINTER(_lib.CT[precision]), C.POINTER(C.c_double)
        check(getattr(lib(), f"mc_american_fit_date_{precision}")(self._ctx, C.byref(s), int(j), b.ctypes.data_as(DP), seed, first_path, W.size,
                                                                   W.ctypes.data_as(RP), V.ctypes.data_as(RP), sums.ctypes.data_as(DP)))
        return W, V, sums

    # ---- asynchronous launches (device triple, caller's stream) ------------------------
    def launch(self, prod, precision, struct, seed, first_path, n_paths, d_triple_ptr: int, stream: int = 0):
        """Enqueue; d_triple_ptr = device address of 3 doubles, stream = hipStream_t handle (0 = the HIP null
        stream; ``self.stream`` is the context's own)."""
        if prod == "american":   # struct: what prepared("american", ...) returned, the contract with its rule
            check(getattr(lib(), f"mc_american_launch_{precision}")(self._ctx, C.byref(struct.struct), struct.beta_ptr, seed, first_path,
                                                                     n_paths, C.c_void_p(d_triple_ptr), C.c_void_p(stream)))
            return
        check(getattr(lib(), f"mc_{prod}_launch_{precision}")(self._ctx, C.byref(struct), seed, first_path,
                                                               n_paths, C.c_void_p(d_triple_ptr),
                                                               C.c_void_p(stream)))

    def prepared(self, prod, precision, inputs):
        """ctypes struct (plus whatever must stay alive) for repeated launch() calls."""
        if prod == "vanilla":
            return _as_option(precision, inputs), None
        if prod == "basket":
            h = _BasketHolder(precision, inputs)
            return h.struct, h
        if prod == "asian":   # inputs: the option's fields plus "n_dates"
            return _as_asian(precision, inputs), None
        if prod == "heston":   # inputs: the option's fields plus "v0", "kappa", "theta", "xi", "rho" and "n_steps"
            return _as_heston(precision, inputs), None
        if prod == "heston_path":   # inputs: those of "heston" without "n_steps", plus "n_dates", "steps_per_date", "payoff", ("barrier", "kind")
            return _as_heston_path(precision, inputs), None
        if prod == "heston_level":   # inputs: those of "heston_path" (the fine walk; "payoff" optional, "asian" if given; steps_per_date even)
            return _as_heston_path(precision, dict(inputs, payoff=inputs.get("payoff", "asian"))), None
        if prod == "localvol":   # inputs: the option's fields plus "sigma", "y_lo", "y_hi", "n_dates", "steps_per_date" and optionally "payoff", "right", "barrier", "kind"
            h = _LocalVolHolder(precision, inputs)
            return h.struct, h
        if prod == "american":   # inputs: the option's fields plus "n_dates", "beta" and optionally "kind", "degree"
            h = _AmericanHolder(precision, inputs, None)
            return h, h
        if prod == "merton":   # inputs: the option's fields plus "lambda", "mu_j", "delta", "n_dates" and optionally "payoff", "barrier", "kind"
            return _as_merton(precision, inputs), None
        if prod == "rainbow":   # inputs: the basket's fields ("d" optional) plus "n_dates" and optionally "kind", "barrier", "barrier_kind"
            h = _RainbowHolder(precision, inputs)
            return h.struct, h
        if prod == "autocall":   # inputs: the basket's fields ("d" optional) plus "n_dates", "autocall", "coupon_barrier", "coupon" and optionally "barrier", "ki", "gearing", "memory", "n_obs"
            h = _AutocallHolder(precision, inputs)
            return h.struct, h
        if prod == "lookback":   # inputs: the option's fields plus "n_dates" and optionally "kind", "monitoring"
            return _as_lookback(precision, inputs), None
        if prod == "barrier":   # inputs: the option's fields plus "barrier", "n_dates" and optionally "kind", "monitoring"
            return _as_barrier(precision, inputs), None
        return _as_cva(precision, inputs), None

    # ---- per-path values (parity tests) ------------------------------------------------
    def _paths(self, prod, X, struct, seed, first, n):
        out = np.empty(n, dtype=NP[X])
        check(getattr(lib(), f"mc_{prod}_paths_{X}")(self._ctx, C.byref(struct), seed, first, n,
                                                      out.ctypes.data_as(C.POINTER(_lib.CT[X]))))
        return out

    def vanilla_paths(self, opt, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("vanilla", precision, _as_option(precision, opt), seed, first_path, n_paths)

    def basket_paths(self, b, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        h = _BasketHolder(precision, b)
        return self._paths("basket", precision, h.struct, seed, first_path, n_paths)

    def cva_paths(self, c, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("cva", precision, _as_cva(precision, c), seed, first_path, n_paths)

    def asian_paths(self, opt, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("asian", precision, _as_asian(precision, opt, n_dates), seed, first_path, n_paths)

    def barrier_paths(self, opt, barrier, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="up-and-out",
                      monitoring="discrete"):
        return self._paths("barrier", precision, _as_barrier(precision, opt, barrier, n_dates, kind, monitoring), seed, first_path, n_paths)

    def rainbow_paths(self, basket, n_dates, n_paths, kind="put-on-min", barrier=None, barrier_kind=None, seed=MC_DEFAULT_SEED, first_path=0,
                      precision="f64"):
        h = _RainbowHolder(precision, basket, n_dates, kind, barrier, barrier_kind)
        return self._paths("rainbow", precision, h.struct, seed, first_path, n_paths)

    def autocall_paths(self, basket, n_dates, n_paths, autocall, coupon_barrier, coupon, barrier=None, ki="dates", gearing=None, memory=True,
                       seed=MC_DEFAULT_SEED, first_path=0, precision="f64", n_obs=None):
        """The per-path present values of autocall() (discounted, unlike the other *_paths)."""
        h = _AutocallHolder(precision, basket, n_dates, autocall, coupon_barrier, coupon, barrier, ki, gearing, memory, n_obs)
        return self._paths("autocall", precision, h.struct, seed, first_path, n_paths)

    def lookback_paths(self, opt, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="floating-call",
                       monitoring="discrete"):
        return self._paths("lookback", precision, _as_lookback(precision, opt, n_dates, kind, monitoring), seed, first_path, n_paths)

    def merton_paths(self, opt, jumps, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("merton", precision, _as_merton(precision, opt, jumps, n_dates, "european"), seed, first_path, n_paths)

    def merton_asian_paths(self, opt, jumps, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("merton", precision, _as_merton(precision, opt, jumps, n_dates, "asian"), seed, first_path, n_paths)

    def merton_barrier_paths(self, opt, jumps, barrier, n_dates, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="up-and-out"):
        return self._paths("merton", precision, _as_merton(precision, opt, jumps, n_dates, "barrier", barrier, kind), seed, first_path, n_paths)

    def american_paths(self, opt, n_dates, beta, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64", kind="put"):
        """The per-path values of american(): in units of the strike, compounded to maturity."""
        h = _AmericanHolder(precision, opt, beta, n_dates, kind)
        out = np.empty(n_paths, dtype=NP[precision])
        check(getattr(lib(), f"mc_american_paths_{precision}")(self._ctx, C.byref(h.struct), h.beta_ptr, seed, first_path, n_paths,
                                                                out.ctypes.data_as(C.POINTER(_lib.CT[precision]))))
        return out

    def heston_paths(self, opt, model, n_steps, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("heston", precision, _as_heston(precision, opt, model, n_steps), seed, first_path, n_paths)

    def heston_asian_paths(self, opt, model, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("heston_path", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "asian"), seed, first_path, n_paths)

    def heston_barrier_paths(self, opt, model, barrier, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64",
                             kind="up-and-out"):
        return self._paths("heston_path", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "barrier", barrier, kind), seed,
                           first_path, n_paths)

    def heston_level_paths(self, opt, model, n_dates, steps_per_date, n_paths, seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        return self._paths("heston_level", precision, _as_heston_path(precision, opt, model, n_dates, steps_per_date, "asian"), seed, first_path, n_paths)

    def localvol_paths(self, opt, surface, n_steps, n_paths, right="call", seed=MC_DEFAULT_SEED, first_path=0, precision="f64"):
        h = _LocalVolHolder(precision, opt, surface, 1, n_steps, "european", right)
        return self._paths("localvol", precision, h.struct, seed, first_path, n_paths)

    def localvol_asian_paths(self, opt, surface, n_dates, steps_per_date, n_paths, right="call", seed=MC_DEFAULT_SEED, first_path=0,
                             precision="f64"):
        h = _LocalVolHolder(precision, opt, surface, n_dates, steps_per_date, "asian", right)
        return self._paths("localvol", precision, h.struct, seed, first_path, n_paths)

    def localvol_barrier_paths(self, opt, surface, barrier, n_dates, steps_per_date, n_paths, right="call", seed=MC_DEFAULT_SEED,
                               first_path=0, precision="f64", kind="up-and-out"):
        h = _LocalVolHolder(precision, opt, surface, n_dates, steps_per_date, "barrier", right, barrier, kind)
        return self._paths("localvol", precision, h.struct, seed, first_path, n_paths)

    def normals(self, seed, domain, first_unit, n_units, block=0, precision="f64"):
        npb = 4 if (precision == "f32" or self._normals_f32) else 8
        out = np.empty(n_units * npb, dtype=NP[precision])
        check(getattr(lib(), f"mc_normals_{precision}")(self._ctx, seed, domain, first_unit, n_units, block,
                                                         out.ctypes.data_as(C.POINTER(_lib.CT[precision]))))
        return out.reshape(n_units, npb)

    def words(self, seed, domain, first_unit, n_units, first_block=0, n_blocks=1):
        """The raw Philox words of blocks first_block .. first_block + n_blocks - 1 of each unit: (n_units, n_blocks, 4) uint32
        (test hook, mc_words)."""
        out = np.empty((n_units, n_blocks, 4), dtype=np.uint32)
        check(lib().mc_words(self._ctx, seed, domain, first_unit, n_units, first_block, n_blocks, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def math_probe(self, op, inputs):
        """The device's own math on caller-chosen inputs (test hook, mc_math_probe): `op` is a key of _lib.PROBE_OPS, `inputs` an
        (n, k <= 4) array of uint64 (doubles as bit patterns, 32-bit words zero-extended); item i runs on lane i mod 256.
        Returns (n, 8) uint64 in the layout include/mc_mi355x_test.h lists."""
        x = np.asarray(inputs, dtype=np.uint64)
        x = x.reshape(len(x), -1)
        n = len(x)
        buf = np.zeros((n, _lib.PROBE_IN), dtype=np.uint64)
        buf[:, :x.shape[1]] = x
        out = np.empty((n, _lib.PROBE_OUT), dtype=np.uint64)
        P = C.POINTER(C.c_uint64)
        check(lib().mc_math_probe(self._ctx, _lib.PROBE_OPS[op], buf.ctypes.data_as(P), n, out.ctypes.data_as(P)))
        return out

    # ---- compatibility mode: the reference's launch geometry and per-thread XORWOW streams (mc_*_run_grid_*) ----
    def run_grid(self, prod, inputs, num_blocks, num_threads, paths_per_block, precision="f64") -> Estimate:
        """num_blocks * paths_per_block paths drawn the reference's way (dp/MonteCarloKernel.cu:285-290: one XORWOW state per
        thread, seed blockIdx + gridDim, subsequence threadIdx; thread t prices paths t, t + T, ... of its block)."""
        struct, keep = self.prepared(prod, precision, inputs)
        r = _lib.Result()
        check(getattr(lib(), f"mc_{prod}_run_grid_{precision}")(self._ctx, C.byref(struct), num_blocks, num_threads, paths_per_block,
                                                                C.byref(r)))
        return _estimate(r)

    def set_grid_form(self, form: str):
        """Launch-geometry mode: 'auto' (fused kernels where they exist), 'staged' (normals through HBM: the checker) or
        'fused' (test hook, mc_mi355x_test.h)."""
        check(lib().mc_context_set_grid_form(self._ctx, _lib.GRID_FORM[form]))

    def paths_grid(self, prod, inputs, num_blocks, num_threads, paths_per_block, precision="f64"):
        """Per-path values of a launch-geometry call in the call's path order, (num_blocks, paths_per_block) (test hook)."""
        struct, keep = self.prepared(prod, precision, inputs)
        out = np.empty((num_blocks, paths_per_block), dtype=NP[precision])
        check(getattr(lib(), f"mc_{prod}_paths_grid_{precision}")(self._ctx, C.byref(struct), num_blocks, num_threads, paths_per_block,
                                                                  out.ctypes.data_as(C.POINTER(_lib.CT[precision]))))
        return out

    def grid_normals(self, num_blocks, num_threads, count):
        """The first `count` normals of every thread's stream: (num_blocks, num_threads, count) float32."""
        out = np.empty((num_blocks, num_threads, count), dtype=np.float32)
        check(lib().mc_grid_normals(self._ctx, num_blocks, num_threads, count, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # ---- test hooks: the simulation kernels on a caller-supplied normal stream -----------------------
    def _from_normals(self, prod, X, struct, normals, n_paths, flags, want_values):
        z = np.ascontiguousarray(normals, dtype=NP[X]).reshape(-1)
        P = C.POINTER(_lib.CT[X])
        vals = np.empty(n_paths, dtype=NP[X]) if want_values else None
        r = _lib.Result()
        f = getattr(lib(), f"mc_{prod}_from_normals_{X}")
        args = [self._ctx, C.byref(struct), z.ctypes.data_as(P), n_paths]
        if prod != "vanilla":
            args.append(flags)
        args += [vals.ctypes.data_as(P) if want_values else None, C.byref(r)]
        check(f(*args))
        return _estimate(r), vals

    def vanilla_from_normals(self, opt, normals, precision="f64", want_values=True):
        """(Estimate, per-path payoffs): the vanilla hot kernel with normals[i] as path i's normal."""
        z = np.asarray(normals).reshape(-1)
        return self._from_normals("vanilla", precision, _as_option(precision, opt), z, len(z), 0, want_values)

    def basket_from_normals(self, b, normals, precision="f64", no_vol=False, want_values=True):
        """normals[i, a]: path i, asset a, in drawing order.  no_vol: the reference dp CPU path's model (goldens only)."""
        h = _BasketHolder(precision, b)
        z = np.asarray(normals).reshape(-1, h.n)
        return self._from_normals("basket", precision, h.struct, z, z.shape[0], _lib.FROM_NORMALS_NO_VOL if no_vol else 0, want_values)

    def cva_from_normals(self, c, normals, precision="f64", host_order=False, want_values=True):
        """normals[i, j - 1]: path i, date j.  host_order: the reference CPU loop's lagged exposure (goldens only)."""
        st = _as_cva(precision, c)
        z = np.asarray(normals).reshape(-1, st.n_grid)
        return self._from_normals("cva", precision, st, z, z.shape[0], _lib.FROM_NORMALS_HOST_ORDER if host_order else 0, want_values)


# ---- host helpers (no GPU needed) -----------------------------------------------------------
def closing(sum_, sum2, n, discount=1.0):
    e, c = C.c_double(), C.c_double()
    lib().mc_closing(sum_, sum2, n, discount, C.byref(e), C.byref(c))
    return e.value, c.value


def pci_bus_id(device):
    """PCI bus id of a visible device ("0000:75:00.0"): which physical GPU an index is."""
    buf = C.create_string_buffer(32)
    check(lib().mc_device_pci_bus_id(device, buf, 32))
    return buf.value.decode()


def shard_range(total, rank, world):
    first, count = C.c_uint64(), C.c_uint64()
    lib().mc_shard_range(total, rank, world, C.byref(first), C.byref(count))
    return first.value, count.value


def basket_control_mean(b, precision="f64"):
    """Closed-form E[max(G - K, 0)] of the geometric-basket control (undiscounted, fp64)."""
    h = _BasketHolder(precision, b)
    m = C.c_double()
    check(getattr(lib(), f"mc_basket_control_mean_{precision}")(C.byref(h.struct), C.byref(m)))
    return m.value


def asian_control_mean(opt, n_dates, precision="f64"):
    """Closed-form E[max(G - K, 0)] of the Asian call's geometric-average control (undiscounted, fp64)."""
    m = C.c_double()
    check(getattr(lib(), f"mc_asian_control_mean_{precision}")(C.byref(_as_asian(precision, opt, n_dates)), C.byref(m)))
    return m.value


def barrier_closed_form(opt, barrier, kind="up-and-out", precision="f64"):
    """Discounted Reiner-Rubinstein price of the continuously monitored single-barrier call (no dividend, no rebate; fp64)."""
    p = C.c_double()
    check(getattr(lib(), f"mc_barrier_closed_form_{precision}")(C.byref(_as_barrier(precision, opt, barrier, 1, kind, "continuous")), C.byref(p)))
    return p.value


def rainbow_closed_form(basket, kind="put-on-min", barrier=None, barrier_kind=None, precision="f64"):
    """Discounted price of the worst-of / best-of option without a barrier on one asset (Black-Scholes) or two (Stulz); fp64, plain
    C, no GPU.  Refuses more assets and a barrier."""
    p = C.c_double()
    h = _RainbowHolder(precision, basket, 1, kind, barrier, barrier_kind)
    check(getattr(lib(), f"mc_rainbow_closed_form_{precision}")(C.byref(h.struct), C.byref(p)))
    return p.value


def lookback_closed_form(opt, kind="floating-call", precision="f64"):
    """Discounted price at inception of the continuously monitored lookback option (Goldman-Sosin-Gatto for the floating strikes,
    Conze-Viswanathan for the fixed ones; no dividend; fp64)."""
    p = C.c_double()
    check(getattr(lib(), f"mc_lookback_closed_form_{precision}")(C.byref(_as_lookback(precision, opt, 1, kind, "continuous")), C.byref(p)))
    return p.value


def merton_closed_form(opt, jumps, precision="f64"):
    """Discounted exact price of the European call under Merton's jump-diffusion (Merton's series of Black-Scholes prices; fp64)."""
    p = C.c_double()
    check(getattr(lib(), f"mc_merton_closed_form_{precision}")(C.byref(_as_merton(precision, opt, jumps, 1, "european")), C.byref(p)))
    return p.value


def merton_thresholds(opt, jumps, n_dates, precision="f64"):
    """The integer thresholds T_0 <= ... <= T_{K-1} of the Poisson(lambda t / n_dates) count drawn from a 32-bit (f32) or 64-bit
    (f64) word: N = #{k : word >= T_k} (mc_merton_thresholds_*).  A uint64 array of length K."""
    out = np.zeros(_lib.MAX_MERTON_JUMPS, dtype=np.uint64)
    n = C.c_int()
    check(getattr(lib(), f"mc_merton_thresholds_{precision}")(C.byref(_as_merton(precision, opt, jumps, n_dates, "european")),
                                                               out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
    return out[:n.value].copy()


def american_solve(sums, degree=3):
    """One date's regression of a Longstaff-Schwartz fit (mc_american_solve): sums = [sum p^k, k = 0..6; sum p^k V, k = 0..3]
    over the paths in the money; the four coefficients of the continuation value, or [inf, 0, 0, 0] ("never exercise")."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.shape != (_lib.AMERICAN_SUMS,):
        raise ValueError(f"sums has shape {sums.shape}, expected ({_lib.AMERICAN_SUMS},)")
    beta = np.empty(4, dtype=np.float64)
    check(lib().mc_american_solve(sums.ctypes.data_as(C.POINTER(C.c_double)), int(degree), beta.ctypes.data_as(C.POINTER(C.c_double))))
    return beta


def american_lattice(opt, n_dates, steps_per_date, kind="put", precision="f64"):
    """Discounted Cox-Ross-Rubinstein price of the Bermudan put or call with exercise on the n_dates dates only, on
    n_dates * steps_per_date steps (mc_american_lattice_*; fp64, no GPU)."""
    p = C.c_double()
    check(getattr(lib(), f"mc_american_lattice_{precision}")(C.byref(_as_american(precision, opt, n_dates, kind, 3)), int(steps_per_date), C.byref(p)))
    return p.value


def mlmc_plan(var, cost, eps):
    """Path counts per level for a variance of eps^2 / 2 at least cost (mc_mlmc_plan; host only):
    n_l = ceil(2 eps^-2 sqrt(V_l / C_l) sum_k sqrt(V_k C_k))."""
    var, cost = np.ascontiguousarray(var, dtype=np.float64), np.ascontiguousarray(cost, dtype=np.float64)
    if var.ndim != 1 or var.shape != cost.shape:
        raise ValueError(f"var and cost have shapes {var.shape} and {cost.shape}, expected two vectors of one length")
    n = np.zeros(var.size, dtype=np.uint64)
    DP = C.POINTER(C.c_double)
    check(lib().mc_mlmc_plan(int(var.size), var.ctypes.data_as(DP), cost.ctypes.data_as(DP), float(eps), n.ctypes.data_as(C.POINTER(C.c_uint64))))
    return [int(x) for x in n]


def heston_closed_form(opt, model, precision="f64"):
    """Discounted exact price of the European call under the continuous Heston model (no dividend; fp64 quadrature)."""
    p = C.c_double()
    check(getattr(lib(), f"mc_heston_closed_form_{precision}")(C.byref(_as_heston(precision, opt, model, 1)), C.byref(p)))
    return p.value


def localvol_sigma(surface, n_steps, step, y, precision="f64"):
    """The volatility the engine reads at step `step` (1-based) of n_steps and log-spot y = ln(S / s) on the surface {sigma, y_lo,
    y_hi}: the interpolant of mc_localvol_run_* in fp64, from the table as rounded for `precision` (mc_localvol_sigma_*; no GPU)."""
    h = _LocalVolHolder(precision, dict(s=1.0, k=1.0, r=0.0, t=1.0), surface, 1, n_steps, "european")
    p = C.c_double()
    check(getattr(lib(), f"mc_localvol_sigma_{precision}")(C.byref(h.struct), int(step), float(y), C.byref(p)))
    return p.value


def chol(c, precision="f64"):
    """Cholesky with the reference's semantics (MonteCarloHost.c:90-105).  Returns (factor, bad_pivots)."""
    c = np.ascontiguousarray(c, dtype=NP[precision])
    n = c.shape[0]
    a = np.zeros_like(c)
    P = C.POINTER(_lib.CT[precision])
    bad = getattr(lib(), f"mc_chol_{precision}")(n, c.ctypes.data_as(P), a.ctypes.data_as(P))
    return a, bad


def factor_from_cov(cov, precision="f64"):
    """Volatilities and Cholesky factor of the correlation matrix from a covariance matrix (mc_factor_from_cov_*).
    Returns (v, factor, bad_pivots); raises ValueError for a non-positive or non-finite diagonal."""
    cov = np.ascontiguousarray(cov, dtype=NP[precision])
    n = cov.shape[0]
    v = np.zeros(n, dtype=NP[precision])
    p = np.zeros((n, n), dtype=NP[precision])
    P = C.POINTER(_lib.CT[precision])
    bad = getattr(lib(), f"mc_factor_from_cov_{precision}")(n, cov.ctypes.data_as(P), v.ctypes.data_as(P), p.ctypes.data_as(P))
    if bad < 0:
        raise ValueError("covariance matrix needs a finite, positive diagonal and finite entries")
    return v, p, bad


# ---- the reference's three entry points ------------------------------------------------------
_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


def _path_count(numBlocks, sims):
    if numBlocks <= 0 or sims // numBlocks <= 0:
        raise ValueError("numBlocks / sims give no paths")
    return numBlocks * (sims // numBlocks)   # MonteCarloKernel.cu:491,508,524 with :413


def _dev(prod, inputs, numBlocks, numThreads, sims, precision) -> OptionValue:
    n = _path_count(numBlocks, sims)
    if os.environ.get("MC_RNG") == "xorwow_grid":   # as the legacy symbols: the reference's launch geometry shapes the sample
        return default_engine().run_grid(prod, inputs, numBlocks, numThreads, n // numBlocks, precision).value()
    return getattr(default_engine(), prod)(inputs, n, precision=precision).value()


def dev_vanillaOpt(opt, numBlocks, numThreads, sims, precision="f64") -> OptionValue:
    return _dev("vanilla", opt, numBlocks, numThreads, sims, precision)


def dev_basketOpt(option, numBlocks, numThreads, sims, precision="f64") -> OptionValue:
    return _dev("basket", option, numBlocks, numThreads, sims, precision)


def dev_cvaEquityOption(cva, numBlocks, numThreads, sims, precision="f64") -> OptionValue:
    return _dev("cva", cva, numBlocks, numThreads, sims, precision)
