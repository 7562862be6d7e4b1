"""ctypes declarations for libmc_mi355x.so (include/mc_mi355x.h, and the test hooks of include/mc_mi355x_test.h).

Loading is strict: if the shared library is missing the import of this module raises -- there
is no Python or CPU fallback for the simulation path.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(CSRC, "libmc_mi355x.so")
LEGACY = {"f64": os.path.join(CSRC, "libmcgpu_f64.so"), "f32": os.path.join(CSRC, "libmcgpu_f32.so")}

MC_OK = 0
MC_DEFAULT_SEED = 0x4D435F4D49333535
DOMAIN_VANILLA, DOMAIN_BASKET, DOMAIN_CVA, DOMAIN_ASIAN, DOMAIN_BARRIER, DOMAIN_HESTON = 1, 2, 3, 4, 5, 6
DOMAIN_LOOKBACK, DOMAIN_LOOKBACK_BRIDGE = 8, 9   # normals; the continuous form's bridge uniforms (raw Philox blocks)
MAX_ASIAN_DATES = 4096   # MC_MAX_ASIAN_DATES
MAX_BARRIER_DATES = 4096   # MC_MAX_BARRIER_DATES
MAX_HESTON_STEPS = 4096   # MC_MAX_HESTON_STEPS
MAX_LOOKBACK_DATES = 4096   # MC_MAX_LOOKBACK_DATES
DOMAIN_MERTON, DOMAIN_MERTON_JUMPS = 10, 11   # normals; the Poisson counts (raw Philox blocks)
MAX_MERTON_DATES = 4096   # MC_MAX_MERTON_DATES
MAX_MERTON_JUMPS = 40   # MC_MAX_MERTON_JUMPS
MERTON_PAYOFFS = {"european": 0, "asian": 1, "barrier": 2}   # MC_MERTON_EUROPEAN, MC_MERTON_ASIAN, MC_MERTON_BARRIER
DOMAIN_AMERICAN, DOMAIN_AMERICAN_FIT = 12, 13   # the pricing pass of the Bermudan options; the fit of their rule
MAX_AMERICAN_DATES = 512   # MC_MAX_AMERICAN_DATES
AMERICAN_MIN_ITM = 32   # MC_AMERICAN_MIN_ITM
AMERICAN_SUMS = 11   # MC_AMERICAN_SUMS
AMERICAN_TYPES = {"put": 0, "call": 1}   # MC_AMERICAN_PUT, MC_AMERICAN_CALL
DOMAIN_RAINBOW = 14   # the worst-of / best-of options: flat (date, factor) entries of the Asian layout
MAX_RAINBOW_ASSETS = 8   # MC_MAX_RAINBOW_ASSETS
MAX_RAINBOW_TABLE = 4096   # MC_MAX_RAINBOW_TABLE: n * n_dates at most
RAINBOW_TYPES = {"call-on-min": 0, "call-on-max": 1, "put-on-min": 2, "put-on-max": 3}   # MC_RAINBOW_CALL_ON_MIN ... MC_RAINBOW_PUT_ON_MAX
RAINBOW_NO_BARRIER = -1   # MC_RAINBOW_NO_BARRIER
DOMAIN_AUTOCALL = 15   # the worst-of autocallable notes: the rainbow's flat layout
MAX_AUTOCALL_TABLE = 4096   # MC_MAX_AUTOCALL_TABLE: n * n_dates + 3 * n_obs at most
AUTOCALL_KI = {None: -1, "dates": 0, "maturity": 1}   # MC_AUTOCALL_KI_NONE, MC_AUTOCALL_KI_DATES, MC_AUTOCALL_KI_MATURITY
BARRIER_TYPES = {"up-and-out": 0, "up-and-in": 1, "down-and-out": 2, "down-and-in": 3}   # MC_BARRIER_UP_OUT ... MC_BARRIER_DOWN_IN
LOOKBACK_TYPES = {"floating-call": 0, "floating-put": 1, "fixed-call": 2, "fixed-put": 3}   # MC_LOOKBACK_FLOAT_CALL ... MC_LOOKBACK_FIXED_PUT
MONITORING = {"discrete": 0, "continuous": 1}   # MC_MONITOR_DISCRETE, MC_MONITOR_CONTINUOUS
MAX_ASSETS = 16          # register-resident basket kernels
MAX_ASSETS_GENERIC = 64  # LDS-staged generic kernel beyond that
NPB = {"f32": 4, "f64": 8}   # normals per block of the stream (include/mc_mi355x.h: MC_STREAM_VERSION 2)
FROM_NORMALS_NO_VOL, FROM_NORMALS_HOST_ORDER = 1, 2   # flags of the mc_*_from_normals_* test hooks
CT = {"f32": C.c_float, "f64": C.c_double}


def build(verbose: bool = False) -> None:
    """Compile every HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "all"], stdout=out)


class OptionF32(C.Structure):
    _fields_ = [("s", C.c_float), ("k", C.c_float), ("r", C.c_float), ("v", C.c_float), ("t", C.c_float)]


class OptionF64(C.Structure):
    _fields_ = [("s", C.c_double), ("k", C.c_double), ("r", C.c_double), ("v", C.c_double), ("t", C.c_double)]


def _basket(R):
    P = C.POINTER(R)

    class Basket(C.Structure):
        _fields_ = [("n", C.c_int), ("s", P), ("v", P), ("p", P), ("d", P), ("w", P), ("k", R), ("t", R), ("r", R)]
    return Basket


BasketF32, BasketF64 = _basket(C.c_float), _basket(C.c_double)


class CvaF32(C.Structure):
    _fields_ = [("defint", C.c_float), ("lgd", C.c_float), ("option", OptionF32), ("n_grid", C.c_int)]


class CvaF64(C.Structure):
    _fields_ = [("defint", C.c_double), ("lgd", C.c_double), ("option", OptionF64), ("n_grid", C.c_int)]


class AsianF32(C.Structure):   # mc_asian_f32
    _fields_ = [("option", OptionF32), ("n_dates", C.c_int)]


class AsianF64(C.Structure):   # mc_asian_f64
    _fields_ = [("option", OptionF64), ("n_dates", C.c_int)]


class BarrierF32(C.Structure):   # mc_barrier_f32
    _fields_ = [("option", OptionF32), ("barrier", C.c_float), ("n_dates", C.c_int), ("type", C.c_int), ("monitoring", C.c_int)]


class BarrierF64(C.Structure):   # mc_barrier_f64
    _fields_ = [("option", OptionF64), ("barrier", C.c_double), ("n_dates", C.c_int), ("type", C.c_int), ("monitoring", C.c_int)]


class LookbackF32(C.Structure):   # mc_lookback_f32
    _fields_ = [("option", OptionF32), ("n_dates", C.c_int), ("type", C.c_int), ("monitoring", C.c_int)]


class LookbackF64(C.Structure):   # mc_lookback_f64
    _fields_ = [("option", OptionF64), ("n_dates", C.c_int), ("type", C.c_int), ("monitoring", C.c_int)]


class MertonF32(C.Structure):   # mc_merton_f32
    _fields_ = [("option", OptionF32), ("lambda_", C.c_float), ("mu_j", C.c_float), ("delta", C.c_float), ("n_dates", C.c_int), ("payoff", C.c_int),
                ("barrier_type", C.c_int), ("barrier", C.c_float)]


class MertonF64(C.Structure):   # mc_merton_f64
    _fields_ = [("option", OptionF64), ("lambda_", C.c_double), ("mu_j", C.c_double), ("delta", C.c_double), ("n_dates", C.c_int), ("payoff", C.c_int),
                ("barrier_type", C.c_int), ("barrier", C.c_double)]


class AmericanF32(C.Structure):   # mc_american_f32
    _fields_ = [("option", OptionF32), ("n_dates", C.c_int), ("type", C.c_int), ("degree", C.c_int)]


class AmericanF64(C.Structure):   # mc_american_f64
    _fields_ = [("option", OptionF64), ("n_dates", C.c_int), ("type", C.c_int), ("degree", C.c_int)]


class HestonF32(C.Structure):   # mc_heston_f32
    _fields_ = [("option", OptionF32), ("v0", C.c_float), ("kappa", C.c_float), ("theta", C.c_float), ("xi", C.c_float), ("rho", C.c_float),
                ("n_steps", C.c_int)]


class HestonF64(C.Structure):   # mc_heston_f64
    _fields_ = [("option", OptionF64), ("v0", C.c_double), ("kappa", C.c_double), ("theta", C.c_double), ("xi", C.c_double), ("rho", C.c_double),
                ("n_steps", C.c_int)]


class HestonPathF32(C.Structure):   # mc_heston_path_f32
    _fields_ = [("heston", HestonF32), ("steps_per_date", C.c_int), ("payoff", C.c_int), ("barrier_type", C.c_int), ("barrier", C.c_float)]


class HestonPathF64(C.Structure):   # mc_heston_path_f64
    _fields_ = [("heston", HestonF64), ("steps_per_date", C.c_int), ("payoff", C.c_int), ("barrier_type", C.c_int), ("barrier", C.c_double)]


def _localvol(O, R):
    class LocalVol(C.Structure):   # mc_localvol_f32 / mc_localvol_f64
        _fields_ = [("option", O), ("sigma", C.POINTER(R)), ("n_times", C.c_int), ("n_nodes", C.c_int), ("y_lo", R), ("y_hi", R),
                    ("n_steps", C.c_int), ("steps_per_date", C.c_int), ("payoff", C.c_int), ("right", C.c_int), ("barrier_type", C.c_int),
                    ("barrier", R)]
    return LocalVol


LocalVolF32, LocalVolF64 = _localvol(OptionF32, C.c_float), _localvol(OptionF64, C.c_double)


class RainbowF32(C.Structure):   # mc_rainbow_f32
    _fields_ = [("basket", BasketF32), ("barrier", C.c_float), ("n_dates", C.c_int), ("type", C.c_int), ("barrier_type", C.c_int)]


class RainbowF64(C.Structure):   # mc_rainbow_f64
    _fields_ = [("basket", BasketF64), ("barrier", C.c_double), ("n_dates", C.c_int), ("type", C.c_int), ("barrier_type", C.c_int)]


def _autocall(B, R):
    P = C.POINTER(R)

    class Autocall(C.Structure):   # mc_autocall_f32 / mc_autocall_f64
        _fields_ = [("basket", B), ("autocall", P), ("coupon_barrier", P), ("coupon", R), ("barrier", R), ("gearing", R),
                    ("n_dates", C.c_int), ("n_obs", C.c_int), ("memory", C.c_int), ("ki_monitoring", C.c_int)]
    return Autocall


AutocallF32, AutocallF64 = _autocall(BasketF32, C.c_float), _autocall(BasketF64, C.c_double)


class Result(C.Structure):
    _fields_ = [("expected", C.c_double), ("confidence", C.c_double), ("sum", C.c_double), ("sum2", C.c_double),
                ("n", C.c_uint64), ("kernel_ms", C.c_float), ("wall_ms", C.c_float)]


class CallStats(C.Structure):   # mc_call_stats: where the last synchronous call's time went
    _fields_ = [(k, C.c_float) for k in ("setup_ms", "table_upload_ms", "launch_ms", "kernel_ms", "readback_ms", "closing_ms", "wall_ms",
                                         "context_create_ms")] + [("first_call", C.c_int)]


class Greeks(C.Structure):
    _fields_ = [("price", Result), ("delta", Result), ("vega", Result)]


class Greeks2(C.Structure):
    _fields_ = [("price", Result), ("delta", Result), ("vega", Result), ("gamma", Result), ("vanna", Result)]


class CvaGreeks(C.Structure):
    _fields_ = [("cva", Result), ("delta", Result), ("vega", Result)]


class BookEntryF32(C.Structure):   # mc_book_entry_f32
    _fields_ = [("option", OptionF32), ("seed", C.c_uint64), ("first_path", C.c_uint64), ("n_paths", C.c_uint64)]


class BookEntryF64(C.Structure):   # mc_book_entry_f64
    _fields_ = [("option", OptionF64), ("seed", C.c_uint64), ("first_path", C.c_uint64), ("n_paths", C.c_uint64)]


OPTION = {"f32": OptionF32, "f64": OptionF64}
BOOK_ENTRY = {"f32": BookEntryF32, "f64": BookEntryF64}
MAX_BOOK = 1 << 20   # MC_MAX_BOOK
BASKET = {"f32": BasketF32, "f64": BasketF64}
CVA = {"f32": CvaF32, "f64": CvaF64}
ASIAN = {"f32": AsianF32, "f64": AsianF64}
BARRIER = {"f32": BarrierF32, "f64": BarrierF64}
LOOKBACK = {"f32": LookbackF32, "f64": LookbackF64}
HESTON = {"f32": HestonF32, "f64": HestonF64}
MERTON = {"f32": MertonF32, "f64": MertonF64}
AMERICAN = {"f32": AmericanF32, "f64": AmericanF64}
HESTON_PATH = {"f32": HestonPathF32, "f64": HestonPathF64}
RAINBOW = {"f32": RainbowF32, "f64": RainbowF64}
AUTOCALL = {"f32": AutocallF32, "f64": AutocallF64}
HESTON_PATH_PAYOFFS = {"asian": 0, "barrier": 1}   # MC_HESTON_PATH_ASIAN, MC_HESTON_PATH_BARRIER
LOCALVOL = {"f32": LocalVolF32, "f64": LocalVolF64}
LOCALVOL_PAYOFFS = {"european": 0, "asian": 1, "barrier": 2}   # MC_LOCALVOL_EUROPEAN, MC_LOCALVOL_ASIAN, MC_LOCALVOL_BARRIER
LOCALVOL_RIGHTS = {"call": 0, "put": 1}                        # MC_LOCALVOL_CALL, MC_LOCALVOL_PUT
MAX_LOCALVOL_STEPS, MAX_LOCALVOL_NODES = 4096, 2048            # MC_MAX_LOCALVOL_STEPS, MC_MAX_LOCALVOL_NODES
DOMAIN_LOCALVOL = 16                                           # MC_DOMAIN_LOCALVOL
DOMAIN_HESTON_LEVEL = 17                                       # MC_DOMAIN_HESTON_LEVEL
MLMC_MAX_LEVELS = 12                                           # MC_MLMC_MAX_LEVELS: the finest level's index
MLMC_LEVEL_STRIDE, MLMC_MAX_PATHS = 1 << 40, 1 << 34           # level l >= 1 owns paths [l 2^40, l 2^40 + n_l), n_l <= 2^34


class MlmcSpec(C.Structure):   # mc_mlmc_spec
    _fields_ = [("eps", C.c_double), ("min_levels", C.c_int), ("max_levels", C.c_int), ("n_pilot", C.c_uint64)]


class MlmcLevel(C.Structure):   # mc_mlmc_level
    _fields_ = [("result", Result), ("n_paths", C.c_uint64), ("first_path", C.c_uint64)]


class MlmcResult(C.Structure):   # mc_mlmc_result
    _fields_ = [("price", C.c_double), ("stderr_", C.c_double), ("bias", C.c_double), ("converged", C.c_int), ("levels", C.c_int),
                ("level", MlmcLevel * (MLMC_MAX_LEVELS + 1))]


# every product has the entry points mc_<product>_launch_*, _run_* and _paths_* over its input struct; the Bermudan ones also take
# the exercise rule, a const double *, behind the struct
PRODUCTS = {"vanilla": OPTION, "basket": BASKET, "cva": CVA, "asian": ASIAN, "barrier": BARRIER, "lookback": LOOKBACK, "rainbow": RAINBOW,
            "autocall": AUTOCALL, "merton": MERTON, "american": AMERICAN, "heston": HESTON, "heston_path": HESTON_PATH,
            "localvol": LOCALVOL, "heston_level": HESTON_PATH}   # a level takes the struct of its fine walk

# every symbol include/mc_mi355x.h declares (the drop-in surface), then the test hooks of include/mc_mi355x_test.h;
# tests/test_abi.py checks that the .so exports each of them and that each is declared in exactly one of the two headers
EXPORTS = ["mc_last_error", "mc_device_count", "mc_device_pci_bus_id", "mc_context_create", "mc_context_destroy", "mc_context_device",
           "mc_context_blocks", "mc_context_stream", "mc_context_info", "mc_context_last_launch", "mc_context_last_call_stats", "mc_context_describe", "mc_context_profile", "mc_context_profile_read",
           "mc_context_set_antithetic", "mc_context_set_control_variate", "mc_context_set_finish", "mc_context_set_timing",
           "mc_context_order", "mc_context_idle", "mc_context_arm_direct", "mc_context_publish", "mc_context_set_generator",
           "mc_context_set_normals", "mc_context_set_cva_date_lanes", "mc_basket_control_mean_f32", "mc_basket_control_mean_f64", "mc_closing", "mc_shard_range",
           "mc_chol_f32", "mc_chol_f64", "mc_factor_from_cov_f32", "mc_factor_from_cov_f64"]
EXPORTS.append("mc_american_solve")
EXPORTS.append("mc_mlmc_plan")
TEST_EXPORTS = ["mc_xorwow_words", "mc_words", "mc_grid_normals", "mc_context_set_grid_form", "mc_math_probe"]
# mc_math_probe (include/mc_mi355x_test.h): operations, and 64-bit words per item in and out
PROBE_OPS = {"neg2log": 0, "sincos": 1, "exp": 2, "sqrt": 3, "recip": 4, "u01": 5, "pair": 6, "f32_block": 7}
PROBE_IN, PROBE_OUT, PROBE_MAX = 4, 8, 1 << 20
for _x in ("f32", "f64"):
    for _p in PRODUCTS:
        EXPORTS += [f"mc_{_p}_launch_{_x}", f"mc_{_p}_run_{_x}", f"mc_{_p}_paths_{_x}"]
    EXPORTS += [f"mc_{_p}_run_grid_{_x}" for _p in ("vanilla", "basket", "cva")]       # the reference's launch geometry
    EXPORTS += [f"mc_vanilla_greeks_run_{_x}", f"mc_vanilla_greeks_lr_run_{_x}", f"mc_basket_greeks_run_{_x}", f"mc_cva_greeks_run_{_x}",
                f"mc_basket_greeks_lr_run_{_x}", f"mc_cva_greeks_lr_run_{_x}"]
    EXPORTS += [f"mc_vanilla_greeks2_run_{_x}", f"mc_basket_gamma_run_{_x}"]
    EXPORTS += [f"mc_vanilla_book_run_{_x}", f"mc_vanilla_book_launch_{_x}"]
    EXPORTS += [f"mc_asian_control_mean_{_x}", f"mc_barrier_closed_form_{_x}", f"mc_lookback_closed_form_{_x}", f"mc_rainbow_closed_form_{_x}"]
    EXPORTS += [f"mc_merton_closed_form_{_x}", f"mc_merton_thresholds_{_x}", f"mc_american_lattice_{_x}", f"mc_american_fit_{_x}"]
    EXPORTS.append(f"mc_heston_closed_form_{_x}")
    EXPORTS.append(f"mc_localvol_sigma_{_x}")
    EXPORTS.append(f"mc_heston_mlmc_run_{_x}")
    TEST_EXPORTS.append(f"mc_american_fit_date_{_x}")
    TEST_EXPORTS.append(f"mc_normals_{_x}")
    TEST_EXPORTS += [f"mc_{_p}_from_normals_{_x}" for _p in ("vanilla", "basket", "cva")]
    TEST_EXPORTS += [f"mc_{_p}_paths_grid_{_x}" for _p in ("vanilla", "basket", "cva")]
GRID_FORM = {"auto": 0, "staged": 1, "fused": 2}


def _declare(L: C.CDLL) -> C.CDLL:
    ctx = C.c_void_p
    u64 = C.c_uint64
    L.mc_last_error.restype = C.c_char_p
    L.mc_last_error.argtypes = []
    L.mc_device_count.restype = C.c_int
    L.mc_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.mc_context_create.argtypes = [C.c_int, C.c_int, C.POINTER(ctx)]
    L.mc_context_destroy.argtypes = [ctx]
    L.mc_context_destroy.restype = None
    L.mc_context_device.argtypes = [ctx]
    L.mc_context_blocks.argtypes = [ctx]
    L.mc_context_stream.argtypes = [ctx]
    L.mc_context_stream.restype = C.c_void_p
    L.mc_context_info.argtypes = [ctx, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mc_context_last_launch.argtypes = [ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mc_context_last_call_stats.argtypes = [ctx, C.POINTER(CallStats)]
    L.mc_context_describe.argtypes = [ctx, C.c_char_p, C.c_int]
    L.mc_context_set_antithetic.argtypes = [ctx, C.c_int]
    L.mc_context_set_control_variate.argtypes = [ctx, C.c_int]
    L.mc_context_set_finish.argtypes = [ctx, C.c_int]
    L.mc_context_set_timing.argtypes = [ctx, C.c_int]
    L.mc_context_order.argtypes = [ctx, C.c_void_p]
    L.mc_context_idle.argtypes = [ctx]
    L.mc_context_arm_direct.argtypes = [ctx, C.POINTER(C.POINTER(C.c_double))]
    L.mc_context_publish.argtypes = [ctx, C.c_void_p, C.c_void_p, C.POINTER(C.POINTER(C.c_double))]
    L.mc_context_set_generator.argtypes = [ctx, C.c_int, C.c_uint64]
    L.mc_context_set_normals.argtypes = [ctx, C.c_int]
    L.mc_context_set_cva_date_lanes.argtypes = [ctx, C.c_int]
    L.mc_grid_normals.argtypes = [ctx, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_float)]
    L.mc_context_set_grid_form.argtypes = [ctx, C.c_int]
    L.mc_words.argtypes = [ctx, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.mc_xorwow_words.argtypes = [ctx, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.mc_math_probe.argtypes = [ctx, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64)]
    L.mc_american_solve.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    L.mc_mlmc_plan.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(u64)]
    for X in ("f32", "f64"):
        getattr(L, f"mc_basket_control_mean_{X}").argtypes = [C.POINTER(BASKET[X]), C.POINTER(C.c_double)]
    L.mc_context_profile.argtypes = [ctx, C.c_int]
    L.mc_context_profile_read.argtypes = [ctx, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.mc_closing.argtypes = [C.c_double, C.c_double, u64, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mc_closing.restype = None
    L.mc_shard_range.argtypes = [u64, C.c_int, C.c_int, C.POINTER(u64), C.POINTER(u64)]
    L.mc_shard_range.restype = None
    for X in ("f32", "f64"):
        R = CT[X]
        RP = C.POINTER(R)
        getattr(L, f"mc_chol_{X}").argtypes = [C.c_int, RP, RP]
        getattr(L, f"mc_factor_from_cov_{X}").argtypes = [C.c_int, RP, RP, RP]
        DP = C.POINTER(C.c_double)
        for prod, S in PRODUCTS.items():
            head = [ctx, C.POINTER(S[X])] + ([DP] if prod == "american" else [])
            getattr(L, f"mc_{prod}_launch_{X}").argtypes = head + [u64, u64, u64, C.c_void_p, C.c_void_p]
            getattr(L, f"mc_{prod}_run_{X}").argtypes = head + [u64, u64, u64, C.POINTER(Result)]
            getattr(L, f"mc_{prod}_paths_{X}").argtypes = head + [u64, u64, u64, RP]
        for prod, S in (("vanilla", OPTION[X]), ("basket", BASKET[X]), ("cva", CVA[X])):
            getattr(L, f"mc_{prod}_run_grid_{X}").argtypes = [ctx, C.POINTER(S), C.c_int, C.c_int, u64, C.POINTER(Result)]
            getattr(L, f"mc_{prod}_paths_grid_{X}").argtypes = [ctx, C.POINTER(S), C.c_int, C.c_int, u64, RP]
        getattr(L, f"mc_normals_{X}").argtypes = [ctx, u64, C.c_uint32, u64, u64, C.c_uint32, RP]
        getattr(L, f"mc_vanilla_from_normals_{X}").argtypes = [ctx, C.POINTER(OPTION[X]), RP, u64, RP, C.POINTER(Result)]
        getattr(L, f"mc_basket_from_normals_{X}").argtypes = [ctx, C.POINTER(BASKET[X]), RP, u64, C.c_int, RP, C.POINTER(Result)]
        getattr(L, f"mc_cva_from_normals_{X}").argtypes = [ctx, C.POINTER(CVA[X]), RP, u64, C.c_int, RP, C.POINTER(Result)]
        getattr(L, f"mc_vanilla_greeks_run_{X}").argtypes = [ctx, C.POINTER(OPTION[X]), u64, u64, u64, C.POINTER(Greeks)]
        getattr(L, f"mc_vanilla_greeks_lr_run_{X}").argtypes = [ctx, C.POINTER(OPTION[X]), u64, u64, u64, C.POINTER(Greeks)]
        getattr(L, f"mc_basket_greeks_run_{X}").argtypes = [ctx, C.POINTER(BASKET[X]), u64, u64, u64, C.POINTER(Result), C.POINTER(Result),
                                                            C.POINTER(Result)]
        getattr(L, f"mc_cva_greeks_run_{X}").argtypes = [ctx, C.POINTER(CVA[X]), u64, u64, u64, C.POINTER(CvaGreeks)]
        getattr(L, f"mc_basket_greeks_lr_run_{X}").argtypes = [ctx, C.POINTER(BASKET[X]), u64, u64, u64, C.POINTER(Result), C.POINTER(Result),
                                                               C.POINTER(Result)]
        getattr(L, f"mc_cva_greeks_lr_run_{X}").argtypes = [ctx, C.POINTER(CVA[X]), u64, u64, u64, C.POINTER(CvaGreeks)]
        getattr(L, f"mc_vanilla_greeks2_run_{X}").argtypes = [ctx, C.POINTER(OPTION[X]), u64, u64, u64, C.POINTER(Greeks2)]
        getattr(L, f"mc_vanilla_book_run_{X}").argtypes = [ctx, C.POINTER(BOOK_ENTRY[X]), C.c_int, C.POINTER(Result)]
        getattr(L, f"mc_vanilla_book_launch_{X}").argtypes = [ctx, C.POINTER(BOOK_ENTRY[X]), C.c_int, C.c_void_p, C.c_void_p]
        getattr(L, f"mc_asian_control_mean_{X}").argtypes = [C.POINTER(ASIAN[X]), DP]
        getattr(L, f"mc_barrier_closed_form_{X}").argtypes = [C.POINTER(BARRIER[X]), DP]
        getattr(L, f"mc_lookback_closed_form_{X}").argtypes = [C.POINTER(LOOKBACK[X]), DP]
        getattr(L, f"mc_rainbow_closed_form_{X}").argtypes = [C.POINTER(RAINBOW[X]), DP]
        getattr(L, f"mc_merton_closed_form_{X}").argtypes = [C.POINTER(MERTON[X]), DP]
        getattr(L, f"mc_merton_thresholds_{X}").argtypes = [C.POINTER(MERTON[X]), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        getattr(L, f"mc_american_lattice_{X}").argtypes = [C.POINTER(AMERICAN[X]), C.c_int, DP]
        getattr(L, f"mc_american_fit_{X}").argtypes = [ctx, C.POINTER(AMERICAN[X]), u64, u64, u64, DP, C.POINTER(Result)]
        getattr(L, f"mc_american_fit_date_{X}").argtypes = [ctx, C.POINTER(AMERICAN[X]), C.c_int, DP, u64, u64, u64, RP, RP, DP]
        getattr(L, f"mc_heston_closed_form_{X}").argtypes = [C.POINTER(HESTON[X]), DP]
        getattr(L, f"mc_localvol_sigma_{X}").argtypes = [C.POINTER(LOCALVOL[X]), C.c_int, C.c_double, DP]
        getattr(L, f"mc_heston_mlmc_run_{X}").argtypes = [ctx, C.POINTER(HESTON_PATH[X]), C.POINTER(MlmcSpec), u64, C.POINTER(MlmcResult)]
        getattr(L, f"mc_basket_gamma_run_{X}").argtypes = [ctx, C.POINTER(BASKET[X]), u64, u64, u64, C.POINTER(Result), C.POINTER(Result)]
    return L


_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP engine has no fallback)")
        _LIB = _declare(C.CDLL(LIB_PATH))
    return _LIB


class McError(RuntimeError):
    pass


def check(rc: int) -> None:
    if rc != MC_OK:
        raise McError(f"mc error {rc}: {lib().mc_last_error().decode()}")
