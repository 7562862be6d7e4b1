/*
 * mc_mi355x.h -- C ABI of libmc_mi355x.so, the MI355X (gfx950) Monte Carlo engine.
 *
 * Plain C: pointers, sizes and PODs only.  This is the boundary a maintainer of the reference
 * (marcomatteo/MonteCarloCUDA) binds to in place of MonteCarloKernel.cu; INTEGRATION.md shows
 * the binding.  Each entry point cites the reference interface it replaces ("dp/" =
 * double_precision/, the single_precision/ twin is the same code with float).
 *
 * Shape of the API
 *   - an opaque context per GPU owns every device buffer (the reference re-allocates and
 *     re-seeds on every call: dp/MonteCarloKernel.cu:296-342,344-363 -- that fixed cost is
 *     what a persistent context removes);
 *   - *_launch_* enqueue the simulation of the path range [first_path, first_path+n_paths) on
 *     a caller-supplied HIP stream and leave {sum, sum2, n} (three doubles) in device memory:
 *     the 24-byte payload of the multi-GPU all-reduce.  No host synchronisation;
 *   - *_run_* are the synchronous forms: launch, wait, close the estimator on the host;
 *   - *_paths_* return per-path values for a (small) path range: used by the parity tests.
 * Sizes: first_path and n_paths are 64-bit; ONE call covers at most 8 segments of 2^31 units (a unit = 4 / 8 vanilla paths in
 * f32 / f64, one basket or CVA path), none crossing a multiple of 2^32 units: up to 6.9e10 / 1.4e11 vanilla paths and
 * 1.7e10 basket or CVA paths per call (MC_ERR_INVALID beyond: "split it").  Larger jobs are several calls on consecutive
 * ranges; their triples add (mc_closing takes the sums).
 * One launch per call: the last workgroup to arrive adds the per-workgroup (sum, sum2) pairs and writes the triple.
 * Contract of a context: it owns one pair buffer, one ticket block and one constant table, so its calls execute one
 * after the other; calls on one stream are ordered by the stream, a call on a DIFFERENT stream than the context's
 * previous call is ordered behind it by the library (event + wait).  For overlap use one context per stream.  A context
 * is not thread-safe: one host thread per context.  Several GPUs from one process: include/mc_multi.h.
 *
 * Random numbers: Philox4x32-10, key = 64-bit seed, counter = {unit_hi, unit_lo, block,
 * domain} (unit = 64-bit index of a path or of a block of vanilla paths: 4 in f32, 8 in f64).  A path's normals depend only on
 * (seed, global path index), never on the launch geometry or on how a range is split over GPUs.  Layout per product:
 * DESIGN.md "RNG".  XORWOW, the reference's generator, is selectable: mc_context_set_generator.
 *
 * Precision suffix: _f32 simulates in float (sums are still accumulated in double),
 * _f64 simulates in double.  Struct layouts equal the reference's of that precision.
 */
#ifndef MC_MI355X_H_
#define MC_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------------------- */
enum {
    MC_OK = 0,
    MC_ERR_INVALID = 1,   /* bad argument (message in mc_last_error)                    */
    MC_ERR_HIP = 2,       /* a HIP runtime call failed                                   */
    MC_ERR_NO_DEVICE = 3, /* no usable gfx950 device                                     */
    MC_ERR_UNSUPPORTED = 4
};
/* Text of the last failure on this thread ("" if none). */
const char *mc_last_error(void);

/* Default seed of the legacy entry points (the reference's device seed is fixed too:
 * dp/MonteCarloKernel.cu:289). */
#define MC_DEFAULT_SEED 0x4D435F4D49333535ull

/* Layout of the random streams (which counter yields which normal).  Results for a given seed are comparable only between
 * builds of the same version.  1: rounds 1-2 (fp64: one Philox block = 2 normals).  2: the fp64 streams draw EIGHT normals
 * from three consecutive Philox blocks -- 96 bits per Box-Muller pair: 52-bit radius, 44-bit angle;
 * a vanilla fp64 unit is 8 paths.  The fp32 streams are unchanged. */
#define MC_STREAM_VERSION 2

/* Stream domains (Philox counter word 3). */
#define MC_DOMAIN_VANILLA 1u
#define MC_DOMAIN_BASKET 2u
#define MC_DOMAIN_CVA 3u
#define MC_DOMAIN_ASIAN 4u
#define MC_DOMAIN_BARRIER 5u
#define MC_DOMAIN_HESTON 6u
#define MC_DOMAIN_HESTON_PATH 7u
#define MC_DOMAIN_LOOKBACK 8u
#define MC_DOMAIN_LOOKBACK_BRIDGE 9u /* the lookback call's uniforms: raw Philox blocks, see mc_lookback_run_* */
#define MC_DOMAIN_MERTON 10u
#define MC_DOMAIN_MERTON_JUMPS 11u /* the jump-diffusion's Poisson counts: raw Philox blocks, see mc_merton_run_* */
#define MC_DOMAIN_AMERICAN 12u /* the pricing pass of the Bermudan options, see mc_american_run_* */
#define MC_DOMAIN_AMERICAN_FIT 13u /* the fit of their exercise rule, see mc_american_fit_*: never the paths the rule is priced on */
#define MC_DOMAIN_RAINBOW 14u /* worst-of / best-of options on a correlated basket walked over dates, see mc_rainbow_run_* */
#define MC_DOMAIN_AUTOCALL 15u /* worst-of autocallable notes on the same walk, see mc_autocall_run_* */
#define MC_DOMAIN_LOCALVOL 16u /* calls and puts under a local-volatility surface, see mc_localvol_run_* */
#define MC_DOMAIN_HESTON_LEVEL 17u /* the coupled fine and coarse Heston walks of a multilevel correction, see mc_heston_level_run_* */

#define MC_MAX_ASSETS 16         /* basket sizes whose constants can travel as kernel arguments: 1..16 */
#define MC_MAX_ASSETS_GENERIC 64 /* largest basket: sizes up to 32 have register-resident kernels, 33..64 a generic one */

/* ---- inputs (layouts == reference MonteCarlo.h of that precision) ------------------- */
typedef struct { float s, k, r, v, t; } mc_option_f32;   /* OptionData, sp/MonteCarlo.h:33-39 */
typedef struct { double s, k, r, v, t; } mc_option_f64;  /* OptionData, dp/MonteCarlo.h:32-38 */

/* Basket with a RUNTIME asset count (the reference fixes N at compile time,
 * dp/MonteCarlo.h:16,41-50).  p = row-major n x n lower-triangular Cholesky factor. */
typedef struct {
    int n;
    const float *s, *v, *p, *d, *w;
    float k, t, r;
} mc_basket_f32;
typedef struct {
    int n;
    const double *s, *v, *p, *d, *w;
    double k, t, r;
} mc_basket_f64;

/* CVA of one call: dp/MonteCarlo.h:57-65 without the unused `ns`. */
typedef struct { float defint, lgd; mc_option_f32 option; int n_grid; } mc_cva_f32;
typedef struct { double defint, lgd; mc_option_f64 option; int n_grid; } mc_cva_f64;

/* Arithmetic-average (Asian) call: n_dates equally spaced monitoring dates t_j = j t / n_dates, j = 1 ... n_dates (t_0 is not
 * in the average).  Not in the reference.  The per-date constants ln S0 + j (r - v^2/2) dt travel as a table of one value per
 * date, folded in fp64 and rounded once, which the kernels read through scalar loads: the cap keeps that table (16 KB in
 * fp32, 32 KB in fp64) the size of the scalar data cache, and the fp32 running sums over the dates (rounding error
 * ~ n_dates 2^-24 relative) at 2.4e-4 of the average in the worst case. */
#define MC_MAX_ASIAN_DATES 4096
typedef struct { mc_option_f32 option; int n_dates; } mc_asian_f32;
typedef struct { mc_option_f64 option; int n_dates; } mc_asian_f64;

/* Single-barrier European call on n_dates equally spaced dates (the Asian call's dates), monitored on those dates only
 * (MC_MONITOR_DISCRETE) or continuously, by the Brownian-bridge survival probability between them (MC_MONITOR_CONTINUOUS).
 * Not in the reference.  The per-date constants sgn (ln B - ln S0 - j a) travel as the Asian call's table does: same cap,
 * same cache argument. */
#define MC_MAX_BARRIER_DATES 4096
enum { MC_BARRIER_UP_OUT = 0, MC_BARRIER_UP_IN = 1, MC_BARRIER_DOWN_OUT = 2, MC_BARRIER_DOWN_IN = 3 };
enum { MC_MONITOR_DISCRETE = 0, MC_MONITOR_CONTINUOUS = 1 };
typedef struct { mc_option_f32 option; float barrier; int n_dates, type, monitoring; } mc_barrier_f32;
typedef struct { mc_option_f64 option; double barrier; int n_dates, type, monitoring; } mc_barrier_f64;

/* Lookback options on n_dates equally spaced dates (the Asian call's dates): the payoff is written on the running maximum or
 * minimum of the spot, taken on those dates only (MC_MONITOR_DISCRETE) or continuously, by sampling the maximum of the Brownian
 * bridge between them (MC_MONITOR_CONTINUOUS); see mc_lookback_run_*.  Not in the reference.  option.k is ignored by the
 * floating-strike types.  The per-date constants sgn j a travel as the Asian call's table does: same cap, same cache argument;
 * the running maximum is a selection, not a sum, so the cap's rounding argument holds for W_j alone. */
#define MC_MAX_LOOKBACK_DATES 4096
enum { MC_LOOKBACK_FLOAT_CALL = 0, MC_LOOKBACK_FLOAT_PUT = 1, MC_LOOKBACK_FIXED_CALL = 2, MC_LOOKBACK_FIXED_PUT = 3 };
typedef struct { mc_option_f32 option; int n_dates, type, monitoring; } mc_lookback_f32;
typedef struct { mc_option_f64 option; int n_dates, type, monitoring; } mc_lookback_f64;

/* European call under the Heston stochastic-volatility model, full-truncation Euler on n_steps equal steps (see
 * mc_heston_run_*).  Not in the reference.  option.v is ignored: the variance starts at v0.  No constant table: every per-step
 * constant is a kernel argument.  The cap keeps the fp32 running sums over the steps at the Asian call's worst-case
 * rounding (~ n_steps 2^-24 relative). */
#define MC_MAX_HESTON_STEPS 4096
typedef struct { mc_option_f32 option; float v0, kappa, theta, xi, rho; int n_steps; } mc_heston_f32;
typedef struct { mc_option_f64 option; double v0, kappa, theta, xi, rho; int n_steps; } mc_heston_f64;

/* Path-dependent calls on the Heston walk (see mc_heston_path_run_*): the arithmetic-average call and the single-barrier call
 * monitored on the dates.  Not in the reference.  heston.n_steps is the TOTAL number of Euler steps; the contract has
 * n_dates = heston.n_steps / steps_per_date equally spaced dates, so the scheme's step can be finer than the monitoring grid.
 * barrier_type is one of MC_BARRIER_*; barrier and barrier_type are ignored by MC_HESTON_PATH_ASIAN.  One table value per
 * date (the Asian call's table). */
enum { MC_HESTON_PATH_ASIAN = 0, MC_HESTON_PATH_BARRIER = 1 };
typedef struct { mc_heston_f32 heston; int steps_per_date, payoff, barrier_type; float barrier; } mc_heston_path_f32;
typedef struct { mc_heston_f64 heston; int steps_per_date, payoff, barrier_type; double barrier; } mc_heston_path_f64;

/* Calls and puts under a local-volatility surface sigma(t, S), log-Euler on n_steps equal steps (see mc_localvol_run_*).  Not in
 * the reference.  sigma points to n_times rows of n_nodes volatilities: row q holds the surface over the q-th of n_times equal
 * slices of [0, t], sampled on n_nodes equally spaced nodes of y = ln(S / s) in [y_lo, y_hi].  The array is copied during the
 * call; no pointer is retained.  The contract has n_dates = n_steps / steps_per_date equally spaced dates.  right gives the
 * sign of the payoff; barrier_type is one of MC_BARRIER_*; barrier and barrier_type are ignored by the other two payoffs, and
 * steps_per_date (which must still divide n_steps) by the European one.  option.v is ignored.  The surface travels as
 * (value, slope) pairs which every workgroup copies into LDS: MC_MAX_LOCALVOL_NODES, the most n_times * n_nodes may be, keeps
 * that copy at 16 KB in fp32 and 32 KB in fp64. */
#define MC_MAX_LOCALVOL_STEPS 4096
#define MC_MAX_LOCALVOL_NODES 2048
enum { MC_LOCALVOL_EUROPEAN = 0, MC_LOCALVOL_ASIAN = 1, MC_LOCALVOL_BARRIER = 2 };
enum { MC_LOCALVOL_CALL = 0, MC_LOCALVOL_PUT = 1 };
typedef struct {
    mc_option_f32 option;
    const float *sigma;
    int n_times, n_nodes;
    float y_lo, y_hi;
    int n_steps, steps_per_date, payoff, right, barrier_type;
    float barrier;
} mc_localvol_f32;
typedef struct {
    mc_option_f64 option;
    const double *sigma;
    int n_times, n_nodes;
    double y_lo, y_hi;
    int n_steps, steps_per_date, payoff, right, barrier_type;
    double barrier;
} mc_localvol_f64;

/* Calls under Merton's jump-diffusion on n_dates equally spaced dates (see mc_merton_run_*): the European call, the
 * arithmetic-average call and the single-barrier call monitored on the dates.  Not in the reference.  lambda is the jump
 * intensity per year, ln J ~ N(mu_j, delta^2) the jump size.  barrier_type is one of MC_BARRIER_*; barrier and barrier_type are
 * ignored by the other two payoffs.  One table value per date (the Asian call's table, same cap, same rounding argument), then
 * the Poisson thresholds and the per-count volatilities: at most MC_MAX_MERTON_JUMPS jumps per date. */
#define MC_MAX_MERTON_DATES 4096
#define MC_MAX_MERTON_JUMPS 40
enum { MC_MERTON_EUROPEAN = 0, MC_MERTON_ASIAN = 1, MC_MERTON_BARRIER = 2 };
typedef struct { mc_option_f32 option; float lambda, mu_j, delta; int n_dates, payoff, barrier_type; float barrier; } mc_merton_f32;
typedef struct { mc_option_f64 option; double lambda, mu_j, delta; int n_dates, payoff, barrier_type; double barrier; } mc_merton_f64;

/* Bermudan put or call on n_dates equally spaced exercise dates t_j = j t / n_dates, j = 1 ... n_dates (t_0 is no exercise date),
 * priced under a GIVEN exercise rule: a table beta of n_dates x 4 doubles, row j - 1 the cubic in the payoff that estimates the
 * value of continuing at date j (see mc_american_run_*).  Not in the reference.  type is MC_AMERICAN_PUT or MC_AMERICAN_CALL;
 * degree (1..3) is the degree of the polynomial a Longstaff-Schwartz fit of the rule regresses on (mc_american_solve); the
 * pricing calls check its range and otherwise ignore it.  The per-date constants travel as a table of SIX values per date
 * (xk_j, g_j, beta_j0..3), folded in fp64 and rounded once, read through scalar loads: the cap is the largest power of two
 * that keeps that table (12 KB in fp32, 24 KB in fp64) within the Asian call's (16 KB, 32 KB), the size of the scalar data
 * cache; 4096 dates would need 96 KB and 192 KB. */
#define MC_MAX_AMERICAN_DATES 512
#define MC_AMERICAN_MIN_ITM 32   /* mc_american_solve: a date with fewer paths in the money gets the never-exercise row */
#define MC_AMERICAN_SUMS 11      /* mc_american_solve: sum p^k, k = 0 ... 6, then sum p^k V, k = 0 ... 3 */
enum { MC_AMERICAN_PUT = 0, MC_AMERICAN_CALL = 1 };
typedef struct { mc_option_f32 option; int n_dates, type, degree; } mc_american_f32;
typedef struct { mc_option_f64 option; int n_dates, type, degree; } mc_american_f64;

/* Worst-of / best-of ("rainbow") option on basket.n correlated assets, 1 <= n <= MC_MAX_RAINBOW_ASSETS, walked over n_dates
 * equally spaced dates t_j = j t / n_dates, j = 1 ... n_dates, with an optional barrier on the same extremum (see
 * mc_rainbow_run_*).  Not in the reference.  basket.s, v, p and w are read as mc_basket_run_* reads them (p the row-major
 * lower-triangular Cholesky factor of the correlation; only its lower triangle is read); basket.k, t and r are the contract's
 * strike, maturity and rate.  basket.d, the reference's shift of the terminal normals, has no meaning on a walk: NULL or all
 * zeros.  type is one of MC_RAINBOW_*; barrier_type is MC_RAINBOW_NO_BARRIER (barrier is then ignored) or one of MC_BARRIER_*.
 * The per-date constants travel as a table of n values per date, folded in fp64 and rounded once, read through scalar loads:
 * the cap on n n_dates keeps that table (16 KB in fp32, 32 KB in fp64) the size of the scalar data cache, as the Asian call's. */
#define MC_MAX_RAINBOW_ASSETS 8
#define MC_MAX_RAINBOW_TABLE 4096   /* n * n_dates at most */
enum { MC_RAINBOW_CALL_ON_MIN = 0, MC_RAINBOW_CALL_ON_MAX = 1, MC_RAINBOW_PUT_ON_MIN = 2, MC_RAINBOW_PUT_ON_MAX = 3 };
enum { MC_RAINBOW_NO_BARRIER = -1 };
typedef struct { mc_basket_f32 basket; float barrier; int n_dates, type, barrier_type; } mc_rainbow_f32;
typedef struct { mc_basket_f64 basket; double barrier; int n_dates, type, barrier_type; } mc_rainbow_f64;

/* Worst-of autocallable ("Phoenix") note on basket.n correlated assets, 1 <= n <= MC_MAX_RAINBOW_ASSETS, walked over n_dates
 * equally spaced dates of which n_obs are observation dates (see mc_autocall_run_*).  Not in the reference.  The basket is read
 * exactly as mc_rainbow_run_* reads it; basket.k is the strike of the put on the worst level.  autocall and coupon_barrier are
 * arrays of n_obs levels, copied during the call: no pointer is retained.  The table holds n values per date and three per
 * observation, read through scalar loads: the cap keeps it the size of the scalar data cache, as MC_MAX_RAINBOW_TABLE does. */
#define MC_MAX_AUTOCALL_TABLE 4096   /* n * n_dates + 3 * n_obs at most */
enum { MC_AUTOCALL_KI_NONE = -1, MC_AUTOCALL_KI_DATES = 0, MC_AUTOCALL_KI_MATURITY = 1 };
typedef struct { mc_basket_f32 basket; const float *autocall; const float *coupon_barrier; float coupon, barrier, gearing;
                 int n_dates, n_obs, memory, ki_monitoring; } mc_autocall_f32;
typedef struct { mc_basket_f64 basket; const double *autocall; const double *coupon_barrier; double coupon, barrier, gearing;
                 int n_dates, n_obs, memory, ki_monitoring; } mc_autocall_f64;

/* ---- outputs ------------------------------------------------------------------------ */
typedef struct {
    double expected;    /* discounted mean payoff (price) or CVA                           */
    double confidence;  /* 1.96 s / sqrt(n)        dp/MonteCarloKernel.cu:421-422          */
    double sum, sum2;   /* sum and sum of squares of the per-path values                   */
    uint64_t n;         /* paths simulated                                                 */
    float kernel_ms;    /* device time of the call's kernels (HIP events around them)       */
    float wall_ms;      /* host wall-clock of the whole call: entry to return, launch, wait and
                         * 24-byte read-back included (what the reference's drivers time around
                         * dev_*: dp/vanillaOpt.cu:77-83); context creation is NOT in it          */
} mc_result;

/* ---- context ------------------------------------------------------------------------ */
typedef struct mc_context mc_context;

int mc_device_count(void);
/* PCI bus id of a visible device ("0000:75:00.0"; buf of >= 13 bytes): which physical GPU an index is -- what
 * bench.py's roster and multiBench print for every rank / device of a multi-GPU run. */
int mc_device_pci_bus_id(int device, char *buf, int len);
/* Create the per-GPU context (replaces dp/MonteCarloKernel.cu:296 MonteCarlo_init).
 * blocks = simulation grid size; 0 picks the default (8 workgroups of 256 per CU).
 * Current device: every call that takes a context makes that context's device the calling thread's current HIP device
 * (hipSetDevice) and leaves it so -- a thread that also drives other devices through HIP re-selects its own afterwards.
 * (libmc_multi, which visits several devices per call, puts the caller's device back itself: mc_multi.h.) */
int mc_context_create(int device, int blocks, mc_context **out);
/* Replaces dp/MonteCarloKernel.cu:344 MonteCarlo_closing. */
void mc_context_destroy(mc_context *ctx);
int mc_context_device(const mc_context *ctx);
/* The non-blocking HIP stream the context owns (the synchronous *_run_* calls use it). */
void *mc_context_stream(const mc_context *ctx);
int mc_context_blocks(const mc_context *ctx);
/* Shape of the context's most recent simulation launch: workgroups and lanes per workgroup (0, 0 before the first).  The
 * committed PMC profiles describe launches of one shape; bench.py compares (profiles/pmc_traffic.json "grid_workgroups").
 * Under MC_RNG_XORWOW it is the call's one launch, whichever kernel runs it: workgroups x lanes is the L of the sample's
 * definition below.  (Under Philox the single-unit masked launches at the edges of a vanilla range are not recorded.) */
int mc_context_last_launch(const mc_context *ctx, int *workgroups, int *group_size);
/* Name / CU count / clock of the context's device, for logs. */
int mc_context_info(const mc_context *ctx, char *name, int name_len, int *compute_units, int *clock_mhz);

/* Estimator switch (not in the reference, whose estimator is plain Monte Carlo).
 * on != 0: antithetic variates -- the sample of path p is the mean of the payoff at its normals z
 * and at -z; n_paths then counts such pairs, the triple and the confidence interval refer to the
 * pair means.  Same random stream, same path indexing; about 1.2-1.9x the time per sample for a
 * 2.7-4x smaller variance on the reference's three products. */
int mc_context_set_antithetic(mc_context *ctx, int on);

/* Basket products only (not in the reference): geometric-basket control variate.
 * on != 0: the per-path value becomes payoff(arithmetic basket) - payoff(geometric basket
 * G = W prod_a S_a(T)^(w_a/W), W = sum w) on the same normals; G is lognormal, so E[max(G-K,0)] has
 * the closed form mc_basket_control_mean_* returns (fp64, undiscounted).  mc_basket_run_* adds it
 * back (expected = discount * (sum/n + mean)); users of mc_basket_launch_* do the same after their
 * all-reduce.  Needs w[a] > 0, s[a] > 0, k > 0.  Combines with antithetic variates.  Typical
 * variance reduction on the BASELINE baskets: ~150x (x2.5 more with antithetic). */
int mc_context_set_control_variate(mc_context *ctx, int on);

/* Device timing of the synchronous *_run_* calls.  on != 0 (default): the call's kernels are bracketed by two HIP
 * events and mc_result.kernel_ms reports them (replaces the reference's cudaEvent pairs, dp/MonteCarloKernel.cu:380-386),
 * the result comes back through a 24-byte copy and a stream synchronize.  on == 0: no events; the last workgroup of the
 * call writes the result straight into pinned host memory and the calling thread polls for it from user space --
 * about 10 us less host time per call (profiles/r02_call_latency.log); kernel_ms is then 0.  The legacy symbols run
 * with timing off unless MC_VERBOSE is set. */
int mc_context_set_timing(mc_context *ctx, int on);

/* Generator switch.  MC_RNG_PHILOX (default): Philox4x32-10, counter-based -- a path's normals depend
 * only on (seed, global path index).  MC_RNG_XORWOW: the reference's generator (cuRAND XORWOW, dp/MonteCarloKernel.cu:
 * 285-290 curand_init, :68,78,250 curand_normal), hand-written for gfx950, with rocRAND's seeding and subsequence
 * layout: lane l of a launch starts at rocrand_init(seed, subsequence_base + l, 0) -- one sequence per lane, as the
 * reference keeps one curandState per thread -- and draws four words per block of normals.  Word for word rocRAND's
 * sequence (tests); cuRAND 7.5's own seeding is not in the reference tree, so the reference's exact stream stays
 * "parity unpinned".  Consequences of a per-lane stream: the sample depends on (seed, subsequence_base, grid size,
 * position in the range) instead of the global path index, first_path only places the range; a call must fit one
 * launch (<= 2^31 units); ranks of a multi-GPU job need disjoint subsequence bases (mc_multi_* sets them); vanilla
 * calls run at Philox speed, baskets on the generic kernel; Greeks are Philox-only.  Subsequence numbers stay below 2^48. */
enum { MC_RNG_PHILOX = 0, MC_RNG_XORWOW = 1 };
int mc_context_set_generator(mc_context *ctx, int generator, uint64_t subsequence_base);
/* Normals of the fp64 kernels.  MC_NORMALS_NATIVE (default): true fp64 normals, two per Philox block (52-bit uniforms,
 * mc_math_f64.hpp).  MC_NORMALS_F32: the reference's own dp arithmetic -- `double z = curand_normal(...)`, a FLOAT normal
 * widened to double (dp/MonteCarloKernel.cu:68,78,250): four normals per Philox block through the hardware
 * fp32 transcendentals, everything downstream of the normal in fp64.  A different (coarser: 24-bit normals, |z| < 6.77)
 * stream than the default, same path indexing; about 1.4-1.7x the paths/s on the 16-asset basket and the 256-date CVA
 * (DESIGN.md).  Philox only; no effect on the _f32 entry points (their Greeks included); the fp64 Greeks entry points refuse it.  Also selected at
 * context creation by the environment variable MC_F64_NORMALS=f32 (how the legacy symbols get it). */
enum { MC_NORMALS_NATIVE = 0, MC_NORMALS_F32 = 1 };
int mc_context_set_normals(mc_context *ctx, int mode);

/* Where a call's per-workgroup (sum, sum2) pairs are added up (replaces the reference's D2H copy and host loop
 * over blocks, dp/MonteCarloKernel.cu:405,416-419).  fused != 0 (default): inside the simulation kernel, by the
 * last workgroup to arrive -- one launch per call.  fused == 0: by a second, one-workgroup launch (the A/B
 * baseline; also selected by the environment variable MC_FINISH=kernel at context creation).  Both add the pairs
 * in the same fixed order: the results are identical bits. */
int mc_context_set_finish(mc_context *ctx, int fused);

/* CVA: how many adjacent lanes share one path's dates (reference: one thread walks all N_GRID dates of its path,
 * dp/MonteCarloKernel.cu:241-262).  lanes == 0 (default): chosen per call from its size -- a large call keeps one lane per path
 * and hands only its last partial wave-trip (n mod 64 x 4 x CUs paths, when that is at most 60 % of a trip) to date-parallel
 * workgroups of the same launch; a small call (up to 7/4 wave-trips on a grid of 64 dates or more, 3/4 of one on a shorter
 * grid) runs date-parallel as a whole -- the reference driver's own 131 072 paths (dp/cvaOpt.cu:12-15) are two
 * trips and keep one lane per path.  lanes == 1: never (the one-lane-per-path kernel only).  lanes == 2, 4, ... 64:
 * the whole call date-parallel with that many lanes per path (capped by the number of 8-date chunks of the grid).  The
 * estimate differs between settings only by the association of two sums per path (1e-16-level in fp64, 1e-7 in fp32);
 * XORWOW calls (one sequence per lane) and grids whose table exceeds 48 KB of LDS always use one lane per path.
 * Also set at context creation by the environment variable MC_CVA_DATE_LANES. */
int mc_context_set_cva_date_lanes(mc_context *ctx, int lanes);
int mc_basket_control_mean_f32(const mc_basket_f32 *opt, double *mean);
int mc_basket_control_mean_f64(const mc_basket_f64 *opt, double *mean);

/* Where the time of the context's last synchronous call (mc_*_run_*, mc_*_run_grid_*) went -- the reference prints the same
 * stages from inside every call (RNG set-up dp/MonteCarloKernel.cu:317-323, allocations :326-341, kernel :380-386, copy :404-409,
 * closing :415-427); here they are returned, and the legacy symbols print them under MC_VERBOSE=1.  Consecutive host-clock
 * intervals, so setup + table_upload + launch + kernel + readback + closing = wall_ms (to the clamping of readback_ms at 0):
 *   setup_ms         work a repeated identical call does not do again: XORWOW jump matrices and start states (the reference's
 *                    randomSetup, paid there on EVERY call), launch-geometry states of a new (numBlocks, numThreads), buffer growth;
 *                    waited for on the device, so that it is not inside kernel_ms
 *   table_upload_ms  constant tables built on the host and uploaded when the inputs changed (CVA per-date rows, tiled basket matrix)
 *   launch_ms        the rest of the host time before the wait: folding the inputs, the launch calls themselves (the library's code
 *                    object is loaded by mc_context_create, not by the first launch: HIP would otherwise spend 7-10 ms inside it)
 *   kernel_ms        device time of the call's kernels (HIP events; 0 with timing off -- the kernel is then inside readback_ms), capped at
 *                    the host's wait (the opening event is stamped at once on an idle device, so whatever the host does inside
 *                    the launch call -- before round 5's preload: the code-object load -- would otherwise be counted twice)
 *   readback_ms      from the last launch call to the triple on the host, minus kernel_ms: launch latency, copy / poll
 *   closing_ms       price and confidence interval on the host
 *   context_create_ms  what mc_context_create took for this context (once; NOT part of wall_ms): HIP runtime start-up and the load
 *                    of the code object on the first context of a process (~240 ms on a fresh box, ~5 ms for a second context),
 *                    stream, buffers.  first_call = 1 on the context's first synchronous call. */
typedef struct {
    float setup_ms, table_upload_ms, launch_ms, kernel_ms, readback_ms, closing_ms, wall_ms, context_create_ms;
    int first_call;
} mc_call_stats;
int mc_context_last_call_stats(const mc_context *ctx, mc_call_stats *out);
/* The context's resolved configuration (device, grid, estimator, generator, kernel-family limits ...) as one line of text;
 * printed to stderr by mc_context_create when MC_VERBOSE >= 2. */
int mc_context_describe(const mc_context *ctx, char *buf, int len);

/* Sampled device timing of the simulation kernel (not the finishing kernel): every `every`-th
 * launch is bracketed by two HIP events on its launch stream (0 = off; at most 512 samples are
 * kept between reads).  Replaces the reference's cudaEvent pair around each launch
 * (dp/MonteCarloKernel.cu:380-386,393-399,447-453), returned instead of printed. */
int mc_context_profile(mc_context *ctx, int every);
/* Waits for the sampled launches; returns their count and summed duration, then resets. */
int mc_context_profile_read(mc_context *ctx, int *samples, double *total_ms);

/* ---- asynchronous launches ------------------------------------------------------------
 * d_triple: DEVICE pointer to 3 doubles, overwritten with {sum, sum2, n}.
 * stream  : hipStream_t passed as void*; NULL = the HIP null stream, as in any HIP API
 *           (mc_context_stream(ctx) is the context's own non-blocking stream).
 * Replace the kernel launch + D2H + host block-sum of dp/MonteCarloKernel.cu:365-419
 * (vanilla :381, basket :394) and :433-465 (CVA :448). */
int mc_vanilla_launch_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                          uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);
int mc_vanilla_launch_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                          uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);
int mc_basket_launch_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed,
                         uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);
int mc_basket_launch_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed,
                         uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);
int mc_cva_launch_f32(mc_context *ctx, const mc_cva_f32 *cva, uint64_t seed,
                      uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);
int mc_cva_launch_f64(mc_context *ctx, const mc_cva_f64 *cva, uint64_t seed,
                      uint64_t first_path, uint64_t n_paths, double *d_triple, void *stream);

/* Order `stream` behind everything `ctx` has enqueued so far (event on the stream of its last call, wait on `stream`):
 * how a consumer of d_triple on ANOTHER stream -- a copy, an RCCL all-reduce -- is sequenced after the launch without
 * a host synchronisation.  A no-op when `stream` is the stream of the last call. */
int mc_context_order(mc_context *ctx, void *stream);

/* Results of asynchronous launches straight into pinned host memory (what include/mc_multi.h reads its devices back with).
 * mc_context_arm_direct: the NEXT mc_*_launch_* call on `ctx` also has its last workgroup store {sum, sum2, n} into a
 * pinned, host-coherent slot the context owns -- n last, with system-scope release semantics.  *slot = the slot's host
 * address; its word 2 is preset to -1 (n is never negative): poll `(*slot)[2] != -1` from user space, then read the
 * three doubles.  No D2H copy command, no event, no sleeping synchronize; d_triple is still written.  One armed launch in
 * flight per context; a synchronous mc_*_run_* call before the launch cancels the arming; needs the fused final
 * reduction (the default).
 * mc_context_publish: enqueues on `stream` a one-lane kernel that copies the three doubles at d_src (device memory: e.g.
 * the output of an all-reduce enqueued on that stream before it) into a second slot of the context, same protocol.
 * ONE publish in flight per context as well: a second publish before the first slot has been read re-arms the same slot. */
int mc_context_arm_direct(mc_context *ctx, const volatile double **slot);
int mc_context_publish(mc_context *ctx, const double *d_src, void *stream, const volatile double **slot);

/* 1 when everything `ctx` has enqueued has completed, 0 while some of it is pending, -1 on error (hipStreamQuery of the
 * stream of its last call): a host may poll this from user space instead of sleeping in a synchronize. */
int mc_context_idle(mc_context *ctx);

/* ---- synchronous runs (launch + wait + closing formulas) --------------------------------
 * Replace dev_vanillaOpt / dev_basketOpt / dev_cvaEquityOption (dp/MonteCarloKernel.cu:
 * 500,483,517) with an explicit seed, a 64-bit path range and a status code. */
int mc_vanilla_run_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                       uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_vanilla_run_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                       uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_basket_run_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed,
                      uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_basket_run_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed,
                      uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_cva_run_f32(mc_context *ctx, const mc_cva_f32 *cva, uint64_t seed,
                   uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_cva_run_f64(mc_context *ctx, const mc_cva_f64 *cva, uint64_t seed,
                   uint64_t first_path, uint64_t n_paths, mc_result *out);

/* ---- arithmetic-average (Asian) call -------------------------------------------------------------
 * Payoff max(A - K, 0), A = (1/m) sum_j S(t_j) over the m = n_dates monitoring dates; GBM walked date by date, one lane per
 * path: ln S_j = ln S0 + j a + bx W_j, a = (r - v^2/2) dt, bx = v sqrt(dt), W_j = z_1 + ... + z_j.  Stream: path p is unit p
 * of MC_DOMAIN_ASIAN, date j (1-based) draws entry (j - 1) % npb of block (j - 1) / npb (npb = 4 in f32, 8 in f64): the CVA's
 * layout under its own domain word, so a path's value depends on (seed, global path index, inputs) only.  Path ranges as
 * for the CVA (a unit is a path).
 * Estimator switches: mc_context_set_antithetic (mean of the value at z and at -z; n counts pairs) and
 * mc_context_set_control_variate -- the per-path value becomes max(A - K, 0) - max(G - K, 0), G = exp((1/m) sum_j ln S_j) the
 * geometric average on the same normals; G is lognormal, mc_asian_control_mean_* returns E[max(G - K, 0)] (fp64,
 * undiscounted):  exp(mu + s2/2) Phi(d1) - K Phi(d2),  mu = ln S0 + a (m + 1)/2,  s2 = v^2 dt (m + 1)(2m + 1)/(6m),
 * d1 = (mu - ln K + s2)/sqrt(s2), d2 = d1 - sqrt(s2).  mc_asian_run_* adds it back (expected = discount * (sum/n + mean));
 * users of mc_asian_launch_* do the same after their all-reduce.  The two switches combine.
 * Several GPUs: mc_asian_launch_* on the ranges of mc_shard_range, the triples added, mc_closing (plus the control mean).
 * MC_ERR_INVALID before anything is enqueued: n_dates outside [1, MC_MAX_ASIAN_DATES], s <= 0, t <= 0, v < 0, a non-finite
 * input, with the control variate on k <= 0 or v == 0, and the range errors of the other products.  MC_ERR_UNSUPPORTED: a
 * XORWOW context (one sequence per lane is another sample definition), MC_NORMALS_F32 on the _f64 calls.  The context
 * stays usable.  mc_asian_paths_* returns the per-path values (undiscounted; n_paths <= 2^26). */
int mc_asian_run_f32(mc_context *ctx, const mc_asian_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_asian_run_f64(mc_context *ctx, const mc_asian_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_asian_launch_f32(mc_context *ctx, const mc_asian_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                        double *d_triple, void *stream);
int mc_asian_launch_f64(mc_context *ctx, const mc_asian_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                        double *d_triple, void *stream);
int mc_asian_paths_f32(mc_context *ctx, const mc_asian_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_asian_paths_f64(mc_context *ctx, const mc_asian_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_asian_control_mean_f32(const mc_asian_f32 *opt, double *mean);
int mc_asian_control_mean_f64(const mc_asian_f64 *opt, double *mean);

/* ---- single-barrier call: discrete and Brownian-bridge continuous monitoring --------------------------
 * The Asian call's walk on m = n_dates dates: dt = t/m, a = (r - v^2/2) dt, bx = v sqrt(dt), W_j = z_1 + ... + z_j,
 * x_j = ln S_j = ln S0 + j a + bx W_j, x_0 = ln S0.  With h = ln barrier and sgn = +1 (up) or -1 (down) the distance to the
 * barrier is d_j = sgn (h - x_j), in natural-log units; the path is on the live side at date j when d_j > 0.
 *   discrete:    P = [min_{1<=j<=m} d_j > 0]                                  (t_0 is not monitored)
 *   continuous:  P = [min_j d_j > 0] prod_{j=1..m} (1 - exp(-2 d_{j-1} d_j / bx^2)),   d_0 = sgn (h - ln S0):
 *                the probability that the Brownian bridge between two monitored points stays on the live side, so the
 *                estimator is unbiased for the continuously monitored price at ANY n_dates, even 1, and needs no extra
 *                normals.  mc_barrier_closed_form_* is that price (Reiner-Rubinstein; discounted, no dividend, no rebate;
 *                fp64; ignores n_dates and monitoring; usable without a GPU; also needs k > 0 and v > 0).
 *   per-path value, undiscounted:  knock-out P (S_T - K)^+,  knock-in (1 - P)(S_T - K)^+,  S_T = exp(x_m).  On a path that
 *   crossed at a date the knock-out value is exactly 0 and the knock-in value exactly the payoff.
 * Stream: path p is unit p of MC_DOMAIN_BARRIER, date j (1-based) draws entry (j - 1) % npb of block (j - 1) / npb: the
 * Asian layout under its own domain word.  mc_context_set_antithetic: the mean of the value at z and at -z; n counts pairs.
 * Path ranges, the finish, timing, arming and ordering as for the other products; several GPUs as for the Asian call.
 * MC_ERR_INVALID before anything is enqueued: n_dates outside [1, MC_MAX_BARRIER_DATES]; type or monitoring out of range;
 * s <= 0, t <= 0, v < 0, barrier <= 0 or a non-finite input; the spot on or beyond the barrier (up with s >= barrier, down
 * with s <= barrier: the product is then the vanilla call or nothing); continuous monitoring with v == 0; the range errors
 * of the other products.  MC_ERR_UNSUPPORTED: a XORWOW context, MC_NORMALS_F32 on the _f64 calls, the control variate
 * switched on (no candidate control reduces the variance with coefficient 1), a context set up for external normals or
 * the launch geometry.  The context stays usable.  No rebate, puts, double barriers, unequal dates or Greeks.
 * mc_barrier_paths_* returns the per-path values (undiscounted; n_paths <= 2^26). */
int mc_barrier_run_f32(mc_context *ctx, const mc_barrier_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_barrier_run_f64(mc_context *ctx, const mc_barrier_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_barrier_launch_f32(mc_context *ctx, const mc_barrier_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                          double *d_triple, void *stream);
int mc_barrier_launch_f64(mc_context *ctx, const mc_barrier_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                          double *d_triple, void *stream);
int mc_barrier_paths_f32(mc_context *ctx, const mc_barrier_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_barrier_paths_f64(mc_context *ctx, const mc_barrier_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_barrier_closed_form_f32(const mc_barrier_f32 *opt, double *price);
int mc_barrier_closed_form_f64(const mc_barrier_f64 *opt, double *price);

/* ---- lookback options: discrete and Brownian-bridge continuous extrema -----------------------------------
 * The Asian call's walk on m = n_dates dates: dt = t/m, a = (r - v^2/2) dt, bx = v sqrt(dt), W_j = z_1 + ... + z_j,
 * x_j = ln S_j = ln S0 + j a + bx W_j, x_0 = ln S0.  With sgn = +1 when the payoff is on the maximum and -1 when it is on the
 * minimum, the signed log excursion is y_j = sgn (x_j - x_0) = sgn (j a + bx W_j), y_0 = 0.
 *   discrete:    Y = max_{1<=j<=m} y_j                                        (t_0 is not monitored)
 *   continuous:  Y = max_{1<=j<=m} M_j,  M_j = (y_{j-1} + y_j + sqrt((y_j - y_{j-1})^2 + bx^2 E_j)) / 2,  E_j = -2 ln u_j, u_j
 *                the date's uniform: the inverse of the bridge law P(max <= y | y_{j-1}, y_j) = 1 - exp(-2 (y - y_{j-1})(y - y_j) / bx^2)
 *                (the law behind the barrier call's survival factor), so the estimator is unbiased for the continuously
 *                monitored price at ANY n_dates, even 1.  M_j >= max(y_{j-1}, y_j): t_0 is included, and continuous >=
 *                discrete on every path.  Needs v > 0.
 *   ext = S0 exp(sgn Y): the running maximum (sgn = +1) or minimum (sgn = -1);  S_T = exp(x_m).
 *   per-path value, undiscounted:   MC_LOOKBACK_FLOAT_CALL  sgn -1  max(S_T - ext, 0)     MC_LOOKBACK_FLOAT_PUT  sgn +1  max(ext - S_T, 0)
 *                                   MC_LOOKBACK_FIXED_CALL  sgn +1  max(ext - k, 0)       MC_LOOKBACK_FIXED_PUT  sgn -1  max(k - ext, 0)
 * mc_context_set_antithetic: the mean of the value at z and at -z, both directions on the SAME E_j (any coupling of the
 * bridge draws is unbiased; sharing them halves the uniform work); n counts pairs.
 * Stream: path p is unit p of MC_DOMAIN_LOOKBACK, date j (1-based) draws entry (j - 1) % npb of block (j - 1) / npb: the Asian
 * layout under its own domain word.  The bridge uniforms, drawn by the continuous form only, are RAW Philox blocks of the same
 * unit in MC_DOMAIN_LOOKBACK_BRIDGE.  f32: date j takes word (j - 1) % 4 of block (j - 1) / 4, u = fmaf((float) word, 2^-32, 2^-33),
 * in (0, 1] (u = 1 gives E = 0, which is valid).  f64: date j takes words 2 ((j - 1) % 2) and 2 ((j - 1) % 2) + 1 of
 * block (j - 1) / 2 as (lo, hi) of u = (((hi:lo) >> 12) + 1/2) 2^-52, strictly inside (0, 1).  A path's value depends on (seed,
 * global path index, inputs) only.  Path ranges, the finish, timing, arming and ordering as for the other products; several
 * GPUs as for the Asian call.
 * mc_lookback_closed_form_*: the discounted price of the CONTINUOUS product at inception (Goldman-Sosin-Gatto for the floating
 * strikes, Conze-Viswanathan for the fixed ones; no dividend; fp64, Phi by erfc; ignores n_dates and monitoring; usable without
 * a GPU).  With D = e^{-rt}, c = v^2/(2r), g = 2r sqrt(t)/v, a1 = (r + v^2/2) sqrt(t)/v, a2 = a1 - v sqrt(t),
 * d1 = (ln(s/k) + (r + v^2/2) t)/(v sqrt(t)), p = (s/k)^(-2r/v^2):
 *   floating call  s Phi(a1) - s D Phi(a2) + s D c [Phi(g - a1) - e^{rt} Phi(-a1)]
 *   floating put   s D Phi(-a2) - s Phi(-a1) + s D c [e^{rt} Phi(a1) - Phi(a1 - g)]
 *   fixed call     k <= s: floating put + s - D k;   k > s: s Phi(d1) - k D Phi(d1 - v sqrt(t)) + s D c [e^{rt} Phi(d1) - p Phi(d1 - g)]
 *   fixed put      k >= s: floating call - s + D k;  k < s: k D Phi(v sqrt(t) - d1) - s Phi(-d1) + s D c [p Phi(g - d1) - e^{rt} Phi(-d1)]
 * It needs v > 0 (and k > 0 for the fixed types) and returns MC_ERR_INVALID for r == 0 (the limit exists but is not
 * implemented); the bracket cancels for small |r|, at about 1e-16 v^2/(2|r|) relative.
 * MC_ERR_INVALID before anything is enqueued: n_dates outside [1, MC_MAX_LOOKBACK_DATES]; type or monitoring out of range;
 * s <= 0, t <= 0, v < 0 or a non-finite input; k <= 0 or non-finite for the fixed types; continuous monitoring with v == 0;
 * drift and volatility that put the simulated spot outside the range of a double; the range errors of the other products.
 * MC_ERR_UNSUPPORTED: the control variate switched on (there is none), a XORWOW context, MC_NORMALS_F32 on the _f64 calls, a
 * context set up for external normals or the launch geometry.  The context stays usable.  No partial lookback period, no
 * extremum carried in from before t_0, no unequal dates, no Greeks.
 * mc_lookback_paths_* returns the per-path values (undiscounted; n_paths <= 2^26). */
int mc_lookback_run_f32(mc_context *ctx, const mc_lookback_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_lookback_run_f64(mc_context *ctx, const mc_lookback_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_lookback_launch_f32(mc_context *ctx, const mc_lookback_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_lookback_launch_f64(mc_context *ctx, const mc_lookback_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_lookback_paths_f32(mc_context *ctx, const mc_lookback_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_lookback_paths_f64(mc_context *ctx, const mc_lookback_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_lookback_closed_form_f32(const mc_lookback_f32 *opt, double *price);
int mc_lookback_closed_form_f64(const mc_lookback_f64 *opt, double *price);

/* ---- European call under the Heston model: full-truncation Euler in log space -----------------------------
 * dS = r S dt + sqrt(V) S dW1,  dV = kappa (theta - V) dt + xi sqrt(V) dW2,  corr(dW1, dW2) = rho,  V(0) = v0.
 * On m = n_steps equal steps: dt = t/m, sdt = sqrt(dt), rho' = sqrt(1 - rho^2), x_0 = ln s, V_0 = v0, and for j = 1 ... m,
 * with the step's two normals (z1_j, z2_j):
 *     V+  = max(V_{j-1}, 0)        s = sqrt(V+)
 *     x_j = x_{j-1} + (r - V+/2) dt + s sdt z1_j
 *     V_j = V_{j-1} + kappa (theta - V+) dt + xi sdt s (rho z1_j + rho' z2_j)
 * Per path, undiscounted, the value is (exp(x_m) - k)^+.  mc_context_set_antithetic: the mean of the value at (z1, z2) and at
 * (-z1, -z2), each with its own V; n counts pairs.  xi = 0, kappa = 0, |rho| = 1 and a violated Feller condition
 * (2 kappa theta < xi^2) are valid inputs.  option.v is ignored.
 * Stream: path p is unit p of MC_DOMAIN_HESTON; step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of block
 * 2(j-1) / npb as z1 and z2 (npb = 4 in f32, 8 in f64): the Asian layout with two entries per step; in f64 that is pair
 * (j-1) of the generator's Box-Muller pairs.  A path's value depends on (seed, global path index, inputs) only.
 * Path ranges, the finish, call statistics, timing, arming and ordering as for the other products; several GPUs:
 * mc_heston_launch_* on the ranges of mc_shard_range, the triples added, mc_closing.
 * MC_ERR_INVALID before anything is enqueued: n_steps outside [1, MC_MAX_HESTON_STEPS]; s <= 0, t <= 0, v0 < 0, kappa < 0,
 * theta < 0, xi < 0, |rho| > 1; a non-finite input; inputs whose scale of drift and volatility over the m steps is beyond the
 * argument range of the device's exponential (a heuristic guard against absurd inputs, not a bound on the variance); the range
 * errors of the other products.  MC_ERR_UNSUPPORTED: the control
 * variate switched on (there is none), a XORWOW context, MC_NORMALS_F32 on the _f64 calls, a context set up for external
 * normals or the launch geometry.  The context stays usable.  No puts, Greeks, book or other discretisation schemes;
 * path-dependent payoffs: mc_heston_path_* below.  mc_heston_paths_* returns the per-path values (undiscounted; n_paths <= 2^26).
 * mc_heston_closed_form_*: the exact price of the call in the CONTINUOUS model (discounted, no dividend) -- not of the Euler
 * scheme, whose bias shrinks with dt.  Heston's P1 / P2 decomposition with the branch-cut-safe ("little Heston trap")
 * characteristic function, integrated in fp64 by 16-point Gauss-Legendre on panels of the fixed width 1 / (4 sd), sd^2 = t times
 * the mean variance over [0, t], until both integrands have stayed below 1e-18 for a whole panel; xi == 0 is Black-Scholes at
 * that mean variance.  Ignores n_steps; usable without a GPU; the input checks above, and k > 0.
 * MC_ERR_INVALID too when the integrands have not decayed within 40000 panels (|rho| = 1 with a tiny variance).
 * Verified: within 1e-11 absolute at s = 100 (measured: 3.6e-13) of an independent quadrature of Lewis's single integral over
 * the cases and strikes of tests/test_heston_ref.py, kappa = 0 and |rho| = 1 included; for 0 < xi << 1 the cancellation in
 * beta - d costs about 1e-16 kappa theta / xi^2 relative (checked to 1e-9 at xi = 1e-3); 6.8061 on the case of Broadie and Kaya. */
int mc_heston_run_f32(mc_context *ctx, const mc_heston_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_run_f64(mc_context *ctx, const mc_heston_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_launch_f32(mc_context *ctx, const mc_heston_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                         double *d_triple, void *stream);
int mc_heston_launch_f64(mc_context *ctx, const mc_heston_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                         double *d_triple, void *stream);
int mc_heston_paths_f32(mc_context *ctx, const mc_heston_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_heston_paths_f64(mc_context *ctx, const mc_heston_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_heston_closed_form_f32(const mc_heston_f32 *opt, double *price);
int mc_heston_closed_form_f64(const mc_heston_f64 *opt, double *price);

/* ---- Asian and discretely monitored barrier calls under the Heston model ----------------------------------
 * The walk of mc_heston_run_* on m = heston.n_steps = n_dates * steps_per_date steps: the same step formulas, two normals per
 * step.  The monitoring dates are t_d = d t / n_dates, d = 1 ... n_dates (t_0 is not monitored); date d falls after step
 * d * steps_per_date, where the log price is
 *     x_d = ln s + r t_d - (dt/2) sum_{j <= d spd} V+_{j-1} + sdt sum_{j <= d spd} s_{j-1} z1_j        (spd = steps_per_date)
 * -- the same real number as the step-by-step x_j of mc_heston_run_*, read from its two running sums.
 *   MC_HESTON_PATH_ASIAN:    per path, undiscounted, ((1/n_dates) sum_d exp(x_d) - k)^+
 *   MC_HESTON_PATH_BARRIER:  h = ln barrier, sgn = +1 (up) or -1 (down), d_d = sgn (h - x_d), P = [min_d d_d > 0];
 *                            knock-out P (exp(x_m) - k)^+, knock-in (1 - P)(exp(x_m) - k)^+.  On a path that crossed at a date the
 *                            knock-out value is exactly 0 and the knock-in value exactly the payoff.
 * The barrier is monitored ON THE DATES ONLY.  Continuous monitoring is not offered: the Brownian-bridge survival probability
 * of mc_barrier_run_* assumes a constant variance between two dates, which under this model is an approximation.
 * mc_context_set_antithetic: the mean of the value at (z1, z2) and at (-z1, -z2), each direction with its own V, its own sums
 * and its own running average or minimum; n counts pairs.
 * Stream: path p is unit p of MC_DOMAIN_HESTON_PATH; step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of block
 * 2(j-1) / npb as z1 and z2: the Heston layout under its own domain word.
 * Path ranges, the finish, call statistics, timing, arming and ordering as for mc_heston_*; several GPUs:
 * mc_heston_path_launch_* on the ranges of mc_shard_range, the triples added, mc_closing.
 * MC_ERR_INVALID before anything is enqueued: everything mc_heston_run_* refuses (its exponent-range guard included);
 * steps_per_date < 1 or not a divisor of heston.n_steps; payoff out of range; for the barrier payoff barrier_type out of
 * range, barrier <= 0 or non-finite, the spot on or beyond the barrier (up with s >= barrier, down with s <= barrier).
 * MC_ERR_UNSUPPORTED: the control variate switched on (there is none), a XORWOW context, MC_NORMALS_F32 on the _f64 calls, a
 * context set up for external normals or the launch geometry.  The context stays usable.  No puts, rebates, double barriers,
 * unequal dates, Greeks or book.  mc_heston_path_paths_* returns the per-path values (undiscounted; n_paths <= 2^26). */
int mc_heston_path_run_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_path_run_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_path_launch_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                              double *d_triple, void *stream);
int mc_heston_path_launch_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                              double *d_triple, void *stream);
int mc_heston_path_paths_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_heston_path_paths_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);

/* ---- multilevel Monte Carlo on the Heston walk: one level, the plan, the driver (Giles 2008) ---------------
 * mc_heston_level_*: the correction of one level, Y = P_fine - P_coarse per path, P the MC_HESTON_PATH_ASIAN payoff (one date:
 * the European call).  opt describes the FINE walk, exactly that of mc_heston_path_* on m = heston.n_steps steps of dt = t/m.  The
 * COARSE walk takes m/2 steps of 2 dt, steps_per_date / 2 of them per date, with the same dates, strike and model, on the SAME
 * Brownian increments: coarse step i = 1 ... m/2 stands on the fine steps a = 2i - 1 and b = 2i.  In the precision of the call,
 *     t_j = c1 z1_j + c2 z2_j                    the fine step's own (c1 = xi sdt rho, c2 = xi sdt rho', rounded constants)
 *     W1_i = z1_a + z1_b      rounded once       the increment of the coarse log price, sqrt(2 dt) z1_c = sdt W1_i
 *     T_i  = t_a + t_b        rounded once       the increment of the coarse variance; W2 = z2_a + z2_b is never formed
 * and with V the coarse variance, V+ = max(V, 0), s = sqrt(V+):
 *     x_c += (r - V+/2) 2 dt + s sdt W1_i,       V += kappa (theta - V+) 2 dt + s T_i
 * where 2 kappa dt, 2 kappa theta dt and 2 (dt/2) are the fine walk's rounded constants doubled (exact).  Date d falls after
 * coarse step d * steps_per_date / 2 and adds the same per-date constant ln s + r t_d as on the fine walk.
 * Per path, undiscounted: Y = P_fine - P_coarse.  mc_context_set_antithetic: the mean of Y at (z1, z2) and Y at (-z1, -z2), the
 * four walks each with their own variance and sums; n counts pairs.  mc_result carries the sums of Y and their closing by mc_closing as
 * for every product (expected = the discounted mean of Y, which may be negative; confidence = mc_closing's 95 % half-width);
 * mc_heston_level_paths_* returns the per-path Y (undiscounted; n_paths <= 2^26).
 * Stream: path p is unit p of MC_DOMAIN_HESTON_LEVEL; FINE step j (1-based) draws entries 2(j-1) % npb and 2(j-1) % npb + 1 of
 * block 2(j-1) / npb: the Heston layout.  Its own domain makes a level independent of mc_heston_path_* on the same indices; a
 * path's value depends on (seed, global path index, inputs) only.  Path ranges, the finish, timing, arming and ordering as for
 * mc_heston_path_*; several GPUs: mc_heston_level_launch_* on the ranges of mc_shard_range, the triples added, mc_closing.
 * MC_ERR_INVALID before anything is enqueued: everything mc_heston_path_run_* refuses; an odd steps_per_date;
 * MC_HESTON_PATH_BARRIER (a discontinuous payoff needs another coupling to be worth a level).  MC_ERR_UNSUPPORTED: the control
 * variate, a XORWOW context, MC_NORMALS_F32 on the _f64 calls, external normals, the launch geometry.  The context stays usable. */
int mc_heston_level_run_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_level_run_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_heston_level_launch_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                               double *d_triple, void *stream);
int mc_heston_level_launch_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                               double *d_triple, void *stream);
int mc_heston_level_paths_f32(mc_context *ctx, const mc_heston_path_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_heston_level_paths_f64(mc_context *ctx, const mc_heston_path_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);

/* mc_mlmc_plan: the path counts that reach a variance of eps^2 / 2 at least cost, from the levels' variances var[l] and costs
 * cost[l] per path:  n[l] = ceil(2 eps^-2 sqrt(var[l] / cost[l]) sum_k sqrt(var[k] cost[k])).  Host only, no GPU.  A level of zero
 * variance gets n = 0.  MC_ERR_INVALID: levels < 1, a NULL pointer, eps <= 0 or not finite, a negative or non-finite variance, a
 * cost <= 0 or not finite, a count beyond 2^52. */
int mc_mlmc_plan(int levels, const double *var, const double *cost, double eps, uint64_t *n);

/* mc_heston_mlmc_run_*: the price of the call of `level0` (MC_HESTON_PATH_ASIAN) to a root-mean-square error eps by multilevel
 * Monte Carlo.  Level 0 is mc_heston_path_run_* on level0 itself; level l >= 1 is mc_heston_level_run_* at heston.n_steps 2^l
 * steps and steps_per_date 2^l per date.  The algorithm, a pure function of (inputs, seed, the context's antithetic setting):
 *   1. L = max(min_levels, 2) (at least three levels, so that the bias test below has two corrections); a pilot of n_pilot paths
 *      on every level 0 ... L;
 *   2. V_l = the sample variance of level l (discounted), C_0 = n_steps, C_l = 1.5 n_steps 2^l (a cost MODEL, no timer);
 *      n = mc_mlmc_plan(V, C, eps); every level with n_l above its paths so far is topped up on the NEXT indices of its range, the
 *      sums added; repeated until no level needs more (the variances move as paths are added);
 *   3. the weak order fixed at 1: bias = max(|m_L|, |m_{L-1}| / 2), m_l the level's discounted mean; converged if bias <= eps / sqrt 2;
 *      otherwise, below max_levels, level L + 1 is added with its pilot and step 2 repeats.
 * Ranges: level 0 owns paths [0, n_0) of MC_DOMAIN_HESTON_PATH; level l >= 1 owns [l 2^40, l 2^40 + n_l) of MC_DOMAIN_HESTON_LEVEL.
 * No level may pass 2^34 paths, the most of one call (MC_ERR_INVALID: eps is then out of reach).  A level's sums are those of ONE
 * mc_heston_path_run_* / mc_heston_level_run_* over its final range, up to the order of the fp64 additions.
 * out: per level its mc_result, with kernel_ms and wall_ms summed over its calls, the paths used and the first path of the range;
 * price = sum of the means, stderr_ = sqrt(sum_l V_l / n_l) with V_l the sample variance of the DISCOUNTED value of level l
 * (mc_closing's half-width is that of the undiscounted one), bias as above, converged 1 or 0.  max_levels reached without convergence is NOT an error: converged = 0, MC_OK.
 * MC_ERR_INVALID before anything is enqueued: what level 0 and level 1 refuse of level0; eps <= 0 or not finite; min_levels < 0;
 * max_levels < max(min_levels, 2) or > MC_MLMC_MAX_LEVELS; n_pilot < 2 or > 2^34; a finest level max_levels beyond
 * MC_MAX_HESTON_STEPS.  MC_ERR_UNSUPPORTED as for mc_heston_level_run_*.  The context stays usable. */
#define MC_MLMC_MAX_LEVELS 12   /* finest level index */
typedef struct { double eps; int min_levels, max_levels; uint64_t n_pilot; } mc_mlmc_spec;
typedef struct { mc_result result; uint64_t n_paths, first_path; } mc_mlmc_level;
typedef struct {
    double price, stderr_, bias;   /* discounted; stderr_ is one standard error, not the 95 % half-width */
    int converged, levels;         /* levels = L + 1, the entries of level[] in use */
    mc_mlmc_level level[MC_MLMC_MAX_LEVELS + 1];
} mc_mlmc_result;
int mc_heston_mlmc_run_f32(mc_context *ctx, const mc_heston_path_f32 *level0, const mc_mlmc_spec *spec, uint64_t seed, mc_mlmc_result *out);
int mc_heston_mlmc_run_f64(mc_context *ctx, const mc_heston_path_f64 *level0, const mc_mlmc_spec *spec, uint64_t seed, mc_mlmc_result *out);

/* ---- calls and puts under a local-volatility surface: European, Asian, discretely monitored barrier -------------
 * dS = r S dt + sigma(t, S) S dW, log-Euler on m = n_steps equal steps: dt = t/m, sdt = sqrt(dt), y = ln(S / s), y_0 = 0, and for
 * step j = 1 ... m with the step's normal z_j
 *     sigma_j = surface(slice(j), y_{j-1})
 *     y_j     = y_{j-1} + (r - sigma_j^2 / 2) dt + sigma_j sdt z_j
 * The first walk here whose table is read at an index of the lane's own: the volatility depends on the path's state.
 * The surface is the caller's array sigma[n_times][n_nodes].  Time axis: piecewise constant over n_times >= 1 equal slices of
 * [0, t]; n_steps must be a multiple of n_times and slice(j) = (j - 1) / (n_steps / n_times) in integers.  Log-spot axis:
 * n_nodes >= 2 equally spaced nodes of y in [y_lo, y_hi], y_lo < y_hi, linear in y between nodes and flat beyond both ends.
 * With h = (y_hi - y_lo) / (n_nodes - 1) and a_i = sigma[slice][i]:
 *     u = clamp((y - y_lo) / h, 0, n_nodes - 1),   i = min(floor(u), n_nodes - 2),   sigma = a_i + (u - i) b_i,   b_i = a_{i+1} - a_i
 * The interpolant is continuous in y, across the nodes and across the clamps.  b_i is computed in fp64 from the a_i of the call's
 * precision and rounded once; the kernels evaluate u as fma(y, 1/h, -y_lo/h) with both constants folded in fp64 and rounded once.
 * The dates are those of mc_heston_path_*: n_dates = n_steps / steps_per_date, date d = 1 ... n_dates falls after step
 * d * steps_per_date (t_0 is not monitored).  Per path, undiscounted, with S_d = s exp(y_d) and phi = +1 (MC_LOCALVOL_CALL) or -1
 * (MC_LOCALVOL_PUT):
 *   MC_LOCALVOL_EUROPEAN   (phi (S_m - k))^+
 *   MC_LOCALVOL_ASIAN      (phi ((1/n_dates) sum_d S_d - k))^+
 *   MC_LOCALVOL_BARRIER    g = ln(barrier / s), sgn = +1 (up) or -1 (down), d_d = sgn (g - y_d), P = [min_d d_d > 0];
 *                          knock-out P (phi (S_m - k))^+, knock-in (1 - P)(phi (S_m - k))^+: value = (c0 + c1 P) payoff.  Monitored
 *                          on the dates only.
 * mc_context_set_antithetic: the mean of the value at z and at -z, each direction with its own y and its own lookups; n counts pairs.
 * Stream: path p is unit p of MC_DOMAIN_LOCALVOL; step j (1-based) draws entry (j-1) % npb of block (j-1) / npb (npb = 4 in
 * f32, 8 in f64): the Asian layout.  A path's value depends on (seed, global path index, inputs) only.
 * Path ranges, the finish, call statistics, timing, arming and ordering as for the other products; several GPUs:
 * mc_localvol_launch_* on the ranges of mc_shard_range, the triples added, mc_closing.
 * MC_ERR_INVALID before anything is enqueued: n_steps outside [1, MC_MAX_LOCALVOL_STEPS]; n_times < 1, n_nodes < 2 or
 * n_times * n_nodes > MC_MAX_LOCALVOL_NODES; n_steps not a multiple of n_times; steps_per_date < 1 or not a divisor of n_steps;
 * sigma NULL, or an entry negative or non-finite; y_lo >= y_hi or either non-finite, or a node spacing so small that 1/h or -y_lo/h
 * is not finite in the call's precision; payoff, right or (barrier payoff)
 * barrier_type out of range; for the barrier payoff barrier <= 0 or non-finite, or the spot on or beyond the barrier (up with
 * s >= barrier, down with s <= barrier); s <= 0, t <= 0, a non-finite s, k, r, t; inputs whose drift and largest volatility over
 * the m steps are beyond the argument range of the device's exponential (the guard of mc_heston_run_* with max sigma in place of
 * the variance).  MC_ERR_UNSUPPORTED: the control variate switched on (there is none), a XORWOW context, MC_NORMALS_F32 on the
 * _f64 calls, a context set up for external normals or the launch geometry.  The context stays usable.
 * Not offered: continuous monitoring, unequal slices or nodes, rates or dividends that vary in time, several assets, Greeks, a
 * control variate, a book.  mc_localvol_paths_* returns the per-path values (undiscounted; n_paths <= 2^26).
 * mc_localvol_sigma_*: the fp64 value of the interpolant above at step `step` (1-based: the slice is slice(step)) and log-spot y,
 * computed from the table as rounded for that precision (a_i as given, b_i rounded once) with u and the sum in fp64.  Usable
 * without a GPU; the input checks above, and step outside [1, n_steps] or a non-finite y is MC_ERR_INVALID. */
int mc_localvol_run_f32(mc_context *ctx, const mc_localvol_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_localvol_run_f64(mc_context *ctx, const mc_localvol_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_localvol_launch_f32(mc_context *ctx, const mc_localvol_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_localvol_launch_f64(mc_context *ctx, const mc_localvol_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_localvol_paths_f32(mc_context *ctx, const mc_localvol_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_localvol_paths_f64(mc_context *ctx, const mc_localvol_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_localvol_sigma_f32(const mc_localvol_f32 *opt, int step, double y, double *sigma);
int mc_localvol_sigma_f64(const mc_localvol_f64 *opt, int step, double y, double *sigma);

/* ---- calls under Merton's jump-diffusion: European, Asian, discretely monitored barrier ----------------------
 * dS/S = (r - lambda kappa) dt + v dW + (J - 1) dN,  N Poisson with rate lambda,  ln J ~ N(mu_j, delta^2),
 * kappa = exp(mu_j + delta^2/2) - 1 (the compensator: e^{-rt} S is a martingale).  The first model here with a DISCONTINUOUS path.
 * On m = n_dates equally spaced dates, dt = t/m, a = (r - lambda kappa - v^2/2) dt, bx = v sqrt(dt), date j draws a count
 * N_j ~ Poisson(lambda dt) and ONE normal z_j: given N_j, the diffusion increment plus the N_j jumps is one normal with mean
 * a + mu_j N_j and deviation s_{N_j}, s_n = sqrt(bx^2 + n delta^2).  So the walk is EXACT IN LAW at any n_dates:
 *     C_j = N_1 + ... + N_j,   A_j = sum_{i<=j} s_{N_i} z_i,   x_j = ln S_j = ln s + j a + mu_j C_j + A_j.
 * Per path, undiscounted:
 *   MC_MERTON_EUROPEAN   (exp(x_m) - k)^+
 *   MC_MERTON_ASIAN      ((1/m) sum_j exp(x_j) - k)^+
 *   MC_MERTON_BARRIER    sgn = +1 (up) or -1 (down), d_j = sgn (ln barrier - x_j), P = [min_j d_j > 0] taken by a select;
 *                        (c0 + c1 P)(exp(x_m) - k)^+, (c0, c1) = (0, 1) knock-out, (1, -1) knock-in.  Monitored ON THE DATES
 *                        ONLY; a crossed knock-out is exactly 0.  (A jump breaks the Brownian-bridge argument: no continuous form.)
 * mc_context_set_antithetic: the mean of the value at z and at -z on the SAME counts N_j (any coupling of the counts is
 * unbiased; sharing them halves the count work, as the lookback's bridge draws are shared); A^-_j = -A_j exactly; n counts pairs.
 * lambda = 0, delta = 0 and mu_j = 0 are valid; lambda = 0 is the constant-volatility product.  v = 0 is valid with any
 * delta: s_0 = 0 is an exact 0 (a date without a jump then adds 0 z = 0, nothing divides by s_n).
 * Stream: path p is unit p of MC_DOMAIN_MERTON, date j (1-based) draws entry (j - 1) % npb of block (j - 1) / npb: the Asian
 * layout under its own domain word.  The counts come from RAW Philox blocks of the same unit in MC_DOMAIN_MERTON_JUMPS, the
 * lookback's bridge layout: f32 date j takes the 32-bit word (j - 1) % 4 of block (j - 1) / 4; f64 date j takes words
 * 2 ((j - 1) % 2) and 2 ((j - 1) % 2) + 1 of block (j - 1) / 2 as (lo, hi) of a 64-bit word.
 * The count is an exact integer inversion of that word w, W = 32 or 64 bits, no float conversion on the device:
 *     N = #{k < K : w >= T_k},   T_0 <= T_1 <= ... <= T_{K-1} < 2^W       (N = 0 iff w < T_0; K = 0: N = 0 always)
 * with p = lambda dt (fp64), f_n = e^{-p} p^n / n! by f_n = f_{n-1} p / n and F_k = f_0 + ... + f_k, both in long double:
 *     T_k = min(floor(F_k 2^W), 2^W - 1),
 *     K   = the smallest k >= 0 with tail_k = sum_{n > k} f_n < 2^-(W+1)   (the tail summed from its small end, never as 1 - F_k),
 * so a count above K has probability below 2^-(W+1): it is folded into N = K.  p = 0 gives K = 0.  K > MC_MAX_MERTON_JUMPS is
 * refused (p <= 5 needs K = 25 at 32 and K = 37 at 64 bits; the cap is reached at p = 12.39 and p = 6.23).  |T_k / 2^W - F_k|
 * <= 2^-W from the floor plus the rounding of F_k, a few 2^-64 in the x87 long double: within the documented 2^-W + 4 2^-53.
 * mc_merton_thresholds_* writes T_0 ... T_{K-1} to out (room for MC_MAX_MERTON_JUMPS values) and K to *count; plain C, no GPU.
 * mc_merton_closed_form_*: the discounted price of MC_MERTON_EUROPEAN (fp64; ignores n_dates, payoff and the barrier; usable
 * without a GPU): Merton's series
 *     sum_n e^{-l t} (l t)^n / n! BS(s, k, r_n, v_n, t),  l = lambda (1 + kappa), v_n^2 = v^2 + n delta^2 / t,
 *     r_n = r - lambda kappa + n ln(1 + kappa) / t,
 * BS the Black-Scholes call (Phi by erfc; v_n = 0: max(s - k e^{-r_n t}, 0)), summed until the Poisson weight left is below
 * 1e-18.  Needs k > 0.  Within 1e-10 of a 30-digit quadrature of the characteristic function at s = 100 (measured: 2e-14 at most).
 * Path ranges, the finish, call statistics, timing, arming and ordering as for the other products; several GPUs as for the
 * Asian call.
 * MC_ERR_INVALID before anything is enqueued: n_dates outside [1, MC_MAX_MERTON_DATES]; payoff out of range; s <= 0, t <= 0,
 * v < 0, lambda < 0, delta < 0 or a non-finite input; for the barrier payoff what mc_barrier_run_* refuses (type, barrier <= 0,
 * the spot on or beyond the barrier); more than MC_MAX_MERTON_JUMPS thresholds; drift, volatility and jumps that can put the
 * exponent |ln s| + m (|a| + |mu_j| K + (bx + delta sqrt(K)) z_max) outside the device exponential's range.
 * MC_ERR_UNSUPPORTED: the control variate switched on (there is none), a XORWOW context, MC_NORMALS_F32 on the _f64 calls, a
 * context set up for external normals or the launch geometry.  The context stays usable.  No puts, no continuous monitoring,
 * no control variate, no Greeks, no book, no other jump law, no jumps on the Heston walk.
 * mc_merton_paths_* returns the per-path values (undiscounted; n_paths <= 2^26). */
int mc_merton_run_f32(mc_context *ctx, const mc_merton_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_merton_run_f64(mc_context *ctx, const mc_merton_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_merton_launch_f32(mc_context *ctx, const mc_merton_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                         double *d_triple, void *stream);
int mc_merton_launch_f64(mc_context *ctx, const mc_merton_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                         double *d_triple, void *stream);
int mc_merton_paths_f32(mc_context *ctx, const mc_merton_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_merton_paths_f64(mc_context *ctx, const mc_merton_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_merton_closed_form_f32(const mc_merton_f32 *opt, double *price);
int mc_merton_closed_form_f64(const mc_merton_f64 *opt, double *price);
int mc_merton_thresholds_f32(const mc_merton_f32 *opt, uint64_t *out, int *count);
int mc_merton_thresholds_f64(const mc_merton_f64 *opt, uint64_t *out, int *count);

/* ---- Bermudan put and call under a given exercise rule (the pricing pass of Longstaff-Schwartz) ---------------------------
 * m = n_dates, dt = t/m, a = (r - v^2/2) dt, bx = v sqrt(dt), W_j = z_1 + ... + z_j, and in units of the strike
 *     x_j = ln(s/k) + j a + bx W_j,   e_j = exp(x_j),   q = -1 (put) or +1 (call),   p_j = max(q (e_j - 1), 0),
 *     g_j = exp(r (t - t_j))          (a payoff taken at t_j, compounded to t).
 * The rule is the m x 4 table beta: C_j(p) = ((beta_j3 p + beta_j2) p + beta_j1) p + beta_j0 estimates, in the same units, the
 * value of NOT exercising at date j.  At date j < m the holder exercises iff p_j > 0 and p_j g_j > C_j(p_j); at date m iff
 * p_m > 0 (row m of beta is ignored, whatever it holds).  A row {+inf, 0, 0, 0} means "never on this date": in the Horner form
 * above it stays free of NaN for every finite p.  Per path, walking forward: the value is p_tau g_tau at the FIRST date tau that
 * exercises, else 0 -- in units of k, compounded to t.  The calls scale the sums by k and k^2 and the closing's exp(-r t) then
 * gives the price, as for every other product; mc_american_paths_* returns the per-path values unscaled (units of k).
 * mc_context_set_antithetic: the mean of the value at z and at -z, each direction with its own exercise date.
 * Any rule gives a LOWER bound of the Bermudan price (it is one admissible exercise policy) as long as beta was not fitted on the
 * paths it is priced on: path p is unit p of MC_DOMAIN_AMERICAN, a domain no fit draws from; date j (1-based) draws entry
 * (j - 1) % npb of block (j - 1) / npb: the Asian layout under its own domain word.  MC_STREAM_VERSION stays 2.
 * MC_ERR_INVALID before anything is enqueued: n_dates outside [1, MC_MAX_AMERICAN_DATES]; type or degree out of range;
 * s <= 0, k <= 0, t <= 0, v < 0 or a non-finite input; in rows 1 ... m - 1 a beta entry that is NaN, or -inf, or infinite outside
 * column 0 (after rounding to the kernel's precision); the control variate switched on (there is none); a generator other than
 * Philox; drift and volatility that can put |ln(s/k)| + m (|a| + bx z_max) outside the device exponential's range.
 * MC_ERR_UNSUPPORTED: MC_NORMALS_F32 on the _f64 calls, a context set up for external normals or the launch geometry.  The
 * context stays usable.  Path ranges, the finish, call statistics, timing, arming and ordering as for the other products;
 * several GPUs through mc_american_launch_* + mc_shard_range + mc_closing.  n_paths <= 2^26 for mc_american_paths_*.
 *
 * mc_american_fit_*: the rule by Longstaff-Schwartz on n_paths <= 2^24 paths of their own.  Backward from maturity, V = p_m; for
 * j = m - 1 ... 1: beta_j = the regression of V on {1, p_j, ..., p_j^degree} over the paths with p_j > 0 (mc_american_solve on sums
 * accumulated in fp64 in both precisions), then V = exercise_j ? p_j g_j : V with the decision above.  The path is never stored:
 * W_m = sqrt(m) z_m and W_j = j/(j+1) W_{j+1} + sqrt(j/(j+1)) z_j, the Brownian bridge from 0, is a Brownian motion at 1 ... m
 * walked backward, exact in law; the per-path state (W, V) lives in device memory owned by the context.  One kernel launch per date
 * and a one-lane solve between two of them, 2 m + 1 launches on the context's stream without a host synchronisation in between.
 * beta receives n_dates x 4 doubles (row m zero; in fp32 the kernels apply each row rounded once to float); *in_sample the
 * estimate from the fit's own paths -- biased HIGH, the rule having seen them -- closed like every other result (kernel_ms spans
 * the whole fit).  Path p is unit p of MC_DOMAIN_AMERICAN_FIT, the Asian layout: whatever seed and range, no path is shared with
 * the pricing pass.  The estimator is always the plain one (mc_context_set_antithetic concerns the pricing pass).  Refusals as
 * for mc_american_run_*, plus n_paths > 2^24; synchronous, on the context's stream.  The fit always brackets its launches with HIP
 * events and reports kernel_ms, also after mc_context_set_timing(ctx, 0) (as the Greeks calls do: it waits on the stream anyway).
 *
 * mc_american_solve (plain C, no GPU): ONE date's regression of a Longstaff-Schwartz fit.  sums holds MC_AMERICAN_SUMS doubles
 * taken over the paths in the money at that date: sums[k] = sum p^k, k = 0 ... 6 (sums[0] their number), sums[7 + k] = sum p^k V,
 * k = 0 ... 3, V the path's value from the later dates (units of k, compounded to t).  Only k <= 2 degree and k <= degree are
 * read.  The normal equations of V on {1, p, ..., p^degree} are solved in fp64 by Cholesky on the Jacobi-scaled matrix (row and
 * column i divided by the root of the i-th diagonal entry): beta[0 ... degree] the coefficients, the rest 0.  Fewer than
 * MC_AMERICAN_MIN_ITM paths in the money, or a pivot that is not positive, give the never-exercise row {+inf, 0, 0, 0}.
 * Returns MC_OK in both cases; MC_ERR_INVALID for a NULL argument or degree outside 1..3.
 *
 * mc_american_lattice_*: the discounted Cox-Ross-Rubinstein binomial price of the SAME contract (exercise on the m dates only)
 * on m steps_per_date steps, u = exp(v sqrt(h)), d = 1/u, h = t / (m steps_per_date), risk-neutral probability
 * (exp(r h) - d)/(u - d); fp64, plain C, no GPU.  Needs v > 0, a probability inside (0, 1) and at most 2^15 steps. */
int mc_american_run_f32(mc_context *ctx, const mc_american_f32 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_american_run_f64(mc_context *ctx, const mc_american_f64 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_american_launch_f32(mc_context *ctx, const mc_american_f32 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_american_launch_f64(mc_context *ctx, const mc_american_f64 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_american_paths_f32(mc_context *ctx, const mc_american_f32 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_american_paths_f64(mc_context *ctx, const mc_american_f64 *opt, const double *beta, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_american_fit_f32(mc_context *ctx, const mc_american_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *beta, mc_result *in_sample);
int mc_american_fit_f64(mc_context *ctx, const mc_american_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *beta, mc_result *in_sample);
int mc_american_solve(const double *sums, int degree, double beta[4]);
int mc_american_lattice_f32(const mc_american_f32 *opt, int steps_per_date, double *price);
int mc_american_lattice_f64(const mc_american_f64 *opt, int steps_per_date, double *price);

/* ---- worst-of / best-of options on a correlated basket walked over dates -----------------------------------
 * n assets, m = n_dates dates, L = basket.p (lower triangle), z_{j,k} the standard normal of date j and factor k:
 *   dt = t/m,  a_i = (r - v_i^2/2) dt,  M = diag(v_i sqrt(dt)) L  (lower triangle, folded in fp64, rounded once)
 *   W_k(j) = z_{1,k} + ... + z_{j,k}
 *   y_i(j) = ln(w_i s_i) + j a_i + sum_{k<=i} M_ik W_k(j)                the log of the weighted level of asset i on date j
 *   e = -1 for the min types, +1 for the max types:  Y(j) = max_i e y_i(j),  X_j = exp(e Y(j))   (the worst / best weighted level)
 *   q = +1 call, -1 put:   payoff = max(q (X_m - k), 0)
 *   barrier, on the SAME extremum, on the dates 1 ... m only (t_0 is not monitored), a touch counts as a hit:
 *     b = +1 up, -1 down:   d_j = b (ln barrier - e Y(j)),   P = [min_{1<=j<=m} d_j > 0]  taken by a select
 *     value = (c0 + c1 P) payoff,  (c0, c1) = (0, 1) knock-out, (1, -1) knock-in, (1, 0) without a barrier
 *   antithetic: the mean of the value at z and at -z
 * The per-date constants e (ln(w_i s_i) + j a_i) are folded in fp64 and rounded once.  w_i = 1/s_i gives performance levels,
 * w_i = 1 absolute ones.  Worst-of knock-in put: MC_RAINBOW_PUT_ON_MIN with MC_BARRIER_DOWN_IN; worst-of knock-out call:
 * MC_RAINBOW_CALL_ON_MIN with MC_BARRIER_DOWN_OUT; best-of call: MC_RAINBOW_CALL_ON_MAX, with or without MC_BARRIER_UP_OUT.  All
 * four types combine with all five barrier choices.  v_i = 0 is valid.
 *
 * Stream: path p is unit p of MC_DOMAIN_RAINBOW.  The normal of date j (1-based) and factor k (0-based) is FLAT entry
 * (j - 1) n + k of the Asian layout: entry % npb of block entry / npb (npb = 4 in f32, 8 in f64).  No normal is drawn and
 * dropped between two dates, whatever n is.
 *
 * mc_rainbow_run_* fills expected with exp(-r t) mean(value); mc_rainbow_launch_* is the asynchronous form (device triple, then
 * mc_closing with the discount exp(-r t); several GPUs: mc_shard_range per device).  mc_rainbow_paths_* returns the per-path
 * values (undiscounted; n_paths <= 2^26).
 *
 * mc_rainbow_closed_form_*: the discounted price of the contract WITHOUT a barrier at n = 1 (Black-Scholes) and n = 2 (fp64,
 * plain C, no GPU; ignores n_dates).  L must be the factor of a CORRELATION matrix: a row whose length differs from 1 by more than
 * fp32 rounding (|L_i0^2 + L_i1^2 - 1| > 1e-5) is refused, since the walk takes L as given and the formulas would price another
 * model.  With S_i = w_i s_i, rho = L_10 L_00 (divided by the second row's length) and sigma^2 = v_1^2 + v_2^2 - 2 rho v_1 v_2, the call on
 * the minimum is Stulz's formula
 *   S_1 M(y_1, -d; -rho_1) + S_2 M(y_2, d - sigma sqrt t; -rho_2) - k e^{-rt} M(y_1 - v_1 sqrt t, y_2 - v_2 sqrt t; rho),
 *   y_i = (ln(S_i/k) + (r + v_i^2/2) t)/(v_i sqrt t),  d = (ln(S_1/S_2) + sigma^2 t/2)/(sigma sqrt t),
 *   rho_1 = (v_1 - rho v_2)/sigma,  rho_2 = (v_2 - rho v_1)/sigma,
 * M the bivariate normal distribution function (Genz's Gauss-Legendre form of Drezner-Wesolowsky, 20 points); the call on the
 * maximum is the two Black-Scholes calls minus it; the puts follow by parity with PV(min) = S_1 - Margrabe(S_1 -> S_2) and
 * PV(max) = S_2 + Margrabe.  It needs k > 0, v_1 > 0, v_2 > 0, sigma sqrt t >= 1e-8 and sigma >= 1e-3 (v_1 + v_2) (MC_ERR_INVALID
 * otherwise: the two assets then move as one); |rho| up to 1 is handled.  Measured against a 30-digit evaluation on five markets
 * of three strikes (r < 0, rho < 0, |rho| = 0.95 and 0.999, levels 1 : 40): within 3.3e-16 max(S_1, S_2); the bound to rely on is
 * 1e-10 max(S_1, S_2).
 * MC_ERR_INVALID for n > 2 and for a barrier_type other than MC_RAINBOW_NO_BARRIER.
 *
 * MC_ERR_INVALID before anything is enqueued: n outside [1, MC_MAX_RAINBOW_ASSETS]; n_dates < 1; n n_dates >
 * MC_MAX_RAINBOW_TABLE; type or barrier_type out of range; s_i <= 0, w_i <= 0, v_i < 0, t <= 0 or a non-finite input; with a
 * barrier, barrier <= 0 or the initial extremum of w_i s_i not strictly on the live side of it (up: >= barrier, down: <=
 * barrier); a nonzero basket.d; the control variate switched on (there is none); the range errors of the other products.
 * MC_ERR_UNSUPPORTED: a XORWOW context, MC_NORMALS_F32 on the _f64 calls, a context set up for external normals or the launch
 * geometry.  The context stays usable.  Not offered: continuous monitoring, unequal dates, per-asset barriers, Asian and lookback payoffs on the basket, Greeks, n > 8. */
int mc_rainbow_run_f32(mc_context *ctx, const mc_rainbow_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_rainbow_run_f64(mc_context *ctx, const mc_rainbow_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_rainbow_launch_f32(mc_context *ctx, const mc_rainbow_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                          double *d_triple, void *stream);
int mc_rainbow_launch_f64(mc_context *ctx, const mc_rainbow_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                          double *d_triple, void *stream);
int mc_rainbow_paths_f32(mc_context *ctx, const mc_rainbow_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_rainbow_paths_f64(mc_context *ctx, const mc_rainbow_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_rainbow_closed_form_f32(const mc_rainbow_f32 *opt, double *price);
int mc_rainbow_closed_form_f64(const mc_rainbow_f64 *opt, double *price);

/* ---- worst-of autocallable notes: memory coupons, early redemption, a knock-in put ---------------
 * The model of mc_rainbow_run_* with the extremum fixed to the minimum: n assets, n_dates equally spaced dates t_j = j t / n_dates,
 *   y(j) = min_i y_i(j) = ln min_i (w_i S_i(t_j))          y_i(j), a_i, M, W_k(j) as stated there; w_i = 1/s_i: performance levels
 * n_obs observation dates, n_dates % n_obs == 0, E = n_dates / n_obs: observation k = 1 ... n_obs falls on date k E.
 *   autocall[k-1] = A_k > 0         the trigger level; INFINITY: not callable at this observation
 *   coupon_barrier[k-1] = C_k >= 0  0: the coupon is unconditional
 *   coupon = c >= 0                 the amount per observation, notional 1;  memory = 0 / 1
 *   barrier = B > 0                 the knock-in level;  ki_monitoring: MC_AUTOCALL_KI_DATES (all walk dates 1 ... n_dates),
 *                                   MC_AUTOCALL_KI_MATURITY (date n_dates only) or MC_AUTOCALL_KI_NONE (the put is always
 *                                   live, barrier is ignored)
 *   gearing = g >= 0                the standard note is g = 1 / basket.k;  g = 0: no put
 * Per path direction, with alive = 1, miss = 0, V = 0, at observation k on date j = k E, in this order:
 *   called = [y(j) >= ln A_k]                  equality counts as reached
 *   paid   = [y(j) >= ln min(A_k, C_k)]        a called note always pays its coupon
 *   cash   = paid ? fma(c memory, miss, c) : 0,  then  miss = paid ? 0 : miss + 1
 *   k < n_obs:  V = fma(alive D_k, cash + called, V),  then  alive = called ? 0 : alive
 *   k = n_obs:  V = fma(alive D_k, fma(-(KI ? g : 0), max(basket.k - exp(y(n_dates)), 0), cash + 1), V)
 *   D_k = exp(-r t k / n_obs), the discount factor of date k E, folded on the host in fp64 and rounded once, as ln A_k and
 *   ln min(A_k, C_k) are (+-infinity allowed: every decision compares the log level with the table value itself)
 *   KI = 1 for MC_AUTOCALL_KI_NONE; otherwise KI = [min over the monitored dates of y(j) <= ln B]: a touch counts, t_0 is not
 *   monitored
 *   antithetic: the mean of V at z and at -z
 * V is a PRESENT VALUE: every flow carries its own discount factor.  mc_autocall_run_* fills expected with mean(V);
 * mc_autocall_launch_* is the asynchronous form (device triple, then mc_closing with the discount 1; several GPUs:
 * mc_shard_range per device).  mc_autocall_paths_* returns V itself (n_paths <= 2^26): unlike the other mc_*_paths_* calls,
 * whose per-path values are undiscounted, these are discounted.
 *
 * Stream: path p is unit p of MC_DOMAIN_AUTOCALL; the rainbow's flat layout unchanged: the normal of date j (1-based) and factor
 * k (0-based) is flat entry (j - 1) n + k.  A path that is called draws no normals it does not need: the values do not depend on it.
 *
 * MC_ERR_INVALID before anything is enqueued: everything mc_rainbow_run_* refuses about the basket and the ranges; n_obs < 1 or
 * n_dates % n_obs != 0; n n_dates + 3 n_obs > MC_MAX_AUTOCALL_TABLE; a NULL array; A_k <= 0 or NaN; C_k < 0, NaN or infinite;
 * coupon < 0, gearing < 0, basket.k <= 0; ki_monitoring out of range; memory not 0 / 1; with a knock-in, barrier <= 0 or the initial
 * worst level <= barrier; the control variate switched on (there is none).  MC_ERR_UNSUPPORTED: as for mc_rainbow_run_* (a
 * XORWOW context, MC_NORMALS_F32 on the _f64 calls, external normals, the launch geometry).  The context stays usable.
 * Not offered: per-asset barriers, continuous knock-in monitoring, unequal observation dates, per-observation coupon amounts, an
 * exact single-asset price, Greeks, a control variate, a book, n > 8. */
int mc_autocall_run_f32(mc_context *ctx, const mc_autocall_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_autocall_run_f64(mc_context *ctx, const mc_autocall_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, mc_result *out);
int mc_autocall_launch_f32(mc_context *ctx, const mc_autocall_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_autocall_launch_f64(mc_context *ctx, const mc_autocall_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths,
                           double *d_triple, void *stream);
int mc_autocall_paths_f32(mc_context *ctx, const mc_autocall_f32 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_autocall_paths_f64(mc_context *ctx, const mc_autocall_f64 *opt, uint64_t seed, uint64_t first_path, uint64_t n_paths, double *h_out);

/* ---- a book of vanilla calls in one launch ----------------------------------------------------
 * Entry i prices option i on its own seed and path range [first_path, first_path + n_paths); out[i] / triple i is that
 * entry's result.  One kernel launch (two with mc_context_set_finish(ctx, 0)) prices the whole book, instead of one launch
 * per option (about 3.3 us per option at best, the device's dispatch floor).
 *   - Same sample as a single call: out[i] and mc_vanilla_run_* on entry i's option, seed and range are built from the
 *     same per-path payoffs, bit for bit (same Philox counters, same per-unit code); only the order in which the sums are
 *     added may differ (in fp32: which payoffs share an fp32 partial sum before it is added in fp64).  The antithetic switch
 *     is honoured with the single call's meaning (n counts pairs).
 *   - An entry's triple depends on that entry alone, bit for bit: not on its index, the other entries, count, the
 *     context's blocks or which workgroup did the work.  The same book gives the same bits on every call, and the fused
 *     and the two-launch finish (MC_FINISH=kernel) give the same bits.
 *   - Philox with native normals only: XORWOW and MC_NORMALS_F32 on the _f64 calls return MC_ERR_UNSUPPORTED.  A book
 *     never runs on caller-supplied normals (the external-normals test hooks) nor in the reference's launch geometry
 *     (mc_*_run_grid_*): those are separate entry points, and a context set up for either is refused the same way.
 *   - Refused with MC_ERR_INVALID before anything is enqueued: count < 1 or > MC_MAX_BOOK, and any entry the single
 *     call would refuse (n_paths == 0, a range that overflows or needs more than one call, an option out of range);
 *     mc_last_error names the index of the first bad entry.  Also refused: a book of more than 2^24 chunks in all (an
 *     entry is at most ~2048 chunks: e.g. more than 8192 entries of 1e8 fp32 paths); the message then names the entry at
 *     which the count passes the limit, itself valid -- split the book there.  The context stays usable.
 *   - Timing off (mc_context_set_timing(ctx, 0)): kernel_ms is 0, as for the single calls.
 *   - kernel_ms and wall_ms are those of the whole book, repeated in every entry; mc_context_last_call_stats describes
 *     the book call.
 * The launch form writes the undiscounted {sum, sum2, n} of entry i to d_triples[3 i .. 3 i + 2] (DEVICE memory,
 * 3 * count doubles), as mc_vanilla_launch_* does for one option.  The book's tables are cached by content: a repeated
 * book uploads nothing, and its launch may then be captured into a hipGraph. */
#define MC_MAX_BOOK (1 << 20)
typedef struct { mc_option_f32 option; uint64_t seed, first_path, n_paths; } mc_book_entry_f32;
typedef struct { mc_option_f64 option; uint64_t seed, first_path, n_paths; } mc_book_entry_f64;
int mc_vanilla_book_run_f32(mc_context *ctx, const mc_book_entry_f32 *entries, int count, mc_result *out);
int mc_vanilla_book_run_f64(mc_context *ctx, const mc_book_entry_f64 *entries, int count, mc_result *out);
int mc_vanilla_book_launch_f32(mc_context *ctx, const mc_book_entry_f32 *entries, int count, double *d_triples, void *stream);
int mc_vanilla_book_launch_f64(mc_context *ctx, const mc_book_entry_f64 *entries, int count, double *d_triples, void *stream);

/* ---- pathwise Greeks of the vanilla call (the reference prices only) -------------
 * One pass, the pricing kernels' stream and path indexing: price, delta = dV/dS and vega = dV/dsigma
 * as discounted means of  I (S_T - K),  I S_T / S,  I S_T (sqrt(T) z - sigma T),  I = [S_T > K],
 * each with its own 95 % half-width.  Plain estimator only. */
typedef struct { mc_result price, delta, vega; } mc_vanilla_greeks;
int mc_vanilla_greeks_run_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                              uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks *out);
int mc_vanilla_greeks_run_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                              uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks *out);

/* Likelihood-ratio forms of the same three numbers: delta = payoff z / (S sigma sqrt T), vega = payoff ((z^2 - 1) / sigma
 * - z sqrt T), z the path's normal.  They differentiate the density instead of the payoff (no indicator), at the price
 * of a larger variance on a smooth payoff like this one; needs v > 0 and t > 0. */
int mc_vanilla_greeks_lr_run_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                                 uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks *out);
int mc_vanilla_greeks_lr_run_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                                 uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks *out);

/* ---- pathwise Greeks of the basket call ------------------------------------------------
 * On the pricing kernels' stream and path indexing (reference formulas dp/MonteCarloKernel.cu:74-101), with
 * B = sum_a w_a S_a(T), I = [B > K]:  price,  delta[a] = dV/dS_a = I w_a S_a(T) / S_a,
 * vega[a] = dV/dv_a = I w_a S_a(T) (bt_a sqrt T - v_a T); discounted means with their own 95 % half-widths.
 * delta and vega are caller arrays of opt->n results.  Plain estimator; one pass over the paths per 8 assets (a lane keeps the
 * (sum, sum2) pairs of the price and of eight assets' two derivatives in registers). */
int mc_basket_greeks_run_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed, uint64_t first_path,
                             uint64_t n_paths, mc_result *price, mc_result *delta, mc_result *vega);
int mc_basket_greeks_run_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed, uint64_t first_path,
                             uint64_t n_paths, mc_result *price, mc_result *delta, mc_result *vega);
/* Likelihood-ratio forms of the same 1 + 2n numbers: the payoff times the score of the terminal prices' joint lognormal
 * density.  With y = L^-T g (the path's normals whitened by the inverse factor, formed on the host):
 *   delta[a] = payoff y_a / (S_a v_a sqrt T),
 *   vega[a]  = payoff [ (y_a (L g)_a - 1) / v_a + (sqrt T d_a - v_a T) y_a / (v_a sqrt T) ]
 * (one asset: the vanilla forms above).  Needs t > 0, every v[a] > 0 and a non-singular factor (every p[a][a] > 0 -- the
 * reference driver's own 3 x 3 correlation is singular, SURVEY 2.3 #10, and is refused). */
int mc_basket_greeks_lr_run_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed, uint64_t first_path,
                                uint64_t n_paths, mc_result *price, mc_result *delta, mc_result *vega);
int mc_basket_greeks_lr_run_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed, uint64_t first_path,
                                uint64_t n_paths, mc_result *price, mc_result *delta, mc_result *vega);

/* ---- second-order Greeks of the vanilla and basket calls ---------------------------------------------
 * The mixed estimator (Glasserman 7.3): the likelihood-ratio derivative of the pathwise delta, so no indicator is
 * differentiated twice.  Same stream and path indexing as the first-order Greeks; plain estimator, Philox with native normals
 * only (antithetic, XORWOW, MC_NORMALS_F32 on the _f64 entry points, and for the basket the control variate: MC_ERR_UNSUPPORTED);
 * needs v > 0 and t > 0 (MC_ERR_INVALID).
 * Vanilla, one pass, z the path's normal, I = [S_T > K]:
 *   gamma = d2V/dS2        = I S_T / S^2 (z / (sigma sqrt T) - 1)
 *   vanna = d2V/dS dsigma  = I S_T / S ((z^2 - 1) / sigma - z sqrt T)
 * discounted means with their own 95 % half-widths; price, delta and vega are the same bits as mc_vanilla_greeks_run_*'s. */
typedef struct { mc_result price, delta, vega, gamma, vanna; } mc_vanilla_greeks2;
int mc_vanilla_greeks2_run_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                               uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks2 *out);
int mc_vanilla_greeks2_run_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                               uint64_t first_path, uint64_t n_paths, mc_vanilla_greeks2 *out);
/* Basket: the symmetric n x n gamma matrix d2V / dS_a dS_b.  With I = [B > K], p_a = I w_a S_a(T) / S_a (the pathwise delta term),
 * y = L^-T g (the LR basket Greeks' whitened normals) and c_b = 1 / (S_b v_b sqrt T):
 *   gamma[a][b] = 1/2 (p_a y_b c_b + p_b y_a c_a) - [a == b] p_a / S_a
 * discounted, each entry with its own half-width.  gamma is a caller array of n*n results, row-major, both triangles filled (the
 * kernel computes the n (n + 1) / 2 entries a <= b, one pass over the paths per 4 x 4 tile of them); price is the same bits as
 * mc_basket_greeks_run_*'s.  Inputs as for mc_basket_greeks_lr_run_*: t > 0, every v[a] > 0, a non-singular factor. */
int mc_basket_gamma_run_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed, uint64_t first_path,
                            uint64_t n_paths, mc_result *price, mc_result *gamma);
int mc_basket_gamma_run_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed, uint64_t first_path,
                            uint64_t n_paths, mc_result *price, mc_result *gamma);

/* ---- CVA with its pathwise delta and vega -------------------------------------------------
 * On the CVA kernel's stream (reference loop dp/MonteCarloKernel.cu:241-262), not discounted, like the CVA itself (:466):
 *   d CVA / d S_0   = LGD sum_j dp_j cnd(d1_j) S_j / S_0
 *   d CVA / d sigma = LGD sum_j dp_j [ S_j phi(d1_j) sqrt(tau_j) + S_j cnd(d1_j) (W_j - sigma t_j) ],  W_j the Brownian
 *                     motion at date j (closed-form vega of the exposure + the path's own sensitivity).  Plain estimator. */
typedef struct { mc_result cva, delta, vega; } mc_cva_greeks;
int mc_cva_greeks_run_f32(mc_context *ctx, const mc_cva_f32 *cva, uint64_t seed, uint64_t first_path,
                          uint64_t n_paths, mc_cva_greeks *out);
int mc_cva_greeks_run_f64(mc_context *ctx, const mc_cva_f64 *cva, uint64_t seed, uint64_t first_path,
                          uint64_t n_paths, mc_cva_greeks *out);
/* Likelihood-ratio forms: only the first transition's density depends on S_0, every transition's on sigma, and the closed-form
 * exposure depends on sigma explicitly (that part stays pathwise):
 *   d CVA / d S_0   = E[ CVA_path z_1 ] / (S_0 sigma sqrt(dt))
 *   d CVA / d sigma = E[ LGD sum_j dp_j S_j phi(d1_j) sqrt(tau_j) + CVA_path sum_j ((z_j^2 - 1) / sigma - z_j sqrt(dt)) ]
 * Same stream, same CVA plane; the variance grows with the number of dates (the scores add up). */
int mc_cva_greeks_lr_run_f32(mc_context *ctx, const mc_cva_f32 *cva, uint64_t seed, uint64_t first_path,
                             uint64_t n_paths, mc_cva_greeks *out);
int mc_cva_greeks_lr_run_f64(mc_context *ctx, const mc_cva_f64 *cva, uint64_t seed, uint64_t first_path,
                             uint64_t n_paths, mc_cva_greeks *out);

/* ---- per-path values, for parity tests ---------------------------------------------------
 * h_out: HOST pointer to n_paths values (undiscounted payoffs / per-path CVA).  Same kernels
 * as above with a store of every value added; n_paths <= 2^26. */
int mc_vanilla_paths_f32(mc_context *ctx, const mc_option_f32 *opt, uint64_t seed,
                         uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_vanilla_paths_f64(mc_context *ctx, const mc_option_f64 *opt, uint64_t seed,
                         uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_basket_paths_f32(mc_context *ctx, const mc_basket_f32 *opt, uint64_t seed,
                        uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_basket_paths_f64(mc_context *ctx, const mc_basket_f64 *opt, uint64_t seed,
                        uint64_t first_path, uint64_t n_paths, double *h_out);
int mc_cva_paths_f32(mc_context *ctx, const mc_cva_f32 *cva, uint64_t seed,
                     uint64_t first_path, uint64_t n_paths, float *h_out);
int mc_cva_paths_f64(mc_context *ctx, const mc_cva_f64 *cva, uint64_t seed,
                     uint64_t first_path, uint64_t n_paths, double *h_out);
/* ---- compatibility mode: the reference's launch geometry and per-thread XORWOW streams ---------------------------
 * The reference's result depends on (numBlocks, numThreads): dp/MonteCarloKernel.cu:285-290 gives every thread of the
 * launch its own cuRAND XORWOW state, curand_init(seed = blockIdx.x + gridDim.x, subsequence = threadIdx.x, offset 0);
 * thread t of a block prices paths t, t + numThreads, ... < N_PATH of that block (:146,191,240) and draws its normals
 * with curand_normal() one after the other (two words per Box-Muller pair, the second member kept for the next call;
 * :68,78,250 -- in the dp build the float normal is widened to double).  These calls reproduce that sample: same seeding
 * geometry, same thread-to-path assignment, same per-thread order of the draws -- a CVA path draws for the dates whose
 * `t -= dt` is still >= 0 (:249) -- with the generator and Box-Muller of rocRAND/hipRAND (rocrand_xorwow.h,
 * rocrand_normal.h), i.e. what a HIP build of the reference draws on this GPU, bit for bit (tests/test_gpu_grid.py).
 * cuRAND itself seeds XORWOW with other constants and is not in this image: equality with an NVIDIA run of the reference
 * is NOT claimed ("parity unpinned").
 *   n = num_blocks * paths_per_block paths are priced (the reference's numBlocks * (sims / numBlocks)).
 * How it runs (round 4): the call IS the reference's launch -- num_blocks workgroups of num_threads threads, every thread
 * with its XORWOW state and Box-Muller pair in registers, pricing its own paths through the per-path code of the hot kernels;
 * no normal touches HBM (1e8 vanilla paths at 512 x 128: 0.40 ms in round 3's staged form, see DESIGN.md for this one).
 * Shapes without a fused kernel (baskets beyond 16 assets, more blocks than the context's pair buffer holds) take round
 * 3's staged form: the normals of the call are written to HBM (one Real per draw) and priced by the simulation kernels
 * of mc_*_run_* through the external-normals policy -- same sample, same per-path values.  MC_GRID_FORM=staged / fused in
 * the environment forces a form.  The start states of a geometry are set up on first use and kept (the last 4 geometries).
 * Plain estimator only; the context's generator / normals settings are ignored.  num_threads <= 1024, at most 2^24 threads
 * and 2^31 paths.  mc_result.kernel_ms covers the pricing kernel only; wall_ms the whole call. */
int mc_vanilla_run_grid_f32(mc_context *ctx, const mc_option_f32 *opt, int num_blocks, int num_threads,
                            uint64_t paths_per_block, mc_result *out);
int mc_vanilla_run_grid_f64(mc_context *ctx, const mc_option_f64 *opt, int num_blocks, int num_threads,
                            uint64_t paths_per_block, mc_result *out);
int mc_basket_run_grid_f32(mc_context *ctx, const mc_basket_f32 *opt, int num_blocks, int num_threads,
                           uint64_t paths_per_block, mc_result *out);
int mc_basket_run_grid_f64(mc_context *ctx, const mc_basket_f64 *opt, int num_blocks, int num_threads,
                           uint64_t paths_per_block, mc_result *out);
int mc_cva_run_grid_f32(mc_context *ctx, const mc_cva_f32 *cva, int num_blocks, int num_threads,
                        uint64_t paths_per_block, mc_result *out);
int mc_cva_run_grid_f64(mc_context *ctx, const mc_cva_f64 *cva, int num_blocks, int num_threads,
                        uint64_t paths_per_block, mc_result *out);
/* ---- host-side helpers -------------------------------------------------------------- */
/* Closing formulas of dp/MonteCarloKernel.cu:420-423 (discount = exp(-rT)) and :466-468
 * (discount = 1), in fp64, from an (all-reduced) triple. */
void mc_closing(double sum, double sum2, uint64_t n, double discount, double *expected,
                double *confidence);
/* Contiguous shard of `total` paths owned by `rank` of `world`: [*first, *first + *count).
 * rank g owns [floor(gP/G), floor((g+1)P/G)). */
void mc_shard_range(uint64_t total, int rank, int world, uint64_t *first, uint64_t *count);
/* Cholesky with the reference's semantics (dp/MonteCarloHost.c:90-105: column-oriented,
 * a non-positive pivot leaves its column zero).  Row-major n x n; returns the number of
 * non-positive pivots met (0 = the input was positive definite). */
int mc_chol_f32(int n, const float *c, float *a);
int mc_chol_f64(int n, const double *c, double *a);
/* Covariance-matrix input (the reference's drivers take volatilities and a correlation matrix and
 * call Chol themselves, dp/basketOpt.cu:34-61,96-99).  cov = row-major n x n covariance of the assets' annualised
 * log-returns; like Chol (dp/MonteCarloHost.c:96-99) only its lower triangle is read.  Out: v[n] = sqrt(cov[a][a])
 * and p[n*n] = Cholesky factor (reference semantics) of the correlation matrix cov[a][b] / (v[a] v[b]) -- the `v`
 * and `p` of mc_basket_* / MultiOptionData.  Returns the number of non-positive pivots (0 = positive definite), or
 * -1 for a bad argument (n < 1, NULL, a non-finite entry, a diagonal entry <= 0). */
int mc_factor_from_cov_f32(int n, const float *cov, float *v, float *p);
int mc_factor_from_cov_f64(int n, const double *cov, double *v, double *p);

#ifdef __cplusplus
}
#endif
#endif /* MC_MI355X_H_ */
