/*
 * hestonPathOpt.c -- the two path-dependent calls on the Heston walk (mc_heston_path_run_*): the arithmetic-average call and the
 * up-and-out call at B = 125 monitored on the dates, each plain and with antithetic variates on the same seed; then the same two
 * contracts at constant variance (xi = kappa = 0, where the log-Euler walk is exact) next to the constant-volatility products
 * of the same contract: mc_asian_run_* with its control variate and mc_barrier_run_* with discrete monitoring.
 * Prints one line per form: price, 95 % half-width, kernel time, and the distance to the line's neighbour (antithetic to plain,
 * constant variance to constant volatility) in units of the two half-widths added.
 * Plain C on the native ABI (include/mc_mi355x.h); built per precision (hestonPathOpt_f64, hestonPathOpt_f32).
 *   hestonPathOpt_f64 [dates] [steps_per_date] [paths]      (default 12 dates x 21 steps, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_heston_path_f32 path_t;
typedef mc_asian_f32 asian_t;
typedef mc_barrier_f32 barrier_t;
#define PATH_RUN mc_heston_path_run_f32
#define ASIAN_RUN mc_asian_run_f32
#define BARRIER_RUN mc_barrier_run_f32
#define PRECISION "f32"
#else
typedef mc_heston_path_f64 path_t;
typedef mc_asian_f64 asian_t;
typedef mc_barrier_f64 barrier_t;
#define PATH_RUN mc_heston_path_run_f64
#define ASIAN_RUN mc_asian_run_f64
#define BARRIER_RUN mc_barrier_run_f64
#define PRECISION "f64"
#endif

static void line(const char *name, const mc_result *r, const mc_result *neighbour)
{
    printf("%s price=%.17g ci=%.6g kernel_ms=%.3f diff_in_ci=%.3f\n", name, r->expected, r->confidence, (double)r->kernel_ms,
           neighbour ? (r->expected - neighbour->expected) / (r->confidence + neighbour->confidence) : 0.0);
}

int main(int argc, char **argv)
{
    const int dates = argc > 1 ? atoi(argv[1]) : 12, spd = argc > 2 ? atoi(argv[2]) : 21;
    const unsigned long long paths = argc > 3 ? strtoull(argv[3], NULL, 10) : 1000000ull;
    path_t h = {.heston = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0, .t = 1}, .v0 = 0.04, .kappa = 2, .theta = 0.04, .xi = 0.3,
                           .rho = -0.7, .n_steps = dates * spd},
                .steps_per_date = spd, .payoff = MC_HESTON_PATH_ASIAN, .barrier_type = MC_BARRIER_UP_OUT, .barrier = 125};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result r[2][2], flat[2], cv, disc;   /* [payoff][antithetic] */
    int rc = MC_OK;
    for (int anti = 0; anti < 2 && rc == MC_OK; ++anti) {
        rc = mc_context_set_antithetic(ctx, anti);
        for (int payoff = 0; payoff < 2 && rc == MC_OK; ++payoff) {
            h.payoff = payoff ? MC_HESTON_PATH_BARRIER : MC_HESTON_PATH_ASIAN;
            rc = PATH_RUN(ctx, &h, MC_DEFAULT_SEED, 0, paths, &r[payoff][anti]);
        }
    }
    if (rc == MC_OK)
        rc = mc_context_set_antithetic(ctx, 0);
    /* the same contracts at constant variance v0 = 0.04, and at the constant volatility 0.2 */
    h.heston.xi = 0;
    h.heston.kappa = 0;
    for (int payoff = 0; payoff < 2 && rc == MC_OK; ++payoff) {
        h.payoff = payoff ? MC_HESTON_PATH_BARRIER : MC_HESTON_PATH_ASIAN;
        rc = PATH_RUN(ctx, &h, MC_DEFAULT_SEED, 0, paths, &flat[payoff]);
    }
    asian_t a = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0.2, .t = 1}, .n_dates = dates};
    barrier_t b = {.option = a.option, .barrier = 125, .n_dates = dates, .type = MC_BARRIER_UP_OUT, .monitoring = MC_MONITOR_DISCRETE};
    if (rc == MC_OK)
        rc = BARRIER_RUN(ctx, &b, MC_DEFAULT_SEED, 0, paths, &disc);
    if (rc == MC_OK)
        rc = mc_context_set_control_variate(ctx, 1);
    if (rc == MC_OK)
        rc = ASIAN_RUN(ctx, &a, MC_DEFAULT_SEED, 0, paths, &cv);
    if (rc != MC_OK) {
        fprintf(stderr, "hestonPathOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Heston path calls (%s): S=100 K=100 r=0.05 T=1 v0=0.04 kappa=2 theta=0.04 xi=0.3 rho=-0.7, dates=%d, steps_per_date=%d, paths=%llu\n",
           PRECISION, dates, spd, paths);
    line("asian_plain", &r[0][0], NULL);
    line("asian_antithetic", &r[0][1], &r[0][0]);
    line("up_out_plain", &r[1][0], NULL);
    line("up_out_antithetic", &r[1][1], &r[1][0]);
    printf("Constant variance (xi = kappa = 0, v0 = 0.04) next to the constant-volatility products (v = 0.2), B=125:\n");
    line("flat_asian", &flat[0], &cv);
    line("mc_asian", &cv, NULL);
    line("flat_up_out", &flat[1], &disc);
    line("mc_barrier", &disc, NULL);
    mc_context_destroy(ctx);
    return 0;
}
