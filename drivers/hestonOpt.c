/*
 * hestonOpt.c -- a European call under the Heston stochastic-volatility model by full-truncation Euler (mc_heston_run_*), plain and
 * with antithetic variates on the same seed, next to the closed-form price of the continuous model (mc_heston_closed_form_*).
 * Prints one line per form: price, 95 % half-width, kernel time, and how many half-widths the estimate lies from the closed
 * form -- the scheme is biased, so that distance grows with the number of paths and shrinks with the number of steps.
 * Plain C on the native ABI (include/mc_mi355x.h); built per precision (hestonOpt_f64, hestonOpt_f32).
 *   hestonOpt_f64 [steps] [paths]      (default 64 steps, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_heston_f32 heston_t;
#define HESTON_RUN mc_heston_run_f32
#define HESTON_EXACT mc_heston_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_heston_f64 heston_t;
#define HESTON_RUN mc_heston_run_f64
#define HESTON_EXACT mc_heston_closed_form_f64
#define PRECISION "f64"
#endif

int main(int argc, char **argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 64;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    heston_t h = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0, .t = 1}, .v0 = 0.04, .kappa = 2, .theta = 0.04, .xi = 0.3, .rho = -0.7,
                  .n_steps = steps};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result plain, anti;
    double exact = 0;
    int rc = HESTON_RUN(ctx, &h, MC_DEFAULT_SEED, 0, paths, &plain);
    if (rc == MC_OK)
        rc = mc_context_set_antithetic(ctx, 1);
    if (rc == MC_OK)
        rc = HESTON_RUN(ctx, &h, MC_DEFAULT_SEED, 0, paths, &anti);
    if (rc == MC_OK)
        rc = HESTON_EXACT(&h, &exact);
    if (rc != MC_OK) {
        fprintf(stderr, "hestonOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Heston call (%s): S=100 K=100 r=0.05 T=1 v0=0.04 kappa=2 theta=0.04 xi=0.3 rho=-0.7, steps=%d, paths=%llu\n", PRECISION, steps, paths);
    printf("plain price=%.17g ci=%.6g kernel_ms=%.3f diff_in_ci=%.3f\n", plain.expected, plain.confidence, (double)plain.kernel_ms,
           (plain.expected - exact) / plain.confidence);
    printf("antithetic price=%.17g ci=%.6g kernel_ms=%.3f diff_in_ci=%.3f\n", anti.expected, anti.confidence, (double)anti.kernel_ms,
           (anti.expected - exact) / anti.confidence);
    printf("closed_form price=%.17g ci=0 kernel_ms=0.000 diff_in_ci=0\n", exact);
    mc_context_destroy(ctx);
    return 0;
}
