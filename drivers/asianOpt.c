/*
 * asianOpt.c -- an arithmetic-average (Asian) call priced twice on the same paths: plain Monte Carlo, and with the geometric
 * average as control variate (mc_context_set_control_variate; mc_asian_run_* adds the control's closed-form mean back).
 * Prints both prices with their 95 % half-widths, the closed-form price of the geometric-average call, and how much narrower
 * the controlled interval is.  Plain C on the native ABI (include/mc_mi355x.h); built per precision (asianOpt_f64, asianOpt_f32).
 *   asianOpt_f64 [dates] [paths]      (default 64 dates, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#include <math.h>

#ifdef MC_SINGLE_PRECISION
typedef mc_asian_f32 asian_t;
#define ASIAN_RUN mc_asian_run_f32
#define ASIAN_MEAN mc_asian_control_mean_f32
#define PRECISION "f32"
#else
typedef mc_asian_f64 asian_t;
#define ASIAN_RUN mc_asian_run_f64
#define ASIAN_MEAN mc_asian_control_mean_f64
#define PRECISION "f64"
#endif

int main(int argc, char **argv)
{
    const int dates = argc > 1 ? atoi(argv[1]) : 64;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    asian_t a = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0.2, .t = 1}, .n_dates = dates};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result plain, control;
    double mean = 0;
    const double t0 = now_s();
    int rc = ASIAN_RUN(ctx, &a, MC_DEFAULT_SEED, 0, paths, &plain);
    if (rc == MC_OK)
        rc = mc_context_set_control_variate(ctx, 1);
    if (rc == MC_OK)
        rc = ASIAN_RUN(ctx, &a, MC_DEFAULT_SEED, 0, paths, &control);
    const double calls_s = now_s() - t0;
    if (rc == MC_OK)
        rc = ASIAN_MEAN(&a, &mean);
    if (rc != MC_OK) {
        fprintf(stderr, "asianOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Asian call (%s): S=100 K=100 r=0.05 v=0.2 T=1, dates=%d, paths=%llu\n", PRECISION, dates, paths);
    printf("plain price=%.17g ci=%.6g kernel_ms=%.3f\n", plain.expected, plain.confidence, (double)plain.kernel_ms);
    printf("control price=%.17g ci=%.6g kernel_ms=%.3f\n", control.expected, control.confidence, (double)control.kernel_ms);
    printf("geometric closed_form=%.17g\n", exp(-(double)a.option.r * (double)a.option.t) * mean);
    printf("interval ratio plain/control=%.1f, both calls %.3f ms\n", plain.confidence / control.confidence, 1e3 * calls_s);
    mc_context_destroy(ctx);
    return 0;
}
