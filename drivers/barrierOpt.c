/*
 * barrierOpt.c -- an up-and-out barrier call priced twice on the same paths: monitored on the dates only, and continuously
 * through the Brownian-bridge survival probability between the dates (mc_barrier_run_*), next to the closed-form price of the
 * continuously monitored call (mc_barrier_closed_form_*, Reiner-Rubinstein).  Prints one line per form: price, 95 % half-width,
 * kernel time.  Plain C on the native ABI (include/mc_mi355x.h); built per precision (barrierOpt_f64, barrierOpt_f32).
 *   barrierOpt_f64 [dates] [paths]      (default 64 dates, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_barrier_f32 barrier_t;
#define BARRIER_RUN mc_barrier_run_f32
#define BARRIER_EXACT mc_barrier_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_barrier_f64 barrier_t;
#define BARRIER_RUN mc_barrier_run_f64
#define BARRIER_EXACT mc_barrier_closed_form_f64
#define PRECISION "f64"
#endif

int main(int argc, char **argv)
{
    const int dates = argc > 1 ? atoi(argv[1]) : 64;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    barrier_t b = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0.2, .t = 1}, .barrier = 120, .n_dates = dates,
                   .type = MC_BARRIER_UP_OUT, .monitoring = MC_MONITOR_DISCRETE};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result discrete, continuous;
    double exact = 0;
    int rc = BARRIER_RUN(ctx, &b, MC_DEFAULT_SEED, 0, paths, &discrete);
    b.monitoring = MC_MONITOR_CONTINUOUS;
    if (rc == MC_OK)
        rc = BARRIER_RUN(ctx, &b, MC_DEFAULT_SEED, 0, paths, &continuous);
    if (rc == MC_OK)
        rc = BARRIER_EXACT(&b, &exact);
    if (rc != MC_OK) {
        fprintf(stderr, "barrierOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Up-and-out call (%s): S=100 K=100 r=0.05 v=0.2 T=1 B=120, dates=%d, paths=%llu\n", PRECISION, dates, paths);
    printf("discrete price=%.17g ci=%.6g kernel_ms=%.3f\n", discrete.expected, discrete.confidence, (double)discrete.kernel_ms);
    printf("continuous price=%.17g ci=%.6g kernel_ms=%.3f\n", continuous.expected, continuous.confidence, (double)continuous.kernel_ms);
    printf("closed_form price=%.17g ci=0 kernel_ms=0.000\n", exact);
    mc_context_destroy(ctx);
    return 0;
}
