/*
 * lookbackOpt.c -- the four lookback options on one market, each priced on the same paths with the extremum taken on the dates
 * only and continuously, through the Brownian-bridge maxima between the dates (mc_lookback_run_*), plain and with antithetic
 * variates, next to the closed-form price of the continuously monitored option (mc_lookback_closed_form_*: Goldman-Sosin-Gatto,
 * Conze-Viswanathan).  Prints one line per type and form: price, 95 % half-width, kernel time.  Plain C on the native ABI
 * (include/mc_mi355x.h); built per precision (lookbackOpt_f64, lookbackOpt_f32).
 *   lookbackOpt_f64 [dates] [paths]      (default 64 dates, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_lookback_f32 lookback_t;
#define LOOKBACK_RUN mc_lookback_run_f32
#define LOOKBACK_EXACT mc_lookback_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_lookback_f64 lookback_t;
#define LOOKBACK_RUN mc_lookback_run_f64
#define LOOKBACK_EXACT mc_lookback_closed_form_f64
#define PRECISION "f64"
#endif

int main(int argc, char **argv)
{
    static const char *const kinds[4] = {"floating-call", "floating-put", "fixed-call", "fixed-put"};   /* MC_LOOKBACK_FLOAT_CALL ... */
    static const char *const forms[4] = {"discrete", "continuous", "antithetic_discrete", "antithetic_continuous"};
    const int dates = argc > 1 ? atoi(argv[1]) : 64;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    printf("Lookback options (%s): S=100 K=100 r=0.05 v=0.2 T=1, dates=%d, paths=%llu\n", PRECISION, dates, paths);
    for (int type = MC_LOOKBACK_FLOAT_CALL; type <= MC_LOOKBACK_FIXED_PUT; ++type) {
        lookback_t b = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0.2, .t = 1}, .n_dates = dates, .type = type};
        mc_result res[4];
        double exact = 0;
        int rc = MC_OK;
        for (int f = 0; f < 4 && rc == MC_OK; ++f) {
            b.monitoring = f & 1 ? MC_MONITOR_CONTINUOUS : MC_MONITOR_DISCRETE;
            rc = mc_context_set_antithetic(ctx, f >> 1);
            if (rc == MC_OK)
                rc = LOOKBACK_RUN(ctx, &b, MC_DEFAULT_SEED, 0, paths, &res[f]);
        }
        if (rc == MC_OK)
            rc = LOOKBACK_EXACT(&b, &exact);
        if (rc != MC_OK) {
            fprintf(stderr, "lookbackOpt: %s\n", mc_last_error());
            mc_context_destroy(ctx);
            return 1;
        }
        for (int f = 0; f < 4; ++f)
            printf("%s %s price=%.17g ci=%.6g kernel_ms=%.3f\n", kinds[type], forms[f], res[f].expected, res[f].confidence, (double)res[f].kernel_ms);
        printf("%s closed_form price=%.17g ci=0 kernel_ms=0.000\n", kinds[type], exact);
    }
    mc_context_destroy(ctx);
    return 0;
}
