/*
 * mertonOpt.c -- calls under Merton's jump-diffusion on one market (mc_merton_run_*): the European call walked over 1 and over 16
 * dates next to its closed-form price (mc_merton_closed_form_*: the walk is exact in law, so both estimate the same number), the
 * arithmetic-average call and the up-and-out call monitored on the dates, each plain and with antithetic variates.  Prints one
 * line per product and form: price, 95 % half-width, kernel time.  Plain C on the native ABI (include/mc_mi355x.h); built per
 * precision (mertonOpt_f64, mertonOpt_f32).
 *   mertonOpt_f64 [dates] [paths]      (default 64 dates for the Asian and barrier calls, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_merton_f32 merton_t;
#define MERTON_RUN mc_merton_run_f32
#define MERTON_EXACT mc_merton_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_merton_f64 merton_t;
#define MERTON_RUN mc_merton_run_f64
#define MERTON_EXACT mc_merton_closed_form_f64
#define PRECISION "f64"
#endif

int main(int argc, char **argv)
{
    static const char *const names[4] = {"european-1", "european-16", "asian", "up-and-out"};
    static const char *const forms[2] = {"plain", "antithetic"};
    const int dates = argc > 1 ? atoi(argv[1]) : 64;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    printf("Merton jump-diffusion (%s): S=100 K=100 r=0.05 v=0.2 T=1 lambda=1 mu_j=-0.1 delta=0.15 barrier=130, dates=%d, paths=%llu\n",
           PRECISION, dates, paths);
    double exact = 0;
    for (int p = 0; p < 4; ++p) {
        merton_t b = {.option = {.s = 100, .k = 100, .r = 0.05, .v = 0.2, .t = 1}, .lambda = 1, .mu_j = -0.1, .delta = 0.15,
                      .n_dates = p == 0 ? 1 : p == 1 ? 16 : dates, .payoff = p < 2 ? MC_MERTON_EUROPEAN : p == 2 ? MC_MERTON_ASIAN : MC_MERTON_BARRIER,
                      .barrier_type = MC_BARRIER_UP_OUT, .barrier = 130};
        mc_result res[2];
        int rc = MC_OK;
        for (int f = 0; f < 2 && rc == MC_OK; ++f) {
            rc = mc_context_set_antithetic(ctx, f);
            if (rc == MC_OK)
                rc = MERTON_RUN(ctx, &b, MC_DEFAULT_SEED, 0, paths, &res[f]);
        }
        if (rc == MC_OK && p == 0)
            rc = MERTON_EXACT(&b, &exact);
        if (rc != MC_OK) {
            fprintf(stderr, "mertonOpt: %s\n", mc_last_error());
            mc_context_destroy(ctx);
            return 1;
        }
        for (int f = 0; f < 2; ++f)
            printf("%s %s price=%.17g ci=%.6g kernel_ms=%.3f\n", names[p], forms[f], res[f].expected, res[f].confidence, (double)res[f].kernel_ms);
        if (p == 1)
            printf("european closed_form price=%.17g ci=0 kernel_ms=0.000\n", exact);
    }
    mc_context_destroy(ctx);
    return 0;
}
