/*
 * rainbowOpt.c -- worst-of and best-of options on correlated assets walked over dates (mc_rainbow_run_*).  First a call on the
 * minimum of two assets at 1 and at 16 dates, plain and with antithetic variates, next to Stulz's closed form
 * (mc_rainbow_closed_form_*: a European payoff, so every date count prices the same contract); then a worst-of-3 knock-in put and
 * its knock-out twin, monitored on the dates, next to the put without a barrier, all three on the same paths (in + out = the
 * put).  Prints one line per form: price, 95 % half-width, kernel time.  Plain C on the native ABI (include/mc_mi355x.h); built
 * per precision (rainbowOpt_f64, rainbowOpt_f32).
 *   rainbowOpt_f64 [dates] [paths]      (default 16 dates, 1000000 paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_rainbow_f32 rainbow_t;
typedef float real_t;
#define RAINBOW_RUN mc_rainbow_run_f32
#define RAINBOW_EXACT mc_rainbow_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_rainbow_f64 rainbow_t;
typedef double real_t;
#define RAINBOW_RUN mc_rainbow_run_f64
#define RAINBOW_EXACT mc_rainbow_closed_form_f64
#define PRECISION "f64"
#endif

static void row(const char *name, const mc_result *r)
{
    printf("%s price=%.17g ci=%.6g kernel_ms=%.3f\n", name, r->expected, r->confidence, (double)r->kernel_ms);
}

int main(int argc, char **argv)
{
    const int dates = argc > 1 ? atoi(argv[1]) : 16;
    const unsigned long long paths = argc > 2 ? strtoull(argv[2], NULL, 10) : 1000000ull;
    /* performance levels: w = 1/s; the factors are the Cholesky factors of the correlations 0.5 (two assets) and 0.5, 0.4, 0.6 (three) */
    static const real_t s2[2] = {100, 50}, v2[2] = {0.2, 0.3}, w2[2] = {0.01, 0.02}, p2[4] = {1, 0, 0.5, 0.8660254037844386};
    static const real_t s3[3] = {100, 50, 200}, v3[3] = {0.2, 0.3, 0.25}, w3[3] = {0.01, 0.02, 0.005};
    static const real_t p3[9] = {1, 0, 0, 0.5, 0.8660254037844386, 0, 0.4, 0.46188021535170065, 0.7916228058025279};
    rainbow_t two = {.basket = {.n = 2, .s = s2, .v = v2, .p = p2, .d = NULL, .w = w2, .k = 1, .t = 1, .r = 0.03}, .barrier = 0, .n_dates = 1,
                     .type = MC_RAINBOW_CALL_ON_MIN, .barrier_type = MC_RAINBOW_NO_BARRIER};
    rainbow_t three = {.basket = {.n = 3, .s = s3, .v = v3, .p = p3, .d = NULL, .w = w3, .k = 1, .t = 1, .r = 0.03}, .barrier = 0.7, .n_dates = dates,
                       .type = MC_RAINBOW_PUT_ON_MIN, .barrier_type = MC_RAINBOW_NO_BARRIER};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result stulz[4], put, knock_in, knock_out;
    double exact = 0;
    int rc = MC_OK;
    for (int i = 0; i < 4 && rc == MC_OK; ++i) {   /* 1 date plain, 1 date antithetic, 16 dates plain, 16 dates antithetic */
        two.n_dates = i < 2 ? 1 : 16;
        mc_context_set_antithetic(ctx, i & 1);
        rc = RAINBOW_RUN(ctx, &two, MC_DEFAULT_SEED, 0, paths, &stulz[i]);
    }
    mc_context_set_antithetic(ctx, 0);
    if (rc == MC_OK)
        rc = RAINBOW_EXACT(&two, &exact);
    if (rc == MC_OK)
        rc = RAINBOW_RUN(ctx, &three, MC_DEFAULT_SEED, 0, paths, &put);
    three.barrier_type = MC_BARRIER_DOWN_IN;
    if (rc == MC_OK)
        rc = RAINBOW_RUN(ctx, &three, MC_DEFAULT_SEED, 0, paths, &knock_in);
    three.barrier_type = MC_BARRIER_DOWN_OUT;
    if (rc == MC_OK)
        rc = RAINBOW_RUN(ctx, &three, MC_DEFAULT_SEED, 0, paths, &knock_out);
    if (rc != MC_OK) {
        fprintf(stderr, "rainbowOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Call on the worse of two performances (%s): v=0.2,0.3 rho=0.5 K=1 r=0.03 T=1, paths=%llu\n", PRECISION, paths);
    row("min2_1_date", &stulz[0]);
    row("min2_1_date_antithetic", &stulz[1]);
    row("min2_16_dates", &stulz[2]);
    row("min2_16_dates_antithetic", &stulz[3]);
    printf("closed_form price=%.17g ci=0 kernel_ms=0.000\n", exact);
    printf("Worst-of-3 put (%s): v=0.2,0.3,0.25 K=1 r=0.03 T=1, down barrier 0.7 on the worst performance, dates=%d, paths=%llu\n", PRECISION, dates, paths);
    row("worst3_put", &put);
    row("worst3_knock_in", &knock_in);
    row("worst3_knock_out", &knock_out);
    mc_context_destroy(ctx);
    return 0;
}
