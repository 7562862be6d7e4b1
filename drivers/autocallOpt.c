/*
 * autocallOpt.c -- a worst-of autocallable note with memory coupons and a knock-in put (mc_autocall_run_*): three assets on
 * performance levels, 5 years, 20 quarterly observations on a walk of 1260 dates; triggers stepping down from 1.00 by 0.01 per
 * observation, the first two observations not callable; coupon 0.02 per observation above 0.70, paid with the missed ones;
 * knock-in at 0.60 on every date, put struck at 1 with gearing 1.  Then the same note with the knock-in looked at on the last
 * date only; then the same note with every trigger infinite and no coupon, which is the discounted notional minus the worst-of
 * knock-in put, next to exp(-r t) - that put priced by mc_rainbow_run_* (another domain of the stream: the two agree within their
 * half-widths).  Prints one line per form, plain and with antithetic variates: price, 95 % half-width, kernel time.  Plain C on
 * the native ABI (include/mc_mi355x.h); built per precision (autocallOpt_f64, autocallOpt_f32).
 *   autocallOpt_f64 [paths]      (default 1000000 paths)
 */
#include <math.h>

#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_autocall_f32 autocall_t;
typedef mc_rainbow_f32 rainbow_t;
typedef float real_t;
#define AUTOCALL_RUN mc_autocall_run_f32
#define RAINBOW_RUN mc_rainbow_run_f32
#define PRECISION "f32"
#else
typedef mc_autocall_f64 autocall_t;
typedef mc_rainbow_f64 rainbow_t;
typedef double real_t;
#define AUTOCALL_RUN mc_autocall_run_f64
#define RAINBOW_RUN mc_rainbow_run_f64
#define PRECISION "f64"
#endif

#define N_OBS 20
#define N_DATES 1260

static void row(const char *name, const char *suffix, const mc_result *r)
{
    printf("%s%s price=%.17g ci=%.6g kernel_ms=%.3f\n", name, suffix, r->expected, r->confidence, (double)r->kernel_ms);
}

int main(int argc, char **argv)
{
    const unsigned long long paths = argc > 1 ? strtoull(argv[1], NULL, 10) : 1000000ull;
    /* performance levels: w = 1/s; p is the Cholesky factor of the correlations 0.5, 0.4, 0.6 */
    static const real_t s[3] = {100, 50, 200}, v[3] = {0.2, 0.3, 0.25}, w[3] = {0.01, 0.02, 0.005};
    static const real_t p[9] = {1, 0, 0, 0.5, 0.8660254037844386, 0, 0.4, 0.46188021535170065, 0.7916228058025279};
    real_t trigger[N_OBS], never[N_OBS], coupon_level[N_OBS];
    for (int k = 0; k < N_OBS; ++k) {
        trigger[k] = k < 2 ? (real_t)INFINITY : (real_t)(1.0 - 0.01 * k);
        never[k] = (real_t)INFINITY;
        coupon_level[k] = (real_t)0.7;
    }
    autocall_t note = {.basket = {.n = 3, .s = s, .v = v, .p = p, .d = NULL, .w = w, .k = 1, .t = 5, .r = 0.03}, .autocall = trigger,
                       .coupon_barrier = coupon_level, .coupon = (real_t)0.02, .barrier = (real_t)0.6, .gearing = 1, .n_dates = N_DATES,
                       .n_obs = N_OBS, .memory = 1, .ki_monitoring = MC_AUTOCALL_KI_DATES};
    rainbow_t put = {.basket = note.basket, .barrier = note.barrier, .n_dates = N_DATES, .type = MC_RAINBOW_PUT_ON_MIN, .barrier_type = MC_BARRIER_DOWN_IN};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result r[3][2], rainbow;
    int rc = MC_OK;
    for (int form = 0; form < 3 && rc == MC_OK; ++form) {
        autocall_t o = note;
        if (form == 1)
            o.ki_monitoring = MC_AUTOCALL_KI_MATURITY;
        if (form == 2)
            o.autocall = never, o.coupon = 0;
        for (int anti = 0; anti < 2 && rc == MC_OK; ++anti) {
            mc_context_set_antithetic(ctx, anti);
            rc = AUTOCALL_RUN(ctx, &o, MC_DEFAULT_SEED, 0, paths, &r[form][anti]);
        }
    }
    mc_context_set_antithetic(ctx, 0);
    if (rc == MC_OK)
        rc = RAINBOW_RUN(ctx, &put, MC_DEFAULT_SEED, 0, paths, &rainbow);
    if (rc != MC_OK) {
        fprintf(stderr, "autocallOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    static const char *names[3] = {"note", "note_ki_maturity", "no_trigger_no_coupon"};
    printf("Worst-of-3 autocallable note (%s): v=0.2,0.3,0.25 r=0.03 T=5, %d observations on %d dates, triggers 1.00 - 0.01 k from the third,\n"
           "coupon 0.02 above 0.70 with memory, knock-in 0.60, strike 1, gearing 1, paths=%llu\n", PRECISION, N_OBS, N_DATES, paths);
    for (int form = 0; form < 3; ++form) {
        row(names[form], "", &r[form][0]);
        row(names[form], "_antithetic", &r[form][1]);
    }
    /* exp(-r t) - gearing * the discounted worst-of down-and-in put, with the put's half-width */
    printf("from_rainbow_put price=%.17g ci=%.6g kernel_ms=%.3f\n", exp(-(double)note.basket.r * (double)note.basket.t) - rainbow.expected,
           rainbow.confidence, (double)rainbow.kernel_ms);
    mc_context_destroy(ctx);
    return 0;
}
