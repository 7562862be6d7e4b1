/*
 * bookOpt.c -- a strike x maturity grid of European calls priced as ONE book (mc_vanilla_book_run_f64): one kernel launch for
 * the whole grid instead of one per option.  Prints, per option, the price, its confidence interval and the error against
 * Black-Scholes, then the microseconds per option of the call.  Plain C on the native ABI (include/mc_mi355x.h).
 *   bookOpt [paths per option]      (default 100000)
 */
#include "driver_util.h"
#include "mc_mi355x.h"

#include <math.h>

#define N_STRIKES 9
#define N_MATURITIES 4

static double bs_call(double s, double k, double r, double v, double t)
{
    const double d1 = (log(s / k) + (r + 0.5 * v * v) * t) / (v * sqrt(t)), d2 = d1 - v * sqrt(t);
    return s * 0.5 * erfc(-d1 / sqrt(2.0)) - k * exp(-r * t) * 0.5 * erfc(-d2 / sqrt(2.0));
}

int main(int argc, char **argv)
{
    const unsigned long long paths = argc > 1 ? strtoull(argv[1], NULL, 10) : 100000ull;
    const double maturities[N_MATURITIES] = {0.25, 0.5, 1.0, 2.0};
    mc_book_entry_f64 book[N_STRIKES * N_MATURITIES];
    mc_result out[N_STRIKES * N_MATURITIES];
    int count = 0;
    for (int m = 0; m < N_MATURITIES; ++m)
        for (int i = 0; i < N_STRIKES; ++i) {
            const mc_option_f64 o = {.s = 100.0, .k = 80.0 + 5.0 * i, .r = 0.05, .v = 0.2, .t = maturities[m]};
            book[count].option = o;
            book[count].seed = MC_DEFAULT_SEED;
            book[count].first_path = 0;
            book[count].n_paths = paths;
            ++count;
        }
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    int rc = mc_vanilla_book_run_f64(ctx, book, count, out);   /* the first call uploads the tables and sizes the buffers */
    const double t0 = now_s();
    if (rc == MC_OK)
        rc = mc_vanilla_book_run_f64(ctx, book, count, out);
    const double call_s = now_s() - t0;
    if (rc != MC_OK) {
        fprintf(stderr, "mc_vanilla_book_run_f64: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Vanilla book: %d calls (S=100, r=0.05, v=0.2), paths=%llu each, one launch\n", count, paths);
    for (int i = 0; i < count; ++i) {
        const mc_option_f64 *o = &book[i].option;
        const double bs = bs_call(o->s, o->k, o->r, o->v, o->t);
        printf("K=%g T=%g price=%.17g ci=%.6g bs_err=%.6g\n", o->k, o->t, out[i].expected, out[i].confidence, fabs(out[i].expected - bs));
    }
    printf("kernel %.3f ms, call %.3f ms: %.3f us per option\n", (double)out[0].kernel_ms, 1e3 * call_s, 1e6 * call_s / count);
    mc_context_destroy(ctx);
    return 0;
}
