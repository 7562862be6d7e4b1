/*
 * localvolOpt.c -- calls and puts under a local-volatility surface (mc_localvol_run_*) on the displaced diffusion
 * sigma(t, S) = sd (S + a e^{-r (T - t)}) / S, sd = 0.2, a = 50, sampled on an 8 x 65 surface over ln(S / S0) in [-1.5, 1.5] at the slice
 * midpoints: the European call and put with antithetic variates next to the exact price of the continuous model (S + a e^{-r (T - t)} is
 * a geometric Brownian motion), the arithmetic-average call and the up-and-out call at B = 130 monitored on the dates, each plain
 * and with antithetic variates on the same seed; then a flat surface (0.2 everywhere) next to Black-Scholes.
 * Prints one line per form: price, 95 % half-width, kernel time, and the exact price or the distance to the plain form in units
 * of the two half-widths added.
 * Plain C on the native ABI (include/mc_mi355x.h); built per precision (localvolOpt_f64, localvolOpt_f32).
 *   localvolOpt_f64 [dates] [steps_per_date] [paths]      (default 16 dates x 4 steps, 1000000 paths; dates * steps_per_date must be a multiple of 8)
 */
#include <math.h>

#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_localvol_f32 lv_t;
typedef float real;
#define LV_RUN mc_localvol_run_f32
#define PRECISION "f32"
#else
typedef mc_localvol_f64 lv_t;
typedef double real;
#define LV_RUN mc_localvol_run_f64
#define PRECISION "f64"
#endif

enum { N_TIMES = 8, N_NODES = 65 };
static const double S0 = 100, K = 100, R = 0.03, T = 1, SD = 0.2, A = 50, Y_LO = -1.5, Y_HI = 1.5, B = 130;

static double phi(double x) { return 0.5 * erfc(-x / sqrt(2.0)); }

/* e^{-rT} [(F + a) Phi(d1) - (K + a) Phi(d2)], F = S0 e^{rT}; a = 0 is Black-Scholes */
static double displaced_call(double a)
{
    const double F = S0 * exp(R * T), sq = SD * sqrt(T), d1 = log((F + a) / (K + a)) / sq + 0.5 * sq;
    return exp(-R * T) * ((F + a) * phi(d1) - (K + a) * phi(d1 - sq));
}

static void line(const char *name, const mc_result *r, const mc_result *plain, const double *exact)
{
    printf("%s price=%.17g ci=%.6g kernel_ms=%.3f", name, r->expected, r->confidence, (double)r->kernel_ms);
    if (exact)
        printf(" exact=%.17g", *exact);
    if (plain)
        printf(" diff_in_ci=%.3f", (r->expected - plain->expected) / (r->confidence + plain->confidence));
    printf("\n");
}

int main(int argc, char **argv)
{
    const int dates = argc > 1 ? atoi(argv[1]) : 16, spd = argc > 2 ? atoi(argv[2]) : 4;
    const unsigned long long paths = argc > 3 ? strtoull(argv[3], NULL, 10) : 1000000ull;
    static real surface[N_TIMES * N_NODES], flat_surface[2];
    for (int q = 0; q < N_TIMES; ++q)
        for (int i = 0; i < N_NODES; ++i) {
            const double t = (q + 0.5) * T / N_TIMES, s = S0 * exp(Y_LO + (Y_HI - Y_LO) * i / (N_NODES - 1));
            surface[q * N_NODES + i] = (real)(SD * (s + A * exp(-R * (T - t))) / s);
        }
    flat_surface[0] = flat_surface[1] = (real)SD;
    lv_t v = {.option = {.s = S0, .k = K, .r = R, .v = 0, .t = T}, .sigma = surface, .n_times = N_TIMES, .n_nodes = N_NODES, .y_lo = Y_LO,
              .y_hi = Y_HI, .n_steps = dates * spd, .steps_per_date = spd, .payoff = MC_LOCALVOL_EUROPEAN, .right = MC_LOCALVOL_CALL,
              .barrier_type = MC_BARRIER_UP_OUT, .barrier = B};
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_result euro[2], r[2][2], flat;   /* [right], [payoff][antithetic] */
    int rc = MC_OK;
    for (int anti = 0; anti < 2 && rc == MC_OK; ++anti) {
        rc = mc_context_set_antithetic(ctx, anti);
        for (int payoff = 0; payoff < 2 && rc == MC_OK; ++payoff) {
            v.payoff = payoff ? MC_LOCALVOL_BARRIER : MC_LOCALVOL_ASIAN;
            rc = LV_RUN(ctx, &v, MC_DEFAULT_SEED, 0, paths, &r[payoff][anti]);
        }
    }
    v.payoff = MC_LOCALVOL_EUROPEAN;   /* antithetic still on */
    for (int right = 0; right < 2 && rc == MC_OK; ++right) {
        v.right = right ? MC_LOCALVOL_PUT : MC_LOCALVOL_CALL;
        rc = LV_RUN(ctx, &v, MC_DEFAULT_SEED, 0, paths, &euro[right]);
    }
    v.right = MC_LOCALVOL_CALL, v.sigma = flat_surface, v.n_times = 1, v.n_nodes = 2;
    if (rc == MC_OK)
        rc = LV_RUN(ctx, &v, MC_DEFAULT_SEED, 0, paths, &flat);
    if (rc != MC_OK) {
        fprintf(stderr, "localvolOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    const double call = displaced_call(A), put = call - S0 + K * exp(-R * T), bs = displaced_call(0);
    printf("Local volatility (%s): S=100 K=100 r=0.03 T=1, displaced diffusion sd=0.2 a=50 on an %d x %d surface over [%g, %g], dates=%d, "
           "steps_per_date=%d, paths=%llu\n", PRECISION, N_TIMES, N_NODES, Y_LO, Y_HI, dates, spd, paths);
    line("european_call", &euro[0], NULL, &call);
    line("european_put", &euro[1], NULL, &put);
    line("asian_plain", &r[0][0], NULL, NULL);
    line("asian_antithetic", &r[0][1], &r[0][0], NULL);
    line("up_out_plain", &r[1][0], NULL, NULL);
    line("up_out_antithetic", &r[1][1], &r[1][0], NULL);
    printf("Flat surface (0.2 everywhere, 1 x 2) next to Black-Scholes:\n");
    line("flat_call", &flat, NULL, &bs);
    mc_context_destroy(ctx);
    return 0;
}
