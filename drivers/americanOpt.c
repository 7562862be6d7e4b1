/*
 * americanOpt.c -- the Bermudan put of Longstaff and Schwartz's Table 1 (k = 40, r = 0.06) in three of its cases: s = 36, v = 0.2,
 * t = 1 on 50 dates; s = 40, v = 0.4, t = 2 on 100 dates; s = 44, v = 0.2, t = 1 on 50 dates.  Per case the exercise rule is fitted on
 * 2^18 paths (mc_american_fit_*), then priced on fresh paths, plain and with antithetic variates (mc_american_run_*): a lower bound
 * of the price.  Beside them the fit's in-sample estimate (biased high), the binomial price of the same contract
 * (mc_american_lattice_*, 16 steps per date) and the European Black-Scholes put.  One line per figure: price, 95 % half-width,
 * kernel time.  Plain C on the native ABI (include/mc_mi355x.h); built per precision (americanOpt_f64, americanOpt_f32).
 *   americanOpt_f64 [paths]      (default 1000000 pricing paths)
 */
#include <math.h>

#include "driver_util.h"
#include "mc_mi355x.h"

#ifdef MC_SINGLE_PRECISION
typedef mc_american_f32 american_t;
#define AMERICAN_FIT mc_american_fit_f32
#define AMERICAN_RUN mc_american_run_f32
#define AMERICAN_LATTICE mc_american_lattice_f32
#define PRECISION "f32"
#else
typedef mc_american_f64 american_t;
#define AMERICAN_FIT mc_american_fit_f64
#define AMERICAN_RUN mc_american_run_f64
#define AMERICAN_LATTICE mc_american_lattice_f64
#define PRECISION "f64"
#endif

static double phi(double x) { return 0.5 * erfc(-x / sqrt(2.0)); }

int main(int argc, char **argv)
{
    static const char *const forms[2] = {"plain", "antithetic"};
    static const double spot[3] = {36, 40, 44}, vol[3] = {0.2, 0.4, 0.2}, mat[3] = {1, 2, 1};
    static const int dates[3] = {50, 100, 50};
    const unsigned long long paths = argc > 1 ? strtoull(argv[1], NULL, 10) : 1000000ull;
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    printf("Bermudan put (%s): K=40 r=0.06, rule fitted on 262144 paths (cubic in the payoff), priced on %llu paths\n", PRECISION, paths);
    for (int p = 0; p < 3; ++p) {
        american_t a = {.option = {.s = spot[p], .k = 40, .r = 0.06, .v = vol[p], .t = mat[p]}, .n_dates = dates[p], .type = MC_AMERICAN_PUT, .degree = 3};
        double beta[100 * 4], lattice = 0;
        mc_result fit, res[2];
        int rc = AMERICAN_FIT(ctx, &a, MC_DEFAULT_SEED, 0, 1ull << 18, beta, &fit);
        for (int f = 0; f < 2 && rc == MC_OK; ++f) {
            rc = mc_context_set_antithetic(ctx, f);
            if (rc == MC_OK)
                rc = AMERICAN_RUN(ctx, &a, beta, MC_DEFAULT_SEED, 0, paths, &res[f]);
        }
        if (rc == MC_OK)
            rc = mc_context_set_antithetic(ctx, 0);
        if (rc == MC_OK)
            rc = AMERICAN_LATTICE(&a, 16, &lattice);
        if (rc != MC_OK) {
            fprintf(stderr, "americanOpt: %s\n", mc_last_error());
            mc_context_destroy(ctx);
            return 1;
        }
        const double s = (double)a.option.s, k = (double)a.option.k, r = (double)a.option.r, v = (double)a.option.v, t = (double)a.option.t;
        const double sd = v * sqrt(t), d1 = (log(s / k) + (r + 0.5 * v * v) * t) / sd;
        const double european = k * exp(-r * t) * phi(sd - d1) - s * phi(-d1);
        printf("case %d: S=%g v=%g T=%g dates=%d\n", p, spot[p], vol[p], mat[p], dates[p]);
        for (int f = 0; f < 2; ++f)
            printf("case %d %s price=%.17g ci=%.6g kernel_ms=%.3f\n", p, forms[f], res[f].expected, res[f].confidence, (double)res[f].kernel_ms);
        printf("case %d in-sample price=%.17g ci=%.6g kernel_ms=%.3f\n", p, fit.expected, fit.confidence, (double)fit.kernel_ms);
        printf("case %d lattice price=%.17g ci=0 kernel_ms=0.000\n", p, lattice);
        printf("case %d european price=%.17g ci=0 kernel_ms=0.000\n", p, european);
    }
    mc_context_destroy(ctx);
    return 0;
}
