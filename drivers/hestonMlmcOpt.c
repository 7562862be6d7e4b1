/*
 * hestonMlmcOpt.c -- a European call under the Heston model (Feller's condition violated, out of the money) priced to a root-mean-square
 * error eps twice: by multilevel Monte Carlo on the Euler walk (mc_heston_mlmc_run_*: level 0 at 4 steps, level l at 4 * 2^l) and by ONE
 * level at the multilevel run's finest step count with N = 2 V / eps^2 paths (V from a pilot of that walk), next to the closed-form
 * price of the continuous model.  Prints one line per estimate -- price, standard error, kernel time, cost in path-steps, distance from
 * the closed form in units of eps -- and one line per level of the multilevel run.
 * Plain C on the native ABI (include/mc_mi355x.h); built per precision (hestonMlmcOpt_f64, hestonMlmcOpt_f32).
 *   hestonMlmcOpt_f64 [eps] [n_pilot]      (default eps 0.05, 10000 pilot paths)
 */
#include "driver_util.h"
#include "mc_mi355x.h"
#include <math.h>

#ifdef MC_SINGLE_PRECISION
typedef mc_heston_path_f32 path_t;
#define MLMC_RUN mc_heston_mlmc_run_f32
#define PATH_RUN mc_heston_path_run_f32
#define HESTON_EXACT mc_heston_closed_form_f32
#define PRECISION "f32"
#else
typedef mc_heston_path_f64 path_t;
#define MLMC_RUN mc_heston_mlmc_run_f64
#define PATH_RUN mc_heston_path_run_f64
#define HESTON_EXACT mc_heston_closed_form_f64
#define PRECISION "f64"
#endif

static double variance_of(const mc_result *r, double disc)
{
    const double n = (double)r->n;
    return disc * disc * (n * r->sum2 - r->sum * r->sum) / (n * (n - 1.0));
}

int main(int argc, char **argv)
{
    const double eps = argc > 1 ? atof(argv[1]) : 0.05;
    const unsigned long long n_pilot = argc > 2 ? strtoull(argv[2], NULL, 10) : 10000ull;
    path_t p = {.heston = {.option = {.s = 100, .k = 110, .r = 0.05, .v = 0, .t = 1}, .v0 = 0.02, .kappa = 1.5, .theta = 0.04, .xi = 0.6, .rho = -0.7,
                           .n_steps = 4},
                .steps_per_date = 4, .payoff = MC_HESTON_PATH_ASIAN};
    const mc_mlmc_spec spec = {.eps = eps, .min_levels = 2, .max_levels = 8, .n_pilot = n_pilot};
    const double disc = exp(-(double)p.heston.option.r * (double)p.heston.option.t);
    mc_context *ctx = NULL;
    if (mc_context_create(0, 0, &ctx) != MC_OK) {
        fprintf(stderr, "mc_context_create: %s\n", mc_last_error());
        return 1;
    }
    mc_mlmc_result ml;
    mc_result pilot, one;
    double exact = 0, cost = 0, kernel_ms = 0;
    path_t fine = p;
    unsigned long long n_one = 0;
    int rc = MLMC_RUN(ctx, &p, &spec, MC_DEFAULT_SEED, &ml);
    if (rc == MC_OK) {
        fine.heston.n_steps = fine.steps_per_date = p.heston.n_steps << (ml.levels - 1);
        rc = PATH_RUN(ctx, &fine, MC_DEFAULT_SEED, 1ull << 36, n_pilot, &pilot);
    }
    if (rc == MC_OK) {
        n_one = (unsigned long long)ceil(2.0 * variance_of(&pilot, disc) / (eps * eps));
        rc = PATH_RUN(ctx, &fine, MC_DEFAULT_SEED, 0, n_one < 2 ? 2 : n_one, &one);
    }
    if (rc == MC_OK)
        rc = HESTON_EXACT(&p.heston, &exact);
    if (rc != MC_OK) {
        fprintf(stderr, "hestonMlmcOpt: %s\n", mc_last_error());
        mc_context_destroy(ctx);
        return 1;
    }
    printf("Heston call (%s) to eps=%g: S=100 K=110 r=0.05 T=1 v0=0.02 kappa=1.5 theta=0.04 xi=0.6 rho=-0.7, level 0 at 4 steps, pilot=%llu\n", PRECISION,
           eps, n_pilot);
    for (int l = 0; l < ml.levels; ++l) {
        const mc_mlmc_level *v = &ml.level[l];
        const double steps = (l ? 1.5 : 1.0) * (double)(p.heston.n_steps << l);
        printf("level %d steps=%d paths=%llu mean=%.6f variance=%.6g kernel_ms=%.3f\n", l, p.heston.n_steps << l, (unsigned long long)v->n_paths,
               v->result.expected, variance_of(&v->result, disc), (double)v->result.kernel_ms);
        cost += steps * (double)v->n_paths, kernel_ms += (double)v->result.kernel_ms;
    }
    printf("mlmc price=%.17g stderr=%.6g kernel_ms=%.3f path_steps=%.6g err_in_eps=%.3f converged=%d bias=%.6g\n", ml.price, ml.stderr_, kernel_ms, cost,
           (ml.price - exact) / eps, ml.converged, ml.bias);
    printf("single price=%.17g stderr=%.6g kernel_ms=%.3f path_steps=%.6g err_in_eps=%.3f steps=%d paths=%llu\n", one.expected,
           sqrt(variance_of(&one, disc) / (double)one.n), (double)one.kernel_ms, (double)fine.heston.n_steps * (double)one.n, (one.expected - exact) / eps,
           fine.heston.n_steps, (unsigned long long)one.n);
    printf("closed_form price=%.17g stderr=0 kernel_ms=0.000 path_steps=0 err_in_eps=0\n", exact);
    mc_context_destroy(ctx);
    return 0;
}
