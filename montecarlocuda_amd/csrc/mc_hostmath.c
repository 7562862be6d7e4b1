/*
 * mc_hostmath.c -- the host-only part of the C ABI (include/mc_mi355x.h "host-side helpers"): plain C, no HIP.
 *
 * Compiled ONCE into an object that is linked into both libmc_mi355x.so (the GPU engine) and libmchost_*.so (the
 * OpenMP CPU twin), so that the CPU twin loads on a machine without the ROCm runtime (SURVEY 8f-3 "no-GPU fallback";
 * tests/test_build_deps.py checks its dynamic section).  What lives here:
 *   mc_closing               closing formulas, dp/MonteCarloKernel.cu:420-423 and :466-468
 *   mc_shard_range           SURVEY 8e partitioning
 *   mc_chol_*                dp/MonteCarloHost.c:90-105 semantics
 *   mc_factor_from_cov_*     SURVEY 8f-2
 *   mc_basket_control_mean_* closed-form mean of the geometric-basket control variate
 *   mc_asian_control_mean_*  closed-form mean of the geometric-average control variate of the Asian call
 *   mc_barrier_closed_form_* Reiner-Rubinstein price of the continuously monitored single-barrier call
 *   mc_lookback_closed_form_* Goldman-Sosin-Gatto / Conze-Viswanathan prices of the continuously monitored lookbacks
 *   mc_rainbow_closed_form_* Black-Scholes / Stulz prices of the worst-of and best-of options on one or two assets without a barrier
 *   mc_merton_closed_form_*  Merton's series for the European call under the jump-diffusion; mc_merton_thresholds_* the integer
 *                            Poisson thresholds of its count draw
 *   mc_american_solve        one date's regression of a Longstaff-Schwartz fit; mc_american_lattice_* the binomial price of the
 *                            Bermudan put or call
 *   mc_heston_closed_form_*  exact price of the European call under the Heston model (Gauss-Legendre quadrature)
 *   mc_last_error / mc_internal_fail   the per-thread error text of whichever library this object is linked into
 */
#include <complex.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/mc_mi355x.h"
#include "mc_hostmath.h"

static _Thread_local char g_last_error[640];

const char *mc_last_error(void) { return g_last_error; }

int mc_internal_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof g_last_error, fmt, ap);
    va_end(ap);
    return code;
}

void mc_closing(double sum, double sum2, uint64_t n, double discount, double *expected, double *confidence)
{
    const double dn = (double)n;
    if (expected) *expected = discount * (sum / dn);
    if (confidence) {
        const double dev = sqrt((dn * sum2 - sum * sum) / (dn * (double)(n - 1)));
        *confidence = 1.96 * dev / sqrt(dn);
    }
}

void mc_shard_range(uint64_t total, int rank, int world, uint64_t *first, uint64_t *count)
{
    if (world < 1) world = 1;
    if (rank < 0) rank = 0;
    if (rank >= world) rank = world - 1;
    /* floor(rank * total / world) without overflowing 64 bits */
    const unsigned __int128 t = total;
    const uint64_t lo = (uint64_t)(t * (unsigned)rank / (unsigned)world);
    const uint64_t hi = (uint64_t)(t * (unsigned)(rank + 1) / (unsigned)world);
    if (first) *first = lo;
    if (count) *count = hi - lo;
}

/* The exact Heston call price in fp64 (mc_heston_closed_form_*; inputs already checked, xi > 0).  Heston's decomposition
 *   C = S P1 - K e^{-rT} P2,   P_j = 1/2 + (1/pi) int_0^inf Re[ e^{-i u ln K} f_j(u) / (i u) ] du,
 * with the characteristic functions in the form whose complex logarithm never leaves the principal branch (Albrecher, Mayer,
 * Schoutens, Tistaert, "The little Heston trap"): beta = b_j - rho xi i u, d = sqrt(beta^2 - xi^2 (2 u_j i u - u^2)),
 * g = (beta - d)/(beta + d),
 *   f_j = exp( i u (ln S + r T) + (kappa theta / xi^2) [ (beta - d) T - 2 ln((1 - g e^{-dT})/(1 - g)) ]
 *              + (v0 / xi^2) (beta - d)(1 - e^{-dT})/(1 - g e^{-dT}) ),     u_1 = 1/2, u_2 = -1/2, b_1 = kappa - rho xi, b_2 = kappa.
 * Quadrature: 16-point Gauss-Legendre on panels of the fixed width h = 1/(4 sd), sd^2 = the mean variance over [0, T] times T
 * (the width of the integrand's bulk is 1/sd), from 0 until both integrands have stayed below 1e-18 for a whole panel
 * (at most 40000 panels; if the integrands have not decayed by then -- |rho| = 1 with a tiny variance decays slowly -- the
 * function returns NaN and the caller refuses).  beta - d cancels to relative 1e-16 kappa/xi^2: the result is good to ~1e-16 S (1 + kappa theta/xi^2). */
static double heston_call_fp64(double s, double k, double r, double t, double v0, double kappa, double theta, double xi, double rho)
{
    static const double gx[8] = {0.0950125098376374, 0.2816035507792589, 0.4580167776572274, 0.6178762444026438,
                                 0.7554044083550030, 0.8656312023878318, 0.9445750230732326, 0.9894009349916499};
    static const double gw[8] = {0.1894506104550685, 0.1826034150449236, 0.1691565193950025, 0.1495959888165767,
                                 0.1246289712555339, 0.0951585116824928, 0.0622535239386479, 0.0271524594117541};
    const double wbar = kappa * t > 1e-8 ? theta + (v0 - theta) * (1.0 - exp(-kappa * t)) / (kappa * t) : v0;
    const double sd = sqrt(fmax(wbar * t, 1e-6)), h = 0.25 / sd;
    const double x = log(s) + r * t, lk = log(k), xi2 = xi * xi;
    double acc[2] = {0.0, 0.0};
    int done = 0;
    for (int panel = 0; panel < 40000; ++panel) {
        const double mid = ((double)panel + 0.5) * h;
        double biggest = 0.0;
        for (int q = 0; q < 16; ++q) {
            const double u = mid + (q < 8 ? -gx[7 - q] : gx[q - 8]) * 0.5 * h, wq = gw[q < 8 ? 7 - q : q - 8] * 0.5 * h;
            for (int j = 0; j < 2; ++j) {
                const double uj = j ? -0.5 : 0.5, b = j ? kappa : kappa - rho * xi;
                const double complex beta = b - rho * xi * u * I;
                const double complex d = csqrt(beta * beta - xi2 * (2.0 * uj * u * I - u * u));
                const double complex g = (beta - d) / (beta + d), e = cexp(-d * t);
                const double complex lnf = u * (x - lk) * I + kappa * theta / xi2 * ((beta - d) * t - 2.0 * clog((1.0 - g * e) / (1.0 - g))) +
                                           v0 / xi2 * (beta - d) * (1.0 - e) / (1.0 - g * e);
                const double complex f = cexp(lnf) / (u * I);
                acc[j] += wq * creal(f);
                biggest = fmax(biggest, cabs(f));
            }
        }
        if (biggest < 1e-18) {
            done = 1;
            break;
        }
    }
    if (!done)
        return NAN;
    const double p1 = 0.5 + acc[0] / M_PI, p2 = 0.5 + acc[1] / M_PI;
    return s * p1 - k * exp(-r * t) * p2;
}

/* One date's regression of a Longstaff-Schwartz fit (the rule is stated in mc_mi355x.h). */
int mc_american_solve(const double *sums, int degree, double beta[4])
{
    if (!sums || !beta)
        return mc_internal_fail(MC_ERR_INVALID, "american solve: NULL argument");
    if (degree < 1 || degree > 3)
        return mc_internal_fail(MC_ERR_INVALID, "american solve: degree=%d outside [1, 3]", degree);
    const int n = degree + 1;
    double d[4], l[4][4], y[4];
    beta[0] = INFINITY, beta[1] = beta[2] = beta[3] = 0.0;
    if (!(sums[0] >= (double)MC_AMERICAN_MIN_ITM))
        return MC_OK;
    for (int i = 0; i < n; ++i) {
        if (!(sums[2 * i] > 0) || !isfinite(sums[2 * i]))
            return MC_OK;
        d[i] = sqrt(sums[2 * i]);
    }
    /* Cholesky of the scaled Gram matrix G_ik = sums[i + k] / (d_i d_k), row by row; its diagonal is 1 */
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k <= i; ++k) {
            double acc = sums[i + k] / (d[i] * d[k]);
            for (int q = 0; q < k; ++q)
                acc -= l[i][q] * l[k][q];
            if (k < i) {
                l[i][k] = acc / l[k][k];
            } else {
                if (!(acc > 0))
                    return MC_OK;
                l[i][i] = sqrt(acc);
            }
        }
    }
    for (int i = 0; i < n; ++i) {   /* L y = b / d */
        double acc = sums[7 + i] / d[i];
        for (int q = 0; q < i; ++q)
            acc -= l[i][q] * y[q];
        y[i] = acc / l[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {   /* L' x = y, beta = x / d */
        double acc = y[i];
        for (int q = i + 1; q < n; ++q)
            acc -= l[q][i] * y[q];
        y[i] = acc / l[i][i];
    }
    for (int i = 0; i < n; ++i)
        if (!isfinite(y[i] / d[i]))
            return MC_OK;
    for (int i = 0; i < n; ++i)
        beta[i] = y[i] / d[i];
    return MC_OK;
}

/* The Cox-Ross-Rubinstein price of the Bermudan put (q = -1) or call (q = +1) with exercise on every `every`-th of `steps` steps
 * (mc_american_lattice_*; inputs already checked).  NaN when the risk-neutral probability leaves (0, 1) or memory runs out. */
static double american_lattice_fp64(double s, double k, double r, double v, double t, double q, int steps, int every)
{
    const double h = t / (double)steps, lu = v * sqrt(h), grow = exp(r * h), u = exp(lu), dn = exp(-lu);
    const double pu = (grow - dn) / (u - dn), disc = 1.0 / grow;
    if (!(pu > 0 && pu < 1))
        return NAN;
    double *val = (double *)malloc(sizeof(double) * ((size_t)steps + 1));
    if (!val)
        return NAN;
    for (int i = 0; i <= steps; ++i)   /* node i of level n: spot s exp((2 i - n) lu) */
        val[i] = fmax(q * (s * exp((double)(2 * i - steps) * lu) - k), 0.0);
    for (int n = steps - 1; n >= 0; --n) {
        const int ex = n > 0 && n % every == 0;
        for (int i = 0; i <= n; ++i) {
            double c = disc * (pu * val[i + 1] + (1.0 - pu) * val[i]);
            if (ex)
                c = fmax(c, q * (s * exp((double)(2 * i - n) * lu) - k));
            val[i] = c;
        }
    }
    const double price = val[0];
    free(val);
    return price;
}

static double mc_norm_cdf(double x) { return 0.5 * erfc(-x / sqrt(2.0)); }

/* The bivariate normal distribution function M(a, b; rho) = P(X <= a, Y <= b), corr(X, Y) = rho, |rho| <= 1, in fp64
 * (mc_rainbow_closed_form_*).  Drezner and Wesolowsky's integral over the correlation in Genz's form ("Numerical computation of
 * rectangular bivariate and trivariate normal and t probabilities", 2004): for |rho| < 0.925 Gauss-Legendre on
 * int_0^{asin rho} exp(-(h^2 + k^2 - 2 h k sin x) / (2 cos^2 x)) dx; beyond it the integral from |rho| to 1 with the integrand's
 * singular part taken out in closed form.  Twenty points throughout. */
static double mc_binorm_cdf(double a, double b, double rho)
{
    static const double gx[10] = {0.076526521133497338, 0.2277858511416451,  0.37370608871541955, 0.51086700195082713, 0.63605368072651502,
                                  0.7463319064601508,   0.83911697182221878, 0.91223442825132584, 0.96397192727791381, 0.99312859918509488};
    static const double gw[10] = {0.15275338713072578, 0.14917298647260366,  0.14209610931838187,  0.13168863844917653,  0.11819453196151825,
                                  0.10193011981724026, 0.083276741576704671, 0.062672048334109443, 0.040601429800386217, 0.017614007139153273};
    const double twopi = 2.0 * M_PI;
    double h = -a, k = -b, hk = h * k, bvn = 0.0;   /* Genz computes P(X > h, Y > k) */
    if (fabs(rho) < 0.925) {
        if (rho != 0) {
            const double hs = 0.5 * (h * h + k * k), asr = asin(rho);
            for (int i = 0; i < 10; ++i)
                for (int is = -1; is <= 1; is += 2) {
                    const double sn = sin(asr * (is * gx[i] + 1.0) * 0.5);
                    bvn += gw[i] * exp((sn * hk - hs) / (1.0 - sn * sn));
                }
            bvn *= asr / (2.0 * twopi);
        }
        return bvn + mc_norm_cdf(-h) * mc_norm_cdf(-k);
    }
    if (rho < 0)
        k = -k, hk = -hk;
    if (fabs(rho) < 1) {
        const double as = (1.0 - rho) * (1.0 + rho), bs = (h - k) * (h - k), c = (4.0 - hk) / 8.0, d = (12.0 - hk) / 16.0;
        double a1 = sqrt(as), asr = -0.5 * (bs / as + hk);
        if (asr > -100)
            bvn = a1 * exp(asr) * (1.0 - c * (bs - as) * (1.0 - d * bs / 5.0) / 3.0 + c * d * as * as / 5.0);
        if (-hk < 100) {
            const double bb = sqrt(bs);
            bvn -= exp(-0.5 * hk) * sqrt(twopi) * mc_norm_cdf(-bb / a1) * bb * (1.0 - c * bs * (1.0 - d * bs / 5.0) / 3.0);
        }
        a1 *= 0.5;
        for (int i = 0; i < 10; ++i)
            for (int is = -1; is <= 1; is += 2) {
                const double x = a1 * (is * gx[i] + 1.0), xs = x * x, rs = sqrt(1.0 - xs);
                asr = -0.5 * (bs / xs + hk);
                if (asr > -100)
                    bvn += a1 * gw[i] * exp(asr) * (exp(-hk * xs / (2.0 * (1.0 + rs) * (1.0 + rs))) / rs - (1.0 + c * xs * (1.0 + d * xs)));
            }
        bvn = -bvn / twopi;
    }
    if (rho > 0)
        return bvn + mc_norm_cdf(-fmax(h, k));
    bvn = -bvn;
    if (k > h)
        bvn += mc_norm_cdf(k) - mc_norm_cdf(h);
    return bvn;
}

/* One body per precision: REAL, SQRT_R, X set by the includer below. */
#define MC_HM_CAT_(a, b) a##_##b
#define MC_HM_CAT(a, b) MC_HM_CAT_(a, b)
#define FN(name) MC_HM_CAT(name, X)

#define REAL float
#define SQRT_R sqrtf
#define X f32
#define BASKET mc_basket_f32
#define ASIAN mc_asian_f32
#define BARRIER mc_barrier_f32
#define LOOKBACK mc_lookback_f32
#define HESTON mc_heston_f32
#define MERTON mc_merton_f32
#define AMERICAN mc_american_f32
#define RAINBOW mc_rainbow_f32
#define LOCALVOL mc_localvol_f32
#define MERTON_BITS 32
#include "mc_hostmath_impl.h"
#undef REAL
#undef SQRT_R
#undef X
#undef BASKET
#undef ASIAN
#undef BARRIER
#undef LOOKBACK
#undef HESTON
#undef MERTON
#undef AMERICAN
#undef RAINBOW
#undef LOCALVOL
#undef MERTON_BITS

#define REAL double
#define SQRT_R sqrt
#define X f64
#define BASKET mc_basket_f64
#define ASIAN mc_asian_f64
#define BARRIER mc_barrier_f64
#define LOOKBACK mc_lookback_f64
#define HESTON mc_heston_f64
#define MERTON mc_merton_f64
#define AMERICAN mc_american_f64
#define RAINBOW mc_rainbow_f64
#define LOCALVOL mc_localvol_f64
#define MERTON_BITS 64
#include "mc_hostmath_impl.h"
#undef REAL
#undef SQRT_R
#undef X
#undef BASKET
#undef ASIAN
#undef BARRIER
#undef LOOKBACK
#undef HESTON
#undef MERTON
#undef AMERICAN
#undef RAINBOW
#undef LOCALVOL
#undef MERTON_BITS
