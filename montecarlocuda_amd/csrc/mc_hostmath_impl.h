/* mc_hostmath_impl.h -- precision-generic body of mc_hostmath.c (REAL, SQRT_R, X, BASKET set by the includer). */

/* Cholesky with the reference's semantics (dp/MonteCarloHost.c:90-105: column by column, a non-positive pivot leaves
 * its column zero).  Returns the number of non-positive pivots met. */
int FN(mc_chol)(int n, const REAL *c, REAL *a)
{
    if (n < 1 || !c || !a)
        return -1;
    REAL *work = (REAL *)malloc(sizeof(REAL) * (size_t)n);
    if (!work)
        return -1;
    int bad = 0;
    for (int col = 0; col < n; ++col) {
        for (int row = 0; row < n; ++row) {
            a[row * n + col] = 0;
            if (row < col)
                continue;
            work[row] = c[row * n + col];
            for (int q = 0; q < col; ++q)
                work[row] -= a[col * n + q] * a[row * n + q];
            if (work[col] > 0)
                a[row * n + col] = work[row] / SQRT_R(work[col]);
            else if (row == col)
                ++bad;
        }
    }
    free(work);
    return bad;
}

/* Covariance input.  The reference's drivers hold volatilities and a CORRELATION matrix and factor
 * the latter with Chol before either path runs (dp/basketOpt.cu:34-61,96-99); a caller who holds the covariance of
 * the annualised log-returns gets both inputs of the basket structs from it here: v_a = sqrt(cov_aa), correlation
 * cov_ab / (v_a v_b) with an exact unit diagonal, then Chol's factorisation (same arithmetic, same zero-pivot rule,
 * dp/MonteCarloHost.c:90-105).  Like Chol, only the lower triangle of the input is read.  All in REAL. */
int FN(mc_factor_from_cov)(int n, const REAL *cov, REAL *v, REAL *p)
{
    if (n < 1 || !cov || !v || !p)
        return -1;
    for (int a = 0; a < n; ++a) {
        const REAL var = cov[a * n + a];
        if (!(var > 0) || !isfinite((double)var))
            return -1;   /* no volatility to extract */
        v[a] = SQRT_R(var);
    }
    REAL *corr = (REAL *)calloc((size_t)n * (size_t)n, sizeof(REAL));
    if (!corr)
        return -1;
    for (int a = 0; a < n; ++a) {
        corr[(size_t)a * n + a] = 1;
        for (int b = 0; b < a; ++b) {
            const REAL c = cov[a * n + b];
            if (!isfinite((double)c)) {
                free(corr);
                return -1;
            }
            corr[(size_t)a * n + b] = corr[(size_t)b * n + a] = c / (v[a] * v[b]);
        }
    }
    const int bad = FN(mc_chol)(n, corr, p);
    free(corr);
    return bad;
}

/* E[max(G - K, 0)] of the geometric-basket control, closed form in fp64 (see mc_mi355x.h) */
int FN(mc_basket_control_mean)(const BASKET *o, double *mean)
{
    if (!o)
        return mc_internal_fail(MC_ERR_INVALID, "NULL basket");
    if (!mean || o->n < 1 || o->n > MC_MAX_ASSETS_GENERIC || !o->s || !o->v || !o->p || !o->d || !o->w)
        return mc_internal_fail(MC_ERR_INVALID, "control variate: bad basket");
    const int n = o->n;
    double W = 0;
    for (int a = 0; a < n; ++a) {
        if (!((double)o->w[a] > 0) || !((double)o->s[a] > 0))
            return mc_internal_fail(MC_ERR_INVALID, "control variate: needs w[a] > 0 and s[a] > 0 for every asset");
        W += (double)o->w[a];
    }
    if (!((double)o->k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "control variate: needs k > 0");
    const double sqrt_t = sqrt((double)o->t);
    double m = log(W), var = 0;
    for (int a = 0; a < n; ++a) {
        const double va = (double)o->v[a];
        m += (double)o->w[a] / W * (log((double)o->s[a]) + ((double)o->r - 0.5 * va * va) * (double)o->t + va * sqrt_t * (double)o->d[a]);
    }
    for (int b = 0; b < n; ++b) {
        double cb = 0;
        for (int a = b; a < n; ++a)
            cb += (double)o->w[a] / W * (double)o->v[a] * sqrt_t * (double)o->p[a * n + b];
        var += cb * cb;
    }
    const double sd = sqrt(var);
    if (sd == 0) {
        const double g = exp(m) - (double)o->k;
        *mean = g > 0 ? g : 0;
        return MC_OK;
    }
    const double d1 = (m - log((double)o->k) + var) / sd, d2 = d1 - sd;
    *mean = exp(m + 0.5 * var) * 0.5 * erfc(-d1 / sqrt(2.0)) - (double)o->k * 0.5 * erfc(-d2 / sqrt(2.0));
    return MC_OK;
}

/* E[max(G - K, 0)] of the geometric-average control of the Asian call, closed form in fp64 (see mc_mi355x.h):
 * ln G = ln S0 + a (m + 1)/2 + (bx/m) sum_j W_j, and sum_j W_j = sum_i (m - i + 1) z_i has variance m (m + 1)(2m + 1)/6 */
int FN(mc_asian_control_mean)(const ASIAN *o, double *mean)
{
    if (!o || !mean)
        return mc_internal_fail(MC_ERR_INVALID, "asian control variate: NULL argument");
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    if (o->n_dates < 1 || o->n_dates > MC_MAX_ASIAN_DATES)
        return mc_internal_fail(MC_ERR_INVALID, "asian: n_dates=%d outside [1, %d]", o->n_dates, MC_MAX_ASIAN_DATES);
    if (!(s > 0) || !(t > 0) || !isfinite(s) || !isfinite(t) || !isfinite(r) || !isfinite(v) || !isfinite(k))
        return mc_internal_fail(MC_ERR_INVALID, "asian: need s>0, t>0 and finite inputs");
    if (!(k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "asian control variate: needs k > 0");
    if (!(v > 0))
        return mc_internal_fail(MC_ERR_INVALID, v == 0 ? "asian control variate: needs v != 0 (v == 0 leaves nothing to control)"
                                                       : "asian: need v >= 0");
    const double m = (double)o->n_dates, dt = t / m;
    const double mu = log(s) + (r - 0.5 * v * v) * dt * (m + 1.0) * 0.5;
    const double var = v * v * dt * (m + 1.0) * (2.0 * m + 1.0) / (6.0 * m), sd = sqrt(var);
    const double d1 = (mu - log(k) + var) / sd, d2 = d1 - sd;
    *mean = exp(mu + 0.5 * var) * 0.5 * erfc(-d1 / sqrt(2.0)) - k * 0.5 * erfc(-d2 / sqrt(2.0));
    return MC_OK;
}

/* The inputs every barrier entry point refuses (see mc_mi355x.h); need_vol: the forms that divide by v.  Internal
 * (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_barrier_check)(const BARRIER *o, int need_vol)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    const double b = (double)o->barrier;
    if (o->n_dates < 1 || o->n_dates > MC_MAX_BARRIER_DATES)
        return mc_internal_fail(MC_ERR_INVALID, "barrier: n_dates=%d outside [1, %d]", o->n_dates, MC_MAX_BARRIER_DATES);
    if (o->type < MC_BARRIER_UP_OUT || o->type > MC_BARRIER_DOWN_IN)
        return mc_internal_fail(MC_ERR_INVALID, "barrier: type=%d is none of MC_BARRIER_UP_OUT ... MC_BARRIER_DOWN_IN", o->type);
    if (o->monitoring != MC_MONITOR_DISCRETE && o->monitoring != MC_MONITOR_CONTINUOUS)
        return mc_internal_fail(MC_ERR_INVALID, "barrier: monitoring=%d is neither MC_MONITOR_DISCRETE nor MC_MONITOR_CONTINUOUS", o->monitoring);
    if (!(s > 0) || !(t > 0) || !(b > 0) || !(v >= 0) || !isfinite(s) || !isfinite(t) || !isfinite(b) || !isfinite(r) || !isfinite(v) || !isfinite(k))
        return mc_internal_fail(MC_ERR_INVALID, "barrier: need s>0, t>0, barrier>0, v>=0 and finite inputs");
    if (o->type <= MC_BARRIER_UP_IN ? s >= b : s <= b)
        return mc_internal_fail(MC_ERR_INVALID, "barrier: the spot %g is on or beyond the %s barrier %g: the product is then the vanilla call or nothing",
                                s, o->type <= MC_BARRIER_UP_IN ? "up" : "down", b);
    if (need_vol && !(v > 0))
        return mc_internal_fail(MC_ERR_INVALID, "barrier: continuous monitoring needs v != 0");
    return MC_OK;
}

/* Discounted Reiner-Rubinstein price of the continuously monitored single-barrier call, no dividend, no rebate (Haug's
 * terms A, B, C, D with phi = 1 and eta = +1 for a down, -1 for an up barrier), fp64, Phi by erfc. */
int FN(mc_barrier_closed_form)(const BARRIER *o, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "barrier closed form: NULL argument");
    int rc = FN(mc_barrier_check)(o, 1);
    if (rc != MC_OK)
        return rc;
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    const double b = (double)o->barrier;
    if (!(k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "barrier closed form: needs k > 0");
    const int up = o->type <= MC_BARRIER_UP_IN, in = o->type == MC_BARRIER_UP_IN || o->type == MC_BARRIER_DOWN_IN;
    const double eta = up ? -1.0 : 1.0;
    const double sd = v * sqrt(t), mu = (r - 0.5 * v * v) / (v * v), shift = (1.0 + mu) * sd, kd = k * exp(-r * t);
    const double x1 = log(s / k) / sd + shift, x2 = log(s / b) / sd + shift;
    const double y1 = log(b * b / (s * k)) / sd + shift, y2 = log(b / s) / sd + shift;
    const double pw = exp(2.0 * mu * log(b / s)), pw1 = pw * (b / s) * (b / s);   /* (B/S)^(2 mu), (B/S)^(2 mu + 2) */
#define MC_PHI(x) (0.5 * erfc(-(x) / sqrt(2.0)))
    const double A = s * MC_PHI(x1) - kd * MC_PHI(x1 - sd);
    const double B = s * MC_PHI(x2) - kd * MC_PHI(x2 - sd);
    const double Cc = s * pw1 * MC_PHI(eta * y1) - kd * pw * MC_PHI(eta * (y1 - sd));
    const double D = s * pw1 * MC_PHI(eta * y2) - kd * pw * MC_PHI(eta * (y2 - sd));
#undef MC_PHI
    double in_price;   /* the knock-in call; the knock-out call is the vanilla call A minus it */
    if (up)
        in_price = k >= b ? A : B - Cc + D;
    else
        in_price = k >= b ? Cc : A - B + D;
    *price = in ? in_price : A - in_price;
    return MC_OK;
}

/* The inputs every rainbow entry point refuses (see mc_mi355x.h); with_dates: the walk's own (the closed form ignores n_dates).
 * Internal (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_rainbow_check)(const RAINBOW *o, int with_dates)
{
    const BASKET *b = &o->basket;
    const int n = b->n;
    if (n < 1 || n > MC_MAX_RAINBOW_ASSETS)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: n=%d outside [1, %d]", n, MC_MAX_RAINBOW_ASSETS);
    if (!b->s || !b->v || !b->p || !b->w)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: NULL s, v, p or w");
    if (with_dates && (o->n_dates < 1 || (long long)n * o->n_dates > MC_MAX_RAINBOW_TABLE))
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: n_dates=%d outside [1, %d / n]", o->n_dates, MC_MAX_RAINBOW_TABLE);
    if (o->type < MC_RAINBOW_CALL_ON_MIN || o->type > MC_RAINBOW_PUT_ON_MAX)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: type=%d is none of MC_RAINBOW_CALL_ON_MIN ... MC_RAINBOW_PUT_ON_MAX", o->type);
    if (o->barrier_type < MC_RAINBOW_NO_BARRIER || o->barrier_type > MC_BARRIER_DOWN_IN)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: barrier_type=%d is neither MC_RAINBOW_NO_BARRIER nor one of MC_BARRIER_UP_OUT ... MC_BARRIER_DOWN_IN",
                                o->barrier_type);
    const double k = (double)b->k, r = (double)b->r, t = (double)b->t;
    if (!(t > 0) || !isfinite(t) || !isfinite(r) || !isfinite(k))
        return mc_internal_fail(MC_ERR_INVALID, "rainbow: need t>0 and finite k, r, t");
    const int use_max = o->type == MC_RAINBOW_CALL_ON_MAX || o->type == MC_RAINBOW_PUT_ON_MAX;
    double ext = 0;
    for (int i = 0; i < n; ++i) {
        const double s = (double)b->s[i], w = (double)b->w[i], v = (double)b->v[i];
        if (!(s > 0) || !(w > 0) || !(v >= 0) || !isfinite(s) || !isfinite(w) || !isfinite(v))
            return mc_internal_fail(MC_ERR_INVALID, "rainbow: need s[i]>0, w[i]>0, v[i]>=0 and finite inputs (asset %d)", i);
        if (b->d && (double)b->d[i] != 0)
            return mc_internal_fail(MC_ERR_INVALID, "rainbow: d[%d] is not zero: a shift of the terminal normals has no meaning on a walk", i);
        for (int q = 0; q <= i; ++q)
            if (!isfinite((double)b->p[i * n + q]))
                return mc_internal_fail(MC_ERR_INVALID, "rainbow: p[%d][%d] is not finite", i, q);
        const double level = w * s;
        ext = i == 0 ? level : use_max ? fmax(ext, level) : fmin(ext, level);
    }
    if (o->barrier_type != MC_RAINBOW_NO_BARRIER) {
        const double B = (double)o->barrier;
        const int up = o->barrier_type <= MC_BARRIER_UP_IN;
        if (!(B > 0) || !isfinite(B))
            return mc_internal_fail(MC_ERR_INVALID, "rainbow: need a finite barrier > 0");
        if (up ? ext >= B : ext <= B)
            return mc_internal_fail(MC_ERR_INVALID, "rainbow: the initial %s level %g is on or beyond the %s barrier %g", use_max ? "best" : "worst", ext,
                                    up ? "up" : "down", B);
    }
    return MC_OK;
}

/* Discounted price of the rainbow contract without a barrier at n = 1 (Black-Scholes) and n = 2 (Stulz), fp64; the formulas are
 * stated in mc_mi355x.h. */
int FN(mc_rainbow_closed_form)(const RAINBOW *o, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: NULL argument");
    int rc = FN(mc_rainbow_check)(o, 0);
    if (rc != MC_OK)
        return rc;
    const BASKET *b = &o->basket;
    if (b->n > 2)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: n=%d, only 1 or 2 assets have one", b->n);
    if (o->barrier_type != MC_RAINBOW_NO_BARRIER)
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: none with a barrier");
    const double k = (double)b->k, r = (double)b->r, t = (double)b->t, st = sqrt(t), kd = k * exp(-r * t);
    const int call = o->type <= MC_RAINBOW_CALL_ON_MAX, use_max = o->type == MC_RAINBOW_CALL_ON_MAX || o->type == MC_RAINBOW_PUT_ON_MAX;
    if (!(k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: needs k > 0");
    double S[2], v[2], y[2], bs[2];
    for (int i = 0; i < b->n; ++i) {
        S[i] = (double)b->w[i] * (double)b->s[i], v[i] = (double)b->v[i];
        if (!(v[i] > 0))
            return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: needs v[%d] > 0", i);
        y[i] = (log(S[i] / k) + (r + 0.5 * v[i] * v[i]) * t) / (v[i] * st);
        bs[i] = S[i] * mc_norm_cdf(y[i]) - kd * mc_norm_cdf(y[i] - v[i] * st);   /* the Black-Scholes call on asset i */
    }
    /* the walk takes M = diag(v sqrt dt) L with L as given; the formulas price the model in which L is the factor of a CORRELATION
     * matrix, rows of unit length (up to the rounding of an fp32 factor): any other factor is refused, not renormalised */
    const double p00 = (double)b->p[0], p10 = b->n == 2 ? (double)b->p[2] : 0.0, p11 = b->n == 2 ? (double)b->p[3] : 1.0;
    if (!(fabs(p00 * p00 - 1.0) <= 1e-5) || !(fabs(p10 * p10 + p11 * p11 - 1.0) <= 1e-5))
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: a row of p is not of unit length: p is not the factor of a correlation matrix");
    if (b->n == 1) {
        *price = call ? bs[0] : bs[0] - S[0] + kd;
        return MC_OK;
    }
    const double rho = (p00 < 0 ? -p10 : p10) / sqrt(p10 * p10 + p11 * p11);   /* L_10 L_00, the rounding of the row's length taken out */
    const double s2 = v[0] * v[0] + v[1] * v[1] - 2.0 * rho * v[0] * v[1], sg = sqrt(s2 > 0 ? s2 : 0);
    if (!(sg * st >= 1e-8) || !(sg >= 1e-3 * (v[0] + v[1])))
        return mc_internal_fail(MC_ERR_INVALID, "rainbow closed form: the two assets move as one (sigma=%g): price the single asset", sg);
    const double d = (log(S[0] / S[1]) + 0.5 * s2 * t) / (sg * st);
    const double rho1 = fmax(-1.0, fmin(1.0, (v[0] - rho * v[1]) / sg)), rho2 = fmax(-1.0, fmin(1.0, (v[1] - rho * v[0]) / sg));
    const double cmin = S[0] * mc_binorm_cdf(y[0], -d, -rho1) + S[1] * mc_binorm_cdf(y[1], d - sg * st, -rho2) -
                        kd * mc_binorm_cdf(y[0] - v[0] * st, y[1] - v[1] * st, rho);
    const double margrabe = S[0] * mc_norm_cdf(d) - S[1] * mc_norm_cdf(d - sg * st);   /* PV of max(S_1 - S_2, 0) */
    const double c = use_max ? bs[0] + bs[1] - cmin : cmin, pv = use_max ? S[1] + margrabe : S[0] - margrabe;
    *price = call ? c : c - pv + kd;
    return MC_OK;
}

/* The inputs every lookback entry point refuses (see mc_mi355x.h).  Internal (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_lookback_check)(const LOOKBACK *o)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    if (o->n_dates < 1 || o->n_dates > MC_MAX_LOOKBACK_DATES)
        return mc_internal_fail(MC_ERR_INVALID, "lookback: n_dates=%d outside [1, %d]", o->n_dates, MC_MAX_LOOKBACK_DATES);
    if (o->type < MC_LOOKBACK_FLOAT_CALL || o->type > MC_LOOKBACK_FIXED_PUT)
        return mc_internal_fail(MC_ERR_INVALID, "lookback: type=%d is none of MC_LOOKBACK_FLOAT_CALL ... MC_LOOKBACK_FIXED_PUT", o->type);
    if (o->monitoring != MC_MONITOR_DISCRETE && o->monitoring != MC_MONITOR_CONTINUOUS)
        return mc_internal_fail(MC_ERR_INVALID, "lookback: monitoring=%d is neither MC_MONITOR_DISCRETE nor MC_MONITOR_CONTINUOUS", o->monitoring);
    if (!(s > 0) || !(t > 0) || !(v >= 0) || !isfinite(s) || !isfinite(t) || !isfinite(r) || !isfinite(v))
        return mc_internal_fail(MC_ERR_INVALID, "lookback: need s>0, t>0, v>=0 and finite inputs");
    if (o->type >= MC_LOOKBACK_FIXED_CALL && (!(k > 0) || !isfinite(k)))
        return mc_internal_fail(MC_ERR_INVALID, "lookback: the fixed-strike types need a finite k > 0");
    if (o->monitoring == MC_MONITOR_CONTINUOUS && !(v > 0))
        return mc_internal_fail(MC_ERR_INVALID, "lookback: continuous monitoring needs v != 0");
    return MC_OK;
}

/* Discounted price at inception of the continuously monitored lookback (Goldman-Sosin-Gatto for the floating strikes,
 * Conze-Viswanathan for the fixed ones; no dividend), fp64, Phi by erfc.  The formulas are stated in mc_mi355x.h. */
int FN(mc_lookback_closed_form)(const LOOKBACK *o, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "lookback closed form: NULL argument");
    LOOKBACK one = *o;
    one.n_dates = 1, one.monitoring = MC_MONITOR_CONTINUOUS;   /* both ignored here; v > 0 is needed */
    int rc = FN(mc_lookback_check)(&one);
    if (rc != MC_OK)
        return rc;
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    if (r == 0)
        return mc_internal_fail(MC_ERR_INVALID, "lookback closed form: the limit r -> 0 is not implemented");
#define MC_PHI(x) (0.5 * erfc(-(x) / sqrt(2.0)))
    const double D = exp(-r * t), G = exp(r * t), sd = v * sqrt(t), c = v * v / (2.0 * r), g = 2.0 * r * sqrt(t) / v;
    const double a1 = (r + 0.5 * v * v) * sqrt(t) / v, a2 = a1 - sd;
    const double float_call = s * MC_PHI(a1) - s * D * MC_PHI(a2) + s * D * c * (MC_PHI(g - a1) - G * MC_PHI(-a1));
    const double float_put = s * D * MC_PHI(-a2) - s * MC_PHI(-a1) + s * D * c * (G * MC_PHI(a1) - MC_PHI(a1 - g));
    double out;
    if (o->type == MC_LOOKBACK_FLOAT_CALL) {
        out = float_call;
    } else if (o->type == MC_LOOKBACK_FLOAT_PUT) {
        out = float_put;
    } else {
        const double d1 = (log(s / k) + (r + 0.5 * v * v) * t) / sd, p = exp(-2.0 * r / (v * v) * log(s / k));
        if (o->type == MC_LOOKBACK_FIXED_CALL)
            out = k <= s ? float_put + s - D * k
                         : s * MC_PHI(d1) - k * D * MC_PHI(d1 - sd) + s * D * c * (G * MC_PHI(d1) - p * MC_PHI(d1 - g));
        else
            out = k >= s ? float_call - s + D * k
                         : k * D * MC_PHI(sd - d1) - s * MC_PHI(-d1) + s * D * c * (p * MC_PHI(g - d1) - G * MC_PHI(-d1));
    }
#undef MC_PHI
    *price = out;
    return MC_OK;
}

/* The inputs every Heston entry point refuses (see mc_mi355x.h).  Internal (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_heston_check)(const HESTON *o)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, t = (double)o->option.t;
    const double v0 = (double)o->v0, kappa = (double)o->kappa, theta = (double)o->theta, xi = (double)o->xi, rho = (double)o->rho;
    if (o->n_steps < 1 || o->n_steps > MC_MAX_HESTON_STEPS)
        return mc_internal_fail(MC_ERR_INVALID, "heston: n_steps=%d outside [1, %d]", o->n_steps, MC_MAX_HESTON_STEPS);
    if (!isfinite(s) || !isfinite(k) || !isfinite(r) || !isfinite(t) || !isfinite(v0) || !isfinite(kappa) || !isfinite(theta) || !isfinite(xi) ||
        !isfinite(rho))
        return mc_internal_fail(MC_ERR_INVALID, "heston: need finite s, k, r, t, v0, kappa, theta, xi, rho");
    if (!(s > 0) || !(t > 0) || !(v0 >= 0) || !(kappa >= 0) || !(theta >= 0) || !(xi >= 0) || !(fabs(rho) <= 1))
        return mc_internal_fail(MC_ERR_INVALID, "heston: need s>0, t>0, v0>=0, kappa>=0, theta>=0, xi>=0, |rho|<=1");
    return MC_OK;
}

/* Discounted exact price of the European call under the Heston model (see mc_mi355x.h and heston_call_fp64).  xi == 0 leaves a
 * deterministic variance: Black-Scholes at the mean variance over [0, t] (the discounted intrinsic value where that is 0). */
int FN(mc_heston_closed_form)(const HESTON *o, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "heston closed form: NULL argument");
    HESTON one = *o;
    one.n_steps = 1;   /* ignored here */
    int rc = FN(mc_heston_check)(&one);
    if (rc != MC_OK)
        return rc;
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, t = (double)o->option.t;
    const double v0 = (double)o->v0, kappa = (double)o->kappa, theta = (double)o->theta, xi = (double)o->xi, rho = (double)o->rho;
    if (!(k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "heston closed form: needs k > 0");
    if (xi == 0 || (v0 == 0 && kappa * theta == 0)) {   /* the second: the variance never leaves 0 */
        const double kt = kappa * t, w = kt > 0 ? theta + (v0 - theta) * (-expm1(-kt)) / kt : v0, sd = sqrt(w * t), kd = k * exp(-r * t);
        if (!(sd > 0)) {
            *price = fmax(s - kd, 0.0);
            return MC_OK;
        }
        const double d1 = (log(s / k) + r * t) / sd + 0.5 * sd;
        *price = s * 0.5 * erfc(-d1 / sqrt(2.0)) - kd * 0.5 * erfc(-(d1 - sd) / sqrt(2.0));
        return MC_OK;
    }
    const double c = heston_call_fp64(s, k, r, t, v0, kappa, theta, xi, rho);
    if (!isfinite(c))
        return mc_internal_fail(MC_ERR_INVALID, "heston closed form: the integrand does not decay within the quadrature's 40000 panels for these inputs");
    *price = c;
    return MC_OK;
}

/* The inputs every jump-diffusion entry point refuses (see mc_mi355x.h); the threshold cap is mc_merton_thresholds_*'s.  Internal
 * (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_merton_check)(const MERTON *o)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    const double lambda = (double)o->lambda, mu = (double)o->mu_j, delta = (double)o->delta;
    if (o->n_dates < 1 || o->n_dates > MC_MAX_MERTON_DATES)
        return mc_internal_fail(MC_ERR_INVALID, "merton: n_dates=%d outside [1, %d]", o->n_dates, MC_MAX_MERTON_DATES);
    if (o->payoff < MC_MERTON_EUROPEAN || o->payoff > MC_MERTON_BARRIER)
        return mc_internal_fail(MC_ERR_INVALID, "merton: payoff=%d is none of MC_MERTON_EUROPEAN, MC_MERTON_ASIAN, MC_MERTON_BARRIER", o->payoff);
    if (!isfinite(s) || !isfinite(k) || !isfinite(r) || !isfinite(v) || !isfinite(t) || !isfinite(lambda) || !isfinite(mu) || !isfinite(delta))
        return mc_internal_fail(MC_ERR_INVALID, "merton: need finite s, k, r, v, t, lambda, mu_j, delta");
    if (!(s > 0) || !(t > 0) || !(v >= 0) || !(lambda >= 0) || !(delta >= 0))
        return mc_internal_fail(MC_ERR_INVALID, "merton: need s>0, t>0, v>=0, lambda>=0, delta>=0");
    if (o->payoff == MC_MERTON_BARRIER) {
        BARRIER b = {.option = o->option, .barrier = o->barrier, .n_dates = o->n_dates, .type = o->barrier_type, .monitoring = MC_MONITOR_DISCRETE};
        return FN(mc_barrier_check)(&b, 0);
    }
    return MC_OK;
}

/* The integer thresholds of the Poisson(lambda dt) count drawn from a MERTON_BITS-bit word (the rule is stated in mc_mi355x.h). */
int FN(mc_merton_thresholds)(const MERTON *o, uint64_t *out, int *count)
{
    if (!o || !out || !count)
        return mc_internal_fail(MC_ERR_INVALID, "merton thresholds: NULL argument");
    int rc = FN(mc_merton_check)(o);
    if (rc != MC_OK)
        return rc;
    enum { TERMS = 256 };   /* p <= MC_MAX_MERTON_JUMPS here: f_256 is below 1e-130 of the mode */
    const double p = (double)o->lambda * ((double)o->option.t / (double)o->n_dates);
    if (!(p <= (double)MC_MAX_MERTON_JUMPS))   /* the mean alone is beyond the cap */
        return mc_internal_fail(MC_ERR_INVALID, "merton: lambda dt = %g needs more than %d Poisson thresholds", p, MC_MAX_MERTON_JUMPS);
    long double f[TERMS], tail[TERMS];   /* tail[k] = sum_{n > k} f_n, summed from the small end */
    f[0] = expl(-(long double)p);
    for (int n = 1; n < TERMS; ++n)
        f[n] = f[n - 1] * (long double)p / (long double)n;
    tail[TERMS - 1] = 0.0L;
    for (int n = TERMS - 1; n > 0; --n)
        tail[n - 1] = tail[n] + f[n];
    const long double eps = ldexpl(1.0L, -(MERTON_BITS + 1)), top = ldexpl(1.0L, MERTON_BITS);
    int K = 0;
    while (K < TERMS - 1 && !(tail[K] < eps))
        ++K;
    if (K > MC_MAX_MERTON_JUMPS)
        return mc_internal_fail(MC_ERR_INVALID, "merton: lambda dt = %g needs %d Poisson thresholds, more than %d", p, K, MC_MAX_MERTON_JUMPS);
    const uint64_t last = MERTON_BITS == 64 ? UINT64_MAX : (uint64_t)0xFFFFFFFFu;
    long double F = 0.0L;
    for (int k = 0; k < K; ++k) {
        F += f[k];
        const long double x = floorl(F * top);
        out[k] = x >= top ? last : (uint64_t)x;
        if (k && out[k] < out[k - 1])   /* cannot happen (F is a sum of non-negative terms); kept as the contract */
            out[k] = out[k - 1];
    }
    *count = K;
    return MC_OK;
}

/* Discounted price of the European call under Merton's jump-diffusion: the Poisson-weighted series of Black-Scholes prices
 * stated in mc_mi355x.h, fp64, Phi by erfc. */
int FN(mc_merton_closed_form)(const MERTON *o, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "merton closed form: NULL argument");
    MERTON one = *o;
    one.n_dates = 1, one.payoff = MC_MERTON_EUROPEAN;   /* both ignored here */
    int rc = FN(mc_merton_check)(&one);
    if (rc != MC_OK)
        return rc;
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    const double lambda = (double)o->lambda, mu = (double)o->mu_j, delta = (double)o->delta;
    if (!(k > 0))
        return mc_internal_fail(MC_ERR_INVALID, "merton closed form: needs k > 0");
    const double kappa = expm1(mu + 0.5 * delta * delta), g = mu + 0.5 * delta * delta;   /* g = ln(1 + kappa) */
    const double lt = lambda * (1.0 + kappa) * t;
    if (!(lt < 700.0))   /* e^{-lt} must not underflow */
        return mc_internal_fail(MC_ERR_INVALID, "merton closed form: lambda (1 + kappa) t = %g is beyond the series' range", lt);
    double w = exp(-lt), sum = 0.0;   /* the Poisson weight of n */
    for (int n = 0; n < 100000; ++n) {
        const double rn = r - lambda * kappa + (double)n * g / t, sd = sqrt(v * v * t + (double)n * delta * delta), kd = k * exp(-rn * t);
        double bs;
        if (!(sd > 0)) {
            bs = fmax(s - kd, 0.0);
        } else {
            const double d1 = (log(s / k) + rn * t) / sd + 0.5 * sd;
            bs = s * 0.5 * erfc(-d1 / sqrt(2.0)) - kd * 0.5 * erfc(-(d1 - sd) / sqrt(2.0));
        }
        sum += w * bs;
        w *= lt / (double)(n + 1);
        /* past the mode the weights fall faster than the geometric series of ratio lt / (n + 2): that bounds what is left */
        if ((double)n >= lt && w < 1e-18 * (1.0 - lt / (double)(n + 2)))
            break;
    }
    *price = sum;
    return MC_OK;
}

/* The inputs every Bermudan entry point refuses (see mc_mi355x.h).  Internal (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_american_check)(const AMERICAN *o)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, v = (double)o->option.v, t = (double)o->option.t;
    if (o->n_dates < 1 || o->n_dates > MC_MAX_AMERICAN_DATES)
        return mc_internal_fail(MC_ERR_INVALID, "american: n_dates=%d outside [1, %d]", o->n_dates, MC_MAX_AMERICAN_DATES);
    if (o->type != MC_AMERICAN_PUT && o->type != MC_AMERICAN_CALL)
        return mc_internal_fail(MC_ERR_INVALID, "american: type=%d is neither MC_AMERICAN_PUT nor MC_AMERICAN_CALL", o->type);
    if (o->degree < 1 || o->degree > 3)
        return mc_internal_fail(MC_ERR_INVALID, "american: degree=%d outside [1, 3]", o->degree);
    if (!isfinite(s) || !isfinite(k) || !isfinite(r) || !isfinite(v) || !isfinite(t))
        return mc_internal_fail(MC_ERR_INVALID, "american: need finite s, k, r, v, t");
    if (!(s > 0) || !(k > 0) || !(t > 0) || !(v >= 0))
        return mc_internal_fail(MC_ERR_INVALID, "american: need s>0, k>0, t>0, v>=0");
    return MC_OK;
}

/* Discounted Cox-Ross-Rubinstein price of the Bermudan put or call (the lattice is stated in mc_mi355x.h). */
int FN(mc_american_lattice)(const AMERICAN *o, int steps_per_date, double *price)
{
    if (!o || !price)
        return mc_internal_fail(MC_ERR_INVALID, "american lattice: NULL argument");
    int rc = FN(mc_american_check)(o);
    if (rc != MC_OK)
        return rc;
    if (steps_per_date < 1 || (long long)steps_per_date * o->n_dates > (1 << 15))
        return mc_internal_fail(MC_ERR_INVALID, "american lattice: n_dates * steps_per_date = %lld outside [1, %d]",
                                (long long)steps_per_date * o->n_dates, 1 << 15);
    if (!((double)o->option.v > 0))
        return mc_internal_fail(MC_ERR_INVALID, "american lattice: needs v > 0");
    const double p = american_lattice_fp64((double)o->option.s, (double)o->option.k, (double)o->option.r, (double)o->option.v, (double)o->option.t,
                                           o->type == MC_AMERICAN_PUT ? -1.0 : 1.0, steps_per_date * o->n_dates, steps_per_date);
    if (!isfinite(p))
        return mc_internal_fail(MC_ERR_INVALID, "american lattice: the risk-neutral probability leaves (0, 1): more steps per date are needed");
    *price = p;
    return MC_OK;
}

/* The inputs every local-volatility entry point refuses (see mc_mi355x.h), the exponent-range guard included: heston_args' rule with
 * the surface's largest volatility in place of the variance (5e6: the argument range of the device's fp64 exponential; 8.58: the
 * generator's largest normal).  Internal (mc_hostmath.h): shared with mc_api.hip, not exported. */
__attribute__((visibility("hidden"))) int FN(mc_localvol_check)(const LOCALVOL *o)
{
    const double s = (double)o->option.s, k = (double)o->option.k, r = (double)o->option.r, t = (double)o->option.t;
    const double y_lo = (double)o->y_lo, y_hi = (double)o->y_hi;
    if (o->n_steps < 1 || o->n_steps > MC_MAX_LOCALVOL_STEPS)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: n_steps=%d outside [1, %d]", o->n_steps, MC_MAX_LOCALVOL_STEPS);
    if (o->n_times < 1 || o->n_nodes < 2 || o->n_times > MC_MAX_LOCALVOL_NODES || o->n_nodes > MC_MAX_LOCALVOL_NODES ||
        (long long)o->n_times * o->n_nodes > MC_MAX_LOCALVOL_NODES)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: need n_times>=1, n_nodes>=2 and n_times * n_nodes <= %d (got %d x %d)",
                                MC_MAX_LOCALVOL_NODES, o->n_times, o->n_nodes);
    if (o->n_steps % o->n_times != 0)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: n_times=%d does not divide n_steps=%d", o->n_times, o->n_steps);
    if (o->steps_per_date < 1 || o->n_steps % o->steps_per_date != 0)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: steps_per_date=%d is below 1 or does not divide n_steps=%d", o->steps_per_date, o->n_steps);
    if (o->payoff < MC_LOCALVOL_EUROPEAN || o->payoff > MC_LOCALVOL_BARRIER)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: payoff=%d is none of MC_LOCALVOL_EUROPEAN, MC_LOCALVOL_ASIAN, MC_LOCALVOL_BARRIER", o->payoff);
    if (o->right != MC_LOCALVOL_CALL && o->right != MC_LOCALVOL_PUT)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: right=%d is neither MC_LOCALVOL_CALL nor MC_LOCALVOL_PUT", o->right);
    if (!isfinite(s) || !isfinite(k) || !isfinite(r) || !isfinite(t) || !isfinite(y_lo) || !isfinite(y_hi))
        return mc_internal_fail(MC_ERR_INVALID, "localvol: need finite s, k, r, t, y_lo, y_hi");
    if (!(s > 0) || !(t > 0) || !(y_lo < y_hi))
        return mc_internal_fail(MC_ERR_INVALID, "localvol: need s>0, t>0, y_lo<y_hi");
    {   /* the two constants of the lookup, as the kernels hold them: a grid too narrow for REAL leaves 1 / h or -y_lo / h infinite */
        const double h = (y_hi - y_lo) / (double)(o->n_nodes - 1);
        if (!isfinite((double)(REAL)(1.0 / h)) || !isfinite((double)(REAL)(-y_lo / h)))
            return mc_internal_fail(MC_ERR_INVALID, "localvol: the node spacing %g of [y_lo, y_hi] is too small for this precision", h);
    }
    if (!o->sigma)
        return mc_internal_fail(MC_ERR_INVALID, "localvol: NULL sigma");
    double vmax = 0;
    for (int q = 0; q < o->n_times * o->n_nodes; ++q) {
        const double a = (double)o->sigma[q];
        if (!isfinite(a) || !(a >= 0))
            return mc_internal_fail(MC_ERR_INVALID, "localvol: sigma[%d][%d]=%g is negative or not finite", q / o->n_nodes, q % o->n_nodes, a);
        vmax = fmax(vmax, a);
    }
    double gap = 0;
    if (o->payoff == MC_LOCALVOL_BARRIER) {
        BARRIER b = {.option = o->option, .barrier = o->barrier, .n_dates = 1, .type = o->barrier_type, .monitoring = MC_MONITOR_DISCRETE};
        b.option.v = 0;
        int rc = FN(mc_barrier_check)(&b, 0);
        if (rc != MC_OK)
            return rc;
        gap = log((double)o->barrier / s);
    }
    const double m = (double)o->n_steps, dt = t / m;
    if (!(fabs(log(s)) + fabs(gap) + fabs(r) * t + m * (0.5 * vmax * vmax * dt + vmax * sqrt(dt) * 8.58) < 5e6))
        return mc_internal_fail(MC_ERR_INVALID, "localvol: drift and volatility put the simulated spot outside the range of a double");
    return MC_OK;
}

/* The interpolant the kernels read at step `step` and log-spot y, in fp64 from the table as rounded for REAL (see mc_mi355x.h). */
int FN(mc_localvol_sigma)(const LOCALVOL *o, int step, double y, double *sigma)
{
    if (!o || !sigma)
        return mc_internal_fail(MC_ERR_INVALID, "localvol sigma: NULL argument");
    int rc = FN(mc_localvol_check)(o);
    if (rc != MC_OK)
        return rc;
    if (step < 1 || step > o->n_steps || !isfinite(y))
        return mc_internal_fail(MC_ERR_INVALID, "localvol sigma: step=%d outside [1, n_steps] or y not finite", step);
    const REAL *row = o->sigma + (size_t)((step - 1) / (o->n_steps / o->n_times)) * (size_t)o->n_nodes;
    const double h = ((double)o->y_hi - (double)o->y_lo) / (double)(o->n_nodes - 1);
    const double u = fmin(fmax((y - (double)o->y_lo) / h, 0.0), (double)(o->n_nodes - 1));
    int i = (int)floor(u);
    if (i > o->n_nodes - 2)
        i = o->n_nodes - 2;
    const REAL b = (REAL)((double)row[i + 1] - (double)row[i]);
    *sigma = (double)row[i] + (u - (double)i) * (double)b;
    return MC_OK;
}
