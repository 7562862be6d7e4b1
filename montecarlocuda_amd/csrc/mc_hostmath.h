/* mc_hostmath.h -- internal: what mc_api.hip / host_path.c take from mc_hostmath.c besides the public symbols. */
#ifndef MC_HOSTMATH_H_
#define MC_HOSTMATH_H_
#include "../../include/mc_mi355x.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Records the calling thread's error text (mc_last_error) and returns `code`. */
int mc_internal_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
/* The input checks of the barrier call, shared by mc_barrier_closed_form_* and the GPU entry points (not exported). */
int mc_barrier_check_f32(const mc_barrier_f32 *o, int need_vol);
int mc_barrier_check_f64(const mc_barrier_f64 *o, int need_vol);
/* The input checks of the rainbow options, shared by mc_rainbow_closed_form_* (with_dates = 0) and the GPU entry points (not exported). */
int mc_rainbow_check_f32(const mc_rainbow_f32 *o, int with_dates);
int mc_rainbow_check_f64(const mc_rainbow_f64 *o, int with_dates);
/* The input checks of the lookback options, shared by mc_lookback_closed_form_* and the GPU entry points (not exported). */
int mc_lookback_check_f32(const mc_lookback_f32 *o);
int mc_lookback_check_f64(const mc_lookback_f64 *o);
/* The input checks of the jump-diffusion calls, shared by mc_merton_closed_form_*, mc_merton_thresholds_* and the GPU entry points (not exported). */
int mc_merton_check_f32(const mc_merton_f32 *o);
int mc_merton_check_f64(const mc_merton_f64 *o);
/* The input checks of the Bermudan options, shared by mc_american_lattice_* and the GPU entry points (not exported). */
int mc_american_check_f32(const mc_american_f32 *o);
int mc_american_check_f64(const mc_american_f64 *o);
/* The input checks of the Heston call, shared by mc_heston_closed_form_* and the GPU entry points (not exported). */
int mc_heston_check_f32(const mc_heston_f32 *o);
int mc_heston_check_f64(const mc_heston_f64 *o);
/* The input checks of the local-volatility products, shared by mc_localvol_sigma_* and the GPU entry points (not exported). */
int mc_localvol_check_f32(const mc_localvol_f32 *o);
int mc_localvol_check_f64(const mc_localvol_f64 *o);
#ifdef __cplusplus
}
#endif
#endif
