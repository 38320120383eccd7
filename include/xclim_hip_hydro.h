/* xclim_hip_hydro.h — the C ABI of the streamflow and snow-melt unit (xclim_amd/csrc/hydro.hip), exported by libxclimhip.so
 * next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py HYDRO_SIGNATURES.
 *
 * Common to the four entry points.  Fields are (T, C) time-major with row pitch ld >= C (DEVICE), all float32 (f64 = 0) or
 * all float64; values are widened to float64 on load and all arithmetic is float64 in the reference's order of operations
 * (the library is built with -ffp-contract=off).  Outputs are float64, counts int32, with row pitch ld_out >= C (DEVICE).
 * Tables marked HOST are read (and checked) on the host before anything is launched; every other pointer is DEVICE memory.
 * At most 65535 periods.  Every check answers before anything is launched and leaves the outputs untouched; a call with
 * P == 0 or C == 0 (T == 0 for xh_antecedent_precip, K == 0 for xh_sen_slope) launches nothing and returns XH_OK. */
#ifndef XCLIM_HIP_HYDRO_H
#define XCLIM_HIP_HYDRO_H

#include "xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The trailing window of xh_melt_period_max and xh_antecedent_precip is a ring of `window` float64 per lane in LDS, 256
 * lanes to a workgroup: 2 KiB per window day, and 32 days fill the 64 KiB a workgroup gets without asking for more (two such
 * workgroups share the 160 KiB of a CU; xh_antecedent_precip adds its `window` weights to that).  A longer window answers
 * XH_ERR_LIMIT. */
#define XH_HYDRO_MAX_WINDOW 32

/* xh_sen_slope keeps one series in LDS: its Y values, its Y (Y - 1) / 2 pair slopes padded to the next power of two (they are
 * sorted in place by a bitonic network) and 256 partial sums, all float64.  Y = 181 has 16 290 pairs, padded to 16 384:
 * (181 + 16 384 + 256) * 8 = 134 568 bytes of the 160 KiB of a gfx950 CU; Y = 182 has 16 471 pairs, and the padding to 32 768
 * no longer fits.  (Y = 64: 2 016 pairs, 18.9 KiB, eight workgroups to a CU.)  More years answer XH_ERR_LIMIT. */
#define XH_SEN_MAX_YEARS 181

/* xh_flow_period_stats: base_flow_index (_hydrology.py:84-89) and rb_flashiness_index (:125-128) and the period statistics
 *   behind them, any subset from one walk of q, one lane per (cell, period).  seg (HOST int64, P + 1): first row of every
 *   period, non-decreasing within [0, T].  A lane also reads the three rows before its period and the three after it (the
 *   7-day window reads across period boundaries) and never writes a (T, C) intermediate.
 *   m7 at row i = ((((((q[i-3] + q[i-2]) + q[i-1]) + q[i]) + q[i+1]) + q[i+2]) + q[i+3]) / 7, NaN if one of the seven is NaN
 *   or lies outside the series (rolling(7, center=True).mean(skipna=False)).
 *   bfi_out: the minimum of the period's non-NaN m7 over the NaN-skipping mean of the period's q; NaN without an m7 or
 *   without a value.  rbi_out: the NaN-skipping sum over the period's rows i >= 1 of |q[i] - q[i-1]| over the NaN-skipping sum
 *   of the period's q (0 / 0 = NaN for a period with nothing to add).  mean_out, sum_out: the NaN-skipping mean (NaN without
 *   a value) and sum of the period's q.  valid_out (int32): the period's rows with a value.  Outputs (P, C); each may be NULL,
 *   not all of them. */
int xh_flow_period_stats(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* q, int64_t P,
                         const int64_t* seg /* host */, double* bfi_out, double* rbi_out, double* mean_out, double* sum_out,
                         int32_t* valid_out, int64_t ld_out);

/* xh_melt_period_max: snow_melt_we_max (:392-399; pr = NULL) and melt_and_precip_max (:429-439), one lane per (cell, period).
 *   total[i] = pr[i] * per_day + (snw[i] - snw[i-1]) * -1 for i >= 1 (without pr: (snw[i] - snw[i-1]) * -1).
 *   agg[i] = total[i-window+1] + ... + total[i], added in row order; NaN if a term is NaN or i - window + 1 < 1.
 *   out (float64 (P, C)): the maximum of the period's non-NaN agg, NaN if there is none.  The window reads across period
 *   boundaries: a lane starts `window` rows before its period.  1 <= window <= XH_HYDRO_MAX_WINDOW (XH_ERR_LIMIT beyond). */
int xh_melt_period_max(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* snw, const void* pr, double per_day,
                       int window, int64_t P, const int64_t* seg /* host */, double* out, int64_t ld_out);

/* xh_antecedent_precip: antecedent_precipitation_index (:698-705).  out (float64 (T, C)):
 *   out[i] = weights[0] * (pr[i-window+1] * per_day) + ... + weights[window-1] * (pr[i] * per_day), the terms added in that
 *   order; NaN for i < window - 1 and where a term is NaN.  weights (HOST float64, window).  The launch is tiled along time:
 *   a lane walks a tile of rows with the window - 1 rows before it, so a row is read about once.
 *   1 <= window <= XH_HYDRO_MAX_WINDOW (XH_ERR_LIMIT beyond). */
int xh_antecedent_precip(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, double per_day, int window,
                         const double* weights /* host */, double* out, int64_t ld_out);

/* xh_sen_slope: the Theil-Sen slope and the Mann-Kendall p value (:926-944, the arithmetic of pymannkendall.original_test)
 *   of Y yearly values per (season, cell); one workgroup (one wave) per series.  x (P, C) float32 or float64 with row pitch
 *   ld.  period_of (HOST int64 (Y, K)): the row of x that holds year y of season k, -1 where the series has no such period.
 *   The Y values in year order; absent and NaN values are dropped, n_out (int32 (K, C), may be NULL) counts the others.
 *   s = sum over i < j of sign(x_j - x_i) on the values left; var = (n (n - 1) (2 n + 5) - sum over groups of t equal values
 *   of t (t - 1) (2 t + 5)) / 18; z = (s - 1) / sqrt(var) for s > 0, (s + 1) / sqrt(var) for s < 0, 0 otherwise;
 *   p_out = 2 (1 - erfc(-|z| / sqrt 2) / 2).  slope_out: the median (the middle one, or the mean of the two middle ones) of
 *   (x_j - x_i) / (j - i) over the pairs i < j of values left, i and j the ORIGINAL year positions; every slope is one IEEE
 *   division, stored and sorted in LDS.  With n < 2 slope and p are NaN.  slope_out, p_out float64 (K, C), each may be NULL,
 *   not both.  0 <= Y <= XH_SEN_MAX_YEARS (XH_ERR_LIMIT beyond), K <= 65535. */
int xh_sen_slope(xh_ctx* ctx, int64_t P, int64_t C, int64_t ld, int f64, const void* x, int64_t Y, int64_t K,
                 const int64_t* period_of /* host */, double* slope_out, double* p_out, int32_t* n_out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_HYDRO_H */
