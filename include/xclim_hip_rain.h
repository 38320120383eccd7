/* xclim_hip_rain.h — the C ABI of the rain-season and hardiness-zone unit (xclim_amd/csrc/rainseason.hip), exported by
 * libxclimhip.so next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the
 * conventions.  ctypes prototypes: xclim_amd/_capi.py RAIN_SIGNATURES.
 *
 * Common to the two entry points.  Fields are time-major with row pitch ld >= C (DEVICE), float32 (f64 = 0) or float64; values
 * are widened to float64 on load and all arithmetic is float64 (the library is built with -ffp-contract=off).  Outputs are
 * float64 with row pitch ld_out >= C (DEVICE).  Tables marked HOST are read (and checked) on the host before anything is
 * launched; every other pointer is DEVICE memory.  Every check answers before anything is launched and leaves the outputs
 * untouched; a call with no period or no cell launches nothing and returns XH_OK.  Every element of an output is stored, NaN
 * included. */
#ifndef XCLIM_HIP_RAIN_H
#define XCLIM_HIP_RAIN_H

#include "xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The longest window that is a SUM (window_wet_start always; window_dry_start and window_dry_end with their "total" method):
 * the value of XH_HYDRO_MAX_WINDOW.  The windows live in one ring per lane in LDS, in the field's dtype, 128 lanes to a
 * workgroup: R = lag + max(window_wet_start, window_dry_end when it is a sum, 1) rows, lag = window_dry_start - 1 (0 when
 * window_dry_start is a "per_day" run of more than the limit, which re-reads its rows instead), so at most 63 rows:
 * 63 * 128 * 8 = 64 512 bytes for a float64 field, two workgroups to the 160 KiB of a CU; the reference's defaults (3, 7 per
 * day, 20 per day) take 9 * 128 * 4 = 4 608 bytes for a float32 field.  "per_day" windows and window_not_dry_start are
 * counters without a limit.  A longer sum window answers XH_ERR_LIMIT. */
#define XH_RAIN_MAX_WINDOW 32

/* Flag bits of xh_rain_season, one uint8 per row (the three date selections of the reference, made on the host). */
#define XH_RAIN_START_WINDOW 1 /* inside date_bounds = (date_min_start, the month-day of the period's last row) */
#define XH_RAIN_START_BOUNDS 2 /* inside (date_min_start, date_max_start) */
#define XH_RAIN_END_BOUNDS 4   /* inside (date_min_end, date_max_end) */

/* The most bin edges xh_rolling_zones takes (they travel as kernel arguments); more answer XH_ERR_LIMIT. */
#define XH_ZONES_MAX_EDGES 32

/* xh_rain_season: rain_season (indices/_agro.py:796-980), one lane per (cell, period), one forward walk of the period.
 *   pr (T, C); a[i] = pr[i] * per_day is the daily amount, i the row within the period [seg[p], seg[p+1]) of n rows.
 *   seg (HOST int64, P + 1): first row of every period, non-decreasing within [0, T].  flags (HOST uint8, T): the XH_RAIN_*
 *   bits of every row; within a period the rows with XH_RAIN_START_WINDOW must be its LAST rows (a date window that ends on the
 *   period's last day is), XH_ERR_ARG otherwise.  doy (HOST int32, T): the day of year of every row, 1 .. 366.
 *   P[i] = a[i] on rows with XH_RAIN_START_WINDOW, NaN elsewhere.  With ww = window_wet_start, wd = window_dry_start,
 *   we = window_dry_end (all >= 1) and window_not_dry_start >= 0:
 *     wet[i]   = i >= ww - 1 and P[i-ww+1] + ... + P[i] >= thresh_wet_start (added in row order; NaN compares false);
 *     stop[i]  = i + wd - 1 <= n - 1 and (total_dry_start == 0: every one of P[i] .. P[i+wd-1] <= thresh_dry_start;
 *                total_dry_start != 0: P[i] + ... + P[i+wd-1] <= thresh_dry_start, in row order);
 *     event[i] = 0 where stop[i], else 1 where wet[i], else event[i-1] (0 before the first row);
 *     a candidate is the first row of a run of event == 1 of at least window_not_dry_start + ww rows;
 *     start    = the first candidate on a row with XH_RAIN_START_BOUNDS; none if there is no such candidate, or if EVERY row
 *                with XH_RAIN_START_BOUNDS is one (the reference's argmax == argmin);
 *     end marks, on rows i > start only: total_dry_end == 0: the first row of every run of P <= thresh_dry_end of at least we
 *                rows that begins after start; total_dry_end != 0: row i when i - we + 1 > start and
 *                P[i-we+1] + ... + P[i] <= thresh_dry_end (the mark sits on the LAST day of the window);
 *     end      = the first end mark on a row with XH_RAIN_END_BOUNDS; none if there is none or if every row of the period with
 *                XH_RAIN_END_BOUNDS is marked.
 *   start_out = doy[start], end_out = doy[end], length_out = end - start, or n - start without an end; all three NaN without
 *   a start.  Outputs float64 (P, C); each may be NULL, not all three.  At most 65535 periods; window_wet_start always, and
 *   window_dry_start / window_dry_end when their total_* is set, at most XH_RAIN_MAX_WINDOW (XH_ERR_LIMIT beyond). */
int xh_rain_season(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, double per_day, int64_t P,
                   const int64_t* seg /* host */, const uint8_t* flags /* host */, const int32_t* doy /* host */,
                   double thresh_wet_start, int window_wet_start, int window_not_dry_start, double thresh_dry_start,
                   int window_dry_start, int total_dry_start, double thresh_dry_end, int window_dry_end, int total_dry_end,
                   double* start_out, double* end_out, double* length_out, int64_t ld_out);

/* xh_rolling_zones: the rolling mean and the bin lookup of hardiness_zones (indices/_agro.py:1429-1430, get_zones of
 *   indices/generic.py:1698-1706), one lane per cell.  x (P, C) float32 or float64, such as the period minima of
 *   xh_resample_reduce / xh_resample_reduce_f64.  mean[t] = (x[t-window+1] + ... + x[t]) / window, added in row order; NaN for
 *   t < window - 1 and where a term is NaN.  edges (HOST float64, nedges >= 2, strictly increasing).
 *   out[t] (float64 (P, C)) = the number of edges <= mean[t], less one (np.digitize(mean, edges) - 1); a mean equal to the
 *   last edge goes to the last zone, nedges - 2; NaN for a mean below the first edge, above the last, or NaN.
 *   window >= 1; nedges <= XH_ZONES_MAX_EDGES (XH_ERR_LIMIT beyond). */
int xh_rolling_zones(xh_ctx* ctx, int64_t P, int64_t C, int64_t ld, int f64, const void* x, int window, int64_t nedges,
                     const double* edges /* host */, double* out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_RAIN_H */
