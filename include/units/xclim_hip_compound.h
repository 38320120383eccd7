/* xclim_hip_compound.h — the C ABI of the compound-extreme unit (xclim_amd/csrc/compound.hip): the four compound percentile-day
 * counts of indices/_multivariate.py:162-423, degree_days_exceedance_date (indices/_threshold.py:3215-3310), blowing_snow
 * (_multivariate.py:1833-1884) and the period sum of water_cycle_intensity (:1888-1918).  Exported by libxclimhip.so next to the
 * entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.  ctypes
 * prototypes: xclim_amd/_capi.py UNIT_SIGNATURES.
 *
 * Common to the four entry points.  Fields are time-major with row pitch ld >= C (DEVICE), float32 (f64 = 0) or float64; values
 * are widened to float64 on load (exact) and all arithmetic is float64 (the library is built with -ffp-contract=off).  Outputs
 * are float64 (P, C) with row pitch ld_out >= C (DEVICE).  Tables marked HOST are read (and checked) on the host before anything
 * is launched; every other pointer is DEVICE memory.  seg (HOST int64, P + 1): the first row of every period, non-decreasing
 * within [0, T]; at most 65535 periods.  Every check answers before anything is launched and leaves the outputs untouched; a
 * call with no period or no cell launches nothing and returns XH_OK.  Every element of a requested output is stored; an output
 * that is NULL costs no load, store or arithmetic. */
#ifndef XCLIM_HIP_COMPOUND_H
#define XCLIM_HIP_COMPOUND_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The four counts of xh_compound_doy_days, as the bits of the output set a launch is compiled for. */
#define XH_CD_COLD_DRY 1 /* tas < tas_lo && pr < pr_lo */
#define XH_CD_WARM_DRY 2 /* tas > tas_hi && pr < pr_lo */
#define XH_CD_WARM_WET 4 /* tas > tas_hi && pr > pr_hi */
#define XH_CD_COLD_WET 8 /* tas < tas_lo && pr > pr_hi */
#define XH_CD_NOUT 4

/* The longest window of xh_blowing_snow_days: a ring of `window` float64 per lane in LDS, 128 lanes to a workgroup
 * (32 * 128 * 8 = 32 768 bytes, four workgroups to the 160 KiB of a CU); the value of XH_HYDRO_MAX_WINDOW.  A longer window
 * answers XH_ERR_LIMIT. */
#define XH_BS_MAX_WINDOW 32

/* xh_compound_doy_days: up to four compound percentile-day counts from ONE walk of tas and pr.
 *   tas, pr (T, C).  tas_lo, tas_hi, pr_lo, pr_hi: per-doy tables (ndoy, C) float64 with row pitch ld_tab >= C, as percentile_doy
 *   leaves them.  tidx (HOST int32, T): the table row of every field row, within [0, ndoy) on the rows of [seg[0], seg[P]).
 *   out[p, c] = the number of rows of period p on which both compares hold (XH_CD_* above); a NaN on either side of a compare is
 *   false.  The compares are float64: a float32 sample is widened, which is exact, so the counts are those of the reference bit
 *   for bit.  The set of outputs is uniform over the launch and chosen at compile time: an output that is NULL is not counted,
 *   and a table that no requested output needs may be NULL and is never read.  A table a requested output needs must not be
 *   NULL (XH_ERR_ARG).  Each field row is read once, each table row once per field row that maps to it; lanes read 16 bytes of
 *   every operand where the base pointers and the pitches allow it (float32: 4 cells, float64: 2), the cells of a last partial
 *   group and of misaligned views one by one. */
int xh_compound_doy_days(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, const void* pr, int64_t ndoy,
                         int64_t ld_tab, const double* tas_lo, const double* tas_hi, const double* pr_lo, const double* pr_hi,
                         const int32_t* tidx /* host */, int64_t P, const int64_t* seg /* host */, double* cold_dry,
                         double* warm_dry, double* warm_wet, double* cold_wet, int64_t ld_out);

/* xh_degree_exceedance_date: one lane per (cell, period), one walk of the period.
 *   c[i] = max(tas[i] - thresh, 0), or max(thresh - tas[i], 0) with below != 0; a NaN row and every row before start[p] add 0
 *   (xarray's cumsum skips NaN); the running sum is float64, added in row order.
 *   start (HOST int64, P): the row the sum starts on, within [seg[p], seg[p+1]), or -1 for a period that does not hold the date:
 *   NaN.  never (HOST float64, P): the value of a period whose running sum is <= sum_thresh on ALL its rows (NaN for None).
 *   doy (HOST int32, T): the day of year of every row, 1 .. 366.
 *   out[p, c] = doy of the first row of the period whose running sum is > sum_thresh; never[p] without one; NaN for a NaN
 *   sum_thresh (no row is above it and not every row is at or below it).  The reference's quirk is kept: its find_boundary_run
 *   (indices/run_length.py:600-610) answers NaN when argmax == argmin, which is also the case when EVERY row of the period is
 *   above sum_thresh — the running sum never decreases, so exactly when the period's FIRST row is (the exceedance on row seg[p]
 *   itself, or a negative sum_thresh, which the 0 of the rows before the start already exceeds): NaN, never[p] included. */
int xh_degree_exceedance_date(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, double thresh, int below,
                              double sum_thresh, int64_t P, const int64_t* seg /* host */, const int64_t* start /* host */,
                              const double* never /* host */, const int32_t* doy /* host */, double* out, int64_t ld_out);

/* xh_blowing_snow_days: one lane per (cell, period).
 *   d[i] = snd[i] - snd[i-1] (i >= 1); s[i] = d[i-window+1] + ... + d[i], added in row order from its first term, defined for
 *   i >= window (the first `window` rows of the series have no full window) and NaN when a term is NaN; the window reaches back
 *   across the period's start.  out[p, c] = the number of rows i of period p with s[i] >= snd_thresh && sfcWind[i] >=
 *   wind_thresh && flags[i] != 0.  flags (HOST uint8, T, or NULL for every row): the rows the indexer selects, applied after the
 *   window sum.  1 <= window <= XH_BS_MAX_WINDOW (XH_ERR_LIMIT beyond). */
int xh_blowing_snow_days(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* snd, const void* sfcWind,
                         double snd_thresh, double wind_thresh, int window, int64_t P, const int64_t* seg /* host */,
                         const uint8_t* flags /* host */, double* out, int64_t ld_out);

/* xh_pair_period_sum: out[p, c] = the sum over the rows of period p of (a[i] + b[i]) * scale, in row order; a NaN term is
 *   skipped and a period without a term is 0 (xarray's resample sum).  One lane per (cell, period); neither the sum field nor the
 *   amount field of the reference exists. */
int xh_pair_period_sum(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* a, const void* b, double scale,
                       int64_t P, const int64_t* seg /* host */, double* out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_COMPOUND_H */
