/* xclim_hip_phase.h — the C ABI of the snow / rain partition unit (xclim_amd/csrc/phase.hip), exported by libxclimhip.so next
 * to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py PHASE_SIGNATURES.
 *
 * Common to the two entry points.  Fields are time-major with row pitch ld >= C (DEVICE), float32 (f64 = 0) or float64; values
 * are widened to float64 on load and all arithmetic is float64 in the reference's order (the library is built with
 * -ffp-contract=off).  Tables marked HOST are read (and checked) on the host before anything is launched; every other pointer
 * is DEVICE memory.  Every check answers before anything is launched and leaves the outputs untouched; a call with no row, no
 * period or no cell launches nothing and returns XH_OK.  Every element of a requested output is stored, NaN included.
 *
 * THE PARTITION of one sample (pr, tas) into snow and rain (snowfall_approximation / rain_approximation of
 * indices/converters.py:1088-1373), by `method`:
 *   XH_PHASE_BINARY        snow = tas <= thresh ? pr : 0 (a NaN tas gives 0); rain = pr - snow.
 *   XH_PHASE_BROWN         f = 1 for tas <= thresh, 0 for tas >= upper, (0 - 1) / (upper - thresh) * (tas - thresh) + 1 between
 *                          (np.interp over [-inf, thresh, upper, +inf]); NaN for a NaN tas.  snow = pr * f; rain = pr - snow.
 *   XH_PHASE_AUER          f = linear interpolation of the table (tab: K nodes, then K values; K = ntab) at
 *                          dtas = (tas + add_K) - thresh: values[j] + slope_j * (dtas - nodes[j]) for the LAST j with
 *                          nodes[j] <= dtas (a dtas on a node gives that node's value); values[0] below the first node,
 *                          values[K-1] at and above the last.  snow = pr * f; rain = pr - snow.
 *   XH_PHASE_DAI_ANNUAL,   f = a * (tanh(b * (t - c)) - d) / 100 with t = tas - sub_C (degC); with clip: f = (f - fmin) / den;
 *   XH_PHASE_DAI_SEASONAL  then f clipped to [0, 1] (NaN stays).  snow = pr * f_snow, rain = pr * f_rain, each with its own
 *                          (a, b, c, d, fmin, den): tab[((phase * 2 + land) * 4 + season) * 6 + k], phase 0 = snow, 1 = rain,
 *                          land 0 = ocean, 1 = land, season 0 .. 3 = DJF, MAM, JJA, SON (0 for the annual method); ntab = 96.
 *   XH_PHASE_GIVEN         the second field IS the solid precipitation: snow = tas, rain = pr - snow (period entry point only).
 * par (HOST float64, XH_PHASE_NPAR): thresh, upper, add_K, sub_C, clip (0 / 1), land (0 / 1: the coefficient set of every cell
 * when `land` is NULL).  land (DEVICE uint8, C, or NULL): 1 = land, 0 = ocean, per cell.  season (HOST uint8, T, or NULL = 0):
 * the season of every row. */
#ifndef XCLIM_HIP_PHASE_H
#define XCLIM_HIP_PHASE_H

#include "xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define XH_PHASE_BINARY 0
#define XH_PHASE_BROWN 1
#define XH_PHASE_AUER 2
#define XH_PHASE_DAI_ANNUAL 3
#define XH_PHASE_DAI_SEASONAL 4
#define XH_PHASE_GIVEN 5

#define XH_PHASE_NPAR 6
#define XH_PHASE_DAI_NTAB 96
#define XH_PHASE_MAX_NODES 4096

/* The outputs of xh_precip_phase_period: bit k of `mask` asks for outs[k]. */
#define XH_PHASE_PR_SUM 0        /* NaN-skipping sums of the daily amounts value * per_day, in row order; 0 for an all-NaN period */
#define XH_PHASE_SOLID_SUM 1
#define XH_PHASE_LIQUID_SUM 2
#define XH_PHASE_PR_N 3          /* the non-NaN samples of pr, of the snow amount, of the rain amount, of the second field */
#define XH_PHASE_SOLID_N 4
#define XH_PHASE_LIQUID_N 5
#define XH_PHASE_TAS_N 6
#define XH_PHASE_SNOW_DAYS 7     /* days with snow_low < snow * per_day <= snow_high (domain_count) */
#define XH_PHASE_SNOW_SUM_OVER 8 /* sum and count of snow * per_day on days where it is >= snow_thresh */
#define XH_PHASE_SNOW_N_OVER 9
#define XH_PHASE_FIRST_SNOW 10   /* day of year of the first / last day with snow * per_day >= snow_thresh; NaN without one */
#define XH_PHASE_LAST_SNOW 11
#define XH_PHASE_HPLT_DAYS 12    /* days with pr >= hplt_pr and tas < hplt_tas (both in the fields' own units) */
#define XH_PHASE_ROFG_DAYS 13    /* rain on frozen ground, see below */
#define XH_PHASE_NOUT 14

#define XH_PHASE_NLIM 7 /* lim (HOST float64): snow_low, snow_high, snow_thresh (mm), hplt_pr, hplt_tas, rofg_pr, rofg_frz */

/* xh_precip_phase_map: snow and / or rain of every sample, one launch, each field read once.  snow_out / rain_out (T, C) with
 *   row pitch ld_out: the dtype of the fields for XH_PHASE_BINARY (a select: bit-identical to the reference), float64 for every
 *   other method; either may be NULL, not both.  XH_PHASE_GIVEN answers XH_ERR_ARG. */
int xh_precip_phase_map(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, const void* tas, int method,
                        const double* par /* host */, const double* tab /* host */, int64_t ntab, const uint8_t* season /* host */,
                        const uint8_t* land, void* snow_out, void* rain_out, int64_t ld_out);

/* xh_precip_phase_period: one lane per (cell, period) walks the rows [seg[p], seg[p+1]) of pr and of the second field once
 *   and stores the outputs `mask` asks for, all float64 (P, C) with row pitch ld_out (counts are whole numbers).
 *   seg (HOST int64, P + 1), at most 65535 periods.  doy (HOST int32, T, or NULL when neither date is asked for): 1 .. 366.
 *   outs (HOST, XH_PHASE_NOUT device pointers; those whose bit is not set are not looked at).
 *   Rain on frozen ground (indices/_multivariate.py:1059-1119): row r counts when pr > rofg_pr, tas > rofg_frz and the `window`
 *   rows before it all have !(tas > rofg_frz) (a NaN tas is frozen); the rows before a period's first are read for this (tas
 *   only, up to `window` of them), and the first `window` rows of the series never count.  window >= 1.
 *   XH_PHASE_GIVEN serves neither XH_PHASE_HPLT_DAYS nor XH_PHASE_ROFG_DAYS (XH_ERR_ARG). */
int xh_precip_phase_period(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, const void* tas, double per_day,
                           int64_t P, const int64_t* seg /* host */, const int32_t* doy /* host */, int method,
                           const double* par /* host */, const double* tab /* host */, int64_t ntab, const uint8_t* season /* host */,
                           const uint8_t* land, const double* lim /* host */, int window, uint32_t mask, void* const* outs /* host */,
                           int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_PHASE_H */
