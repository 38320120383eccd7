/* xclim_hip_flags.h — the C ABI of the data-quality-flag unit (xclim_amd/csrc/dataflags.hip), exported by libxclimhip.so next to
 * the entry points of xclim_hip.h, which this header includes for the context, the return codes, the XH_OP_* operators and the
 * conventions.  ctypes prototypes: xclim_amd/_capi.py FLAGS_SIGNATURES.  Reference: xclim.core.dataflags (core/dataflags.py).
 *
 * Common to the two entry points.  Fields are time-major with row pitch ld >= C (DEVICE), float32 (f64 = 0) or float64, read
 * natively; all fields and tables of one call share the dtype.  Tables marked HOST are read (and checked) on the host before
 * anything is launched; every other pointer is DEVICE memory.  Every check answers before anything is launched and leaves the
 * outputs untouched; a call with T == 0, C == 0 or no period (xh_data_flags: P == 0 or K == 0; xh_doy_bounds: ndoy == 0) launches
 * nothing, writes nothing and returns XH_OK.
 *
 * ASSUMPTION (the convention of xh_compare_map_f64): a sample compared with a double operand (a, b below) is widened to float64
 * and compared there.  numpy >= 2 compares a float32 field with a Python float in float32; the two differ only for operands
 * that are not float32 values.  Samples compared with samples or with the bound tables are compared in the field's dtype. */
#ifndef XCLIM_HIP_FLAGS_H
#define XCLIM_HIP_FLAGS_H

#include "xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most checks one call of xh_data_flags evaluates (they travel as kernel arguments); more answer XH_ERR_LIMIT. */
#define XH_FLAGS_MAX_CHECKS 16

/* Check kinds; v = x[t, c]. */
#define XH_FLAG_CMP 0     /* v op a (IEEE: a NaN sample is false except for XH_OP_NE) */
#define XH_FLAG_OUTSIDE 1 /* v < a || v > b (a NaN sample is false) */
#define XH_FLAG_PAIR 2    /* v op y[other][t, c], other = 0 or 1 (a NaN on either side is false except for XH_OP_NE) */
#define XH_FLAG_REPEAT 3  /* row t belongs to a run of at least n >= 1 consecutive equal values whose value satisfies op a
                           * (op = -1: no threshold).  Equality is IEEE == on the field's dtype: every NaN is a run of one, -0.0 and
                           * 0.0 belong to one run.  Runs are found over the whole series, not per period (suspicious_run_1d,
                           * indices/run_length.py:1668-1714). */
#define XH_FLAG_CLIM 4    /* !(lo[tidx[t], c] < v && v < hi[tidx[t], c]): a NaN sample or a NaN bound is flagged, and so is every
                           * sample of a day of year whose deviation is 0 (~within_bnds_doy, core/calendar.py:934-954) */

/* One check.  Fields a kind does not name are ignored. */
typedef struct xh_flag_check {
  int32_t kind;  /* XH_FLAG_* */
  int32_t op;    /* XH_OP_* (CMP, PAIR, REPEAT; REPEAT also -1) */
  int32_t n;     /* REPEAT: the least run length */
  int32_t other; /* PAIR: the companion, 0 (y0) or 1 (y1) */
  double a, b;   /* CMP, REPEAT: the operand a; OUTSIDE: the bounds a, b */
} xh_flag_check;

/* xh_data_flags: the checks of data_flags (core/dataflags.py:581-746) on one variable, aggregated; one lane per cell walks the
 *   whole series once.
 *   x (T, C), pitch ld; companions y0 / y1 (T, C) with pitches ld_y0 / ld_y1 >= C, NULL when no PAIR check names them.
 *   checks (HOST, K <= XH_FLAGS_MAX_CHECKS entries).  XH_ERR_ARG for an unknown kind, an operator outside XH_OP_GT .. XH_OP_NE
 *   (REPEAT: or -1), n < 1, other outside {0, 1} or a PAIR without its companion; XH_ERR_LIMIT for K > XH_FLAGS_MAX_CHECKS.
 *   seg (HOST int64, P + 1): first row of every period, seg[0] == 0, seg[P] == T, non-decreasing (empty periods are allowed);
 *   anything else is XH_ERR_ARG.  P == T with one row per period gives the element-wise masks.  T < 2^31 - 1 (XH_ERR_LIMIT).
 *   With a CLIM check: tidx (HOST int32, T), the row of the bound tables of every time step, inside [0, D); lo / hi (D, C) in
 *   the field's dtype with pitch ld_tab >= C, such as those of xh_doy_bounds.  Without one, tidx, D, lo, hi and ld_tab are
 *   ignored.
 *   out (uint8).  reduce_cells == 0: out[(k * P + p) * ld_out + c] = 1 when check k flags cell c on a row of period p, else 0
 *   (0 for an empty period); every element of the K * P rows is stored.  reduce_cells != 0: out[k * P + p] = 1 when check k
 *   flags any cell on a row of period p, else 0 (ld_out is checked but not used): the entry point zeroes the K * P bytes
 *   before the launch and lanes store the byte 1. */
int xh_data_flags(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const void* y0, int64_t ld_y0,
                  const void* y1, int64_t ld_y1, int K, const xh_flag_check* checks /* host */, int64_t P,
                  const int64_t* seg /* host */, const int32_t* tidx /* host */, int64_t D, const void* lo, const void* hi,
                  int64_t ld_tab, int reduce_cells, uint8_t* out, int64_t ld_out);

/* xh_doy_bounds: the two bound tables of outside_n_standard_deviations_of_climatology (core/dataflags.py:508-509) from
 *   climatological_mean_doy (core/calendar.py:907-931); the float64-capable, pitched sibling of xh_doy_mean_std.
 *   x (T, C).  tbase (HOST int32, nyears * ndoy): the row of (year, day of year), -1 when absent, as for xh_doy_mean_std; every
 *   entry inside [-1, T), XH_ERR_ARG otherwise.  window >= 1, nyears >= 1.
 *   For every (day of year d, cell): the samples are the rows t + j - window / 2, j = 0 .. window - 1, of every t = tbase[y, d]
 *   >= 0, in (year, window) order; rows outside [0, T) and NaN samples are left out.  With m samples, in float64:
 *   mu = sum / m, sig = sqrt(sum((v - mu)^2) / m).  Both are rounded to the field's dtype; then, every product and sum rounded
 *   in the field's dtype, lo[d, c] = mu - n * sig and hi[d, c] = mu + n * sig (n rounded to the field's dtype first).  NaN
 *   where m == 0.  lo / hi (ndoy, C) in the field's dtype with pitch ld_out >= C; every element is stored. */
int xh_doy_bounds(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const int32_t* tbase /* host */,
                  int nyears, int ndoy, int window, double n, void* lo, void* hi, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_FLAGS_H */
