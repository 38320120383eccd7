/* xclim_hip_partition.h — the C ABI of the ensemble uncertainty-partitioning unit (xclim_amd/csrc/partition.hip), exported by
 * libxclimhip.so next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the
 * conventions.  ctypes prototypes: xclim_amd/_capi.py UNIT_SIGNATURES; checked by tests/test_abi_units_cpu.py.
 *
 * The unit serves xclim.ensembles._partitioning (hawkins_sutton, lafferty_sriver, general_partition) and ensemble_mean_std_max_min
 * of xclim.ensembles._base.  Where the reference fits one polynomial per series in Python whenever a value is NaN and then reads
 * the smoothed cube seven to nine times, xh_partition_smooth fits and smooths every series in one launch and
 * xh_partition_components folds the member axes into the variance components in another.  All arithmetic is float64 on values
 * widened on load (the library is built with -ffp-contract=off); float32 and float64 fields are read natively.  Integer fields are
 * not served. */
#ifndef XCLIM_HIP_PARTITION_H
#define XCLIM_HIP_PARTITION_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the longest series and the highest degree of xh_partition_smooth */
#define XH_PT_MAX_T 512
#define XH_PT_MAX_DEG 4

/* the rolling statistic of the residual: the centred mean over 10 rows, or the centred variance (ddof 0) over 11 rows */
#define XH_PT_ROLL_MEAN 0
#define XH_PT_ROLL_VAR 1

/* the status byte of a series */
#define XH_PT_FITTED 0
#define XH_PT_ALLNAN 1   /* no year has a value: sm and roll are NaN, as the reference gives them */
#define XH_PT_ILLPOSED 2 /* fewer than deg + 1 years with a value, or a Cholesky pivot below T 2^-52 times the largest diagonal
                            entry of the Gram matrix (the analogue of lstsq's rcond): sm and roll are NaN and the flag is raised;
                            the reference's minimum-norm answer is not reproduced */

/* the baseline of xh_partition_smooth */
#define XH_PT_BASE_NONE 0
#define XH_PT_BASE_SUB 1 /* kind "+": sm - ref */
#define XH_PT_BASE_DIV 2 /* kind "*": sm / ref */

/* the member axes of xh_partition_components: at most 4, each of at most 64 entries, their product at most 4096; at most 8
 * components */
#define XH_PT_MAX_AXES 4
#define XH_PT_MAX_AXIS 64
#define XH_PT_MAX_MEMBERS 4096
#define XH_PT_MAX_COMP 8

/* the rule of a component */
#define XH_PT_VAR_THEN_MEAN 0 /* the variance over the axis, then the mean over the pooled other axes */
#define XH_PT_MEAN_THEN_VAR 1 /* the mean over the pooled other axes, then the variance over the axis */

/* the weights of a component */
#define XH_PT_W_NONE 0
#define XH_PT_W_COUNT 1 /* VAR_THEN_MEAN only: the mean over the others is weighted by the number of non-NaN entries along the axis */
#define XH_PT_W_USER 2  /* the host vector `weights` over `w_axis`: VAR_THEN_MEAN needs axis == w_axis (a weighted variance),
                           MEAN_THEN_VAR needs axis != w_axis (a weighted inner mean) */

/* the variability rule of a launch */
#define XH_PT_VARIAB_MEAN_ALL 0 /* the mean of roll[t] over all members */
#define XH_PT_VARIAB_HS 1       /* per entry of w_axis the pooled variance of roll over (the other axes, rows >= t0), then the mean
                                   over w_axis weighted by `weights`: one value per cell, written into every row */

/* the rows of the output of xh_ensemble_stats */
#define XH_ES_MEAN 0
#define XH_ES_STD 1
#define XH_ES_MAX 2
#define XH_ES_MIN 3
#define XH_ES_NSTAT 4

/* xh_partition_smooth: the polynomial fit over time, its masked values and the centred rolling statistic of the residual of every
 * (series n < N, cell c < C), one lane per series, one launch.
 *
 *   y            DEVICE field (T, N, C), float32 or float64 (f64 != 0): element (t, n, c) at t * ld + n * stride_n + c, with
 *                stride_n >= C and ld >= (N - 1) * stride_n + C.  NaN years are left out of the fit.  May be NULL when sm_in is
 *                given and roll is NULL.
 *   sm_in        DEVICE field of the same type and layout, or NULL.  Given: nothing is fitted (q is NULL, deg is 0); it is taken
 *                as is, NOT masked by y; n_valid counts its non-NaN years and every series is XH_PT_FITTED.
 *   q, deg       HOST float64 (T, deg + 1), deg in 0 .. XH_PT_MAX_DEG: the orthonormal basis of the polynomials of degree <= deg
 *                over ALL T years (the Q factor of the Vandermonde matrix of the centred and scaled abscissa).  A lane adds
 *                G = sum q q^T and b = sum q y over its non-NaN years in row order, solves G a = b by Cholesky and evaluates
 *                sum_k a_k q[t][k], k ascending.
 *   window, stat the rolling statistic of the residual y - sm: (10, XH_PT_ROLL_MEAN) or (11, XH_PT_ROLL_VAR); any other pair
 *                is XH_ERR_ARG.  The window of row i covers rows i - window / 2 .. i + (window - 1) / 2, its values are added in
 *                row order, and the result is NaN unless every row of the window exists and is not NaN.
 *   base_kind, b0, b1   XH_PT_BASE_SUB / _DIV: the written sm is sm - ref or sm / ref with ref the mean, in row order, of the
 *                non-NaN sm of rows [b0, b1), 0 <= b0 <= b1 <= T (NaN when there is none).  roll always uses the unshifted sm.
 *   sm, roll     DEVICE float64 (T, N, C): element (t, n, c) at t * ld_out + n * stride_n_out + c, same conditions.  sm is NaN
 *                where y is NaN (where sm_in is NaN).  Either may be NULL, not both (XH_ERR_ARG).
 *   n_valid      DEVICE int32 (N, C), row pitch ld_nc >= C, or NULL: the years that entered the fit.
 *   status       DEVICE uint8 (N, C), row pitch ld_nc, or NULL: XH_PT_*.
 *   flag         DEVICE uint8 (1) or NULL: set to 0 by the call, then to 1 by every ill-posed series.
 *
 * Every element (., n, c < C) of every given output is written by every call that returns XH_OK, nothing beyond column C of a
 * row.  T in 1 .. XH_PT_MAX_T (XH_ERR_LIMIT above), N in 1 .. 65535.  Every check answers before anything is launched; C == 0
 * launches nothing and returns XH_OK.  The window is a register file of 11 residuals per lane that shifts by one per row: no
 * LDS and no work buffer. */
int xh_partition_smooth(xh_ctx* ctx, const void* y, const void* sm_in, int64_t T, int64_t N, int64_t C, int64_t ld, int64_t stride_n,
                        int f64, const double* q /* host */, int deg, int window, int stat, int base_kind, int64_t b0, int64_t b1,
                        double* sm, double* roll, int64_t ld_out, int64_t stride_n_out, int32_t* n_valid, uint8_t* status,
                        int64_t ld_nc, uint8_t* flag);

/* xh_partition_components: the variance components of every (row t < T, cell c < C), one lane each.
 *
 *   sm, roll     DEVICE float64 (T, A0, A1, A2, A3, C): element (t, n, c) at t * ld + n * stride_n + c with the member index
 *                n = ((i0 A1 + i1) A2 + i2) A3 + i3, same conditions as above.
 *   dims         HOST int64 (XH_PT_MAX_AXES): A0 .. A3, each in 1 .. XH_PT_MAX_AXIS, product at most XH_PT_MAX_MEMBERS
 *                (XH_ERR_LIMIT above); an absent axis has length 1.
 *   comps, K     HOST int32 (K, 3): {axis, rule, weight} of each component, 0 <= K <= XH_PT_MAX_COMP.
 *   weights, w_axis   HOST float64 (dims[w_axis]) for XH_PT_W_USER and XH_PT_VARIAB_HS, or NULL.  When given, the mean over
 *                w_axis in g is weighted as well.
 *   variab, t0   one of XH_PT_VARIAB_*; t0 in 0 .. T is the first row of the HS variance.
 *   g_order      HOST int32 (XH_PT_MAX_AXES): a permutation of 0 .. 3, the order in which g takes its nested means.
 *   out          DEVICE float64 (K + 2, T, C): element (k, t, c) at (k T + t) ld_out + c.  Plane 0 is the variability, planes
 *                1 .. K the components in the order of comps, plane K + 1 the total: the variability plus the components, added
 *                in that order.
 *   g            DEVICE float64 (T, C), row pitch ld_out, or NULL: mean over g_order[3] of the mean over g_order[2] of ...
 *
 * Every reduction skips NaN, has ddof 0 (a variance is sum (x - mean)^2 / n around the mean of the same values, a weighted one
 * sum w (x - mean_w)^2 / sum w), adds in index order and is NaN when nothing is valid; a NaN inner result is skipped by the
 * outer reduction, and carries no weight.  Every element (k, t, c < C) of out and g is written, nothing beyond column C.  Every
 * check answers before anything is launched; C == 0 launches nothing.  XH_PT_VARIAB_HS runs a second small kernel, one lane per
 * cell, before the main one; its C values live in the context's work buffer. */
int xh_partition_components(xh_ctx* ctx, const double* sm, const double* roll, int64_t T, const int64_t* dims /* host */, int64_t C,
                            int64_t ld, int64_t stride_n, const int32_t* comps /* host */, int K, const double* weights /* host */,
                            int w_axis, int variab, int64_t t0, const int32_t* g_order /* host */, double* out, int64_t ld_out,
                            double* g);

/* xh_ensemble_stats: mean, standard deviation (ddof 0), maximum and minimum over the realizations of every element e < E, one
 * lane each.
 *
 *   x            DEVICE field (R, E), float32 or float64 (f64 != 0), row pitch ld >= E.  NaN values are skipped.
 *   weights      HOST float64 (R) or NULL: the mean is sum w x / sum w and the variance sum w (x - mean)^2 / sum w over the
 *                non-NaN values.
 *   min_members  an element with fewer non-NaN realizations has NaN in all four rows.
 *   out          DEVICE float64 (XH_ES_NSTAT, E), row pitch ld_out >= E.
 *
 * Every element (k, e < E) of out is written, nothing beyond column E.  R in 1 .. 65535; E == 0 launches nothing. */
int xh_ensemble_stats(xh_ctx* ctx, const void* x, int64_t R, int64_t E, int64_t ld, int f64, const double* weights /* host */,
                      int min_members, double* out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_PARTITION_H */
