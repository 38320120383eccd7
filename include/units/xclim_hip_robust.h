/* xclim_hip_robust.h — the C ABI of the ensemble change-robustness unit (xclim_amd/csrc/robust.hip), exported by libxclimhip.so
 * next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py UNIT_SIGNATURES; checked by tests/test_abi_units_cpu.py.
 *
 * The unit serves xclim.ensembles._robustness (robustness_fractions, _robustness.py:74-333, and its significance tests,
 * :518-633): where the reference makes one scipy call per (cell, realization), xh_change_test is one launch with one lane per
 * (realization, cell) series pair, and xh_robust_fractions folds the members of a cell into the seven fractions.  All
 * arithmetic is float64 on values widened on load, in the order of operations of scipy 1.15 and numpy's pairwise sum (the
 * library is built with -ffp-contract=off).  Integer fields are not served. */
#ifndef XCLIM_HIP_ROBUST_H
#define XCLIM_HIP_ROBUST_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the tests of xh_change_test */
#define XH_CT_MOMENTS 0 /* delta, mean_ref and the counts only: test=None, "threshold", "ipcc-ar6-c" */
#define XH_CT_TTEST 1   /* ttest_1samp(f, mean_ref, nan_policy="omit") */
#define XH_CT_WELCH 2   /* ttest_ind(f, r, equal_var=False, nan_policy="omit") */
#define XH_CT_MWU 3     /* mannwhitneyu(f, r, nan_policy="omit"), two-sided, method="auto" */
#define XH_CT_BF 4      /* levene(f, r, center="median") */
#define XH_CT_NTESTS 5

/* the status byte of a series pair */
#define XH_CT_DONE 0          /* stat, df and pvals written as scipy gives them */
#define XH_CT_NAN 1           /* NaN where scipy answers NaN: an all-NaN series, n < 2 for the t-tests, 0 / 0 in t, a NaN for BF */
#define XH_CT_EXACT_PENDING 2 /* MWU by the exact route with counts other than (T1, T2): stat = U1 written, pvals NaN; the host
                                 finishes the pair from the null distribution of its own counts */

/* the longest series, and the staged length (non-NaN slots of both series, T1 + T2) up to which a lane's sample lives in LDS;
 * a longer one is staged slot-major in the context's work buffer by the same code */
#define XH_CT_MAX_T 512
#define XH_CT_LDS_SLOTS 64

/* the rows of the output of xh_robust_fractions, in the order of the reference's Dataset */
#define XH_RF_CHANGED 0
#define XH_RF_POSITIVE 1
#define XH_RF_CHANGED_POSITIVE 2
#define XH_RF_NEGATIVE 3
#define XH_RF_CHANGED_NEGATIVE 4
#define XH_RF_VALID 5
#define XH_RF_AGREE 6
#define XH_RF_NFRAC 7

/* the threshold of xh_robust_fractions */
#define XH_RF_THRESH_NONE 0
#define XH_RF_THRESH_ABS 1 /* changed = |delta| > thresh */
#define XH_RF_THRESH_REL 2 /* changed = |delta / mean_ref| > thresh */

/* the most pooled values of xh_robust_coefficient: R T1 + R and T2 + R, padded to a power of two, are sorted in LDS.  The block's
 * LDS is the padded pool (at most 64 KiB) + the R member means + 64 lane sums: 8 (npad + R + 64) bytes, 66 176 for 16 members of
 * 511 values, at most 8 (8192 + 8191 + 64) bytes; above 64 KiB the launch asks for the larger dynamic allocation first */
#define XH_RC_MAX_POOL 8192

/* xh_change_test: the change statistics of every (realization r < R, cell c < C) series pair, one launch.
 *
 *   fut, ref     DEVICE fields, both float32 or both float64 (f64 != 0).  Element (r, t, c) of fut is at r * stride_r_fut +
 *                t * ld_fut + c (t < T1), of ref at r * stride_r_ref + t * ld_ref + c (t < T2); ld_* >= C; nothing is transposed.
 *                stride_r_ref == 0 serves a ref without realizations.  NaN values are dropped.
 *   test         one of XH_CT_* (XH_ERR_ARG otherwise).
 *   sf, nsf      HOST float64: for XH_CT_MWU with min(T1, T2) <= 8, the survival function sf[0 .. T1 * T2] of U under the null
 *                hypothesis for the full counts (T1, T2), nsf == T1 * T2 + 1 (XH_ERR_ARG otherwise).  Otherwise NULL, 0: with both
 *                lengths above 8 the exact route is taken by pairs with dropped values only, which are XH_CT_EXACT_PENDING.
 *   delta        DEVICE float64 (R, C): mean of the non-NaN fut values - mean of the non-NaN ref values, each mean numpy's pairwise
 *                sum of the compacted series / count (NaN for an empty series).
 *   mean_ref     DEVICE float64 (R, C): that mean of ref.
 *   n_fut, n_ref DEVICE int32 (R, C): the non-NaN counts.
 *   stat, df, pvals, status   DEVICE float64, float64, float64, uint8 (R, C); needed unless test == XH_CT_MOMENTS, where they are
 *                not touched and may be NULL.
 *                  TTEST  stat = t = (mean - mean_ref) / sqrt(var_ddof1 / n), df = n - 1, pvals = 2 sf_t(|t|, df).
 *                  WELCH  stat = t = (m1 - m2) / sqrt(v1 / n1 + v2 / n2), df = scipy's (1 where the formula is NaN).
 *                  MWU    stat = U1 (of fut), df = the tie term sum(t^3 - t), both exact integers found by counting.  Both counts
 *                         > 8, or a tie: z = (max(U1, U2) - n1 n2 / 2 - 0.5) / s, pvals = min(1, erfc(z / sqrt 2)), s == 0 gives 1.
 *                         Otherwise the exact route: counts == (T1, T2) gives pvals = min(1, 2 sf[max(U1, U2)]), other counts
 *                         XH_CT_EXACT_PENDING.
 *                  BF     stat = W in scipy's order with the medians by counting selection, df = N - 2, pvals = sf_F(W, 1, N - 2);
 *                         a NaN in either series gives NaN (the reference passes no nan_policy).
 *                Both tails are one regularized incomplete beta function (xclim_amd/csrc/betainc.h).  A constant series that
 *                differs from the mean gives t = +-inf and pvals = 0.
 *   ld_out       the row pitch of all outputs, >= C.
 *
 * Every element (r, c < C) of the outputs named above is written by every call that returns XH_OK, nothing beyond column C of a
 * row.  T1, T2 in 1 .. XH_CT_MAX_T (XH_ERR_LIMIT above), R in 1 .. 65535.  Every check answers before anything is launched;
 * C == 0 launches nothing and returns XH_OK.  A lane stages its compacted sample in the fields' type: T1 + T2 <= XH_CT_LDS_SLOTS
 * in LDS, longer slot-major in the context's work buffer ((T1 + T2) R C elements). */
int xh_change_test(xh_ctx* ctx, const void* fut, const void* ref, int64_t R, int64_t T1, int64_t T2, int64_t C, int64_t ld_fut,
                   int64_t stride_r_fut, int64_t ld_ref, int64_t stride_r_ref, int f64, int test, const double* sf /* host */,
                   int64_t nsf, double* delta, double* mean_ref, int32_t* n_fut, int32_t* n_ref, double* stat, double* df,
                   double* pvals, uint8_t* status, int64_t ld_out);

/* xh_robust_fractions: the seven fractions of _robustness.py:257-271, 319 for every cell c < C, one lane per cell.
 *
 *   delta        DEVICE float64 (R, C), row pitch ld >= C.
 *   changed      DEVICE uint8 (R, C), pitch ld, or NULL: every member changed (or the threshold decides, below).
 *   valid        DEVICE uint8 (R, C), pitch ld, or NULL: a member is valid where its delta is not NaN.
 *   mean_ref     DEVICE float64 (R, C), pitch ld: needed for XH_RF_THRESH_REL only.
 *   weights      HOST float64 (R).
 *   strict_sign  != 0: positive is delta > 0 and negative delta < 0; 0: >= and <=.
 *   thresh_kind, thresh   XH_RF_THRESH_ABS / _REL: changed is decided here and `changed` must be NULL (XH_ERR_ARG otherwise).
 *   out          DEVICE float64 (XH_RF_NFRAC, C), row pitch ld_out >= C.  With n_valid = the sum of w over the valid members,
 *                added in realization order like every sum here: changed, positive, changed_positive, negative and
 *                changed_negative are the sums of w over the valid members with the property / n_valid; valid = n_valid / R;
 *                agree = max(positive, negative, 1 - positive - negative).  A NaN (no valid member) is written as 0.
 *
 * Every element (k, c < C) of out is written, nothing beyond column C.  R >= 1; C == 0 launches nothing. */
int xh_robust_fractions(xh_ctx* ctx, const double* delta, const uint8_t* changed, const uint8_t* valid, const double* mean_ref,
                        int64_t R, int64_t C, int64_t ld, const double* weights /* host */, int strict_sign, int thresh_kind,
                        double thresh, double* out, int64_t ld_out);

/* xh_robust_coefficient: the robustness coefficient of Knutti and Sedlacek (_robustness.py:430-515) for every cell c < C, one
 * wave per cell.
 *
 *   fut          DEVICE field (R, T1, C), float32 or float64 (f64 != 0): element (r, t, c) at r * stride_r_fut + t * ld_fut + c.
 *   ref          DEVICE field (T2, C) of the same type, row pitch ld_ref >= C.
 *   out          DEVICE float64 (C): 1 - A1 / A2 with A1 = A(v_fut, v_favg), A2 = A(v_ref, v_favg); v_fut the R T1 future values,
 *                v_favg the R per-member time means (numpy's pairwise mean), v_ref the T2 reference values, and
 *                A(x1, x2) = sum_k (x_{k+1} - x_k) (cnt1_k / n1 - cnt2_k / n2)^2 over the pooled sorted values with the inclusive
 *                counts of each sample: the reference's np.insert construction (equal values have no width, their order is
 *                free).  The pool is sorted in LDS by a bitonic network; the terms, all non-negative, are added per lane and
 *                the 64 lane sums in lane order.  Any NaN in the cell gives NaN.
 *   a1, a2       DEVICE float64 (C) or NULL: A1 and A2.
 *
 * Every element c < C of out (and of a1, a2 when given) is written.  R T1 + R and T2 + R at most XH_RC_MAX_POOL and T1 at most
 * XH_CT_MAX_T (XH_ERR_LIMIT above).  Every check answers before anything is launched; C == 0 launches nothing. */
int xh_robust_coefficient(xh_ctx* ctx, const void* fut, const void* ref, int64_t R, int64_t T1, int64_t T2, int64_t C, int64_t ld_fut,
                          int64_t stride_r_fut, int64_t ld_ref, int f64, double* out, double* a1, double* a2);

/* xh_ar6_gamma: the threshold gamma of the reference's _ipcc_ar6_c (_robustness.py:636-661) from ANNUAL values, one lane per
 * (realization r < R, cell c < C).
 *
 *   y            DEVICE field (R, T, C), float32 or float64 (f64 != 0): element (r, t, c) at r * stride_r + t * ld + c; NaN years
 *                are left out of the fit and of the statistics.
 *   x            HOST float64 (T): the abscissa of the years (days since the first stamp).
 *   deg          1 or 2: the least-squares polynomial that is subtracted, fitted on x centred on its mean and scaled by its largest
 *                distance from it over the years that are not NaN.
 *   seg, nb      HOST int64 (nb + 1) non-decreasing offsets into the years: the residuals are averaged per block [seg[k], seg[k+1])
 *                first (a block without a value is left out); nb == 0 and seg NULL: no blocks.
 *   gamma        DEVICE float64 (R, C), row pitch ld_out >= C: factor * std (ddof 0) of the residuals, or of their block means;
 *                NaN where fewer than deg + 1 years have a value.
 *
 * Every element (r, c < C) of gamma is written, nothing beyond column C.  T at most XH_CT_MAX_T (XH_ERR_LIMIT above), R in
 * 1 .. 65535.  Every check answers before anything is launched; C == 0 launches nothing. */
int xh_ar6_gamma(xh_ctx* ctx, const void* y, int64_t R, int64_t T, int64_t C, int64_t ld, int64_t stride_r, int f64,
                 const double* x /* host */, int deg, const int64_t* seg /* host */, int64_t nb, double factor, double* gamma,
                 int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_ROBUST_H */
