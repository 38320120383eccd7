/* xclim_hip_distfit.h — the C ABI of the distribution-fit unit (xclim_amd/csrc/distfit.hip), exported by libxclimhip.so next to
 * the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py UNIT_SIGNATURES.  (Headers under include/units/ belong to units added while the ABI tests
 * over include/ *.h and include/ext/ *.h are frozen; every header of this directory is checked by tests/test_abi_units_cpu.py.)
 *
 * The unit is the other half of xclim.indices.stats (stats.py:45-548): fit, parametric_quantile / _cdf / _pdf, fa and
 * frequency_analysis for six scipy distributions.  One lane per cell; all arithmetic is float64 on the widened values, in the
 * order of operations of scipy 1.15 (the library is built with -ffp-contract=off).  The fit machinery (pairwise sums, the
 * penalized negative log-likelihood, Nelder-Mead, brentq, gammainc, digamma) is the one of xh_si_fit (xclim_amd/csrc/fitcore.h). */
#ifndef XCLIM_HIP_DISTFIT_H
#define XCLIM_HIP_DISTFIT_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the distributions; norm and gumbel_r have the parameters (loc, scale), the others (shape, loc, scale) */
#define XH_DIST_NORM 0
#define XH_DIST_GUMBEL_R 1
#define XH_DIST_GENEXTREME 2
#define XH_DIST_GAMMA 3
#define XH_DIST_FISK 4
#define XH_DIST_LOGNORM 5
#define XH_DIST_NDISTS 6

/* the methods of _fitfunc_1d: APP = the start values of _fit_start, ML = scipy's <dist>.fit(method="mle") from them */
#define XH_DIST_APP 0
#define XH_DIST_ML 1

/* the functions of xh_dist_eval, and of the fused levels of xh_dist_fit (PPF or ISF there) */
#define XH_DIST_PPF 0
#define XH_DIST_ISF 1
#define XH_DIST_CDF 2
#define XH_DIST_PDF 3

/* the most fused levels of one xh_dist_fit call (they travel in the kernel's arguments); more answer XH_ERR_LIMIT */
#define XH_DISTFIT_MAX_Q 16

/* the status byte of a cell */
#define XH_DISTFIT_FITTED 0  /* parameters written */
#define XH_DISTFIT_NAN 1     /* NaN by the reference's rules: fewer than two values, or a parameter that is NaN */
#define XH_DISTFIT_BUDGET 2  /* Nelder-Mead stopped at maxfun = 200 N evaluations; the parameters are its best vertex */
#define XH_DISTFIT_SUPPORT 3 /* a value at or below a fixed floc (gamma, lognorm): NaN parameters */

/* xh_dist_fit: the parameters of `dist` for every cell c < C of the (T, C) field x, one launch.
 *
 *   x, ld, f64   DEVICE field, float32 or float64 (f64 != 0), row pitch ld >= C.  NaN values of a cell are dropped; a cell with
 *                fewer than two values left gives NaN parameters (XH_DISTFIT_NAN).
 *   dist         one of XH_DIST_* (XH_ERR_ARG otherwise).
 *   method       XH_DIST_ML:
 *                  norm        mean, sqrt(mean((x - mean)^2));
 *                  gumbel_r    the root in scale of mean(x) - avg(x, weights exp(-x / scale)) - scale by brentq (rtol = xtol =
 *                              1e-14) on (0.5, 2) widened by halving and doubling until the signs differ, then
 *                              loc = -scale (logsumexp(-x / scale) - log n);
 *                  genextreme  Nelder-Mead (optimize.fmin, xtol = ftol = 1e-4, maxiter = maxfun = 600) over (c, loc, scale) on
 *                              _penalized_nnlf from (0.1, m - 0.57722 s, s), s = sqrt(6 var) / pi;
 *                  gamma, fisk as xh_si_fit: gamma with floc by brentq on log a - digamma a, otherwise Nelder-Mead over three
 *                              parameters, or two with floc, from the values of _fit_start;
 *                  lognorm     needs has_floc (XH_ERR_NOTIMPL without): scale = exp(mean(log(x - floc))), shape =
 *                              sqrt(mean((log(x - floc) - log scale)^2)); a cell whose smallest value is <= floc is
 *                              XH_DISTFIT_SUPPORT.
 *                XH_DIST_APP: genextreme (0.1, m - 0.57722 s, s); gamma, fisk, lognorm the values of _fit_start with loc =
 *                floc, or without has_floc with its loc estimate; norm and gumbel_r answer XH_ERR_NOTIMPL.
 *   has_floc, floc   a fixed loc: gamma, fisk and lognorm only (XH_ERR_NOTIMPL for the others).
 *   q, nq, qfunc HOST float64 (nq), 0 <= nq <= XH_DISTFIT_MAX_Q (XH_ERR_ARG below, XH_ERR_LIMIT above), qfunc XH_DIST_PPF or
 *                XH_DIST_ISF: levels[j * ld_levels + c] = qfunc(q[j]) of the cell's parameters, from the registers that hold them;
 *                bit for bit what xh_dist_eval gives on the stored parameters.  nq == 0: q and levels may be NULL.
 *   params       DEVICE float64 (nparams, C) with row pitch ld_params >= C; nparams = 2 for norm and gumbel_r, else 3.
 *   nfev         DEVICE int32 (C) or NULL: the objective evaluations of the cell's Nelder-Mead (0 for the other routes).
 *   status       DEVICE uint8 (C) or NULL: XH_DISTFIT_*.
 *   levels       DEVICE float64 (nq, C) with row pitch ld_levels >= C.
 *
 * Every element (k, c < C) of params, nfev, status and levels is written by every call that returns XH_OK with C > 0, and nothing
 * beyond column C of a row.  The sample of a lane is staged once as float64: T <= 32 in LDS (256 bytes per lane), a longer
 * series slot-major in the context's scratch (8 T C bytes).  Every check answers before anything is launched; C == 0 launches
 * nothing and returns XH_OK.  Where scipy raises for a cell (brentq without a sign change, Nelder-Mead ending off the parameter
 * domain) the cell is XH_DISTFIT_NAN. */
int xh_dist_fit(xh_ctx* ctx, const void* x, int64_t T, int64_t C, int64_t ld, int f64, int dist, int method, int has_floc,
                double floc, const double* q /* host */, int nq, int qfunc, double* params, int64_t ld_params, int32_t* nfev,
                uint8_t* status, double* levels, int64_t ld_levels);

/* xh_dist_eval: out[j * ld_out + c] = func(v[j]) of scipy's rv_continuous of `dist` with the parameters of cell c.
 *
 *   func     XH_DIST_PPF / _ISF (v: probabilities; NaN outside [0, 1], the ends of the support at 0 and 1), XH_DIST_CDF / _PDF
 *            (v: values; 0 below the support, 1 above it for the cdf).  NaN for NaN or invalid parameters, as scipy's badvalue.
 *            gamma's ppf and isf invert the regularized incomplete gamma function by safeguarded Newton steps (isf(q) as
 *            ppf(1 - q)); everything else is scipy's _ppf / _isf / _cdf / _pdf in its order of operations.
 *   params   DEVICE float64 (nparams, C), row pitch ld_params >= C.
 *   v, nv    HOST float64 (nv), nv >= 0 (at most 65535: XH_ERR_LIMIT above).
 *   out      DEVICE float64 (nv, C), row pitch ld_out >= C; every element (j, c < C) is written, nothing beyond column C. */
int xh_dist_eval(xh_ctx* ctx, int dist, int func, const double* params, int64_t C, int64_t ld_params, const double* v /* host */,
                 int nv, double* out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_DISTFIT_H */
