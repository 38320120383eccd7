// stdidx.hip — standardized indices (SPI / SPEI): the per-group distribution fits and the probability transform of
// indices/stats.py.
//
// Reference: _fitfunc_1d (stats.py:40-113), _fit_start (:576-684), standardized_index_fit_params (:855-964) and
// standardized_index (:967-1197); underneath them scipy 1.15's gamma_gen.fit (the floc special case), rv_continuous.fit
// -> optimize.fmin (_minimize_neldermead, non-adaptive), _penalized_nnlf / _nnlf_and_penalty, gammainc, burr._cdf and
// norm.ppf.  The reference fits one (cell, group) at a time through a Python-level scipy call; here one lane owns one
// (cell, group), lanes run along the cells (every row of a group's sample is one coalesced read), and the whole fit —
// start values, brentq or Nelder–Mead — runs in registers in float64.
//
// Arithmetic is written in the reference's order so that a fit follows scipy's trajectory: numpy's pairwise sums are
// reproduced for samples of up to 128 values (np.add.reduce: 8 interleaved partial sums past 7 values; longer samples are
// summed in that form over their whole length, where numpy splits recursively), the simplex moves use scipy's
// coefficients as written, and the file is built with -ffp-contract=off (no FMA contraction).  What can still differ
// is the last bit of log / pow / lgamma, which can send a Nelder–Mead fit down a slightly different path to the same
// optimum (tests/test_gpu_stdidx.py reports the share of fits that match scipy to 1e-8).
//
// The fit and the transform are templates on the field's element type: float (xh_si_fit / xh_si_apply) and double
// (xh_si_fit_f64 / xh_si_apply_f64).  A float64 field is read, compared against zero and staged as double, never narrowed;
// past the read both instances run the same float64 arithmetic.
#include "fitcore.h"

namespace {

template <typename E>
struct FitArgs {
  const E* x;
  int64_t C, st;
  const int32_t* rows;  // the calibration rows of every group, group after group
  const int32_t* off;   // (G + 1) offsets into rows
  int dist, method, has_floc, zero_inflated, lds;
  double floc;
  E* work;  // global staging (lds == 0): (rows, C)
  double* params;  // (G, 3, C)
  double* nzeros;  // (G, C) or NULL
  double* nnotnull;
  int32_t* nfev;  // (G, C) or NULL
};

template <typename E>
__global__ void __launch_bounds__(FIT_BLOCK) k_si_fit(FitArgs<E> a) {
  extern __shared__ float lds_f[];  // the kernel's only LDS, at offset 0: aligned for double
  E* lds = reinterpret_cast<E*>(lds_f);
  const int64_t c = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
  const int g = blockIdx.y;
  if (c >= a.C) return;
  const int r0 = a.off[g], m = a.off[g + 1] - r0;
  // stage the sample: drop NaN (and zeros when zero-inflated), count the zeros and the valid values
  E* dst = a.lds ? lds + threadIdx.x : a.work + (int64_t)r0 * a.C + c;
  const int64_t dstride = a.lds ? FIT_BLOCK : a.C;
  int n = 0, nz = 0, nn = 0;
  for (int k = 0; k < m; ++k) {
    const E v = a.x[(int64_t)a.rows[r0 + k] * a.st + c];
    if (v != v) continue;
    ++nn;
    if (v == (E)0) {
      ++nz;
      if (a.zero_inflated) continue;
    }
    dst[(int64_t)n * dstride] = v;
    ++n;
  }
  const Sample<E> s{dst, dstride, n};
  double pr[3] = {NAN, NAN, NAN};
  int nfev = 0;
  if (n > 1) {
    if (a.method == XH_SI_APP) {
      double p0, scale0;
      fit_start(a.dist, s, a.floc, p0, scale0);
      pr[0] = p0;
      pr[1] = a.floc;
      pr[2] = scale0;
    } else if (a.dist == XH_SI_GAMMA && a.has_floc) {
      // gamma_gen.fit's floc case: every value must lie above floc (scipy raises FitDataError; NaN here)
      bool ok = true;
      for (int k = 0; k < n; ++k) ok = ok && s[k] > a.floc;
      if (ok) {
        PwSum sx, sl;
        sx.init(n);
        sl.init(n);
        for (int k = 0; k < n; ++k) {
          const double d = a.floc != 0.0 ? s[k] - a.floc : s[k];
          sx.add(k, d);
          sl.add(k, log(d));
        }
        const double xbar = sx.sum() / (double)n;
        const double sv = log(xbar) - sl.sum() / (double)n;
        const double sh = gamma_shape_root(sv);
        pr[0] = sh;
        pr[1] = a.floc;
        pr[2] = xbar / sh;
      }
    } else {
      const double loc0 = a.has_floc ? a.floc : loc_estimation(s);
      double p0, scale0;
      fit_start(a.dist, s, loc0, p0, scale0);
      double xv[3] = {p0, loc0, scale0};
      if (!isnan64(p0) && !isnan64(loc0) && !isnan64(scale0)) {
        nfev = a.has_floc ? nelder_mead<2>(a.dist, s, a.floc, xv) : nelder_mead<3>(a.dist, s, 0.0, xv);
        // rv_continuous.fit raises FitError off the parameter domain: NaN here
        if (xv[0] > 0.0 && xv[2] > 0.0) {
          pr[0] = xv[0];
          pr[1] = xv[1];
          pr[2] = xv[2];
        }
      }
    }
    if (isnan64(pr[0]) || isnan64(pr[1]) || isnan64(pr[2])) pr[0] = pr[1] = pr[2] = NAN;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) a.params[((int64_t)g * 3 + k) * a.C + c] = pr[k];
  // a group without calibration rows is absent from the reference's parameters: NaN counts after its reindexing
  if (a.nzeros) a.nzeros[(int64_t)g * a.C + c] = m > 0 ? (double)nz : NAN;
  if (a.nnotnull) a.nnotnull[(int64_t)g * a.C + c] = m > 0 ? (double)nn : NAN;
  if (a.nfev) a.nfev[(int64_t)g * a.C + c] = nfev;
}

template <typename E>
struct ApplyArgs {
  const E* x;
  int64_t T, C, st, st_out;
  const int32_t* group;  // (T) device: group of every row, -1 = none (NaN out)
  const double* params;  // (G, 3, C)
  const double* nzeros;  // (G, C) or NULL: no zero-inflated mixture
  const double* nnotnull;
  int dist;
  double alpha, beta, interp;
  double* out;
};

// standardized_index (stats.py:1156-1190): cdf, the zero-inflated mixture, norm.ppf, clip to +-8.21; one thread per value
template <typename E>
__global__ void k_si_apply(ApplyArgs<E> a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.T * a.C) return;
  const int64_t t = i / a.C, c = i - t * a.C;
  const int g = a.group[t];
  double si = NAN;
  if (g >= 0) {
    const double v = (double)a.x[t * a.st + c];
    const double* pp = a.params + (int64_t)g * 3 * a.C + c;
    const double p0 = pp[0], loc = pp[a.C], scale = pp[2 * a.C];
    double prob;
    if (a.nzeros) {
      const double nz = a.nzeros[(int64_t)g * a.C + c], nn = a.nnotnull[(int64_t)g * a.C + c];
      const double den = ((nn + 1.0) - a.alpha) - a.beta;
      const double rank1 = (1.0 - a.alpha) / den;
      const double rankn = (nz - a.alpha) / den;
      if (v == 0.0) prob = (1.0 - a.interp) * rank1 + a.interp * rankn;
      else prob = rankn + (1.0 - rankn) * dist_cdf(a.dist, v, p0, loc, scale);
    } else {
      prob = dist_cdf(a.dist, v, p0, loc, scale);
    }
    si = norm_ppf_clipped(prob);
  }
  a.out[t * a.st_out + c] = si;
}

// ---- host entry points (one template per pair of twins; fn names the entry point in error messages) -------------
template <typename E>
int si_fit(const char* fn, xh_ctx* ctx, const E* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G, int dist,
           int method, int has_floc, double floc, int zero_inflated, int staging, double* params, double* nzeros,
           double* nnotnull, int32_t* nfev) {
  constexpr int lds_max = LDS_MAX_N<E>;
  XH_REQUIRE(ctx && group && params, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && C >= 0 && G >= 1 && G <= 65535, XH_ERR_ARG, "%s: bad shape (T %lld, C %lld, G %d)", fn,
             (long long)T, (long long)C, G);
  XH_REQUIRE(T == 0 || C == 0 || (x && st >= C), XH_ERR_LAYOUT, "%s: needs a time-major view (st >= C)", fn);
  XH_REQUIRE(dist == XH_SI_GAMMA || dist == XH_SI_FISK, XH_ERR_ARG, "%s: unknown distribution %d", fn, dist);
  XH_REQUIRE(method == XH_SI_APP || method == XH_SI_ML, XH_ERR_ARG, "%s: unknown method %d", fn, method);
  XH_REQUIRE(method != XH_SI_APP || has_floc, XH_ERR_ARG, "%s: the APP method needs floc", fn);
  XH_REQUIRE(staging >= XH_SI_STAGE_AUTO && staging <= XH_SI_STAGE_LDS, XH_ERR_ARG, "%s: unknown staging %d", fn, staging);
  XH_REQUIRE((nzeros == nullptr) == (nnotnull == nullptr), XH_ERR_ARG, "%s: nzeros and nnotnull go together", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  // the rows of every group, in time order
  int32_t* off = (int32_t*)calloc((size_t)G + 1, sizeof(int32_t));
  int32_t* rows = (int32_t*)malloc(sizeof(int32_t) * (size_t)(T > 0 ? T : 1));
  if (!off || !rows) {
    free(off);
    free(rows);
    xh_set_error("%s: out of host memory", fn);
    return XH_ERR_HIP;
  }
  for (int64_t t = 0; t < T; ++t) {
    if (group[t] < -1 || group[t] >= G) {
      free(off);
      free(rows);
      xh_set_error("%s: group[%lld] = %d outside -1..%d", fn, (long long)t, (int)group[t], G - 1);
      return XH_ERR_ARG;
    }
    if (group[t] >= 0) ++off[group[t] + 1];
  }
  int maxm = 0;
  for (int g = 0; g < G; ++g) {
    maxm = off[g + 1] > maxm ? off[g + 1] : maxm;
    off[g + 1] += off[g];
  }
  const int nrows = off[G];
  {
    int32_t* fill = (int32_t*)malloc(sizeof(int32_t) * (size_t)G);
    if (!fill) {
      free(off);
      free(rows);
      xh_set_error("%s: out of host memory", fn);
      return XH_ERR_HIP;
    }
    memcpy(fill, off, sizeof(int32_t) * (size_t)G);
    for (int64_t t = 0; t < T; ++t)
      if (group[t] >= 0) rows[fill[group[t]]++] = (int32_t)t;
    free(fill);
  }
  bool lds = staging == XH_SI_STAGE_LDS || (staging == XH_SI_STAGE_AUTO && maxm <= lds_max);
  if (staging == XH_SI_STAGE_LDS && maxm > lds_max) {
    free(off);
    free(rows);
    xh_set_error("%s: LDS staging holds at most %d values per group, got %d", fn, lds_max, maxm);
    return XH_ERR_LIMIT;
  }
  size_t cur = 0;
  void* d_off = nullptr;
  void* d_rows = nullptr;
  int rc = xh_scratch_upload(ctx, &cur, off, sizeof(int32_t) * ((size_t)G + 1), &d_off);
  if (!rc) rc = xh_scratch_upload(ctx, &cur, rows, sizeof(int32_t) * (size_t)(nrows > 0 ? nrows : 1), &d_rows);
  free(off);
  free(rows);
  if (rc) return rc;
  FitArgs<E> a{};
  a.x = x;
  a.C = C;
  a.st = st;
  a.rows = (const int32_t*)d_rows;
  a.off = (const int32_t*)d_off;
  a.dist = dist;
  a.method = method;
  a.has_floc = has_floc != 0;
  a.zero_inflated = zero_inflated != 0;
  a.floc = floc;
  a.lds = lds;
  a.params = params;
  a.nzeros = nzeros;
  a.nnotnull = nnotnull;
  a.nfev = nfev;
  if (!lds && nrows > 0) {
    void* w = nullptr;
    rc = xh_big_scratch(ctx, sizeof(E) * (size_t)nrows * (size_t)C, &w);
    if (rc) return rc;
    a.work = (E*)w;
  }
  const size_t shmem = lds ? sizeof(E) * FIT_BLOCK * (size_t)(maxm > 0 ? maxm : 1) : 0;
  hipLaunchKernelGGL(k_si_fit<E>, dim3((unsigned)cdiv64(C, FIT_BLOCK), (unsigned)G), dim3(FIT_BLOCK), shmem, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

template <typename E>
int si_apply(const char* fn, xh_ctx* ctx, const E* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G,
             const double* params, const double* nzeros, const double* nnotnull, int dist, double alpha, double beta,
             double interp, double* out, int64_t st_out) {
  XH_REQUIRE(ctx && group && params && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && C >= 0 && G >= 1, XH_ERR_ARG, "%s: bad shape", fn);
  XH_REQUIRE(T == 0 || C == 0 || (x && st >= C && st_out >= C), XH_ERR_LAYOUT, "%s: needs time-major views", fn);
  XH_REQUIRE(dist == XH_SI_GAMMA || dist == XH_SI_FISK, XH_ERR_ARG, "%s: unknown distribution %d", fn, dist);
  XH_REQUIRE((nzeros == nullptr) == (nnotnull == nullptr), XH_ERR_ARG, "%s: nzeros and nnotnull go together", fn);
  if (T == 0 || C == 0) return XH_OK;
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40) && T * st_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  for (int64_t t = 0; t < T; ++t)
    XH_REQUIRE(group[t] >= -1 && group[t] < G, XH_ERR_ARG, "%s: group[%lld] = %d outside -1..%d", fn, (long long)t,
               (int)group[t], G - 1);
  size_t cur = 0;
  void* d_group = nullptr;
  int rc = xh_scratch_upload(ctx, &cur, group, sizeof(int32_t) * (size_t)T, &d_group);
  if (rc) return rc;
  ApplyArgs<E> a{};
  a.x = x;
  a.T = T;
  a.C = C;
  a.st = st;
  a.st_out = st_out;
  a.group = (const int32_t*)d_group;
  a.params = params;
  a.nzeros = nzeros;
  a.nnotnull = nnotnull;
  a.dist = dist;
  a.alpha = alpha;
  a.beta = beta;
  a.interp = interp;
  a.out = out;
  hipLaunchKernelGGL(k_si_apply<E>, dim3((unsigned)cdiv64(T * C, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

}  // namespace

int xh_si_fit(xh_ctx* ctx, const float* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G, int dist,
              int method, int has_floc, double floc, int zero_inflated, int staging, double* params, double* nzeros,
              double* nnotnull, int32_t* nfev) {
  return si_fit("xh_si_fit", ctx, x, T, C, st, group, G, dist, method, has_floc, floc, zero_inflated, staging, params, nzeros,
                nnotnull, nfev);
}

int xh_si_fit_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G, int dist,
                  int method, int has_floc, double floc, int zero_inflated, int staging, double* params, double* nzeros,
                  double* nnotnull, int32_t* nfev) {
  return si_fit("xh_si_fit_f64", ctx, x, T, C, st, group, G, dist, method, has_floc, floc, zero_inflated, staging, params,
                nzeros, nnotnull, nfev);
}

int xh_si_apply(xh_ctx* ctx, const float* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G,
                const double* params, const double* nzeros, const double* nnotnull, int dist, double alpha, double beta,
                double interp, double* out, int64_t st_out) {
  return si_apply("xh_si_apply", ctx, x, T, C, st, group, G, params, nzeros, nnotnull, dist, alpha, beta, interp, out, st_out);
}

int xh_si_apply_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, const int32_t* group, int G,
                    const double* params, const double* nzeros, const double* nnotnull, int dist, double alpha, double beta,
                    double interp, double* out, int64_t st_out) {
  return si_apply("xh_si_apply_f64", ctx, x, T, C, st, group, G, params, nzeros, nnotnull, dist, alpha, beta, interp, out,
                  st_out);
}
