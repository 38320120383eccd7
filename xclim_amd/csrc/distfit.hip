// distfit.hip — distribution fits and return levels: fit, parametric_quantile / _cdf / _pdf, fa and frequency_analysis of
// indices/stats.py (the C ABI and its limits: include/units/xclim_hip_distfit.h).
//
// Reference: _fitfunc_1d (stats.py:45-112), _fit_start (:576-684), parametric_quantile (:221-292); underneath them scipy 1.15's
// norm_gen.fit, gumbel_r_gen.fit (root_scalar -> brentq), lognorm_gen.fit (the floc case), gamma_gen.fit, rv_continuous.fit ->
// optimize.fmin on _penalized_nnlf, and rv_continuous.ppf / isf / cdf / pdf around each distribution's _ppf / _isf / _cdf / _pdf.
// The reference fits one cell at a time through a Python-level scipy call; here one lane owns one cell, lanes run along the
// cells (every row of the field is one coalesced read), and the whole fit runs in float64 on the lane's staged sample with the
// machinery of fitcore.h, shared with stdidx.hip.  With nq > 0 the lane also writes the return levels from the parameters it
// still holds, so fa / frequency_analysis are one launch after the period maxima.
//
// The sample is staged once as float64 whatever the field's type: in LDS for T <= 32 (value k of lane t at lds[k * FIT_BLOCK +
// t]), otherwise slot-major in the context's scratch (value k of cell c at work[k * C + c]).
#include "fitcore.h"

#include "../../include/units/xclim_hip_distfit.h"

namespace {

constexpr int DF_LDS_N = LDS_MAX_N<double>;  // 32 values per lane
constexpr double SQRT_2PI = 2.50662827463100024161;  // np.sqrt(2 * np.pi)
typedef Sample<double> Smp;

__device__ __forceinline__ bool two_params(int dist) { return dist == XH_DIST_NORM || dist == XH_DIST_GUMBEL_R; }

// x.mean() of numpy: the pairwise sum / n
__device__ double sample_mean(const Smp& s) {
  PwSum a;
  a.init(s.n);
  for (int k = 0; k < s.n; ++k) a.add(k, s[k]);
  return a.sum() / (double)s.n;
}

// mean((x - m)^2): x.var() with m = x.mean(), the square of norm's scale
__device__ double sample_msd(const Smp& s, double m) {
  PwSum a;
  a.init(s.n);
  for (int k = 0; k < s.n; ++k) {
    const double d = s[k] - m;
    a.add(k, d * d);
  }
  return a.sum() / (double)s.n;
}

// ---- gumbel_r_gen.fit ---------------------------------------------------------------------------------------------------
// func(scale) = data.mean() - _average_with_log_weights(data, -data / scale) - scale
__device__ __noinline__ double gumbel_func(const Smp& s, double mean, double scale) {
  double mx = -INFINITY;
  bool unordered = false;
  for (int k = 0; k < s.n; ++k) {
    const double v = -s[k] / scale;
    unordered = unordered || v != v;
    mx = v > mx ? v : mx;
  }
  if (unordered) return NAN;  // np.max of an array with a NaN
  PwSum sw, sxw;
  sw.init(s.n);
  sxw.init(s.n);
  for (int k = 0; k < s.n; ++k) {
    const double w = exp(-s[k] / scale - mx);
    sw.add(k, w);
    sxw.add(k, s[k] * w);
  }
  return (mean - sxw.sum() / sw.sum()) - scale;
}

__device__ double np_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : NAN)); }

__device__ void fit_gumbel(const Smp& s, double (&pr)[3]) {
  const double mean = sample_mean(s);
  double lb = 0.5, rb = 2.0;
  // widen until the signs differ (np.sign: a NaN differs from everything, itself included)
  double fl = gumbel_func(s, mean, lb), fr = gumbel_func(s, mean, rb);
  while (!(np_sign(fl) != np_sign(fr)) && (lb > 0.0 || rb < INFINITY)) {
    lb /= 2.0;
    rb *= 2.0;
    fl = gumbel_func(s, mean, lb);
    fr = gumbel_func(s, mean, rb);
  }
  if (isnan64(fl) || isnan64(fr)) return;  // root_scalar raises on a NaN function value
  auto f = [&](double sc) { return gumbel_func(s, mean, sc); };
  const double scale = brentq(f, lb, rb, 1e-14, 1e-14);
  if (isnan64(scale)) return;
  // loc = -scale * (logsumexp(-data / scale) - log(n))
  double mx = -INFINITY;
  for (int k = 0; k < s.n; ++k) {
    const double v = -s[k] / scale;
    mx = v > mx ? v : mx;
  }
  PwSum se;
  se.init(s.n);
  for (int k = 0; k < s.n; ++k) se.add(k, exp(-s[k] / scale - mx));
  pr[1] = -scale * ((log(se.sum()) + mx) - log((double)s.n));
  pr[2] = scale;
}

// ---- lognorm ---------------------------------------------------------------------------------------------------------------
// _fit_start's lognorm branch (stats.py:673-682): std and exp(mean) of log(x - loc0) over the values above loc0
__device__ void lognorm_start(const Smp& s, double loc0, double& shape0, double& scale0) {
  int npos = 0;
  for (int k = 0; k < s.n; ++k) npos += (s[k] - loc0 > 0.0);
  PwSum a;
  a.init(npos);
  int p = 0;
  for (int k = 0; k < s.n; ++k) {
    const double xp = s[k] - loc0;
    if (xp > 0.0) a.add(p++, log(xp));
  }
  const double m = a.sum() / (double)npos;  // empty -> NaN, as numpy's mean of an empty array
  a.init(npos);
  p = 0;
  for (int k = 0; k < s.n; ++k) {
    const double xp = s[k] - loc0;
    if (xp > 0.0) {
      const double d = log(xp) - m;
      a.add(p++, d * d);
    }
  }
  shape0 = sqrt(a.sum() / (double)npos);
  scale0 = exp(m);
}

// lognorm_gen.fit with floc: scale = exp(mean(log(x - loc))), shape = sqrt(mean((log(x - loc) - log(scale))^2))
__device__ void lognorm_floc(const Smp& s, double loc, double& shape, double& scale) {
  PwSum a;
  a.init(s.n);
  for (int k = 0; k < s.n; ++k) a.add(k, log(s[k] - loc));
  scale = exp(a.sum() / (double)s.n);
  const double ls = log(scale);
  a.init(s.n);
  for (int k = 0; k < s.n; ++k) {
    const double d = log(s[k] - loc) - ls;
    a.add(k, d * d);
  }
  shape = sqrt(a.sum() / (double)s.n);
}

// ---- one cell's fit: pr = (shape, loc, scale), shape unused for norm and gumbel_r ----------------------------------------------
__device__ void fit_cell(int dist, int method, bool has_floc, double floc, const Smp& s, double (&pr)[3], int& nfev, int& status) {
  pr[0] = pr[1] = pr[2] = NAN;
  nfev = 0;
  status = XH_DISTFIT_NAN;
  if (s.n <= 1) return;
  const bool two = two_params(dist);
  bool support = false;
  if (dist == XH_DIST_NORM) {
    pr[1] = sample_mean(s);
    pr[2] = sqrt(sample_msd(s, pr[1]));
  } else if (dist == XH_DIST_GUMBEL_R) {
    fit_gumbel(s, pr);
  } else if (dist == XH_DIST_GENEXTREME) {
    const double m = sample_mean(s);
    const double sc = sqrt(6.0 * sample_msd(s, m)) / 3.14159265358979311600;
    double xv[3] = {0.1, m - 0.57722 * sc, sc};
    if (method == XH_DIST_APP) {
      pr[0] = xv[0];
      pr[1] = xv[1];
      pr[2] = xv[2];
    } else if (!isnan64(xv[1]) && !isnan64(xv[2])) {
      nfev = nelder_mead<3, OBJ_GEV>(0, s, 0.0, xv);
      // rv_continuous.fit raises FitError off the parameter domain: NaN here
      if (isfinite64(xv[0]) && xv[2] > 0.0) {
        pr[0] = xv[0];
        pr[1] = xv[1];
        pr[2] = xv[2];
      }
    }
  } else if (dist == XH_DIST_LOGNORM) {
    if (method == XH_DIST_APP) {
      pr[1] = has_floc ? floc : loc_estimation(s);
      lognorm_start(s, pr[1], pr[0], pr[2]);
    } else {
      double mn = INFINITY;
      for (int k = 0; k < s.n; ++k) mn = s[k] < mn ? s[k] : mn;
      if (floc >= mn) {
        support = true;
      } else {
        lognorm_floc(s, floc, pr[0], pr[2]);
        pr[1] = floc;
        // (scipy hands a shape or scale that is not positive to the generic fit: NaN here)
        if (!(pr[0] > 0.0 && pr[2] > 0.0)) pr[0] = NAN;
      }
    }
  } else {  // gamma, fisk: as k_si_fit (stdidx.hip)
    const int sd = dist == XH_DIST_GAMMA ? XH_SI_GAMMA : XH_SI_FISK;
    if (method == XH_DIST_APP) {
      pr[1] = has_floc ? floc : loc_estimation(s);
      fit_start(sd, s, pr[1], pr[0], pr[2]);
    } else if (dist == XH_DIST_GAMMA && has_floc) {
      bool ok = true;
      for (int k = 0; k < s.n; ++k) ok = ok && s[k] > floc;
      if (!ok) {
        support = true;
      } else {
        PwSum sx, sl;
        sx.init(s.n);
        sl.init(s.n);
        for (int k = 0; k < s.n; ++k) {
          const double d = floc != 0.0 ? s[k] - floc : s[k];
          sx.add(k, d);
          sl.add(k, log(d));
        }
        const double xbar = sx.sum() / (double)s.n;
        const double sh = gamma_shape_root(log(xbar) - sl.sum() / (double)s.n);
        pr[0] = sh;
        pr[1] = floc;
        pr[2] = xbar / sh;
      }
    } else {
      const double loc0 = has_floc ? floc : loc_estimation(s);
      double p0, scale0;
      fit_start(sd, s, loc0, p0, scale0);
      double xv[3] = {p0, loc0, scale0};
      if (!isnan64(p0) && !isnan64(loc0) && !isnan64(scale0)) {
        nfev = has_floc ? nelder_mead<2>(sd, s, floc, xv) : nelder_mead<3>(sd, s, 0.0, xv);
        if (xv[0] > 0.0 && xv[2] > 0.0) {
          pr[0] = xv[0];
          pr[1] = xv[1];
          pr[2] = xv[2];
        }
      }
    }
  }
  // any NaN parameter makes all of them NaN (stats.py:108-110)
  if ((!two && isnan64(pr[0])) || isnan64(pr[1]) || isnan64(pr[2])) {
    pr[0] = pr[1] = pr[2] = NAN;
    status = support ? XH_DISTFIT_SUPPORT : XH_DISTFIT_NAN;
    return;
  }
  const int budget = (has_floc ? 2 : 3) * 200;  // maxfun = 200 N: fmin's warnflag 1
  status = nfev >= budget ? XH_DISTFIT_BUDGET : XH_DISTFIT_FITTED;
}

// ---- scipy's ppf / isf / cdf / pdf --------------------------------------------------------------------------------------------
// cephes ndtr, which scipy.special.ndtr is
__device__ double ndtr(double a) {
  const double x = a * 0.70710678118654752440;
  const double z = fabs(x);
  if (z < 0.70710678118654752440) return 0.5 + 0.5 * erf(x);
  const double y = 0.5 * erfc(z);
  return x > 0.0 ? 1.0 - y : y;
}

__device__ double xlogy(double x, double y) { return (x == 0.0 && y == y) ? 0.0 : x * log(y); }

// The x with gammainc(a, x) = p, 0 < p < 1: Newton steps with Halley's correction on P(a, x) - p, kept inside the bracket the
// signs seen so far give (a step that leaves it is replaced by its midpoint, or by doubling while no upper end is known), from
// the Wilson-Hilferty value, or from the first term of the series, x^a / Gamma(a + 1) = p, for shapes below 1.
__device__ double gammainc_inv(double a, double p) {
  double x;
  const double g = 1.0 / (9.0 * a);
  const double t = 1.0 - g + normcdfinv(p) * sqrt(g);
  x = a * t * t * t;
  if (a < 1.0 || !(t > 0.0)) x = exp((log(p) + lgamma(a + 1.0)) / a);
  if (!(x > 0.0) || !isfinite64(x)) x = a;
  double lo = 0.0, hi = INFINITY;
  const double lg = lgamma(a);
  for (int it = 0; it < 200; ++it) {
    const double f = gammainc(a, x) - p;
    if (f == 0.0) break;
    if (f > 0.0) hi = x;
    else lo = x;
    const double d = exp((a - 1.0) * log(x) - x - lg);  // the density: dP/dx
    double xn = x;
    if (d > 0.0 && isfinite64(d)) {
      const double u = f / d;
      const double h = u * ((a - 1.0) / x - 1.0);
      xn = x - u / (1.0 - 0.5 * (h < 1.0 ? h : 1.0));
    }
    if (!(xn > lo && xn < hi) || xn == x) {
      if (xn == x && d > 0.0 && isfinite64(d)) break;  // the step is below the spacing of x
      xn = hi < INFINITY ? 0.5 * (lo + hi) : 2.0 * x;
    }
    const bool done = fabs(xn - x) <= 4.0 * MACHEP * xn;
    x = xn;
    if (done) break;
  }
  return x;
}

// _ppf / _isf of the standardized distribution, 0 < q < 1
__device__ double std_quantile(int dist, bool isf, double q, double c) {
  switch (dist) {
    case XH_DIST_NORM: return isf ? -normcdfinv(q) : normcdfinv(q);
    case XH_DIST_GUMBEL_R: return isf ? -log(-log1p(-q)) : -log(-log(q));
    case XH_DIST_GENEXTREME: {
      const double x = isf ? -log(-log1p(-q)) : -log(-log(q));
      return (x == x && c != 0.0) ? -expm1(-c * x) / c : x;
    }
    case XH_DIST_GAMMA: return gammainc_inv(c, isf ? 1.0 - q : q);
    case XH_DIST_FISK:  // burr._ppf / _isf with d = 1
      return isf ? pow(expm1(-1.0 * log1p(-q)), -1.0 / c) : pow(pow(q, -1.0) - 1.0, -1.0 / c);
    default: return isf ? exp(c * -normcdfinv(q)) : exp(c * normcdfinv(q));  // lognorm
  }
}

__device__ double std_cdf(int dist, double x, double c) {
  switch (dist) {
    case XH_DIST_NORM: return ndtr(x);
    case XH_DIST_GUMBEL_R: return exp(-exp(-x));
    case XH_DIST_GENEXTREME: return exp(-exp(c != 0.0 ? log1p(-c * x) / c : -x));
    case XH_DIST_GAMMA: return gammainc(c, x);
    case XH_DIST_FISK: return pow(1.0 + pow(x, -c), -1.0);
    default: return ndtr(log(x) / c);
  }
}

__device__ double std_pdf(int dist, double x, double c) {
  switch (dist) {
    case XH_DIST_NORM: return exp(-(x * x) / 2.0) / SQRT_2PI;
    case XH_DIST_GUMBEL_R: return exp(-x - exp(-x));
    case XH_DIST_GENEXTREME: return exp(gev_logpdf(x, c));
    case XH_DIST_GAMMA: return exp(xlogy(c - 1.0, x) - x - lgamma(c));
    case XH_DIST_FISK:
      if (x == 0.0) return c * 1.0 * pow(x, c * 1.0 - 1.0) / (1.0 + pow(x, c));
      return c * 1.0 * pow(x, -c - 1.0) / pow(1.0 + pow(x, -c), 1.0 + 1.0);
    default:
      if (x == 0.0) return 0.0;  // exp(-inf)
      return exp(-(log(x) * log(x)) / (2.0 * (c * c)) - log(c * x * SQRT_2PI));
  }
}

// rv_continuous.ppf / isf / cdf / pdf (scipy _distn_infrastructure.py) of `dist` with (c, loc, scale)
__device__ __noinline__ double dist_func(int dist, int func, double v, double c, double loc, double scale) {
  const bool argok = two_params(dist) || (dist == XH_DIST_GENEXTREME ? isfinite64(c) : c > 0.0);
  double a = -INFINITY, b = INFINITY;
  if (dist == XH_DIST_GENEXTREME) gev_support(c, a, b);
  else if (!two_params(dist)) a = 0.0;
  if (func == XH_DIST_PPF || func == XH_DIST_ISF) {
    if (!(argok && scale > 0.0 && loc == loc) || !(v >= 0.0 && v <= 1.0)) return NAN;
    const bool isf = func == XH_DIST_ISF;
    if (v == 0.0) return (isf ? b : a) * scale + loc;
    if (v == 1.0) return (isf ? a : b) * scale + loc;
    return std_quantile(dist, isf, v, c) * scale + loc;
  }
  if (!(argok && scale > 0.0)) return NAN;
  const double x = (v - loc) / scale;
  if (isnan64(x)) return NAN;
  if (func == XH_DIST_CDF) {
    if (x >= b) return 1.0;
    return (a < x && x < b) ? std_cdf(dist, x, c) : 0.0;
  }
  // the support is closed for the density, except lognorm's (_open_support_mask)
  const bool in = dist == XH_DIST_LOGNORM ? (a < x && x < b) : (a <= x && x <= b);
  return in ? std_pdf(dist, x, c) / scale : 0.0;
}

struct DistFitArgs {
  const void* x;
  int64_t C, ld, ld_params, ld_levels;
  int T, dist, method, has_floc, lds, nq, qfunc;
  double floc;
  double q[XH_DISTFIT_MAX_Q];
  double* work;  // (T, C) float64, slot-major (lds == 0)
  double* params;
  int32_t* nfev;
  uint8_t* status;
  double* levels;
};

template <typename E>
__global__ void __launch_bounds__(FIT_BLOCK) k_dist_fit(DistFitArgs a) {
  extern __shared__ double lds_d[];  // the kernel's only LDS
  const int64_t c = (int64_t)blockIdx.x * FIT_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  // stage the sample: drop NaN, widen to float64
  double* dst = a.lds ? lds_d + threadIdx.x : a.work + c;
  const int64_t dstride = a.lds ? FIT_BLOCK : a.C;
  const E* x = (const E*)a.x + c;
  int n = 0;
  for (int k = 0; k < a.T; ++k) {
    const E v = x[(int64_t)k * a.ld];
    if (v != v) continue;
    dst[(int64_t)n * dstride] = (double)v;
    ++n;
  }
  const Smp s{dst, dstride, n};
  double pr[3];
  int nfev, status;
  fit_cell(a.dist, a.method, a.has_floc != 0, a.floc, s, pr, nfev, status);
  if (two_params(a.dist)) {
    a.params[c] = pr[1];
    a.params[a.ld_params + c] = pr[2];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.params[(int64_t)k * a.ld_params + c] = pr[k];
  }
  if (a.nfev) a.nfev[c] = nfev;
  if (a.status) a.status[c] = (uint8_t)status;
  for (int j = 0; j < a.nq; ++j) a.levels[(int64_t)j * a.ld_levels + c] = dist_func(a.dist, a.qfunc, a.q[j], pr[0], pr[1], pr[2]);
}

struct DistEvalArgs {
  const double* params;
  const double* v;  // (nv) device
  int64_t C, ld_params, ld_out;
  int dist, func;
  double* out;
};

// one thread per (value, cell): blockIdx.y is the value
__global__ void k_dist_eval(DistEvalArgs a) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  const int j = blockIdx.y;
  double p0 = 0.0, loc, scale;
  if (two_params(a.dist)) {
    loc = a.params[c];
    scale = a.params[a.ld_params + c];
  } else {
    p0 = a.params[c];
    loc = a.params[a.ld_params + c];
    scale = a.params[2 * a.ld_params + c];
  }
  a.out[(int64_t)j * a.ld_out + c] = dist_func(a.dist, a.func, a.v[j], p0, loc, scale);
}

}  // namespace

int xh_dist_fit(xh_ctx* ctx, const void* x, int64_t T, int64_t C, int64_t ld, int f64, int dist, int method, int has_floc,
                double floc, const double* q, int nq, int qfunc, double* params, int64_t ld_params, int32_t* nfev, uint8_t* status,
                double* levels, int64_t ld_levels) {
  const char* fn = "xh_dist_fit";
  XH_REQUIRE(ctx && params, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && T <= 0x7fffffff && C >= 0, XH_ERR_ARG, "%s: bad shape (T %lld, C %lld)", fn, (long long)T, (long long)C);
  XH_REQUIRE(dist >= 0 && dist < XH_DIST_NDISTS, XH_ERR_ARG, "%s: unknown distribution %d", fn, dist);
  XH_REQUIRE(method == XH_DIST_APP || method == XH_DIST_ML, XH_ERR_ARG, "%s: unknown method %d", fn, method);
  XH_REQUIRE(nq >= 0, XH_ERR_ARG, "%s: nq %d", fn, nq);
  XH_REQUIRE(nq <= XH_DISTFIT_MAX_Q, XH_ERR_LIMIT, "%s: at most %d fused levels, got %d", fn, XH_DISTFIT_MAX_Q, nq);
  XH_REQUIRE(nq == 0 || (q && levels && (qfunc == XH_DIST_PPF || qfunc == XH_DIST_ISF)), XH_ERR_ARG,
             "%s: fused levels need q, levels and qfunc PPF or ISF", fn);
  const bool two = dist == XH_DIST_NORM || dist == XH_DIST_GUMBEL_R;
  XH_REQUIRE(!(two && method == XH_DIST_APP), XH_ERR_NOTIMPL, "%s: no APP method for norm and gumbel_r", fn);
  XH_REQUIRE(!(has_floc && (two || dist == XH_DIST_GENEXTREME)), XH_ERR_NOTIMPL, "%s: floc is served for gamma, fisk and lognorm", fn);
  XH_REQUIRE(!(dist == XH_DIST_LOGNORM && method == XH_DIST_ML && !has_floc), XH_ERR_NOTIMPL, "%s: lognorm ML needs floc", fn);
  XH_REQUIRE(!has_floc || floc == floc, XH_ERR_ARG, "%s: floc is NaN", fn);
  XH_REQUIRE(C == 0 || (ld_params >= C && (nq == 0 || ld_levels >= C)), XH_ERR_LAYOUT, "%s: an output pitch below C", fn);
  XH_REQUIRE(T == 0 || C == 0 || (x && ld >= C), XH_ERR_LAYOUT, "%s: needs a time-major view (ld >= C)", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(T * ld + C < ((int64_t)1 << 40) && T * C < ((int64_t)1 << 36), XH_ERR_LIMIT, "%s: field too large", fn);
  DistFitArgs a{};
  a.x = x;
  a.C = C;
  a.ld = ld;
  a.ld_params = ld_params;
  a.ld_levels = ld_levels;
  a.T = (int)T;
  a.dist = dist;
  a.method = method;
  a.has_floc = has_floc != 0;
  a.floc = floc;
  a.lds = T <= DF_LDS_N;
  a.nq = nq;
  a.qfunc = qfunc;
  for (int j = 0; j < nq; ++j) a.q[j] = q[j];
  a.params = params;
  a.nfev = nfev;
  a.status = status;
  a.levels = levels;
  if (!a.lds) {
    void* w = nullptr;
    const int rc = xh_big_scratch(ctx, sizeof(double) * (size_t)T * (size_t)C, &w);
    if (rc) return rc;
    a.work = (double*)w;
  }
  const size_t shmem = a.lds ? sizeof(double) * FIT_BLOCK * (size_t)(T > 0 ? T : 1) : 0;
  const dim3 grid((unsigned)cdiv64(C, FIT_BLOCK));
  if (f64) hipLaunchKernelGGL(k_dist_fit<double>, grid, dim3(FIT_BLOCK), shmem, ctx->stream, a);
  else hipLaunchKernelGGL(k_dist_fit<float>, grid, dim3(FIT_BLOCK), shmem, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_dist_eval(xh_ctx* ctx, int dist, int func, const double* params, int64_t C, int64_t ld_params, const double* v, int nv,
                 double* out, int64_t ld_out) {
  const char* fn = "xh_dist_eval";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(dist >= 0 && dist < XH_DIST_NDISTS, XH_ERR_ARG, "%s: unknown distribution %d", fn, dist);
  XH_REQUIRE(func >= XH_DIST_PPF && func <= XH_DIST_PDF, XH_ERR_ARG, "%s: unknown function %d", fn, func);
  XH_REQUIRE(C >= 0 && nv >= 0, XH_ERR_ARG, "%s: bad shape (C %lld, nv %d)", fn, (long long)C, nv);
  XH_REQUIRE(nv <= 65535, XH_ERR_LIMIT, "%s: at most 65535 values, got %d", fn, nv);
  if (C == 0 || nv == 0) return XH_OK;
  XH_REQUIRE(params && v && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(ld_params >= C && ld_out >= C, XH_ERR_LAYOUT, "%s: a pitch below C", fn);
  XH_REQUIRE((int64_t)nv * ld_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: output too large", fn);
  size_t cur = 0;
  void* d_v = nullptr;
  const int rc = xh_scratch_upload(ctx, &cur, v, sizeof(double) * (size_t)nv, &d_v);
  if (rc) return rc;
  DistEvalArgs a{};
  a.params = params;
  a.v = (const double*)d_v;
  a.C = C;
  a.ld_params = ld_params;
  a.ld_out = ld_out;
  a.dist = dist;
  a.func = func;
  a.out = out;
  hipLaunchKernelGGL(k_dist_eval, dim3((unsigned)cdiv64(C, XH_BLOCK), (unsigned)nv), dim3(XH_BLOCK), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}
