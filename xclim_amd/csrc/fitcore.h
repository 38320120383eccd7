// fitcore.h — the per-lane distribution-fit machinery shared by stdidx.hip (the standardized indices) and distfit.hip (fit,
// frequency analysis): numpy's pairwise sum, digamma and gammainc, the staged sample of a lane, scipy's _penalized_nnlf,
// the start values of _fit_start, brentq and the Nelder–Mead of optimize.fmin.  Everything is file-local to the unit that
// includes it; both units are built with -ffp-contract=off and every function keeps the reference's order of operations.
#ifndef XCLIM_AMD_FITCORE_H
#define XCLIM_AMD_FITCORE_H
#include <math.h>

#include "common.h"

namespace {

// The objective of a Nelder–Mead fit is a template parameter, so that a unit's kernels hold only the log-densities they fit:
// OBJ_SI is gamma / fisk picked by the run-time `dist` (XH_SI_GAMMA / XH_SI_FISK), OBJ_GEV is scipy's genextreme.
constexpr int OBJ_SI = 0;
constexpr int OBJ_GEV = 1;

constexpr int FIT_BLOCK = 128;
// LDS staging: 256 B per lane, FIT_BLOCK * 256 B = 32 KB per block (4 blocks of 2 waves per SIMD fit in a CU's LDS):
// 64 float values or 32 double values per lane
template <typename E>
constexpr int LDS_MAX_N = 256 / (int)sizeof(E);
constexpr double LOGXMAX = 7.09782712893383973096e+02;  // log(DBL_MAX): scipy's _LOGXMAX
constexpr double XATOL = 1e-4, FATOL = 1e-4;             // fmin(xtol=1e-4, ftol=1e-4)
constexpr double MACHEP = 1.11022302462515654042e-16;
constexpr double SI_CLIP = 8.21;

__device__ __forceinline__ bool isnan64(double x) { return x != x; }
__device__ __forceinline__ bool isfinite64(double x) { return x - x == 0.0; }

// np.add.reduce of a 1-D float64 array of known length n whose values arrive in order (position p = 0 .. n-1): below 8
// values a running sum from 0.0; from 8 on, 8 interleaved partial sums over the whole blocks, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remainder added in order (numpy's pairwise_sum, n <= 128).
struct PwSum {
  double r[8];
  double res;
  int n, nfull;
  __device__ void init(int n_) {
    n = n_;
    nfull = n >= 8 ? n - n % 8 : 0;
    res = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = 0.0;
  }
  __device__ double combine() const { return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])); }
  __device__ void add(int p, double v) {
    if (n < 8) {
      res += v;
    } else if (p < nfull) {
      const int q = p & 7;
      const bool first = p < 8;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j == q) r[j] = first ? v : r[j] + v;
    } else {
      if (p == nfull) res = combine();
      res += v;
    }
  }
  __device__ double sum() const { return (n >= 8 && nfull == n) ? combine() : res; }
};

// ---- special functions -----------------------------------------------------------------------------------------
// digamma for x > 0: recurrence up to x >= 10, then the asymptotic series (Bernoulli numbers; cephes psi's form).
__device__ double digamma_pos(double x) {
  double w = 0.0;
  while (x < 10.0) {
    w += 1.0 / x;
    x += 1.0;
  }
  const double z = 1.0 / (x * x);
  const double y = z * (8.33333333333333333333E-2 +
                        z * (-8.33333333333333333333E-3 +
                             z * (3.96825396825396825397E-3 +
                                  z * (-4.16666666666666666667E-3 +
                                       z * (7.57575757575757575758E-3 + z * (-2.10927960927960927961E-2 + z * 8.33333333333333333333E-2))))));
  return log(x) - 0.5 / x - y - w;
}

// Regularized lower incomplete gamma P(a, x), a > 0, x >= 0 (cephes igam / igamc, which scipy.special.gammainc uses
// outside its large-a asymptotic region): the power series where x <= 1 or x <= a, else 1 - the continued fraction of
// Q.  The prefactor x^a e^-x / Gamma(a) is taken in log space, so large shapes lose only ~a*log(a)*eps relative.
// Very large shapes (a > 1e6, where the series and the continued fraction need O(sqrt(a)) terms and the fraction's
// recurrences overflow): Temme's uniform expansion with its first correction term, Q = erfc(eta sqrt(a/2)) / 2 +
// exp(-a eta^2 / 2) / sqrt(2 pi a) C0(eta), eta^2 / 2 = lambda - 1 - log(lambda), lambda = x / a; the next term is
// O(a^-3/2).  cephes switches to the same expansion (with more terms) from a > 20 near x = a.
__device__ double gammainc_temme(double a, double x) {
  const double mu = (x - a) / a;
  double h;  // lambda - 1 - log(lambda)
  if (fabs(mu) < 1e-3) h = mu * mu * (0.5 - mu * (1.0 / 3.0 - mu * (0.25 - mu * 0.2)));
  else h = mu - log1p(mu);
  const double eta = (mu < 0.0 ? -1.0 : 1.0) * sqrt(2.0 * h);
  const double c0 = fabs(mu) < 1e-3 ? -1.0 / 3.0 + eta / 12.0 : 1.0 / mu - 1.0 / eta;
  const double r = exp(-a * h) / sqrt(2.0 * 3.14159265358979311600 * a) * c0;
  if (mu < 0.0) return 0.5 * erfc(-eta * sqrt(0.5 * a)) - r;  // P directly in the lower tail
  return 1.0 - (0.5 * erfc(eta * sqrt(0.5 * a)) + r);
}

__device__ double gammainc(double a, double x) {
  if (x == 0.0) return 0.0;
  if (isinf(x)) return 1.0;
  if (a > 1e6) return gammainc_temme(a, x);
  double ax = a * log(x) - x - lgamma(a);
  if (x > 1.0 && x > a) {
    if (ax < -LOGXMAX) return 1.0;
    ax = exp(ax);
    const double big = 4.503599627370496e15, biginv = 2.22044604925031308085e-16;
    double y = 1.0 - a, z = x + y + 1.0, c = 0.0;
    double pkm2 = 1.0, qkm2 = x, pkm1 = x + 1.0, qkm1 = z * x;
    double ans = pkm1 / qkm1, t;
    int it = 0;
    do {
      c += 1.0;
      y += 1.0;
      z += 2.0;
      const double yc = y * c;
      const double pk = pkm1 * z - pkm2 * yc;
      const double qk = qkm1 * z - qkm2 * yc;
      if (qk != 0.0) {
        const double r = pk / qk;
        t = fabs((ans - r) / r);
        ans = r;
      } else {
        t = 1.0;
      }
      pkm2 = pkm1;
      pkm1 = pk;
      qkm2 = qkm1;
      qkm1 = qk;
      if (fabs(pk) > big) {
        pkm2 *= biginv;
        pkm1 *= biginv;
        qkm2 *= biginv;
        qkm1 *= biginv;
      }
    } while (t > MACHEP && ++it < 10000);
    return 1.0 - ans * ax;
  }
  if (ax < -LOGXMAX) return 0.0;
  ax = exp(ax);
  double r = a, c = 1.0, ans = 1.0;
  int it = 0;
  do {
    r += 1.0;
    c *= x / r;
    ans += c;
  } while (c / ans > MACHEP && ++it < 100000);
  return ans * ax / a;
}

// scipy's rv_continuous.cdf for gamma (a, loc, scale) and fisk (c, loc, scale): NaN for invalid parameters or x, 0 at and
// below the support's start, 1 at +inf.
__device__ double dist_cdf(int dist, double v, double p0, double loc, double scale) {
  if (!(p0 > 0.0) || !(scale > 0.0) || isnan64(v) || isnan64(loc)) return NAN;
  const double x = (v - loc) / scale;
  if (isnan64(x)) return NAN;
  if (!(x > 0.0)) return 0.0;
  if (isinf(x)) return 1.0;
  if (dist == XH_SI_GAMMA) return gammainc(p0, x);
  return 1.0 / (1.0 + pow(x, -p0));  // burr._cdf(x, c, 1) = (1 + x**-c)**-1
}

// forced inline here and in gamma_shape_root: called from two kernel instances, they would otherwise be outlined, which
// would change the float32 instance's code
__device__ __forceinline__ double norm_ppf_clipped(double p) {
  if (isnan64(p) || p < 0.0 || p > 1.0) return NAN;
  const double s = normcdfinv(p);
  return s < -SI_CLIP ? -SI_CLIP : (s > SI_CLIP ? SI_CLIP : s);
}

// ---- the sample of one lane ---------------------------------------------------------------------------------------
// The compacted sample (NaN dropped, zeros too when zero-inflated) is staged once, either in LDS (value k of lane t at
// lds[k * FIT_BLOCK + t]) or in a global work buffer laid out like the field (value k at work[(row0 + k) * C + c]).
template <typename E>
struct Sample {
  const E* base;
  int64_t stride;
  int n;
  __device__ double operator[](int k) const { return (double)base[(int64_t)k * stride]; }
};

// _penalized_nnlf(theta, x) (scipy _distn_infrastructure.py): inf off the parameter domain; points outside the support
// or with a non-finite log-density add 100 * log(DBL_MAX) each instead of their log-density; + n * log(scale).
// genextreme._logpdf(x, c) of scipy 1.15, branch for branch (x finite): cx = c x where c != 0, else 0; log(-log cdf) =
// log1p(-c x) / c where c != 0, else -x; -inf where cx == 1 or cx == -inf, and 0 at c == 1, x == 1.
__device__ __forceinline__ double gev_logpdf(double x, double c) {
  const double cx = c != 0.0 ? c * x : 0.0;
  const double logex2 = log1p(-cx);
  const double logpex2 = c != 0.0 ? log1p(-c * x) / c : -x;
  const double pex2 = exp(logpex2);
  double lp = (cx == 1.0 || cx == -INFINITY) ? -INFINITY : (-pex2 + logpex2) - logex2;
  if (c == 1.0 && x == 1.0) lp = 0.0;
  return lp;
}

// genextreme._get_support(c): (1 / min(c, -tiny), inf) for c < 0, (-inf, 1 / max(c, tiny)) for c > 0, the line for c == 0
__device__ __forceinline__ void gev_support(double c, double& a, double& b) {
  const double tiny = 2.2250738585072014e-308;
  b = c > 0.0 ? 1.0 / (c > tiny ? c : tiny) : INFINITY;
  a = c < 0.0 ? 1.0 / (c < -tiny ? c : -tiny) : -INFINITY;
}

template <int OBJ, typename E>
__device__ __noinline__ double nnlf(int dist, const Sample<E>& s, double p0, double loc, double scale) {
  if constexpr (OBJ == OBJ_GEV) {
    // genextreme._argcheck is isfinite(c); the support [a, b] is closed (rv_continuous._support_mask)
    if (!isfinite64(p0) || !(scale > 0.0)) return INFINITY;
    double lo, hi;
    gev_support(p0, lo, hi);
    int nfin = s.n;
    PwSum acc;
    for (int pass = 0; pass < 2; ++pass) {
      acc.init(nfin);
      int p = 0, bad = 0;
      for (int k = 0; k < s.n; ++k) {
        const double x = (s[k] - loc) / scale;
        if (!(lo <= x && x <= hi)) {
          ++bad;
          continue;
        }
        const double lp = gev_logpdf(x, p0);
        if (!isfinite64(lp)) {
          ++bad;
          continue;
        }
        acc.add(p++, lp);
      }
      if (bad == 0 || pass == 1) {
        const double tot = -(0.0 + acc.sum()) + (double)bad * LOGXMAX * 100.0;
        return tot + (double)s.n * log(scale);
      }
      nfin = s.n - bad;
    }
    return INFINITY;  // not reached
  }
  if (!(p0 > 0.0) || !(scale > 0.0)) return INFINITY;
  double cst, am1;
  if (dist == XH_SI_GAMMA) {
    cst = lgamma(p0);
    am1 = p0 - 1.0;
  } else {
    cst = log(p0) + 0.0;  // np.log(c) + np.log(d), d = 1
    am1 = -p0 - 1.0;      // xlogy(-c - 1, x)
  }
  // fast pass: every point in the support with a finite log-density (the sum then has n terms); otherwise a second pass
  // with the count of finite terms known, which is what numpy's pairwise sum needs
  int nfin = s.n;
  PwSum acc;
  for (int pass = 0; pass < 2; ++pass) {
    acc.init(nfin);
    int p = 0, bad = 0;
    for (int k = 0; k < s.n; ++k) {
      const double x = (s[k] - loc) / scale;
      if (!(x >= 0.0)) {  // outside the support [0, inf]
        ++bad;
        continue;
      }
      double lp;
      if (dist == XH_SI_GAMMA) {
        const double xl = am1 == 0.0 ? 0.0 : am1 * log(x);  // sc.xlogy(a - 1, x)
        lp = xl - x - cst;
      } else if (x == 0.0) {  // burr._logpdf's x == 0 branch with d = 1
        const double cm1 = p0 - 1.0;
        lp = cst + (cm1 == 0.0 ? 0.0 : cm1 * log(x)) - 2.0 * log1p(pow(x, p0));
      } else {
        lp = (cst + am1 * log(x)) - 2.0 * log1p(pow(x, -p0));  // + xlogy(-c-1, x) - xlog1py(d + 1, x**-c)
      }
      if (!isfinite64(lp)) {
        ++bad;
        continue;
      }
      acc.add(p++, lp);
    }
    if (bad == 0 || pass == 1) {
      const double tot = -(0.0 + acc.sum()) + (double)bad * LOGXMAX * 100.0;
      return tot + (double)s.n * log(scale);
    }
    nfin = s.n - bad;
  }
  return INFINITY;  // not reached
}

// _loc_estimation (stats.py:609-620): from the two smallest values and the largest
template <typename E>
__device__ double loc_estimation(const Sample<E>& s) {
  double x1 = INFINITY, x2 = INFINITY, xn = -INFINITY;
  for (int k = 0; k < s.n; ++k) {
    const double v = s[k];
    if (v < x1) {
      x2 = x1;
      x1 = v;
    } else if (v < x2) {
      x2 = v;
    }
    xn = v > xn ? v : xn;
  }
  const double xp = x2;
  const double loc0 = (x1 * xn - xp * xp) / (x1 + xn - 2.0 * xp);
  return loc0 < x1 ? loc0 : x1 - 0.0001 * fabs(x1);
}

// The start values of _fit_start (stats.py:622-673) for gamma / fisk with loc0 given: (shape0, scale0) from the values
// above loc0.  Each mean is numpy's (pairwise sum over the filtered values) / count.
template <typename E>
__device__ void fit_start(int dist, const Sample<E>& s, double loc0, double& p0, double& scale0) {
  int npos = 0;
  for (int k = 0; k < s.n; ++k) npos += (s[k] - loc0 > 0.0);
  PwSum s1, s2;
  s1.init(npos);
  s2.init(npos);
  int p = 0;
  for (int k = 0; k < s.n; ++k) {
    const double xp = s[k] - loc0;
    if (!(xp > 0.0)) continue;
    s1.add(p, xp);
    s2.add(p, dist == XH_SI_GAMMA ? log(xp) : xp * xp);
    ++p;
  }
  const double m = s1.sum() / (double)npos;  // empty -> NaN, as numpy's mean of an empty array
  if (dist == XH_SI_GAMMA) {
    const double A = log(m) - s2.sum() / (double)npos;
    p0 = (1.0 + sqrt(1.0 + 4.0 * A / 3.0)) / (4.0 * A);
    scale0 = m / p0;
  } else {
    const double m2 = s2.sum() / (double)npos;
    scale0 = 2.0 * pow(m, 3.0) / (m2 + pow(m, 2.0));
    p0 = 3.14159265358979311600 * m / 1.73205080756887719318 / sqrt(m2 - pow(m, 2.0));  // np.pi * m / np.sqrt(3) / ...
  }
}

// scipy's brentq (Zeros/brentq.c, 100 iterations) on the bracket [xa, xb]; NaN where scipy raises (no sign change).
template <typename F>
__device__ __forceinline__ double brentq(F f, double xa, double xb, double xtol, double rtol) {
  double xpre = xa, xcur = xb;
  double xblk = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
  double fpre = f(xpre), fcur = f(xcur);
  if (fpre == 0.0) return xpre;
  if (fcur == 0.0) return xcur;
  if (signbit(fpre) == signbit(fcur)) return NAN;  // brentq raises: the root is not bracketed
  for (int i = 0; i < 100; ++i) {
    if (fpre != 0.0 && fcur != 0.0 && signbit(fpre) != signbit(fcur)) {
      xblk = xpre;
      fblk = fpre;
      spre = scur = xcur - xpre;
    }
    if (fabs(fblk) < fabs(fcur)) {
      xpre = xcur;
      xcur = xblk;
      xblk = xpre;
      fpre = fcur;
      fcur = fblk;
      fblk = fpre;
    }
    const double delta = (xtol + rtol * fabs(xcur)) / 2.0;
    const double sbis = (xblk - xcur) / 2.0;
    if (fcur == 0.0 || fabs(sbis) < delta) return xcur;
    if (fabs(spre) > delta && fabs(fcur) < fabs(fpre)) {
      double stry;
      if (xpre == xblk) {
        stry = -fcur * (xcur - xpre) / (fcur - fpre);
      } else {
        const double dpre = (fpre - fcur) / (xpre - xcur);
        const double dblk = (fblk - fcur) / (xblk - xcur);
        stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre));
      }
      if (2.0 * fabs(stry) < fmin(fabs(spre), 3.0 * fabs(sbis) - delta)) {
        spre = scur;
        scur = stry;
      } else {
        spre = sbis;
        scur = sbis;
      }
    } else {
      spre = sbis;
      scur = sbis;
    }
    xpre = xcur;
    fpre = fcur;
    if (fabs(scur) > delta) xcur += scur;
    else xcur += (sbis > 0.0 ? delta : -delta);
    fcur = f(xcur);
  }
  return xcur;
}

// gamma_gen.fit with floc (scipy _continuous_distns.py): the root of log(a) - digamma(a) = s by brentq (xtol 2e-12,
// rtol 4 eps) on [0.6, 1.4] * the Choi-Wette estimate.
__device__ __forceinline__ double gamma_shape_root(double s) {
  if (!(s > 0.0)) return NAN;  // identical values: the bracket is [inf, inf] and brentq fails in the reference
  const double aest = (3.0 - s + sqrt((s - 3.0) * (s - 3.0) + 24.0 * s)) / (12.0 * s);
  auto f = [s](double a) { return log(a) - digamma_pos(a) - s; };
  return brentq(f, aest * (1.0 - 0.4), aest * (1.0 + 0.4), 2e-12, 4.0 * 2.220446049250313e-16);
}

// optimize.fmin(func, x0, xtol=1e-4, ftol=1e-4, disp=0): _minimize_neldermead, non-adaptive (rho 1, chi 2, psi 1/2,
// sigma 1/2), maxiter = maxfun = 200 N.  A call past maxfun ends the iteration where it stands, as scipy's
// _MaxFuncCallError does.  N = 3: (shape, loc, scale); N = 2: (shape, scale) with loc fixed.  Returns the evaluations.
template <int N, int OBJ = OBJ_SI, typename E>
__device__ __noinline__ int nelder_mead(int dist, const Sample<E>& s, double floc, double (&x)[3]) {
  double sim[N + 1][N], fs[N + 1];
  const int maxfun = 200 * N, maxiter = 200 * N;
  int fcalls = 0;
  auto func = [&](const double (&v)[N]) {
    return N == 3 ? nnlf<OBJ>(dist, s, v[0], v[1], v[2]) : nnlf<OBJ>(dist, s, v[0], floc, v[N - 1]);
  };
  auto sort = [&]() {  // stable insertion sort of the vertices by value (np.argsort of N + 1 values), fully unrolled
#pragma unroll
    for (int i = 1; i <= N; ++i)
#pragma unroll
      for (int j = i; j > 0; --j) {
        const bool sw = fs[j] < fs[j - 1];
        const double t0 = fs[j], t1 = fs[j - 1];
        fs[j] = sw ? t1 : t0;
        fs[j - 1] = sw ? t0 : t1;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double u0 = sim[j][k], u1 = sim[j - 1][k];
          sim[j][k] = sw ? u1 : u0;
          sim[j - 1][k] = sw ? u0 : u1;
        }
      }
  };
#pragma unroll
  for (int k = 0; k < N; ++k) sim[0][k] = N == 3 ? x[k] : x[k == 0 ? 0 : 2];
#pragma unroll
  for (int j = 1; j <= N; ++j)
#pragma unroll
    for (int k = 0; k < N; ++k) sim[j][k] = (k == j - 1) ? (sim[0][k] != 0.0 ? (1.0 + 0.05) * sim[0][k] : 0.00025) : sim[0][k];
#pragma unroll
  for (int j = 0; j <= N; ++j) {
    fs[j] = func(sim[j]);
    ++fcalls;
  }
  sort();
  int iterations = 1;
  while (fcalls < maxfun && iterations < maxiter) {
    bool conv = true;
#pragma unroll
    for (int j = 1; j <= N; ++j) {
#pragma unroll
      for (int k = 0; k < N; ++k) conv = conv && fabs(sim[j][k] - sim[0][k]) <= XATOL;
      conv = conv && fabs(fs[0] - fs[j]) <= FATOL;
    }
    if (conv) break;
    double xbar[N], xr[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double t = sim[0][k];
#pragma unroll
      for (int j = 1; j < N; ++j) t = t + sim[j][k];
      xbar[k] = t / (double)N;
      xr[k] = 2.0 * xbar[k] - sim[N][k];
    }
    bool stop = false;
    // evaluation under the budget: false = the call would exceed maxfun (scipy raises before calling)
    auto eval = [&](const double (&v)[N], double& fv) {
      if (fcalls >= maxfun) return false;
      ++fcalls;
      fv = func(v);
      return true;
    };
    double fxr;
    if (!eval(xr, fxr)) {
      stop = true;
    } else if (fxr < fs[0]) {
      double xe[N], fxe;
#pragma unroll
      for (int k = 0; k < N; ++k) xe[k] = 3.0 * xbar[k] - 2.0 * sim[N][k];
      if (!eval(xe, fxe)) {
        stop = true;
      } else if (fxe < fxr) {
#pragma unroll
        for (int k = 0; k < N; ++k) sim[N][k] = xe[k];
        fs[N] = fxe;
      } else {
#pragma unroll
        for (int k = 0; k < N; ++k) sim[N][k] = xr[k];
        fs[N] = fxr;
      }
    } else if (fxr < fs[N - 1]) {
#pragma unroll
      for (int k = 0; k < N; ++k) sim[N][k] = xr[k];
      fs[N] = fxr;
    } else {
      bool doshrink = false;
      if (fxr < fs[N]) {
        double xc[N], fxc;
#pragma unroll
        for (int k = 0; k < N; ++k) xc[k] = 1.5 * xbar[k] - 0.5 * sim[N][k];
        if (!eval(xc, fxc)) {
          stop = true;
        } else if (fxc <= fxr) {
#pragma unroll
          for (int k = 0; k < N; ++k) sim[N][k] = xc[k];
          fs[N] = fxc;
        } else {
          doshrink = true;
        }
      } else {
        double xcc[N], fxcc;
#pragma unroll
        for (int k = 0; k < N; ++k) xcc[k] = 0.5 * xbar[k] + 0.5 * sim[N][k];
        if (!eval(xcc, fxcc)) {
          stop = true;
        } else if (fxcc < fs[N]) {
#pragma unroll
          for (int k = 0; k < N; ++k) sim[N][k] = xcc[k];
          fs[N] = fxcc;
        } else {
          doshrink = true;
        }
      }
      if (doshrink) {
#pragma unroll
        for (int j = 1; j <= N; ++j) {
          if (stop) continue;
#pragma unroll
          for (int k = 0; k < N; ++k) sim[j][k] = sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]);
          if (!eval(sim[j], fs[j])) stop = true;
        }
      }
    }
    if (!stop) ++iterations;
    sort();
    if (stop) break;
  }
  if (N == 3) {
    x[0] = sim[0][0];
    x[1] = sim[0][1];
    x[2] = sim[0][2];
  } else {
    x[0] = sim[0][0];
    x[1] = floc;
    x[2] = sim[0][N - 1];
  }
  return fcalls;
}

}  // namespace
#endif  // XCLIM_AMD_FITCORE_H
