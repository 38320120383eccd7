// betainc.h — the regularized incomplete beta function I_x(a, b) for device code, and the two tails built on it: Student's t
// and Fisher's F with one numerator degree of freedom.  Reusable like esat.h: it needs the HIP runtime header and <math.h> only and defines nothing but
// the functions below.  Float64 throughout; a and b are any positive reals (Welch's df is not an integer).
#ifndef XCLIM_AMD_BETAINC_H
#define XCLIM_AMD_BETAINC_H
#include <hip/hip_runtime.h>
#include <math.h>

// The continued fraction of I_x(a, b) by the modified Lentz recurrence (DLMF 8.17.22); it converges in O(sqrt(max(a, b)))
// steps for x < (a + 1) / (a + b + 2).
__device__ __forceinline__ double xh_betacf(double a, double b, double x) {
  const double tiny = 1e-300, eps = 1.11022302462515654042e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 1000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= eps) break;
  }
  return h;
}

// I_x(a, b) with xc = 1 - x given by the caller, who usually knows it without the cancellation: the prefactor
// x^a (1 - x)^b / B(a, b) in log space, the fraction on the side where it converges fast (the symmetry I_x(a, b) =
// 1 - I_{1-x}(b, a)).  NaN in gives NaN out.
__device__ __forceinline__ double xh_betainc(double a, double b, double x, double xc) {
  if (x != x || xc != xc || a != a || b != b) return x + xc + a + b;
  if (x <= 0.0) return 0.0;
  if (xc <= 0.0) return 1.0;
  const double bt = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(xc));
  if (x < (a + 1.0) / (a + b + 2.0)) return bt * xh_betacf(a, b, x) / a;
  return 1.0 - bt * xh_betacf(b, a, xc) / b;
}

// sf of Student's t with df > 0 degrees of freedom at t >= 0: 1/2 I_{df / (df + t^2)}(df / 2, 1/2)
__device__ __forceinline__ double xh_sf_t(double t, double df) {
  if (t != t || df != df) return t + df;
  if (isinf(t)) return 0.0;
  const double t2 = t * t, s = df + t2;
  return 0.5 * xh_betainc(0.5 * df, 0.5, df / s, t2 / s);
}

// sf of Fisher's F with (1, d2) degrees of freedom at w >= 0: I_{d2 / (d2 + w)}(d2 / 2, 1/2)
__device__ __forceinline__ double xh_sf_f1(double w, double d2) {
  if (w != w || d2 != d2) return w + d2;
  if (isinf(w)) return 0.0;
  const double s = d2 + w;
  return xh_betainc(0.5 * d2, 0.5, d2 / s, w / s);
}

#endif  // XCLIM_AMD_BETAINC_H
