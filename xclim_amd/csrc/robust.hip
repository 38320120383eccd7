// robust.hip — the ensemble change-robustness unit (include/units/xclim_hip_robust.h): xclim.ensembles._robustness.
//
// xh_change_test: one lane per (realization, cell) series pair; neighbouring lanes are neighbouring cells, so every row load
// is coalesced.  A lane walks its two series once, compacts the non-NaN values into a staged sample (fitcore.h's Sample:
// slot-major in LDS, value k of lane t at lds[k * CT_BLOCK + t], or slot-major in the context's work buffer, one code path)
// and computes the test from it in float64, in scipy's order of operations with numpy's pairwise sums (pwsum.h).
// Mann-Whitney's U and tie term and Brown-Forsythe's medians are found by counting: no sort, no data-dependent index.
// xh_robust_fractions: one lane per cell, the members added in realization order.
#include "../../include/units/xclim_hip_robust.h"
#include "betainc.h"
#include "hostargs.h"
#include "pwsum.h"

namespace {

constexpr int CT_BLOCK = 64;

struct ChangeArgs {
  const void* fut;
  const void* ref;
  int64_t C, ld_fut, sr_fut, ld_ref, sr_ref, ld_out, work_stride;
  int T1, T2, test, lds, has_sf;
  const double* sf;  // device copy of the host table
  void* work;
  double* delta;
  double* mean_ref;
  int32_t* n_fut;
  int32_t* n_ref;
  double* stat;
  double* df;
  double* pvals;
  uint8_t* status;
};

// numpy's mean of values [k0, k0 + n) of the sample mapped through f: pairwise sum / n (0 / 0 = NaN for an empty range)
template <typename E, typename F>
__device__ __forceinline__ double pw_mean(const Sample<E>& s, int k0, int n, F f) {
  PwSumLong acc;
  acc.init(n);
  for (int k = 0; k < n; ++k) acc.add(k, f(s[k0 + k]));
  return acc.sum() / (double)n;
}

// scipy's _var(x, ddof=1): mean((x - mean)^2) * (n / (n - 1)); n == 1 gives 0 * inf = NaN
template <typename E>
__device__ __forceinline__ double var_ddof1(const Sample<E>& s, int k0, int n, double mean) {
  const double m2 = pw_mean(s, k0, n, [mean](double v) {
    const double d = v - mean;
    return d * d;
  });
  return m2 * ((double)n / (double)(n - 1));
}

// np.median by counting selection: the k-th smallest is the value with #less <= k < #less + #equal
template <typename E>
__device__ __forceinline__ double median_count(const Sample<E>& s, int k0, int n) {
  const int ka = (n - 1) / 2, kb = n / 2;
  double a = 0.0, b = 0.0;
  for (int i = 0; i < n; ++i) {
    const double v = s[k0 + i];
    int less = 0, eq = 0;
    for (int j = 0; j < n; ++j) {
      const double u = s[k0 + j];
      less += u < v;
      eq += u == v;
    }
    if (less <= ka && ka < less + eq) a = v;
    if (less <= kb && kb < less + eq) b = v;
  }
  return ka == kb ? a : (a + b) / 2.0;
}

// Walk one series (row pitch ld) and append its non-NaN values to the staged sample from slot n on; returns the new count.
// Eight rows are loaded before the first is looked at, so that eight loads are in flight per lane, not one.
template <typename E>
__device__ __forceinline__ int stage_series(const E* __restrict__ src, int T, int64_t ld, E* dst, int64_t dstride, int n) {
  int t = 0;
  for (; t + 8 <= T; t += 8) {
    E v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(t + u) * ld];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (v[u] == v[u]) {
        dst[(int64_t)n * dstride] = v[u];
        ++n;
      }
  }
  for (; t < T; ++t) {
    const E v = src[(int64_t)t * ld];
    if (v != v) continue;
    dst[(int64_t)n * dstride] = v;
    ++n;
  }
  return n;
}

template <typename E>
__global__ void __launch_bounds__(CT_BLOCK) k_change_test(ChangeArgs a) {
  extern __shared__ double lds_raw[];  // the kernel's only LDS
  const int64_t c = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t r = blockIdx.y;
  E* dst = a.lds ? reinterpret_cast<E*>(lds_raw) + threadIdx.x : reinterpret_cast<E*>(a.work) + r * a.C + c;
  const int64_t dstride = a.lds ? CT_BLOCK : a.work_stride;
  const E* f = reinterpret_cast<const E*>(a.fut) + r * a.sr_fut + c;
  const E* g = reinterpret_cast<const E*>(a.ref) + r * a.sr_ref + c;
  const int n1 = stage_series(f, a.T1, a.ld_fut, dst, dstride, 0);
  const int n2 = stage_series(g, a.T2, a.ld_ref, dst, dstride, n1) - n1;
  const Sample<E> s{dst, dstride, n1 + n2};
  auto id = [](double v) { return v; };
  const double m1 = pw_mean(s, 0, n1, id), m2 = pw_mean(s, n1, n2, id);
  const int64_t o = r * a.ld_out + c;
  a.delta[o] = m1 - m2;
  a.mean_ref[o] = m2;
  a.n_fut[o] = n1;
  a.n_ref[o] = n2;
  if (a.test == XH_CT_MOMENTS) return;

  const double nan = xh_nan64();
  double stat = nan, df = nan, p = nan;
  int status = XH_CT_DONE;
  if (a.test == XH_CT_BF ? (n1 < a.T1 || n2 < a.T2) : (n1 == 0 || n2 == 0)) {
    status = XH_CT_NAN;  // the reference's guard (and levene on a NaN)
  } else if (a.test == XH_CT_TTEST) {
    const double d = m1 - m2;
    const double v = var_ddof1(s, 0, n1, m1);
    stat = d / sqrt(v / (double)n1);
    df = (double)(n1 - 1);
    p = 2.0 * xh_sf_t(fabs(stat), df);
  } else if (a.test == XH_CT_WELCH) {
    const double vn1 = var_ddof1(s, 0, n1, m1) / (double)n1, vn2 = var_ddof1(s, n1, n2, m2) / (double)n2;
    const double sv = vn1 + vn2;
    df = (sv * sv) / ((vn1 * vn1) / (double)(n1 - 1) + (vn2 * vn2) / (double)(n2 - 1));
    if (df != df) df = 1.0;
    stat = (m1 - m2) / sqrt(sv);
    p = 2.0 * xh_sf_t(fabs(stat), df);
  } else if (a.test == XH_CT_MWU) {
    // 2 U1 = sum_i sum_j (2 [x_i > y_j] + [x_i == y_j]); sum(t^3 - t) = sum_k (e_k^2 - 1), e_k the pooled values equal to value k
    long long twoU = 0, ties = 0;
    const int n = n1 + n2;
    for (int i = 0; i < n; ++i) {
      const double v = s[i];
      int gt = 0, eq1 = 0, eq2 = 0;
      for (int j = 0; j < n1; ++j) eq1 += s[j] == v;
      for (int j = n1; j < n; ++j) {
        const double u = s[j];
        gt += v > u;
        eq2 += v == u;
      }
      if (i < n1) twoU += 2 * gt + eq2;
      const long long e = eq1 + eq2;
      ties += e * e - 1;
    }
    const double nn = (double)((long long)n1 * n2);
    const double U1 = (double)twoU / 2.0, U2 = nn - U1;
    const double U = U1 > U2 ? U1 : U2;
    stat = U1;
    df = (double)ties;
    if ((n1 > 8 && n2 > 8) || ties > 0) {
      const double sd = sqrt(nn / 12.0 * ((double)(n + 1) - (double)ties / (double)((long long)n * (n - 1))));
      const double z = (U - nn / 2.0 - 0.5) / sd;
      p = 2.0 * (0.5 * erfc(z / 1.41421356237309514547));
      p = p > 1.0 ? 1.0 : p;
    } else if (n1 == a.T1 && n2 == a.T2 && a.has_sf) {
      p = 2.0 * a.sf[(long long)U];  // without ties U is an integer
      p = p > 1.0 ? 1.0 : p;
    } else {
      status = XH_CT_EXACT_PENDING;
    }
  } else {  // XH_CT_BF: levene(center="median"), k = 2 samples
    const double med1 = median_count(s, 0, n1), med2 = median_count(s, n1, n2);
    const double zb1 = pw_mean(s, 0, n1, [med1](double v) { return fabs(v - med1); });
    const double zb2 = pw_mean(s, n1, n2, [med2](double v) { return fabs(v - med2); });
    const double N1 = (double)n1, N2 = (double)n2, N = N1 + N2;
    double zbar = 0.0;
    zbar += zb1 * N1;
    zbar += zb2 * N2;
    zbar /= N;
    const double e1 = zb1 - zbar, e2 = zb2 - zbar;
    const double numer = (N - 2.0) * (N1 * (e1 * e1) + N2 * (e2 * e2));
    auto sq = [](const Sample<E>& smp, int k0, int cnt, double med, double zb) {
      PwSumLong acc;
      acc.init(cnt);
      for (int k = 0; k < cnt; ++k) {
        const double d = fabs(smp[k0 + k] - med) - zb;
        acc.add(k, d * d);
      }
      return acc.sum();
    };
    double dvar = 0.0;
    dvar += sq(s, 0, n1, med1, zb1);
    dvar += sq(s, n1, n2, med2, zb2);
    stat = numer / (1.0 * dvar);
    df = N - 2.0;
    p = xh_sf_f1(stat, df);
  }
  if (status == XH_CT_DONE && p != p) status = XH_CT_NAN;
  a.stat[o] = stat;
  a.df[o] = df;
  a.pvals[o] = p;
  a.status[o] = (uint8_t)status;
}

struct FracArgs {
  const double* delta;
  const uint8_t* changed;
  const uint8_t* valid;
  const double* mean_ref;
  const double* w;  // device copy of the host weights
  int64_t R, C, ld, ld_out;
  int strict, kind;
  double thresh;
  double* out;
};

__global__ void __launch_bounds__(XH_BLOCK) k_robust_fractions(FracArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  double nv = 0.0, ch = 0.0, pos = 0.0, neg = 0.0, chpos = 0.0, chneg = 0.0;
  for (int64_t r = 0; r < a.R; ++r) {
    const int64_t i = r * a.ld + c;
    const double d = a.delta[i], w = a.w[r];
    const bool ok = a.valid ? a.valid[i] != 0 : d == d;
    if (!ok) continue;
    bool changed = true;
    if (a.kind == XH_RF_THRESH_ABS) changed = fabs(d) > a.thresh;
    else if (a.kind == XH_RF_THRESH_REL) changed = fabs(d / a.mean_ref[i]) > a.thresh;
    else if (a.changed) changed = a.changed[i] != 0;
    const bool p = a.strict ? d > 0.0 : d >= 0.0, n = a.strict ? d < 0.0 : d <= 0.0;
    nv += w;
    ch += changed ? w : 0.0;
    pos += p ? w : 0.0;
    neg += n ? w : 0.0;
    chpos += (p && changed) ? w : 0.0;
    chneg += (n && changed) ? w : 0.0;
  }
  const double fp = pos / nv, fn = neg / nv, fz = 1.0 - fp - fn;
  double agree = fp;  // xarray's max skips NaN: all three are NaN together
  agree = fn > agree ? fn : agree;
  agree = fz > agree ? fz : agree;
  auto put = [&](int k, double v) { a.out[(int64_t)k * a.ld_out + c] = v == v ? v : 0.0; };
  put(XH_RF_CHANGED, ch / nv);
  put(XH_RF_POSITIVE, fp);
  put(XH_RF_CHANGED_POSITIVE, chpos / nv);
  put(XH_RF_NEGATIVE, fn);
  put(XH_RF_CHANGED_NEGATIVE, chneg / nv);
  put(XH_RF_VALID, nv / (double)a.R);
  put(XH_RF_AGREE, agree);
}

// ---- xh_robust_coefficient ------------------------------------------------------------------------------------------
constexpr int RC_BLOCK = 64;  // one wave per cell

struct CoefArgs {
  const void* fut;
  const void* ref;
  int64_t C, ld_fut, sr_fut, ld_ref;
  int R, T1, T2, np1, np2, npad;  // np1, np2: the powers of two >= R T1 + R and >= T2 + R; npad their maximum
  double* out;
  double* a1;
  double* a2;
};

// A(x1, favg) with x1 = pool[0 .. n1): the pool of both samples is sorted in LDS (the bitonic network of k_sen_slope over np
// slots, padded with +inf), then every step between two different neighbours adds its width times the squared difference of
// the two empirical CDFs below it.  The pool's rank of the step is k + 1 values, of which #(favg <= value) are the means'.
// Equal neighbours have no width, so their order in the pool is free.  Lane partials are added in lane order by lane 0.
__device__ double cdf_sq_area(double* pool, const double* favg, double* part, int n1, int R, int np) {
  const int lane = threadIdx.x, n = n1 + R;
  for (int r = lane; r < R; r += RC_BLOCK) pool[n1 + r] = favg[r];
  for (int i = n + lane; i < np; i += RC_BLOCK) pool[i] = INFINITY;
  __syncthreads();
  for (int kk = 2; kk <= np; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = lane; i < np; i += RC_BLOCK) {
        const int o = i ^ jj;
        if (o > i) {
          const double u = pool[i], v = pool[o];
          const bool up = (i & kk) == 0;
          if (up ? u > v : u < v) pool[i] = v, pool[o] = u;
        }
      }
      __syncthreads();
    }
  }
  double acc = 0.0;
  for (int k = lane; k + 1 < n; k += RC_BLOCK) {
    const double v = pool[k], w = pool[k + 1] - v;
    if (!(w > 0.0)) continue;
    int c2 = 0;
    for (int r = 0; r < R; ++r) c2 += favg[r] <= v;
    const double d = (double)(k + 1 - c2) / (double)n1 - (double)c2 / (double)R;
    acc += w * (d * d);
  }
  part[lane] = acc;
  __syncthreads();
  double tot = 0.0;
  if (lane == 0)
    for (int t = 0; t < RC_BLOCK; ++t) tot += part[t];
  __syncthreads();
  return tot;  // lane 0 only
}

template <typename E>
__global__ void __launch_bounds__(RC_BLOCK) k_robust_coefficient(CoefArgs a) {
  extern __shared__ double rc_lds[];  // pool[npad] | favg[R] | part[RC_BLOCK]
  double* pool = rc_lds;
  double* favg = pool + a.npad;
  double* part = favg + a.R;
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int nf = a.R * a.T1;
  int bad = 0;
  for (int i = lane; i < nf; i += RC_BLOCK) {
    const int r = i / a.T1, t = i - r * a.T1;
    const double v = xh_ldw<E>(a.fut, (int64_t)r * a.sr_fut + (int64_t)t * a.ld_fut + c);
    pool[i] = v;
    bad += v != v;
  }
  for (int t = lane; t < a.T2; t += RC_BLOCK) {
    const double v = xh_ldw<E>(a.ref, (int64_t)t * a.ld_ref + c);
    bad += v != v;
  }
  part[lane] = (double)bad;
  __syncthreads();
  // the multimodel means: numpy's mean along the contiguous time axis, one member per lane
  for (int r = lane; r < a.R; r += RC_BLOCK) {
    PwSumLong acc;
    acc.init(a.T1);
    for (int t = 0; t < a.T1; ++t) acc.add(t, pool[r * a.T1 + t]);
    favg[r] = acc.sum() / (double)a.T1;
  }
  double nbad = 0.0;
  for (int t = 0; t < RC_BLOCK; ++t) nbad += part[t];
  __syncthreads();
  if (nbad > 0.0) {  // any NaN in the cell: NaN (uniform over the wave)
    if (lane == 0) {
      a.out[c] = xh_nan64();
      if (a.a1) a.a1[c] = xh_nan64();
      if (a.a2) a.a2[c] = xh_nan64();
    }
    return;
  }
  const double A1 = cdf_sq_area(pool, favg, part, nf, a.R, a.np1);
  for (int t = lane; t < a.T2; t += RC_BLOCK) pool[t] = xh_ldw<E>(a.ref, (int64_t)t * a.ld_ref + c);
  const double A2 = cdf_sq_area(pool, favg, part, a.T2, a.R, a.np2);
  if (lane == 0) {
    a.out[c] = 1.0 - A1 / A2;
    if (a.a1) a.a1[c] = A1;
    if (a.a2) a.a2[c] = A2;
  }
}

// ---- xh_ar6_gamma ---------------------------------------------------------------------------------------------------
struct GammaArgs {
  const void* y;
  const double* x;     // (T) device copy of the host abscissa
  const int64_t* seg;  // (nb + 1) device copy of the block offsets, or NULL
  int64_t C, ld, sr, ld_out;
  int T, deg, nb;
  double factor;
  double* gamma;
};

// One lane per (realization, cell): the least-squares polynomial of degree 1 or 2 over the non-NaN years on the abscissa
// centred on its mean and scaled by its largest distance from it (the values centred on their mean as well: the fit with an
// intercept does not move), by the normal equations of at most three unknowns; then the residuals, their block means where
// there are blocks, and factor * std (ddof 0) of what is not NaN.  The series is read from memory in each pass.
template <typename E>
__global__ void __launch_bounds__(XH_BLOCK) k_ar6_gamma(GammaArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t r = blockIdx.y;
  const E* y = reinterpret_cast<const E*>(a.y) + r * a.sr + c;
  auto at = [&](int t) { return (double)y[(int64_t)t * a.ld]; };
  int n = 0;
  double sx = 0.0, sy = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const double v = at(t);
    if (v != v) continue;
    ++n;
    sx += a.x[t];
    sy += v;
  }
  const int64_t o = r * a.ld_out + c;
  if (n <= a.deg) {  // no fit (the reference's polyfit gives NaN coefficients)
    a.gamma[o] = xh_nan64();
    return;
  }
  const double xm = sx / n, ym = sy / n;
  double xs = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const double v = at(t);
    if (v == v) xs = fmax(xs, fabs(a.x[t] - xm));
  }
  xs = xs > 0.0 ? xs : 1.0;
  double s1 = 0, s2 = 0, s3 = 0, s4 = 0, b0 = 0, b1 = 0, b2 = 0;
  for (int t = 0; t < a.T; ++t) {
    const double v = at(t);
    if (v != v) continue;
    const double u = (a.x[t] - xm) / xs, u2 = u * u, w = v - ym;
    s1 += u, s2 += u2, s3 += u2 * u, s4 += u2 * u2;
    b0 += w, b1 += u * w, b2 += u2 * w;
  }
  double c0, c1, c2 = 0.0;
  const double s0 = (double)n;
  if (a.deg == 1) {
    const double det = s0 * s2 - s1 * s1;
    c0 = (b0 * s2 - s1 * b1) / det;
    c1 = (s0 * b1 - s1 * b0) / det;
  } else {  // Cramer's rule on [[s0 s1 s2] [s1 s2 s3] [s2 s3 s4]]
    const double m00 = s2 * s4 - s3 * s3, m01 = s1 * s4 - s2 * s3, m02 = s1 * s3 - s2 * s2;
    const double det = s0 * m00 - s1 * m01 + s2 * m02;
    c0 = (b0 * m00 - s1 * (b1 * s4 - s3 * b2) + s2 * (b1 * s3 - s2 * b2)) / det;
    c1 = (s0 * (b1 * s4 - s3 * b2) - b0 * m01 + s2 * (s1 * b2 - b1 * s2)) / det;
    c2 = (s0 * (s2 * b2 - b1 * s3) - s1 * (s1 * b2 - b1 * s2) + b0 * m02) / det;
  }
  auto resid = [&](int t, double v) {
    const double u = (a.x[t] - xm) / xs;
    return (v - ym) - (c0 + u * (c1 + u * c2));
  };
  // two passes over the items (years, or block means): their mean, then the mean squared deviation
  double mean = 0.0, acc = 0.0;
  int items = 0;
  for (int pass = 0; pass < 2; ++pass) {
    acc = 0.0;
    items = 0;
    const int groups = a.nb > 0 ? a.nb : 1;
    for (int k = 0; k < groups; ++k) {
      const int t0 = a.nb > 0 ? (int)a.seg[k] : 0, t1 = a.nb > 0 ? (int)a.seg[k + 1] : a.T;
      double bs = 0.0;
      int bn = 0;
      for (int t = t0; t < t1; ++t) {
        const double v = at(t);
        if (v != v) continue;
        const double e = resid(t, v);
        if (a.nb > 0) {
          bs += e;
          ++bn;
        } else {
          acc += pass ? (e - mean) * (e - mean) : e;
          ++items;
        }
      }
      if (a.nb > 0 && bn > 0) {
        const double bm = bs / bn;
        acc += pass ? (bm - mean) * (bm - mean) : bm;
        ++items;
      }
    }
    if (!pass) mean = acc / items;
  }
  a.gamma[o] = a.factor * sqrt(acc / items);
}

}  // namespace

int xh_change_test(xh_ctx* ctx, const void* fut, const void* ref, int64_t R, int64_t T1, int64_t T2, int64_t C, int64_t ld_fut,
                   int64_t stride_r_fut, int64_t ld_ref, int64_t stride_r_ref, int f64, int test, const double* sf, int64_t nsf,
                   double* delta, double* mean_ref, int32_t* n_fut, int32_t* n_ref, double* stat, double* df, double* pvals,
                   uint8_t* status, int64_t ld_out) {
  const char* fn = "xh_change_test";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(test >= 0 && test < XH_CT_NTESTS, XH_ERR_ARG, "%s: unknown test %d", fn, test);
  XH_REQUIRE(R >= 1 && R <= 65535 && T1 >= 1 && T2 >= 1 && C >= 0, XH_ERR_ARG, "%s: bad shape (R %lld, T1 %lld, T2 %lld, C %lld)", fn,
             (long long)R, (long long)T1, (long long)T2, (long long)C);
  XH_REQUIRE(T1 <= XH_CT_MAX_T && T2 <= XH_CT_MAX_T, XH_ERR_LIMIT, "%s: at most %d values per series, got %lld and %lld", fn,
             XH_CT_MAX_T, (long long)T1, (long long)T2);
  XH_REQUIRE(ld_fut >= C && ld_ref >= C && ld_out >= C, XH_ERR_LAYOUT, "%s: a row pitch below C", fn);
  XH_REQUIRE(stride_r_fut >= 0 && stride_r_ref >= 0, XH_ERR_LAYOUT, "%s: a negative realization stride", fn);
  const bool exact_table = test == XH_CT_MWU && (T1 <= 8 || T2 <= 8);
  XH_REQUIRE(exact_table ? (sf && nsf == T1 * T2 + 1) : (!sf && nsf == 0), XH_ERR_ARG,
             "%s: sf must hold T1 * T2 + 1 values for the Mann-Whitney test with a length of at most 8, and be NULL otherwise", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(fut && ref && delta && mean_ref && n_fut && n_ref, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(test == XH_CT_MOMENTS || (stat && df && pvals && status), XH_ERR_ARG, "%s: the test needs stat, df, pvals and status", fn);
  const int64_t lim = (int64_t)1 << 40;
  XH_REQUIRE((R - 1) * stride_r_fut + T1 * ld_fut + C < lim && (R - 1) * stride_r_ref + T2 * ld_ref + C < lim && R * ld_out + C < lim &&
                 (T1 + T2) * R * C < ((int64_t)1 << 36),
             XH_ERR_LIMIT, "%s: field too large", fn);
  ChangeArgs a{};
  a.fut = fut;
  a.ref = ref;
  a.C = C;
  a.ld_fut = ld_fut;
  a.sr_fut = stride_r_fut;
  a.ld_ref = ld_ref;
  a.sr_ref = stride_r_ref;
  a.ld_out = ld_out;
  a.T1 = (int)T1;
  a.T2 = (int)T2;
  a.test = test;
  a.lds = T1 + T2 <= XH_CT_LDS_SLOTS;
  a.delta = delta;
  a.mean_ref = mean_ref;
  a.n_fut = n_fut;
  a.n_ref = n_ref;
  a.stat = stat;
  a.df = df;
  a.pvals = pvals;
  a.status = status;
  const size_t esize = f64 ? sizeof(double) : sizeof(float);
  size_t cur = 0;
  if (exact_table) {
    void* d_sf = nullptr;
    const int rc = xh_scratch_upload(ctx, &cur, sf, sizeof(double) * (size_t)nsf, &d_sf);
    if (rc) return rc;
    a.sf = (const double*)d_sf;
    a.has_sf = 1;
  }
  if (!a.lds) {
    void* w = nullptr;
    const int rc = xh_big_scratch(ctx, esize * (size_t)(T1 + T2) * (size_t)R * (size_t)C, &w);
    if (rc) return rc;
    a.work = w;
    a.work_stride = R * C;
  }
  const size_t shmem = a.lds ? esize * CT_BLOCK * (size_t)(T1 + T2) : 0;
  const dim3 grid((unsigned)cdiv64(C, CT_BLOCK), (unsigned)R);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_change_test<XH_WIDTH(w)>, grid, dim3(CT_BLOCK), shmem, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_robust_fractions(xh_ctx* ctx, const double* delta, const uint8_t* changed, const uint8_t* valid, const double* mean_ref, int64_t R,
                        int64_t C, int64_t ld, const double* weights, int strict_sign, int thresh_kind, double thresh, double* out,
                        int64_t ld_out) {
  const char* fn = "xh_robust_fractions";
  const int rc0 = xh_check_pitched(fn, ctx, R, C, ld, XH_RF_NFRAC, ld_out);
  if (rc0) return rc0;
  XH_REQUIRE(R >= 1, XH_ERR_ARG, "%s: needs R >= 1", fn);
  XH_REQUIRE(thresh_kind >= XH_RF_THRESH_NONE && thresh_kind <= XH_RF_THRESH_REL, XH_ERR_ARG, "%s: unknown threshold kind %d", fn, thresh_kind);
  XH_REQUIRE(thresh_kind == XH_RF_THRESH_NONE || !changed, XH_ERR_ARG, "%s: a threshold and `changed` are both given", fn);
  XH_REQUIRE(weights, XH_ERR_ARG, "%s: NULL weights", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(delta && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(thresh_kind != XH_RF_THRESH_REL || mean_ref, XH_ERR_ARG, "%s: the relative threshold needs mean_ref", fn);
  size_t cur = 0;
  void* d_w = nullptr;
  const int rc = xh_scratch_upload(ctx, &cur, weights, sizeof(double) * (size_t)R, &d_w);
  if (rc) return rc;
  FracArgs a{};
  a.delta = delta;
  a.changed = changed;
  a.valid = valid;
  a.mean_ref = mean_ref;
  a.w = (const double*)d_w;
  a.R = R;
  a.C = C;
  a.ld = ld;
  a.ld_out = ld_out;
  a.strict = strict_sign != 0;
  a.kind = thresh_kind;
  a.thresh = thresh;
  a.out = out;
  hipLaunchKernelGGL(k_robust_fractions, dim3((unsigned)cdiv64(C, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_robust_coefficient(xh_ctx* ctx, const void* fut, const void* ref, int64_t R, int64_t T1, int64_t T2, int64_t C, int64_t ld_fut,
                          int64_t stride_r_fut, int64_t ld_ref, int f64, double* out, double* a1, double* a2) {
  const char* fn = "xh_robust_coefficient";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(R >= 1 && T1 >= 1 && T2 >= 1 && C >= 0, XH_ERR_ARG, "%s: bad shape (R %lld, T1 %lld, T2 %lld, C %lld)", fn, (long long)R,
             (long long)T1, (long long)T2, (long long)C);
  XH_REQUIRE(T1 <= XH_CT_MAX_T && R <= XH_RC_MAX_POOL && R * T1 + R <= XH_RC_MAX_POOL && T2 + R <= XH_RC_MAX_POOL, XH_ERR_LIMIT,
             "%s: R T1 + R and T2 + R of at most %d values and T1 of at most %d are served, got R %lld, T1 %lld, T2 %lld", fn, XH_RC_MAX_POOL,
             XH_CT_MAX_T, (long long)R, (long long)T1, (long long)T2);
  XH_REQUIRE(ld_fut >= C && ld_ref >= C && stride_r_fut >= 0, XH_ERR_LAYOUT, "%s: a row pitch below C, or a negative realization stride", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(fut && ref && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE((R - 1) * stride_r_fut + T1 * ld_fut + C < ((int64_t)1 << 40) && T2 * ld_ref + C < ((int64_t)1 << 40) && C <= 0x7fffffff,
             XH_ERR_LIMIT, "%s: field too large", fn);
  auto pow2 = [](int64_t n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
  };
  CoefArgs a{};
  a.fut = fut;
  a.ref = ref;
  a.C = C;
  a.ld_fut = ld_fut;
  a.sr_fut = stride_r_fut;
  a.ld_ref = ld_ref;
  a.R = (int)R;
  a.T1 = (int)T1;
  a.T2 = (int)T2;
  a.np1 = pow2(R * T1 + R);
  a.np2 = pow2(T2 + R);
  a.npad = a.np1 > a.np2 ? a.np1 : a.np2;
  a.out = out;
  a.a1 = a1;
  a.a2 = a2;
  const size_t lds = sizeof(double) * ((size_t)a.npad + (size_t)R + RC_BLOCK);
  const dim3 g((unsigned)C), b(RC_BLOCK);
  const int rc = xh_by_width(f64, [&](auto w) { return xh_launch_lds(k_robust_coefficient<XH_WIDTH(w)>, g, b, lds, ctx->stream, a); });
  if (rc) return rc;
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_ar6_gamma(xh_ctx* ctx, const void* y, int64_t R, int64_t T, int64_t C, int64_t ld, int64_t stride_r, int f64, const double* x,
                 int deg, const int64_t* seg, int64_t nb, double factor, double* gamma, int64_t ld_out) {
  const char* fn = "xh_ar6_gamma";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(R >= 1 && R <= 65535 && T >= 1 && C >= 0, XH_ERR_ARG, "%s: bad shape (R %lld, T %lld, C %lld)", fn, (long long)R, (long long)T,
             (long long)C);
  XH_REQUIRE(T <= XH_CT_MAX_T, XH_ERR_LIMIT, "%s: at most %d years, got %lld", fn, XH_CT_MAX_T, (long long)T);
  XH_REQUIRE(deg == 1 || deg == 2, XH_ERR_ARG, "%s: deg must be 1 or 2, got %d", fn, deg);
  XH_REQUIRE(x, XH_ERR_ARG, "%s: NULL abscissa", fn);
  XH_REQUIRE(nb >= 0 && nb <= T && (nb == 0) == (seg == nullptr), XH_ERR_ARG, "%s: nb blocks need nb + 1 offsets, no blocks none", fn);
  if (nb > 0) {
    const int rc = xh_check_offsets(fn, seg, nb, T, "block", XH_CT_MAX_T);
    if (rc) return rc;
  }
  XH_REQUIRE(ld >= C && ld_out >= C && stride_r >= 0, XH_ERR_LAYOUT, "%s: a row pitch below C, or a negative realization stride", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(y && gamma, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE((R - 1) * stride_r + T * ld + C < ((int64_t)1 << 40) && R * ld_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  size_t cur = 0;
  void* d_x = nullptr;
  void* d_seg = nullptr;
  int rc = xh_scratch_upload(ctx, &cur, x, sizeof(double) * (size_t)T, &d_x);
  if (rc) return rc;
  if (nb > 0) {
    rc = xh_scratch_upload(ctx, &cur, seg, sizeof(int64_t) * (size_t)(nb + 1), &d_seg);
    if (rc) return rc;
  }
  GammaArgs a{};
  a.y = y;
  a.x = (const double*)d_x;
  a.seg = (const int64_t*)d_seg;
  a.C = C;
  a.ld = ld;
  a.sr = stride_r;
  a.ld_out = ld_out;
  a.T = (int)T;
  a.deg = deg;
  a.nb = (int)nb;
  a.factor = factor;
  a.gamma = gamma;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)R);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_ar6_gamma<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
