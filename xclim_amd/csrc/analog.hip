// analog.hip — the eight dissimilarity metrics of xclim.analog (analog.py:181-628) between one target sample and the candidate
// sample of every grid cell.  C ABI and the exact definition of every result: include/ext/xclim_hip_analog.h.
//
// k_analog: one lane per candidate cell, 256 lanes to a workgroup, lanes striding over the cells (c, c + G, ...).  The target
// table — x (n, d), its column means, deviations and variances, the method's parameters — is copied to LDS once per workgroup
// and read from there at wave-uniform addresses (a broadcast); that copy is the kernel's only barrier.  A lane's own sample is
// never held: point i, index k of cell c is element i * ld + c of field k, so a wave reads 64 consecutive elements and the
// re-reads of the pair loops come from the caches.  What a lane keeps in registers is ONE point and the per-index statistics of
// its cell (arrays of XH_ANALOG_MAX_D, indexed by fully unrolled loops only).  The per-lane arrays whose index is data — Prim's
// keys and sides, the KS counters, kldiv's smallest distances — are in the work buffer, slot-major: slot s of lane g is element
// s * G + g, so neighbouring lanes touch neighbouring addresses.
//
// The method is a template argument: a kernel carries the loops of its own metric only.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/ext/xclim_hip_analog.h"
#include "hostargs.h"

namespace {

constexpr int MAXD = XH_ANALOG_MAX_D;
constexpr size_t WORK_BYTES = (size_t)1 << 30;

struct AnalogArgs {
  const void* y[MAXD];
  const double* tab;  // x (n d) | mean x (d) | std x (d) | var x (d) | par (npar)
  const double* r;    // kldiv: (nk, n)
  int32_t k[XH_ANALOG_MAX_NK];
  double* out;
  void* work;
  int64_t C, ld, ld_out, G;
  int n, m, d, nk, kmax, ntab, all_nan;
};

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7FF0000000000000LL); }

// the d coordinates of a pooled point (p < n: of x, from LDS; else point p - n of the lane's cell) into registers
template <typename TE>
__device__ __forceinline__ void point(const AnalogArgs& a, const double* x, int64_t c, int p, double (&pc)[MAXD]) {
#pragma unroll
  for (int k = 0; k < MAXD; ++k) {
    pc[k] = 0.0;
    if (k < a.d) pc[k] = p < a.n ? x[p * a.d + k] : xh_ldw<TE>(a.y[k], (int64_t)(p - a.n) * a.ld + c);
  }
}

// the squared distance from the point in registers to pooled point q.  PLAIN: sum_k (pc_k - q_k)^2; SCALED: sum_k (pc_k - q_k)^2 / v_k
// (scipy's seuclidean); DIVIDED: sum_k (pc_k - q_k / v_k)^2, pc divided already (the reference's standardize)
enum { PLAIN, SCALED, DIVIDED };
template <typename TE, int MODE>
__device__ __forceinline__ double dist2(const AnalogArgs& a, const double* x, int64_t c, const double (&pc)[MAXD], int q,
                                        const double (&v)[MAXD]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MAXD; ++k) {
    if (k < a.d) {
      double qk = q < a.n ? x[q * a.d + k] : xh_ldw<TE>(a.y[k], (int64_t)(q - a.n) * a.ld + c);
      if (MODE == DIVIDED) qk = qk / v[k];
      const double t = pc[k] - qk;
      s += MODE == SCALED ? (t * t) / v[k] : t * t;
    }
  }
  return s;
}

template <typename TE, int M>
__global__ void __launch_bounds__(XH_BLOCK) k_analog(AnalogArgs a) {
  extern __shared__ double tab[];
  for (int i = threadIdx.x; i < a.ntab; i += XH_BLOCK) tab[i] = a.tab[i];
  __syncthreads();
  const int n = a.n, m = a.m, d = a.d, N = a.n + a.m;
  const double* x = tab;
  const double* mx = tab + n * d;
  const double* sx = mx + d;
  const double* vx = sx + d;
  const double* par = vx + d;
  const int64_t G = a.G;
  const int64_t g = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  const double nan = xh_nan64();
  const int nout = M == XH_ANALOG_KLDIV ? a.nk : 1;
  constexpr bool STATS = M == XH_ANALOG_SEUCLIDEAN || M == XH_ANALOG_MAHALANOBIS || M == XH_ANALOG_NEAREST_NEIGHBOR ||
                         M == XH_ANALOG_ZECH_ASLAN || M == XH_ANALOG_SZEKELY_RIZZO;

  for (int64_t c = g; c < a.C; c += G) {
    // the cell's NaN test, column means and (ddof = 1) deviations, in row order
    bool bad = a.all_nan != 0;
    double my[MAXD], sy[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) my[k] = sy[k] = 0.0;
    if (!bad) {
      for (int i = 0; i < m; ++i) {
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
          if (k < d) {
            const double v = xh_ldw<TE>(a.y[k], (int64_t)i * a.ld + c);
            bad |= v != v;
            my[k] += v;
          }
        }
      }
    }
    if (bad || (M == XH_ANALOG_KLDIV && (n < 5 || m < 5))) {
      for (int q = 0; q < nout; ++q) a.out[q * a.ld_out + c] = nan;
      continue;
    }
    if (STATS) {
#pragma unroll
      for (int k = 0; k < MAXD; ++k) my[k] = my[k] / (double)m;
      if (M != XH_ANALOG_SEUCLIDEAN && M != XH_ANALOG_MAHALANOBIS) {
        for (int i = 0; i < m; ++i) {
#pragma unroll
          for (int k = 0; k < MAXD; ++k) {
            if (k < d) {
              const double t = xh_ldw<TE>(a.y[k], (int64_t)i * a.ld + c) - my[k];
              sy[k] += t * t;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < MAXD; ++k) sy[k] = sqrt(sy[k] / (double)(m - 1));
      }
    }

    double res = nan;
    double pc[MAXD], v[MAXD];
#pragma unroll
    for (int k = 0; k < MAXD; ++k) v[k] = 1.0;

    if (M == XH_ANALOG_SEUCLIDEAN) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < MAXD; ++k) {
        if (k < d) {
          const double t = mx[k] - my[k];
          s += (t * t) / vx[k];
        }
      }
      res = sqrt(s);
    } else if (M == XH_ANALOG_MAHALANOBIS) {
#pragma unroll
      for (int k = 0; k < MAXD; ++k) pc[k] = k < d ? mx[k] - my[k] : 0.0;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < MAXD; ++j) {
        if (j < d) {
          double t = 0.0;
#pragma unroll
          for (int i = 0; i < MAXD; ++i)
            if (i < d) t += pc[i] * par[i * d + j];
          s += t * pc[j];
        }
      }
      res = sqrt(s);
    } else if (M == XH_ANALOG_ZECH_ASLAN || M == XH_ANALOG_SZEKELY_RIZZO) {
      const bool zech = M == XH_ANALOG_ZECH_ASLAN;
      if (zech || par[0] != 0.0) {
#pragma unroll
        for (int k = 0; k < MAXD; ++k) v[k] = k < d ? sx[k] * sy[k] : 1.0;
      }
      const double dmin = zech ? par[0] : 0.0;
      double sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int i = 0; i < N; ++i) {
        point<TE>(a, x, c, i, pc);
        double own = 0.0, cross = 0.0;
        // x_i against x_j, j > i; y_i against y_j, j > i (the pairs of one sample), and y_i against every x_j
        for (int j = i + 1; j < (i < n ? n : N); ++j) {
          double t = sqrt(dist2<TE, SCALED>(a, x, c, pc, j, v));
          if (zech) t = log(t < dmin ? dmin : t);
          own += t;
        }
        if (i >= n) {
          for (int j = 0; j < n; ++j) {
            double t = sqrt(dist2<TE, SCALED>(a, x, c, pc, j, v));
            if (zech) t = log(t < dmin ? dmin : t);
            cross += t;
          }
          syy += own;
          sxy += cross;
        } else {
          sxx += own;
        }
      }
      const double dn = (double)n, dm = (double)m;
      if (zech) {
        res = (-sxx) / (dn * (dn - 1.0)) + (-syy) / (dm * (dm - 1.0)) - (-sxy) / (dn * dm);
      } else {
        const double sXY = sxy / (dn * dm), sXX = sxx * 2.0 / (dn * dn), sYY = syy * 2.0 / (dm * dm);
        const double w = (dn * dm) / (dn + dm);
        res = w * (sXY + sXY - sXX - sYY);
      }
    } else if (M == XH_ANALOG_NEAREST_NEIGHBOR) {
#pragma unroll
      for (int k = 0; k < MAXD; ++k) v[k] = k < d ? sqrt(sx[k] * sy[k]) : 1.0;
      int same = 0;
      bool finite = true;
      for (int p = 0; p < N; ++p) {
        point<TE>(a, x, c, p, pc);
#pragma unroll
        for (int k = 0; k < MAXD; ++k) pc[k] = pc[k] / v[k];
        double best = inf64();
        int bq = -1;
        for (int q = 0; q < N; ++q) {
          if (q == p) continue;
          const double t = dist2<TE, DIVIDED>(a, x, c, pc, q, v);
          finite &= (t - t) == 0.0;
          if (t < best) best = t, bq = q;
        }
        same += (bq >= 0 && (p < n) == (bq < n)) ? 1 : 0;
      }
      res = finite ? (double)same / (double)N : nan;
    } else if (M == XH_ANALOG_FRIEDMAN_RAFSKY) {
      double* key = static_cast<double*>(a.work) + g;  // slot s: key[s * G]; sides in slots N .. 2 N - 1
      double* side = key + (int64_t)N * G;
      for (int j = 0; j < N; ++j) key[j * G] = inf64(), side[j * G] = 0.0;
      key[0] = -1.0;  // in the tree
      int cur = 0, cross = 0;
      bool whole = true;
      for (int step = 1; step < N; ++step) {
        point<TE>(a, x, c, cur, pc);
        const double cs = cur < n ? 1.0 : 0.0;
        double best = inf64(), bs = 0.0;
        int bq = -1;
        for (int j = 0; j < N; ++j) {
          double kj = key[j * G];
          if (kj < 0.0) continue;
          double sj = side[j * G];
          const double t = dist2<TE, PLAIN>(a, x, c, pc, j, v);
          if (t < kj) {
            kj = t, sj = cs;
            key[j * G] = kj, side[j * G] = sj;
          }
          if (kj < best) best = kj, bq = j, bs = sj;
        }
        if (bq < 0) {
          whole = false;
          break;
        }
        cross += (bs != 0.0) != (bq < n) ? 1 : 0;
        key[bq * G] = -1.0;
        cur = bq;
      }
      res = whole ? 1.0 - (1.0 + (double)cross) / (double)N : nan;
    } else if (M == XH_ANALOG_KOLMOGOROV_SMIRNOV) {
      int32_t* cnt = static_cast<int32_t*>(a.work) + g;
      const int nc = 1 << d;
      double best = 0.0;
      for (int p = 0; p < N; ++p) {
        point<TE>(a, x, c, p, pc);
        for (int s = 0; s < nc; ++s) cnt[s * G] = 0;
        for (int q = 0; q < N; ++q) {
          int code = 0;
#pragma unroll
          for (int k = 0; k < MAXD; ++k) {
            if (k < d) {
              const double qk = q < n ? x[q * d + k] : xh_ldw<TE>(a.y[k], (int64_t)(q - n) * a.ld + c);
              code |= (pc[k] <= qk ? 1 : 0) << k;
            }
          }
          cnt[code * G] += q < n ? 1 : 65536;
        }
        for (int s = 0; s < nc; ++s) {
          const int32_t t = cnt[s * G];
          if (t != 0) {
            const double dd = fabs((double)(t & 0xFFFF) / (double)n - (double)(t >> 16) / (double)m);
            best = dd > best ? dd : best;
          }
        }
      }
      res = best;
    } else if (M == XH_ANALOG_KLDIV) {
      double* list = static_cast<double*>(a.work) + g;
      const int kmax = a.kmax;
      double acc[XH_ANALOG_MAX_NK];
#pragma unroll
      for (int q = 0; q < XH_ANALOG_MAX_NK; ++q) acc[q] = 0.0;
      for (int i = 0; i < n; ++i) {
        point<TE>(a, x, c, i, pc);
        for (int s = 0; s < kmax; ++s) list[s * G] = inf64();
        for (int j = n; j < N; ++j) {
          const double t = dist2<TE, PLAIN>(a, x, c, pc, j, v);
          if (t < list[(int64_t)(kmax - 1) * G]) {  // insert into the ascending list, after its equals
            int s = kmax - 1;
            while (s > 0) {
              const double u = list[(int64_t)(s - 1) * G];
              if (!(u > t)) break;
              list[s * G] = u;
              --s;
            }
            list[s * G] = t;
          }
        }
#pragma unroll
        for (int q = 0; q < XH_ANALOG_MAX_NK; ++q) {
          if (q < a.nk) {
            const double s = sqrt(list[(int64_t)(a.k[q] - 1) * G]);
            acc[q] += log(a.r[q * n + i] / s);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < XH_ANALOG_MAX_NK; ++q)
        if (q < a.nk) a.out[q * a.ld_out + c] = (-acc[q]) * (double)d / (double)n + log((double)m / ((double)n - 1.0));
    }
    if (M != XH_ANALOG_KLDIV) a.out[c] = res;
  }
}

// bytes of the per-lane arrays of a method
size_t lane_bytes(int method, int64_t N, int d, int kmax) {
  if (method == XH_ANALOG_FRIEDMAN_RAFSKY) return (size_t)(2 * N) * sizeof(double);
  if (method == XH_ANALOG_KOLMOGOROV_SMIRNOV) return ((size_t)1 << d) * sizeof(int32_t);
  if (method == XH_ANALOG_KLDIV) return (size_t)kmax * sizeof(double);
  return 0;
}

template <typename F>
void analog_by_method(int method, F&& f) {
  xh_pick<XH_ANALOG_SEUCLIDEAN, XH_ANALOG_NEAREST_NEIGHBOR, XH_ANALOG_ZECH_ASLAN, XH_ANALOG_SZEKELY_RIZZO, XH_ANALOG_FRIEDMAN_RAFSKY,
          XH_ANALOG_KOLMOGOROV_SMIRNOV, XH_ANALOG_KLDIV, XH_ANALOG_MAHALANOBIS>(method, f);
}

}  // namespace

int xh_analog(xh_ctx* ctx, int method, int64_t n, int64_t m, int d, const double* x, int64_t C, int64_t ld, int f64,
              const void* const* y, const double* par, int64_t npar, const int32_t* k, int64_t nk, double* out, int64_t ld_out) {
  const char* fn = "xh_analog";
  const bool kl = method == XH_ANALOG_KLDIV;
  int rc = xh_check_pitched(fn, ctx, m, C, ld, kl ? nk : 1, ld_out);
  if (rc) return rc;
  XH_REQUIRE(method >= 0 && method < XH_ANALOG_NMETHODS, XH_ERR_ARG, "%s: unknown method %d", fn, method);
  XH_REQUIRE(n >= 1 && m >= 1 && d >= 1, XH_ERR_ARG, "%s: n, m and d must be at least 1, got %lld, %lld, %d", fn, (long long)n,
             (long long)m, d);
  XH_REQUIRE(n <= XH_ANALOG_MAX_SAMPLE && m <= XH_ANALOG_MAX_SAMPLE, XH_ERR_LIMIT, "%s: samples of up to %d points, got %lld and %lld",
             fn, XH_ANALOG_MAX_SAMPLE, (long long)n, (long long)m);
  XH_REQUIRE(d <= XH_ANALOG_MAX_D, XH_ERR_LIMIT, "%s: at most %d indices, got %d", fn, XH_ANALOG_MAX_D, d);
  XH_REQUIRE(method != XH_ANALOG_KOLMOGOROV_SMIRNOV || d <= XH_ANALOG_KS_MAX_D, XH_ERR_LIMIT,
             "%s: kolmogorov_smirnov takes at most %d indices, got %d", fn, XH_ANALOG_KS_MAX_D, d);
  XH_REQUIRE(x && y && out, XH_ERR_ARG, "%s: NULL argument", fn);
  for (int j = 0; j < d; ++j) XH_REQUIRE(y[j], XH_ERR_ARG, "%s: field %d is NULL", fn, j);
  const int64_t want = method == XH_ANALOG_ZECH_ASLAN || method == XH_ANALOG_SZEKELY_RIZZO ? 1
                       : method == XH_ANALOG_MAHALANOBIS                                       ? (int64_t)d * d
                                                                                               : 0;
  XH_REQUIRE(npar == want && (want == 0 || par), XH_ERR_ARG, "%s: method %d takes %lld parameters, got %lld", fn, method, (long long)want,
             (long long)npar);
  int kmax = 0;
  if (kl) {
    XH_REQUIRE(k && nk >= 1, XH_ERR_ARG, "%s: kldiv needs at least one k", fn);
    XH_REQUIRE(nk <= XH_ANALOG_MAX_NK, XH_ERR_LIMIT, "%s: at most %d values of k, got %lld", fn, XH_ANALOG_MAX_NK, (long long)nk);
    for (int64_t q = 0; q < nk; ++q) {
      XH_REQUIRE(k[q] >= 1, XH_ERR_ARG, "%s: k must be at least 1, got %d", fn, k[q]);
      XH_REQUIRE(k[q] <= XH_ANALOG_MAX_K, XH_ERR_LIMIT, "%s: k of up to %d, got %d", fn, XH_ANALOG_MAX_K, k[q]);
      kmax = k[q] > kmax ? k[q] : kmax;
    }
  } else {
    XH_REQUIRE(nk == 0, XH_ERR_ARG, "%s: only kldiv takes k", fn);
  }
  if (C == 0) return XH_OK;

  // the target table: x, its column means, deviations and variances as numpy computes them (row order, ddof = 1), the parameters
  const size_t nd = (size_t)n * d;
  std::vector<double> tab(nd + 3 * (size_t)d + (size_t)npar, 0.0);
  bool all_nan = false;
  for (size_t i = 0; i < nd; ++i) tab[i] = x[i], all_nan |= x[i] != x[i];
  double *mx = tab.data() + nd, *sx = mx + d, *vx = sx + d;
  for (int j = 0; j < d; ++j) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i * d + j];
    mx[j] = s / (double)n;
    s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double t = x[i * d + j] - mx[j];
      s += t * t;
    }
    vx[j] = s / (double)(n - 1);
    sx[j] = sqrt(vx[j]);
  }
  for (int64_t i = 0; i < npar; ++i) tab[nd + 3 * (size_t)d + (size_t)i] = par[i];

  AnalogArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, (const double*)tab.data(), tab.size(), &a.tab);
  if (rc) return rc;
  if (kl) {
    // r: the (k + 1)-th smallest of the distances from x_i to the points of x, its own 0 among them
    std::vector<double> r((size_t)nk * (size_t)n), dist((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      for (int64_t j = 0; j < n; ++j) {
        double s = 0.0;
        for (int q = 0; q < d; ++q) {
          const double t = x[i * d + q] - x[j * d + q];
          s += t * t;
        }
        dist[(size_t)j] = s;
      }
      std::sort(dist.begin(), dist.end());
      for (int64_t q = 0; q < nk; ++q) r[(size_t)(q * n + i)] = k[q] < n ? sqrt(dist[(size_t)k[q]]) : (double)INFINITY;
    }
    rc = xh_upload(ctx, &cur, (const double*)r.data(), r.size(), &a.r);
    if (rc) return rc;
    for (int64_t q = 0; q < nk; ++q) a.k[q] = k[q];
  }
  for (int j = 0; j < d; ++j) a.y[j] = y[j];
  a.out = out;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.n = (int)n, a.m = (int)m, a.d = d, a.nk = (int)nk, a.kmax = kmax, a.ntab = (int)tab.size(), a.all_nan = all_nan;

  // the launch: lanes whose arrays fit the work buffer, at most 8 workgroups per CU, never more than the cells need
  const size_t per_lane = lane_bytes(method, n + m, d, kmax);
  int64_t blocks = cdiv64(C, XH_BLOCK);
  const int64_t resident = (int64_t)(ctx->num_cu > 0 ? ctx->num_cu : 256) * 8;
  blocks = blocks < resident ? blocks : resident;
  if (per_lane) {
    const int64_t fit = (int64_t)(WORK_BYTES / (per_lane * XH_BLOCK));
    blocks = blocks < fit ? blocks : (fit < 1 ? 1 : fit);
  }
  if (const char* e = xh_diag_env("XH_ANALOG_MAX_BLOCKS")) {  // diagnostics: a small launch, so that few cells already stride
    const int64_t cap = atoll(e);
    if (cap >= 1 && cap < blocks) blocks = cap;
  }
  a.G = blocks * XH_BLOCK;
  if (per_lane) {
    rc = xh_big_scratch(ctx, per_lane * (size_t)a.G, &a.work);
    if (rc) return rc;
  }
  const dim3 g((unsigned)blocks), b(XH_BLOCK);
  const size_t lds = tab.size() * sizeof(double);
  xh_by_width(f64, [&](auto w) {
    using TE = XH_WIDTH(w);
    analog_by_method(method, [&](auto mm) { hipLaunchKernelGGL((k_analog<TE, decltype(mm)::value>), g, b, lds, ctx->stream, a); });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
