// f64red.hip — float64 FIELD twins of the period reductions: thresholded sums / statistics (degree days), the two-field
// temperature ranges, domain and bivariate counts, and the rolling window statistics of select_rolling_resample_op.
//
// The reference computes in the dtype of its data: (data - thresh).clip(0).resample().sum() of a float64 tas is a float64
// sum (indices/generic.py:1514-1552, 1323-1357, 1278-1320), high - low of float64 fields is float64 (:1076-1105, 1360-1414),
// and rolling(time=w).<op>() adds its window in float64 (:128-174).  The float32 kernels (reduce2.hip, elemwise.hip,
// reduce.hip, window.hip) form those differences in float32 and write float32; these twins read the float64 field as it is,
// form every difference and compare in float64 and write float64 (counts stay int32).  A float32 side of a two-field call
// is widened exactly (numpy promotion); a float32 side compared against a scalar compares against the float32-rounded
// scalar (numpy's weak-scalar rule, as the float32 kernels do).
//
// Every sum is added in row order t0, t0 + 1, ... (oracle._nanreduce / numpy's axis-0 sum of a C-contiguous group, and
// oracle.generic.rolling: window rows first to last), so the results are bit-identical to the oracle run on the float64
// arrays.  The valid counts (MissingAny's non-NaN steps per period) are those of the float32 twins.
//
// The marches follow f64.hip / f64run.hip: one lane per cell or two cells per lane (16-byte double2 loads, 8-byte float2
// for a float32 side), rows in double-buffered batches of 8, periods from seg_off over blockIdx.y, the grid sized from the
// number of cells per lane that is launched.
#include <stdlib.h>

#include "common.h"
#include "f64util.h"

namespace {

// Run-time operator as wave-uniform masks (common.h xh_cmp_f32 in float64): the loop bodies stay branch-free, so the waits
// for a batch of rows are counted instead of draining every load at a divergent branch (numpy: NaN compares False
// except for !=)
struct Cmp64 {
  bool gt, lt, eq, un;
};
__host__ __device__ inline Cmp64 cmp_masks(int op) {
  return Cmp64{op == XH_OP_GT || op == XH_OP_GE || op == XH_OP_NE, op == XH_OP_LT || op == XH_OP_LE || op == XH_OP_NE,
               op == XH_OP_GE || op == XH_OP_LE || op == XH_OP_EQ, op == XH_OP_NE};
}
__device__ __forceinline__ bool cmpm(double a, const Cmp64& m, double b) {
  return (m.gt & (a > b)) | (m.lt & (a < b)) | (m.eq & (a == b)) | (m.un & ((a != a) | (b != b)));
}

// ---- thresholded reductions (reduce2.hip k_thresholded_reduce in float64) ------------------------------------------
// mode 0: thresholded_statistics: reducer of data.where(data op thr)          (gen:1278-1320)
// mode 1: temperature_sum: direction * sum((data - thr).where(data op thr))   (gen:1323-1357)
// mode 2: cumulative_difference: sum(clip(data - thr, 0)) for > / >=, sum(clip(thr - data, 0)) for < / <=  (gen:1514-1552)
template <int VEC, int MODE>
__global__ void __launch_bounds__(XH_BLOCK)
k_thresholded_reduce_f64(const double* __restrict__ x, int64_t C, int64_t st, int op, double thr, int reducer,
                         const int64_t* __restrict__ seg_off, int P, double* __restrict__ out, int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const bool below = (op == XH_OP_LT || op == XH_OP_LE);
  const Cmp64 m = cmp_masks(op);
  const bool want_min = reducer == XH_RED_MIN;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
    double s[VEC], ext[VEC];
    int n[VEC], val[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s[i] = 0.0, ext[i] = 0.0, n[i] = 0, val[i] = 0;
    march<VEC>(x + c, st, t0, t1, [&](int64_t, const VR<double, VEC>& xv) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double v = xv.v[i];
        val[i] += (v == v) ? 1 : 0;
        double d;
        bool take;
        if (MODE == 2) {
          d = below ? (thr - v) : (v - thr);
          d = d < 0.0 ? 0.0 : d;  // clip(0); NaN stays NaN and is skipped by the sum
          take = d == d;
        } else {
          d = (MODE == 1) ? (v - thr) : v;
          take = cmpm(v, m, thr);
        }
        s[i] = take ? s[i] + d : s[i];
        if (MODE == 0) {
          ext[i] = (take && (n[i] == 0 || (want_min ? d < ext[i] : d > ext[i]))) ? d : ext[i];
          n[i] += take ? 1 : 0;
        }
      }
    });
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double r;
      if (MODE == 2) r = s[i];
      else if (MODE == 1) r = below ? -s[i] : s[i];
      else if (reducer == XH_RED_SUM) r = s[i];
      else if (n[i] == 0) r = xh_nan64();
      else if (reducer == XH_RED_MEAN) r = s[i] / (double)n[i];
      else r = ext[i];
      out[o + i] = r;
      if (valid_out) valid_out[o + i] = val[i];
    }
  }
}

// ---- two-field ranges (elemwise.hip k_range_reduce in float64) -------------------------------------------------------
// mode 0: reducer of (high - low)  1: mean |diff(high - low)| (the value of day t is attributed to t; the first day of a
// period differences against the last day of the one before, day 0 of the series has none)  2: max(high) - min(low)
template <int VEC, int MODE, typename TL, typename TH>
__global__ void __launch_bounds__(XH_BLOCK)
k_range_reduce_f64(const TL* __restrict__ lo, const TH* __restrict__ hi, int64_t C, int64_t st_lo, int64_t st_hi, int reducer, const int64_t* __restrict__ seg_off, int P, double* __restrict__ out,
                   int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const bool want_min = reducer == XH_RED_MIN;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
    double s[VEC], e1[VEC], e2[VEC], prev[VEC];
    int n[VEC], n2[VEC], val[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      s[i] = 0.0; e1[i] = 0.0; e2[i] = 0.0; n[i] = 0; n2[i] = 0; val[i] = 0;
      prev[i] = xh_nan64();
    }
    if (MODE == 1 && t0 > 0) {
      const VR<TL, VEC> a = ldv<VEC>(lo + (t0 - 1) * st_lo + c);
      const VR<TH, VEC> b = ldv<VEC>(hi + (t0 - 1) * st_hi + c);
#pragma unroll
      for (int i = 0; i < VEC; ++i) prev[i] = (double)b.v[i] - (double)a.v[i];
    }
    march2<VEC>(lo + c, st_lo, hi + c, st_hi, t0, t1, [&](int64_t, const VR<TL, VEC>& a, const VR<TH, VEC>& b) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double l = (double)a.v[i], h = (double)b.v[i];
        val[i] += (l == l && h == h) ? 1 : 0;
        if (MODE == 2) {  // max(high) and min(low), each over its own valid days
          e1[i] = (h == h && (n[i] == 0 || h > e1[i])) ? h : e1[i];
          n[i] += h == h ? 1 : 0;
          e2[i] = (l == l && (n2[i] == 0 || l < e2[i])) ? l : e2[i];
          n2[i] += l == l ? 1 : 0;
        } else {
          const double d = h - l;
          double v = d;
          if (MODE == 1) {
            v = fabs(d - prev[i]);
            prev[i] = d;
          }
          const bool ok = v == v;
          s[i] = ok ? s[i] + v : s[i];
          e1[i] = (ok && (n[i] == 0 || (want_min ? v < e1[i] : v > e1[i]))) ? v : e1[i];
          n[i] += ok ? 1 : 0;
        }
      }
    });
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double r;
      if (MODE == 2) r = (n[i] == 0 || n2[i] == 0) ? xh_nan64() : e1[i] - e2[i];
      else if (MODE == 1 || reducer == XH_RED_MEAN) r = n[i] == 0 ? xh_nan64() : s[i] / (double)n[i];
      else if (reducer == XH_RED_SUM) r = s[i];
      else r = n[i] == 0 ? xh_nan64() : e1[i];
      out[o + i] = r;
      if (valid_out) valid_out[o + i] = val[i];
    }
  }
}

// ---- domain_count (gen:364-392) and bivariate_count_occurrences (gen:1002-1073) in float64 ---------------------------
template <int VEC>
__global__ void __launch_bounds__(XH_BLOCK)
k_domain_count_f64(const double* __restrict__ x, int64_t C, int64_t st, int op1, double thr1, int op2, double thr2, int combine,
                   const int64_t* __restrict__ seg_off, int P, int32_t* __restrict__ count_out, int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const Cmp64 m1 = cmp_masks(op1), m2 = cmp_masks(op2);
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
    int cnt[VEC], val[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) cnt[i] = 0, val[i] = 0;
    march<VEC>(x + c, st, t0, t1, [&](int64_t, const VR<double, VEC>& xv) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const bool a = cmpm(xv.v[i], m1, thr1), b = cmpm(xv.v[i], m2, thr2);
        cnt[i] += ((combine == 1) ? (a && b) : (a || b)) ? 1 : 0;
        val[i] += (xv.v[i] == xv.v[i]) ? 1 : 0;
      }
    });
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      count_out[o + i] = cnt[i];
      if (valid_out) valid_out[o + i] = val[i];
    }
  }
}

// thr1 / thr2 arrive rounded to float32 for a float32 side (the launcher): the widened float32 value compared in float64
// against the widened float32 threshold is the float32 compare
template <int VEC, typename TA, typename TB>
__global__ void __launch_bounds__(XH_BLOCK)
k_bivariate_count_f64(const TA* __restrict__ x1, const TB* __restrict__ x2, int64_t C, int64_t st1, int64_t st2, int op1,
                      double thr1, int op2, double thr2, int combine, const int64_t* __restrict__ seg_off, int P,
                      int32_t* __restrict__ count_out, int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const Cmp64 m1 = cmp_masks(op1), m2 = cmp_masks(op2);
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
    int cnt[VEC], val[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) cnt[i] = 0, val[i] = 0;
    march2<VEC>(x1 + c, st1, x2 + c, st2, t0, t1, [&](int64_t, const VR<TA, VEC>& a, const VR<TB, VEC>& b) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double u = (double)a.v[i], w = (double)b.v[i];
        const bool ca = cmpm(u, m1, thr1), cb = cmpm(w, m2, thr2);
        cnt[i] += ((combine == 1) ? (ca && cb) : (ca || cb)) ? 1 : 0;
        val[i] += (u == u && w == w) ? 1 : 0;
      }
    });
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      count_out[o + i] = cnt[i];
      if (valid_out) valid_out[o + i] = val[i];
    }
  }
}

// ---- rolling window statistics (reduce.hip k_rolling_reduce / window.hip k_rolling_ring in float64) --------------------
// Window of step t: [t - left, t + right].  min_periods = window (xarray's default): an incomplete window or a NaN in it
// gives NaN; count is the number of valid values of the (possibly partial) window.  Sum and mean add the window rows
// first to last (oracle.generic.rolling), std / var are numpy's two passes (mean, then the squared deviations added in the
// same order), population form.
constexpr int WMAX = 8;

template <int RED>
__device__ __forceinline__ double win_finish(double s, double e, int n, bool nan, int w) {
  if (RED == XH_RED_COUNT) return (double)n;
  double r;
  if (RED == XH_RED_MIN || RED == XH_RED_MAX) r = e;
  else if (RED == XH_RED_MEAN) r = s / (double)w;
  else r = s;
  return nan ? xh_nan64() : r;
}

// statistic of a ring of exactly W rows (slot 0 = oldest): a compile-time window, so no slot is walked under a predicate
template <int RED, int W>
__device__ __forceinline__ double ring_stat(const double (&r)[W]) {
  double s = 0.0, e = 0.0;
  bool nan = false;
  int n = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const double v = r[k];
    nan |= v != v;
    n += v == v ? 1 : 0;
    if (RED == XH_RED_MIN) e = (k == 0 || v < e) ? v : e;
    else if (RED == XH_RED_MAX) e = (k == 0 || v > e) ? v : e;
    else s = k == 0 ? v : s + v;
  }
  if (RED == XH_RED_STD || RED == XH_RED_VAR) {
    const double m = s / (double)W;
    double s2 = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double d = r[k] - m;
      s2 = k == 0 ? d * d : s2 + d * d;
    }
    const double v = s2 / (double)W;
    return nan ? xh_nan64() : (RED == XH_RED_VAR ? v : sqrt(v));
  }
  return win_finish<RED>(s, e, n, nan, W);
}

// the same over rows [a, a + w) read from memory (windows longer than the ring); rows outside [0, T) count as NaN
template <int RED>
__device__ __forceinline__ double mem_stat(const double* __restrict__ p, int64_t st, int64_t T, int64_t a, int w) {
  double s = 0.0, e = 0.0;
  bool nan = false;
  int n = 0;
  const int64_t k0 = a < 0 ? 0 : a, k1 = a + w > T ? T : a + w;
  if (RED != XH_RED_COUNT && (k0 != a || k1 != a + w)) return xh_nan64();
#pragma unroll 8
  for (int64_t k = k0; k < k1; ++k) {
    const double v = p[k * st];
    nan |= v != v;
    n += v == v ? 1 : 0;
    if (RED == XH_RED_MIN) e = (k == k0 || v < e) ? v : e;
    else if (RED == XH_RED_MAX) e = (k == k0 || v > e) ? v : e;
    else s = k == k0 ? v : s + v;
  }
  if (RED == XH_RED_STD || RED == XH_RED_VAR) {
    const double m = s / (double)w;
    double s2 = 0.0;
#pragma unroll 8
    for (int64_t k = k0; k < k1; ++k) {
      const double d = p[k * st] - m;
      s2 = k == k0 ? d * d : s2 + d * d;
    }
    const double v = s2 / (double)w;
    return nan ? xh_nan64() : (RED == XH_RED_VAR ? v : sqrt(v));
  }
  return win_finish<RED>(s, e, n, nan, w);
}

template <int VEC>
__device__ __forceinline__ void store2(double* p, const double (&r)[VEC]) {
  if constexpr (VEC == 2) *reinterpret_cast<double2*>(p) = make_double2(r[0], r[1]);
  else p[0] = r[0];
}

// W in 1 .. 8: the window is a compile-time ring of W rows, every row read once and shifted through it; the chunk's halo
// rows are marched first without output, then every row of the main march completes one window and stores it (no branch
// around the store, so the double-buffered batch waits once).  W == 0: windows longer than the ring, one cell per lane,
// each window read from memory (its rows were read by the previous steps: L1 / L2 hits).  The time axis is cut into
// chunks over blockIdx.y.
template <int VEC, int RED, int W>
__global__ void __launch_bounds__(XH_BLOCK)
k_rolling_reduce_f64(const double* __restrict__ x, int64_t T, int64_t C, int64_t st, int w, int left, int right,
                     double* __restrict__ out, int64_t out_st) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const int64_t chunk = cdiv64(T, (int64_t)gridDim.y);
  const int64_t ta = (int64_t)blockIdx.y * chunk;
  const int64_t tb = ta + chunk > T ? T : ta + chunk;
  if (ta >= tb) return;
  if constexpr (W == 0) {
    for (int64_t t = ta; t < tb; ++t) {
      double r[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) r[i] = mem_stat<RED>(x + c + i, st, T, t - left, w);
      store2<VEC>(out + t * out_st + c, r);
    }
  } else {
    double ring[VEC][W];
#pragma unroll
    for (int i = 0; i < VEC; ++i)
#pragma unroll
      for (int k = 0; k < W; ++k) ring[i][k] = xh_nan64();
    auto push = [&](const VR<double, VEC>& xv) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
#pragma unroll
        for (int k = 0; k < W - 1; ++k) ring[i][k] = ring[i][k + 1];
        ring[i][W - 1] = xv.v[i];
      }
    };
    // the window of t = tp - right is complete once row tp is in the ring
    auto emit = [&](int64_t tp) {
      const int64_t t = tp - right;
      const bool whole = (t - left >= 0) && (t + right < T);
      double r[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double s = ring_stat<RED, W>(ring[i]);
        r[i] = (RED == XH_RED_COUNT || whole) ? s : xh_nan64();
      }
      store2<VEC>(out + t * out_st + c, r);
    };
    const int64_t r0 = ta - left < 0 ? 0 : ta - left;
    const int64_t r1 = tb + right > T ? T : tb + right;
    const int64_t rm = ta + right < r1 ? ta + right : r1;  // rows before rm only fill the ring
    march<VEC>(x + c, st, r0, rm, [&](int64_t, const VR<double, VEC>& xv) { push(xv); });
    march<VEC>(x + c, st, rm, r1, [&](int64_t tp, const VR<double, VEC>& xv) {
      push(xv);
      emit(tp);
    });
    VR<double, VEC> nanrow;  // windows that reach past the end of the series
#pragma unroll
    for (int i = 0; i < VEC; ++i) nanrow.v[i] = xh_nan64();
    for (int64_t tp = r1; tp < tb + right; ++tp) {
      push(nanrow);
      if (tp - right >= ta) emit(tp);
    }
  }
}

}  // namespace

extern "C" {

int xh_thresholded_reduce_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int op, double thr,
                              int mode, int reducer, const int64_t* seg_off, int P, double* out, int32_t* valid_out) {
  int rc = xh_check_field("xh_thresholded_reduce_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(out, XH_ERR_ARG, "xh_thresholded_reduce_f64: out is NULL");
  XH_REQUIRE(mode >= 0 && mode <= 2, XH_ERR_ARG, "xh_thresholded_reduce_f64: mode must be 0, 1 or 2");
  XH_REQUIRE(op >= XH_OP_GT && op <= XH_OP_NE, XH_ERR_OP, "Operation `%d` not recognized.", op);
  XH_REQUIRE(mode != 0 || (reducer >= XH_RED_SUM && reducer <= XH_RED_MAX), XH_ERR_OP,
             "xh_thresholded_reduce_f64: reducer %d not recognized", reducer);
  XH_REQUIRE(mode == 0 || op <= XH_OP_LE, XH_ERR_OP, "Condition not supported: '%d'.", op);
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_thresholded_reduce_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (C == 0) return XH_OK;
  const int vec = xh_pick_vec64(x, C, st);
  const dim3 grid = xh_period_grid(C, vec, P);
  xh_pick<0, 1, 2>(mode, [&](auto M) {
    xh_pick<2, 1>(vec, [&](auto V) {
      hipLaunchKernelGGL((k_thresholded_reduce_f64<decltype(V)::value, decltype(M)::value>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C,
                         st, op, thr, reducer, d_seg, P, out, valid_out);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_range_reduce_f64(xh_ctx* ctx, const void* low, const void* high, int64_t T, int64_t C, int64_t st_low, int64_t st_high,
                        int dtypes, int mode, int reducer, const int64_t* seg_off, int P, double* out, int32_t* valid_out) {
  XH_REQUIRE(out, XH_ERR_ARG, "xh_range_reduce_f64: NULL argument");
  int rc = xh_check_fields2("xh_range_reduce_f64", ctx, low, high, T, C, st_low, st_high);
  if (rc) return rc;
  XH_REQUIRE(dtypes >= 0 && dtypes <= 2, XH_ERR_ARG,
             "xh_range_reduce_f64: dtypes must be 0 (low, high float64), 1 (low float32) or 2 (high float32)");
  XH_REQUIRE(mode >= 0 && mode <= 2, XH_ERR_ARG, "xh_range_reduce_f64: mode must be 0 (range), 1 (interday) or 2 (extreme)");
  XH_REQUIRE(mode != 0 || (reducer >= XH_RED_SUM && reducer <= XH_RED_MAX), XH_ERR_OP,
             "xh_range_reduce_f64: reducer %d not recognized", reducer);
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_range_reduce_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (C == 0) return XH_OK;
  const size_t el = dtypes == 1 ? 4 : 8, eh = dtypes == 2 ? 4 : 8;
  const int vec = (xh_pick_vec64(low, C, st_low, el) == 2 && xh_pick_vec64(high, C, st_high, eh) == 2) ? 2 : 1;
  const dim3 grid = xh_period_grid(C, vec, P);
  xh_pick<0, 1, 2>(dtypes, [&](auto DT) {  // 1: low is float32, 2: high is
    using TL = std::conditional_t<decltype(DT)::value == 1, float, double>;
    using TH = std::conditional_t<decltype(DT)::value == 2, float, double>;
    xh_pick<2, 1>(vec, [&](auto V) {
      xh_pick<0, 1, 2>(mode, [&](auto M) {
        hipLaunchKernelGGL((k_range_reduce_f64<decltype(V)::value, decltype(M)::value, TL, TH>), grid, dim3(XH_BLOCK), 0, ctx->stream,
                           (const TL*)low, (const TH*)high, C, st_low, st_high, reducer, d_seg, P, out, valid_out);
      });
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_domain_count_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int op1, double thr1, int op2,
                        double thr2, int combine, const int64_t* seg_off, int P, int32_t* count_out, int32_t* valid_out) {
  int rc = xh_check_field("xh_domain_count_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(count_out, XH_ERR_ARG, "xh_domain_count_f64: count_out is NULL");
  XH_REQUIRE(op1 >= XH_OP_GT && op1 <= XH_OP_NE && op2 >= XH_OP_GT && op2 <= XH_OP_NE, XH_ERR_OP,
             "Operation `%d/%d` not recognized.", op1, op2);
  XH_REQUIRE(combine == 1 || combine == 2, XH_ERR_ARG, "xh_domain_count_f64: combine must be 1 (and) or 2 (or)");
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_domain_count_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (C == 0) return XH_OK;
  const int vec = xh_pick_vec64(x, C, st);
  const dim3 grid = xh_period_grid(C, vec, P);
  if (vec == 2)
    hipLaunchKernelGGL((k_domain_count_f64<2>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C, st, op1, thr1, op2, thr2, combine, d_seg,
                       P, count_out, valid_out);
  else
    hipLaunchKernelGGL((k_domain_count_f64<1>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C, st, op1, thr1, op2, thr2, combine, d_seg,
                       P, count_out, valid_out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_bivariate_count_f64(xh_ctx* ctx, const void* x1, const void* x2, int64_t T, int64_t C, int64_t st1, int64_t st2, int dtypes,
                           int op1, double thr1, int op2, double thr2, int combine, const int64_t* seg_off, int P,
                           int32_t* count_out, int32_t* valid_out) {
  XH_REQUIRE(count_out, XH_ERR_ARG, "xh_bivariate_count_f64: NULL argument");
  int rc = xh_check_fields2("xh_bivariate_count_f64", ctx, x1, x2, T, C, st1, st2);
  if (rc) return rc;
  XH_REQUIRE(dtypes >= 0 && dtypes <= 2, XH_ERR_ARG,
             "xh_bivariate_count_f64: dtypes must be 0 (x1, x2 float64), 1 (x1 float32) or 2 (x2 float32)");
  XH_REQUIRE(op1 >= XH_OP_GT && op1 <= XH_OP_NE && op2 >= XH_OP_GT && op2 <= XH_OP_NE, XH_ERR_OP,
             "Operation `%d/%d` not recognized.", op1, op2);
  XH_REQUIRE(combine == 1 || combine == 2, XH_ERR_ARG, "xh_bivariate_count_f64: combine must be 1 (all) or 2 (any)");
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_bivariate_count_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (C == 0) return XH_OK;
  // a float32 side compares in float32 against the float32-rounded threshold (numpy: a python float is a weak scalar)
  const double t1 = dtypes == 1 ? (double)(float)thr1 : thr1, t2 = dtypes == 2 ? (double)(float)thr2 : thr2;
  const size_t e1 = dtypes == 1 ? 4 : 8, e2 = dtypes == 2 ? 4 : 8;
  const int vec = (xh_pick_vec64(x1, C, st1, e1) == 2 && xh_pick_vec64(x2, C, st2, e2) == 2) ? 2 : 1;
  const dim3 grid = xh_period_grid(C, vec, P);
  xh_pick<0, 1, 2>(dtypes, [&](auto DT) {  // 1: x1 is float32, 2: x2 is
    using TA = std::conditional_t<decltype(DT)::value == 1, float, double>;
    using TB = std::conditional_t<decltype(DT)::value == 2, float, double>;
    xh_pick<2, 1>(vec, [&](auto V) {
      hipLaunchKernelGGL((k_bivariate_count_f64<decltype(V)::value, TA, TB>), grid, dim3(XH_BLOCK), 0, ctx->stream, (const TA*)x1,
                         (const TB*)x2, C, st1, st2, op1, t1, op2, t2, combine, d_seg, P, count_out, valid_out);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_rolling_reduce_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int window, int center,
                          int reducer, double* out, int64_t out_st) {
  int rc = xh_check_field("xh_rolling_reduce_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(out, XH_ERR_ARG, "xh_rolling_reduce_f64: out NULL");
  rc = xh_check_rows("xh_rolling_reduce_f64", out_st, C, "out_st");
  if (rc) return rc;
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "xh_rolling_reduce_f64: window must be >= 1");
  XH_REQUIRE(reducer >= XH_RED_SUM && reducer <= XH_RED_COUNT, XH_ERR_OP, "xh_rolling_reduce_f64: reducer %d not recognized", reducer);
  if (T == 0 || C == 0) return XH_OK;
  // xarray: center=True -> window covers [t - w//2, t + w - 1 - w//2]; else trailing [t - w + 1, t]
  const int left = center ? window / 2 : window - 1;
  const int right = window - 1 - left;
  const bool ring = window <= WMAX;
  const int vec = (ring && xh_pick_vec64(x, C, st) == 2 && xh_pick_vec64(out, C, out_st) == 2) ? 2 : 1;
  const int64_t cblocks = cdiv64(cdiv64(C, vec), XH_BLOCK);
  int64_t gy = cdiv64((int64_t)ctx->num_cu * 8, cblocks);
  if (gy < 1) gy = 1;
  if (gy > cdiv64(T, 64)) gy = cdiv64(T, 64);  // chunks of >= 64 rows: the halo stays a small share
  if (gy > 1024) gy = 1024;
  const dim3 grid((unsigned)cblocks, (unsigned)gy);
  // (compile-time window, cells per lane) as one code: the windows of the register ring with two cells or one, else the
  // re-reading kernel with one
  const int wv = ring ? window * 10 + vec : 1;
  xh_pick<XH_RED_SUM, XH_RED_MEAN, XH_RED_MIN, XH_RED_MAX, XH_RED_STD, XH_RED_VAR, XH_RED_COUNT>(reducer, [&](auto R) {
    xh_pick<12, 11, 22, 21, 32, 31, 42, 41, 52, 51, 62, 61, 72, 71, 82, 81, 1>(wv, [&](auto WV) {
      hipLaunchKernelGGL((k_rolling_reduce_f64<decltype(WV)::value % 10, decltype(R)::value, decltype(WV)::value / 10>), grid,
                         dim3(XH_BLOCK), 0, ctx->stream, x, T, C, st, window, left, right, out, out_st);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

}  // extern "C"
