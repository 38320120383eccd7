// partition.hip — the ensemble uncertainty-partitioning unit (include/units/xclim_hip_partition.h): xclim.ensembles._partitioning
// and ensemble_mean_std_max_min of xclim.ensembles._base.
//
// xh_partition_smooth: one lane per (series, cell); neighbouring lanes are neighbouring cells, so every row load and store is
// coalesced.  A lane walks its series twice.  The first walk adds the Gram matrix and the right-hand side of the least-squares
// fit in the orthonormal basis q (read with wave-uniform indices: scalar loads, no LDS) over the years that are not NaN and
// solves the (deg + 1) x (deg + 1) system by Cholesky in registers.  The second walk evaluates the fit, writes it and keeps the
// last `window` residuals in a register file that shifts by one per row (static indices only: no scratch, no LDS), from which
// the centred rolling mean or variance of each complete window is written.
// xh_partition_components: one lane per (row, cell); the member axes are folded by loops whose indices are wave-uniform, every
// sum in index order.  No traffic between lanes anywhere in this unit.
#include "../../include/units/xclim_hip_partition.h"
#include "hostargs.h"

namespace {

constexpr int PT_BLOCK = 128;

__device__ __forceinline__ double pt_nan() { return __builtin_nan(""); }

struct SmoothArgs {
  const void* y;
  const void* sm_in;
  const double* q;  // device copy of the host basis
  int64_t C, ld, sn, ld_out, sn_out, ld_nc;
  int T, base_kind, b0, b1;
  double* sm;
  double* roll;
  int32_t* n_valid;
  uint8_t* status;
  uint8_t* flag;
};

// The Cholesky solve of the NP x NP system G a = b, G packed by rows of its lower triangle (entry (i, j <= i) at i (i + 1) / 2 + j).
// Returns false when a pivot is not above thr.
template <int NP>
__device__ __forceinline__ bool chol_solve(const double (&G)[NP * (NP + 1) / 2], const double (&b)[NP], double thr, double (&a)[NP]) {
  double L[NP * (NP + 1) / 2];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    double s = G[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
    ok = ok && (s > thr);
    const double d = sqrt(s);
    L[j * (j + 1) / 2 + j] = d;
#pragma unroll
    for (int i = j + 1; i < NP; ++i) {
      double u = G[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) u -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      L[i * (i + 1) / 2 + j] = u / d;
    }
  }
  double z[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    double u = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) u -= L[i * (i + 1) / 2 + k] * z[k];
    z[i] = u / L[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; --i) {
    double u = z[i];
#pragma unroll
    for (int k = i + 1; k < NP; ++k) u -= L[k * (k + 1) / 2 + i] * a[k];
    a[i] = u / L[i * (i + 1) / 2 + i];
  }
  return ok;
}

// NP = deg + 1 basis columns (NP == 0: sm_in is given, nothing is fitted); W = 10: rolling mean, W = 11: rolling variance
template <typename E, int NP, int W>
__global__ void __launch_bounds__(PT_BLOCK) k_partition_smooth(SmoothArgs a) {
  const int64_t c = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t n = blockIdx.y;
  const int T = a.T;
  const E* y = a.y ? reinterpret_cast<const E*>(a.y) + n * a.sn + c : nullptr;
  const E* given = a.sm_in ? reinterpret_cast<const E*>(a.sm_in) + n * a.sn + c : nullptr;
  constexpr int NC = NP > 0 ? NP : 1;
  double coef[NC];
  int nv = 0;
  int status = XH_PT_FITTED;
  bool good = true;
  if constexpr (NP > 0) {
    double G[NP * (NP + 1) / 2], b[NP];
#pragma unroll
    for (int k = 0; k < NP * (NP + 1) / 2; ++k) G[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) b[k] = 0.0;
    for (int t = 0; t < T; ++t) {
      const double v = (double)y[(int64_t)t * a.ld];
      if (v != v) continue;
      ++nv;
      double qt[NP];
#pragma unroll
      for (int k = 0; k < NP; ++k) qt[k] = a.q[t * NP + k];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        b[i] += qt[i] * v;
#pragma unroll
        for (int j = 0; j <= i; ++j) G[i * (i + 1) / 2 + j] += qt[i] * qt[j];
      }
    }
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < NP; ++k) dmax = fmax(dmax, G[k * (k + 1) / 2 + k]);
    good = chol_solve<NP>(G, b, (double)T * 0x1p-52 * dmax, coef) && nv >= NP;
    if (nv == 0) {
      status = XH_PT_ALLNAN;
    } else if (!good) {
      status = XH_PT_ILLPOSED;
      if (a.flag) *a.flag = 1;
    }
  }
  auto fitted = [&](int t) {
    if constexpr (NP > 0) {
      double f = 0.0;
#pragma unroll
      for (int k = 0; k < NP; ++k) f += coef[k] * a.q[t * NP + k];
      return good ? f : pt_nan();
    } else {
      return (double)given[(int64_t)t * a.ld];
    }
  };
  // the smoothed value of a row: the fit where y has a value, the given sm as it is
  auto smoothed = [&](int t, double v) {
    if constexpr (NP > 0) return v == v ? fitted(t) : pt_nan();
    return fitted(t);
  };
  double ref = 0.0;
  if (a.base_kind != XH_PT_BASE_NONE) {
    double s = 0.0;
    int cnt = 0;
    for (int t = a.b0; t < a.b1; ++t) {
      const double v = NP > 0 ? (double)y[(int64_t)t * a.ld] : 0.0;
      const double f = smoothed(t, v);
      if (f == f) {
        s += f;
        ++cnt;
      }
    }
    ref = cnt > 0 ? s / (double)cnt : pt_nan();
  }
  double w[W];
#pragma unroll
  for (int k = 0; k < W; ++k) w[k] = pt_nan();
  constexpr int AHEAD = (W - 1) / 2;  // the rows of a window after its centre
  double* sm = a.sm ? a.sm + n * a.sn_out + c : nullptr;
  double* roll = a.roll ? a.roll + n * a.sn_out + c : nullptr;
  for (int t = 0; t < T; ++t) {
    const double v = y ? (double)y[(int64_t)t * a.ld] : pt_nan();
    const double f = smoothed(t, v);
    if (NP == 0 && f == f) ++nv;
    if (sm) sm[(int64_t)t * a.ld_out] = a.base_kind == XH_PT_BASE_SUB ? f - ref : (a.base_kind == XH_PT_BASE_DIV ? f / ref : f);
    if (roll) {
#pragma unroll
      for (int k = 0; k + 1 < W; ++k) w[k] = w[k + 1];
      w[W - 1] = v - f;
      const int i = t - AHEAD;
      if (i >= 0) {
        double r = pt_nan();
        if (t >= W - 1) {  // a NaN residual makes the sums NaN: min_periods = window
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < W; ++k) s += w[k];
          const double m = s / (double)W;
          if (W == 10) {
            r = m;
          } else {
            double q2 = 0.0;
#pragma unroll
            for (int k = 0; k < W; ++k) q2 += (w[k] - m) * (w[k] - m);
            r = q2 / (double)W;
          }
        }
        roll[(int64_t)i * a.ld_out] = r;
      }
    }
  }
  if (roll)
    for (int i = T - AHEAD > 0 ? T - AHEAD : 0; i < T; ++i) roll[(int64_t)i * a.ld_out] = pt_nan();
  if (a.n_valid) a.n_valid[n * a.ld_nc + c] = nv;
  if (a.status) a.status[n * a.ld_nc + c] = (uint8_t)status;
}

struct CompArgs {
  const double* sm;
  const double* roll;
  const double* w;    // device copy of the host weights, or NULL
  const double* hsv;  // the HS variability of every cell (the pre-pass), or NULL
  int64_t C, ld, sn, ld_out;
  int T, K, N, w_axis, variab, t0;
  int A[XH_PT_MAX_AXES], S[XH_PT_MAX_AXES], order[XH_PT_MAX_AXES];
  int comps[XH_PT_MAX_COMP][3];
  double* out;
  double* g;
};

// member j of the pooled other axes of axis ax, at index 0 of ax
__device__ __forceinline__ int pooled(const CompArgs& a, int ax, int j) {
  const int s = a.S[ax];
  return (j / s) * (a.A[ax] * s) + (j % s);
}

// the weight of member n under the user's weights
__device__ __forceinline__ double user_w(const CompArgs& a, int n) { return a.w[(n / a.S[a.w_axis]) % a.A[a.w_axis]]; }

__device__ __forceinline__ double var_then_mean(const CompArgs& a, const double* x, int ax, int weight) {
  const int len = a.A[ax], s = a.S[ax], J = a.N / len;
  double num = 0.0, den = 0.0;
  for (int j = 0; j < J; ++j) {
    const double* p = x + (int64_t)pooled(a, ax, j) * a.sn;
    double sx = 0.0, sw = 0.0;
    int cnt = 0;
    for (int i = 0; i < len; ++i) {
      const double v = p[(int64_t)i * s * a.sn];
      if (v != v) continue;
      const double wi = weight == XH_PT_W_USER ? a.w[i] : 1.0;
      sx += wi * v;
      sw += wi;
      ++cnt;
    }
    if (sw == 0.0) continue;
    const double m = sx / sw;
    double q2 = 0.0;
    for (int i = 0; i < len; ++i) {
      const double v = p[(int64_t)i * s * a.sn];
      if (v != v) continue;
      const double wi = weight == XH_PT_W_USER ? a.w[i] : 1.0;
      q2 += wi * ((v - m) * (v - m));
    }
    const double var = q2 / sw;
    if (var != var) continue;
    const double wo = weight == XH_PT_W_COUNT ? (double)cnt : 1.0;
    num += wo * var;
    den += wo;
  }
  return den != 0.0 ? num / den : pt_nan();
}

// the mean of x over the pooled other axes at index i of axis ax
__device__ __forceinline__ double pooled_mean(const CompArgs& a, const double* x, int ax, int i, int weight) {
  const int J = a.N / a.A[ax];
  double sx = 0.0, sw = 0.0;
  for (int j = 0; j < J; ++j) {
    const int n = pooled(a, ax, j) + i * a.S[ax];
    const double v = x[(int64_t)n * a.sn];
    if (v != v) continue;
    const double wj = weight == XH_PT_W_USER ? user_w(a, n) : 1.0;
    sx += wj * v;
    sw += wj;
  }
  return sw != 0.0 ? sx / sw : pt_nan();
}

__device__ __forceinline__ double mean_then_var(const CompArgs& a, const double* x, int ax, int weight) {
  const int len = a.A[ax];
  double s = 0.0;
  int cnt = 0;
  for (int i = 0; i < len; ++i) {
    const double m = pooled_mean(a, x, ax, i, weight);
    if (m == m) {
      s += m;
      ++cnt;
    }
  }
  if (cnt == 0) return pt_nan();
  const double mean = s / (double)cnt;
  double q2 = 0.0;
  for (int i = 0; i < len; ++i) {  // the inner means again: nothing is kept per lane
    const double m = pooled_mean(a, x, ax, i, weight);
    if (m == m) q2 += (m - mean) * (m - mean);
  }
  return q2 / (double)cnt;
}

// mean over order[3] of the mean over order[2] of the mean over order[1] of the mean over order[0]; weighted along w_axis
__device__ __forceinline__ double nested_mean(const CompArgs& a, const double* x) {
  const int o0 = a.order[0], o1 = a.order[1], o2 = a.order[2], o3 = a.order[3];
  const bool has_w = a.w != nullptr;
  double s3 = 0.0, w3 = 0.0;
  for (int i3 = 0; i3 < a.A[o3]; ++i3) {
    double s2 = 0.0, w2 = 0.0;
    for (int i2 = 0; i2 < a.A[o2]; ++i2) {
      double s1 = 0.0, w1 = 0.0;
      for (int i1 = 0; i1 < a.A[o1]; ++i1) {
        double s0 = 0.0, w0 = 0.0;
        const int base = i1 * a.S[o1] + i2 * a.S[o2] + i3 * a.S[o3];
        for (int i0 = 0; i0 < a.A[o0]; ++i0) {
          const double v = x[(int64_t)(base + i0 * a.S[o0]) * a.sn];
          if (v != v) continue;
          const double wi = has_w && o0 == a.w_axis ? a.w[i0] : 1.0;
          s0 += wi * v;
          w0 += wi;
        }
        if (w0 == 0.0) continue;
        const double wi = has_w && o1 == a.w_axis ? a.w[i1] : 1.0;
        s1 += wi * (s0 / w0);
        w1 += wi;
      }
      if (w1 == 0.0) continue;
      const double wi = has_w && o2 == a.w_axis ? a.w[i2] : 1.0;
      s2 += wi * (s1 / w1);
      w2 += wi;
    }
    if (w2 == 0.0) continue;
    const double wi = has_w && o3 == a.w_axis ? a.w[i3] : 1.0;
    s3 += wi * (s2 / w2);
    w3 += wi;
  }
  return w3 != 0.0 ? s3 / w3 : pt_nan();
}

__global__ void __launch_bounds__(PT_BLOCK) k_partition_components(CompArgs a) {
  const int64_t c = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int t = blockIdx.y;
  const double* sm = a.sm + (int64_t)t * a.ld + c;
  double variab;
  if (a.variab == XH_PT_VARIAB_HS) {
    variab = a.hsv[c];
  } else {
    const double* r = a.roll + (int64_t)t * a.ld + c;
    double s = 0.0;
    int cnt = 0;
    for (int n = 0; n < a.N; ++n) {
      const double v = r[(int64_t)n * a.sn];
      if (v == v) {
        s += v;
        ++cnt;
      }
    }
    variab = cnt > 0 ? s / (double)cnt : pt_nan();
  }
  double* out = a.out + (int64_t)t * a.ld_out + c;
  const int64_t plane = (int64_t)a.T * a.ld_out;
  out[0] = variab;
  double total = variab;
  for (int k = 0; k < a.K; ++k) {
    const int ax = a.comps[k][0], weight = a.comps[k][2];
    const double u = a.comps[k][1] == XH_PT_VAR_THEN_MEAN ? var_then_mean(a, sm, ax, weight) : mean_then_var(a, sm, ax, weight);
    out[(k + 1) * plane] = u;
    total += u;
  }
  out[(a.K + 1) * plane] = total;
  if (a.g) a.g[(int64_t)t * a.ld_out + c] = nested_mean(a, sm);
}

// the HS variability: per entry m of w_axis the variance of roll pooled over the other axes and the rows from t0 on, then the
// mean over m weighted by w.  One lane per cell.
__global__ void __launch_bounds__(PT_BLOCK) k_partition_hs_variability(CompArgs a, double* hsv) {
  const int64_t c = (int64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int ax = a.w_axis, J = a.N / a.A[ax];
  double num = 0.0, den = 0.0;
  for (int m = 0; m < a.A[ax]; ++m) {
    double mean = 0.0, q2 = 0.0;
    int cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
      double acc = 0.0;
      for (int j = 0; j < J; ++j) {
        const double* p = a.roll + (int64_t)(pooled(a, ax, j) + m * a.S[ax]) * a.sn + c;
        for (int t = a.t0; t < a.T; ++t) {
          const double v = p[(int64_t)t * a.ld];
          if (v != v) continue;
          if (pass == 0) {
            acc += v;
            ++cnt;
          } else {
            acc += (v - mean) * (v - mean);
          }
        }
      }
      if (cnt == 0) break;
      if (pass == 0) mean = acc / (double)cnt;
      else q2 = acc / (double)cnt;
    }
    if (cnt == 0 || q2 != q2) continue;
    num += a.w[m] * q2;
    den += a.w[m];
  }
  hsv[c] = den != 0.0 ? num / den : pt_nan();
}

struct StatsArgs {
  const void* x;
  const double* w;  // device copy of the host weights, or NULL
  int64_t E, ld, ld_out;
  int R, min_members;
  double* out;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_ensemble_stats(StatsArgs a) {
  const int64_t e = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (e >= a.E) return;
  const TE* x = reinterpret_cast<const TE*>(a.x) + e;
  double sx = 0.0, sw = 0.0, mx = pt_nan(), mn = pt_nan();
  int cnt = 0;
  for (int r = 0; r < a.R; ++r) {
    const double v = (double)x[(int64_t)r * a.ld];
    if (v != v) continue;
    const double wr = a.w ? a.w[r] : 1.0;
    sx += wr * v;
    sw += wr;
    mx = cnt == 0 || v > mx ? v : mx;
    mn = cnt == 0 || v < mn ? v : mn;
    ++cnt;
  }
  double mean = pt_nan(), sd = pt_nan();
  if (sw != 0.0) {
    mean = sx / sw;
    double q2 = 0.0;
    for (int r = 0; r < a.R; ++r) {
      const double v = (double)x[(int64_t)r * a.ld];
      if (v != v) continue;
      const double wr = a.w ? a.w[r] : 1.0;
      q2 += wr * ((v - mean) * (v - mean));
    }
    sd = sqrt(q2 / sw);
  }
  if (cnt < a.min_members) mean = sd = mx = mn = pt_nan();
  a.out[XH_ES_MEAN * a.ld_out + e] = mean;
  a.out[XH_ES_STD * a.ld_out + e] = sd;
  a.out[XH_ES_MAX * a.ld_out + e] = mx;
  a.out[XH_ES_MIN * a.ld_out + e] = mn;
}

template <typename E, int W>
void launch_smooth(int np, dim3 grid, hipStream_t stream, const SmoothArgs& a) {
  xh_pick<0, 1, 2, 3, 4, 5>(np, [&](auto tag) {
    hipLaunchKernelGGL((k_partition_smooth<E, decltype(tag)::value, W>), grid, dim3(PT_BLOCK), 0, stream, a);
  });
}

// the (T, N, C) layout shared by both entry points: rows of series that do not overlap
int check_cube(const char* fn, int64_t T, int64_t N, int64_t C, int64_t ld, int64_t sn, const char* what) {
  XH_REQUIRE(sn >= C && ld >= (N - 1) * sn + C, XH_ERR_LAYOUT, "%s: %s needs stride_n >= C and ld >= (N - 1) stride_n + C, got ld %lld, stride_n %lld", fn,
             what, (long long)ld, (long long)sn);
  XH_REQUIRE(T * ld + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  return XH_OK;
}

}  // namespace

int xh_partition_smooth(xh_ctx* ctx, const void* y, const void* sm_in, int64_t T, int64_t N, int64_t C, int64_t ld, int64_t stride_n,
                        int f64, const double* q, int deg, int window, int stat, int base_kind, int64_t b0, int64_t b1, double* sm,
                        double* roll, int64_t ld_out, int64_t stride_n_out, int32_t* n_valid, uint8_t* status, int64_t ld_nc,
                        uint8_t* flag) {
  const char* fn = "xh_partition_smooth";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(T >= 1 && N >= 1 && N <= 65535 && C >= 0, XH_ERR_ARG, "%s: bad shape (T %lld, N %lld, C %lld)", fn, (long long)T, (long long)N,
             (long long)C);
  XH_REQUIRE(T <= XH_PT_MAX_T, XH_ERR_LIMIT, "%s: at most %d years, got %lld", fn, XH_PT_MAX_T, (long long)T);
  XH_REQUIRE((window == 10 && stat == XH_PT_ROLL_MEAN) || (window == 11 && stat == XH_PT_ROLL_VAR), XH_ERR_ARG,
             "%s: the rolling mean over 10 rows and the rolling variance over 11 rows are served, got window %d, statistic %d", fn, window, stat);
  XH_REQUIRE(sm_in ? (!q && deg == 0) : (q && deg >= 0 && deg <= XH_PT_MAX_DEG), XH_ERR_ARG,
             "%s: a basis of degree 0 .. %d, or sm_in without a basis (deg %d)", fn, XH_PT_MAX_DEG, deg);
  XH_REQUIRE(base_kind >= XH_PT_BASE_NONE && base_kind <= XH_PT_BASE_DIV, XH_ERR_ARG, "%s: unknown baseline kind %d", fn, base_kind);
  XH_REQUIRE(base_kind == XH_PT_BASE_NONE || (0 <= b0 && b0 <= b1 && b1 <= T), XH_ERR_ARG, "%s: baseline rows [%lld, %lld) outside [0, %lld]", fn,
             (long long)b0, (long long)b1, (long long)T);
  XH_REQUIRE(sm || roll, XH_ERR_ARG, "%s: sm and roll are both NULL", fn);
  int rc = check_cube(fn, T, N, C, ld, stride_n, "the field");
  if (!rc) rc = check_cube(fn, T, N, C, ld_out, stride_n_out, "the output");
  if (rc) return rc;
  XH_REQUIRE(ld_nc >= C, XH_ERR_LAYOUT, "%s: ld_nc below C", fn);
  XH_REQUIRE(N * ld_nc + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(y || (sm_in && !roll), XH_ERR_ARG, "%s: y is needed for the fit and for roll", fn);
  SmoothArgs a{};
  a.y = y;
  a.sm_in = sm_in;
  a.C = C;
  a.ld = ld;
  a.sn = stride_n;
  a.ld_out = ld_out;
  a.sn_out = stride_n_out;
  a.ld_nc = ld_nc;
  a.T = (int)T;
  a.base_kind = base_kind;
  a.b0 = (int)b0;
  a.b1 = (int)b1;
  a.sm = sm;
  a.roll = roll;
  a.n_valid = n_valid;
  a.status = status;
  a.flag = flag;
  size_t cur = 0;
  if (q) {
    rc = xh_upload(ctx, &cur, q, (size_t)T * (size_t)(deg + 1), &a.q);
    if (rc) return rc;
  }
  if (flag) XH_CHECK_HIP(hipMemsetAsync(flag, 0, 1, ctx->stream));
  const dim3 grid((unsigned)cdiv64(C, PT_BLOCK), (unsigned)N);
  const int np = sm_in ? 0 : deg + 1;
  xh_by_width(f64, [&](auto w) {
    if (window == 10) launch_smooth<XH_WIDTH(w), 10>(np, grid, ctx->stream, a);
    else launch_smooth<XH_WIDTH(w), 11>(np, grid, ctx->stream, a);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_partition_components(xh_ctx* ctx, const double* sm, const double* roll, int64_t T, const int64_t* dims, int64_t C, int64_t ld,
                            int64_t stride_n, const int32_t* comps, int K, const double* weights, int w_axis, int variab, int64_t t0,
                            const int32_t* g_order, double* out, int64_t ld_out, double* g) {
  const char* fn = "xh_partition_components";
  XH_REQUIRE(ctx && dims && g_order, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 1 && T <= 65535 && C >= 0, XH_ERR_ARG, "%s: bad shape (T %lld, C %lld)", fn, (long long)T, (long long)C);
  XH_REQUIRE(K >= 0 && K <= XH_PT_MAX_COMP && (K == 0 || comps), XH_ERR_ARG, "%s: 0 .. %d components, got %d", fn, XH_PT_MAX_COMP, K);
  int64_t N = 1;
  for (int k = 0; k < XH_PT_MAX_AXES; ++k) {
    XH_REQUIRE(dims[k] >= 1, XH_ERR_ARG, "%s: axis %d has length %lld", fn, k, (long long)dims[k]);
    XH_REQUIRE(dims[k] <= XH_PT_MAX_AXIS, XH_ERR_LIMIT, "%s: at most %d entries per axis, axis %d has %lld", fn, XH_PT_MAX_AXIS, k, (long long)dims[k]);
    N *= dims[k];
  }
  XH_REQUIRE(N <= XH_PT_MAX_MEMBERS, XH_ERR_LIMIT, "%s: at most %d members, got %lld", fn, XH_PT_MAX_MEMBERS, (long long)N);
  XH_REQUIRE(!weights || (w_axis >= 0 && w_axis < XH_PT_MAX_AXES), XH_ERR_ARG, "%s: w_axis %d", fn, w_axis);
  XH_REQUIRE(variab == XH_PT_VARIAB_MEAN_ALL || (variab == XH_PT_VARIAB_HS && weights), XH_ERR_ARG,
             "%s: the variability rule is MEAN_ALL, or HS with weights (got %d)", fn, variab);
  XH_REQUIRE(t0 >= 0 && t0 <= T, XH_ERR_ARG, "%s: t0 %lld outside [0, %lld]", fn, (long long)t0, (long long)T);
  for (int k = 0; k < K; ++k) {
    const int ax = comps[3 * k], rule = comps[3 * k + 1], wt = comps[3 * k + 2];
    XH_REQUIRE(ax >= 0 && ax < XH_PT_MAX_AXES && (rule == XH_PT_VAR_THEN_MEAN || rule == XH_PT_MEAN_THEN_VAR) && wt >= XH_PT_W_NONE &&
                   wt <= XH_PT_W_USER,
               XH_ERR_ARG, "%s: component %d is {%d, %d, %d}", fn, k, ax, rule, wt);
    XH_REQUIRE(wt != XH_PT_W_COUNT || rule == XH_PT_VAR_THEN_MEAN, XH_ERR_ARG, "%s: component %d: count weights go with VAR_THEN_MEAN", fn, k);
    XH_REQUIRE(wt != XH_PT_W_USER || (weights && (rule == XH_PT_VAR_THEN_MEAN) == (ax == w_axis)), XH_ERR_ARG,
               "%s: component %d: user weights need `weights`, along the axis for VAR_THEN_MEAN and along another for MEAN_THEN_VAR", fn, k);
  }
  int seen = 0;
  for (int k = 0; k < XH_PT_MAX_AXES; ++k) {
    XH_REQUIRE(g_order[k] >= 0 && g_order[k] < XH_PT_MAX_AXES, XH_ERR_ARG, "%s: g_order[%d] = %d", fn, k, g_order[k]);
    seen |= 1 << g_order[k];
  }
  XH_REQUIRE(seen == (1 << XH_PT_MAX_AXES) - 1, XH_ERR_ARG, "%s: g_order is not a permutation", fn);
  int rc = check_cube(fn, T, N, C, ld, stride_n, "the field");
  if (rc) return rc;
  XH_REQUIRE(ld_out >= C, XH_ERR_LAYOUT, "%s: ld_out below C", fn);
  XH_REQUIRE((K + 2) * T * ld_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: output too large", fn);
  if (C == 0) return XH_OK;
  XH_REQUIRE(sm && roll && out, XH_ERR_ARG, "%s: NULL argument", fn);
  CompArgs a{};
  a.sm = sm;
  a.roll = roll;
  a.C = C;
  a.ld = ld;
  a.sn = stride_n;
  a.ld_out = ld_out;
  a.T = (int)T;
  a.K = K;
  a.N = (int)N;
  a.w_axis = weights ? w_axis : 0;
  a.variab = variab;
  a.t0 = (int)t0;
  int s = 1;
  for (int k = XH_PT_MAX_AXES - 1; k >= 0; --k) {
    a.A[k] = (int)dims[k];
    a.S[k] = s;
    s *= (int)dims[k];
    a.order[k] = g_order[k];
  }
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < 3; ++j) a.comps[k][j] = comps[3 * k + j];
  a.out = out;
  a.g = g;
  size_t cur = 0;
  if (weights) {
    rc = xh_upload(ctx, &cur, weights, (size_t)dims[w_axis], &a.w);
    if (rc) return rc;
  }
  if (variab == XH_PT_VARIAB_HS) {
    void* hsv = nullptr;
    rc = xh_big_scratch(ctx, sizeof(double) * (size_t)C, &hsv);
    if (rc) return rc;
    a.hsv = (const double*)hsv;
    hipLaunchKernelGGL(k_partition_hs_variability, dim3((unsigned)cdiv64(C, PT_BLOCK)), dim3(PT_BLOCK), 0, ctx->stream, a, (double*)hsv);
    XH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_partition_components, dim3((unsigned)cdiv64(C, PT_BLOCK), (unsigned)T), dim3(PT_BLOCK), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_ensemble_stats(xh_ctx* ctx, const void* x, int64_t R, int64_t E, int64_t ld, int f64, const double* weights, int min_members,
                      double* out, int64_t ld_out) {
  const char* fn = "xh_ensemble_stats";
  const int rc0 = xh_check_pitched(fn, ctx, R, E, ld, XH_ES_NSTAT, ld_out);
  if (rc0) return rc0;
  XH_REQUIRE(R >= 1 && R <= 65535, XH_ERR_ARG, "%s: needs 1 .. 65535 realizations, got %lld", fn, (long long)R);
  if (E == 0) return XH_OK;
  XH_REQUIRE(x && out, XH_ERR_ARG, "%s: NULL argument", fn);
  StatsArgs a{};
  a.x = x;
  a.E = E;
  a.ld = ld;
  a.ld_out = ld_out;
  a.R = (int)R;
  a.min_members = min_members;
  a.out = out;
  size_t cur = 0;
  if (weights) {
    const int rc = xh_upload(ctx, &cur, weights, (size_t)R, &a.w);
    if (rc) return rc;
  }
  xh_by_width(f64, [&](auto w) {
    hipLaunchKernelGGL(k_ensemble_stats<XH_WIDTH(w)>, dim3((unsigned)cdiv64(E, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, a);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
