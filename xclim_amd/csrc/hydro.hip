// hydro.hip — the streamflow and snow-melt indices of indices/_hydrology.py: base_flow_index (:84-89), rb_flashiness_index
// (:125-128), snow_melt_we_max (:392-399), melt_and_precip_max (:429-439), antecedent_precipitation_index (:698-705) and
// sen_slope (:926-944, the arithmetic of pymannkendall.original_test).
//
// The three field kernels have one lane per cell (consecutive lanes on consecutive cells, so a wave reads 64 consecutive
// elements of a row).  k_flow and k_melt have periods along y: a lane walks the rows of its period once, with the few rows
// before and after it that its windows need, and issues the loads of HYDRO_BATCH rows before it uses the first of them (the
// addresses depend on nothing that was loaded).  k_api has tiles of API_TILE rows along y and walks a tile with the
// window - 1 rows before it.  None of them writes a (T, C) intermediate.
//
// Values are widened to float64 on load and all arithmetic is float64 in the reference's order of operations (the build has
// -ffp-contract=off).  ASSUMPTION: a window is added in row order (m7: its seven values, agg: its `window` totals, the API: its
// `window` products), every window from its first term; where xarray runs on bottleneck the reference keeps a running sum,
// which rounds differently, and its `dot` leaves the order to BLAS.
//
// The trailing windows of k_melt and k_api live in LDS, one column per lane (ring[k * XH_BLOCK + lane]): a lane reads and
// writes its own column only, so the ring needs no barrier, and a window of up to XH_HYDRO_MAX_WINDOW days costs no registers.
// k_api also keeps its weights there (one barrier at the start of the kernel).
//
// k_sen_slope: one workgroup of one wave per (season, cell) series.  The series' values and all its pair slopes — each one IEEE
// division, computed once — are stored in LDS; the slopes are sorted there by a bitonic network over the next power of two
// (the tail, and the slopes of pairs with a dropped value, are +inf, which sorts behind every slope kept), and the median is
// read from the sorted array.  The Mann-Kendall score is added up while the slopes are written.
#include "../../include/xclim_hip_hydro.h"
#include "hostargs.h"

namespace {

constexpr int HYDRO_BATCH = 8;
constexpr int API_TILE = 128;
constexpr int SEN_BLOCK = 64;

__device__ __forceinline__ double hydro_inf() { return __longlong_as_double(0x7FF0000000000000LL); }

// ---- xh_flow_period_stats -------------------------------------------------------------------------------------------
struct FlowArgs {
  const void* q;
  const int64_t* seg;  // (P + 1)
  double *bfi_out, *rbi_out, *mean_out, *sum_out;
  int32_t* valid_out;
  int64_t T, C, ld, ld_out;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_flow(FlowArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  const double nan = xh_nan64();
  // w[k] holds q of row i - 3 + k of the WHOLE series once row i is being worked on (NaN outside the series)
  double w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = nan;
  if (r0 < r1) {
#pragma unroll
    for (int k = 1; k < 7; ++k) {
      const int64_t r = r0 - 4 + k;
      if (r >= 0 && r < a.T) w[k] = (double)xh_ld<TE>(a.q, r * a.ld + c);
    }
  }
  double sum = 0.0, dsum = 0.0, m7min = nan;
  int32_t valid = 0;
  for (int64_t i0 = r0; i0 < r1; i0 += HYDRO_BATCH) {
    TE nx[HYDRO_BATCH];
#pragma unroll
    for (int u = 0; u < HYDRO_BATCH; ++u) {
      const int64_t r = i0 + u + 3;
      nx[u] = (TE)nan;
      if (i0 + u < r1 && r < a.T) nx[u] = xh_ld<TE>(a.q, r * a.ld + c);
    }
#pragma unroll
    for (int u = 0; u < HYDRO_BATCH; ++u) {
      if (i0 + u >= r1) break;
#pragma unroll
      for (int k = 0; k < 6; ++k) w[k] = w[k + 1];
      w[6] = (double)nx[u];
      const double x = w[3];
      if (x == x) sum += x, valid += 1;
      const double d = fabs(x - w[2]);  // (_hydrology.py:125; row 0 has no difference: w[2] is NaN there)
      if (d == d) dsum += d;
      const double m7 = ((((((w[0] + w[1]) + w[2]) + w[3]) + w[4]) + w[5]) + w[6]) / 7;  // :84
      if (m7 == m7) m7min = (m7min != m7min || m7 < m7min) ? m7 : m7min;
    }
  }
  const double mean = valid > 0 ? sum / (double)valid : nan;
  const int64_t o = p * a.ld_out + c;
  if (a.bfi_out) a.bfi_out[o] = m7min / mean;  // :88
  if (a.rbi_out) a.rbi_out[o] = dsum / sum;    // :127
  if (a.mean_out) a.mean_out[o] = mean;
  if (a.sum_out) a.sum_out[o] = sum;
  if (a.valid_out) a.valid_out[o] = valid;
}

// ---- xh_melt_period_max ---------------------------------------------------------------------------------------------
struct MeltArgs {
  const void *snw, *pr;
  const int64_t* seg;
  double* out;
  int64_t T, C, ld, ld_out;
  double per_day;
  int window;
};

template <typename TE, bool PR>
__global__ void __launch_bounds__(XH_BLOCK) k_melt(MeltArgs a) {
  extern __shared__ double melt_ring[];  // [window][XH_BLOCK]
  double* ring = melt_ring + threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  const int W = a.window;
  double mx = xh_nan64();
  if (r0 < r1 && r1 > 1) {
    // total[j] exists for j >= 1; agg[i] needs total[i - W + 1 .. i]: the walk starts W - 1 rows before the period
    const int64_t j0 = r0 - W + 1 > 1 ? r0 - W + 1 : 1;
    double prev = (double)xh_ld<TE>(a.snw, (j0 - 1) * a.ld + c);
    int slot = 0, have = 0;  // the next ring slot (the oldest total once the ring is full); totals in the ring
    for (int64_t jb = j0; jb < r1; jb += HYDRO_BATCH) {
      TE s[HYDRO_BATCH], f[HYDRO_BATCH];
#pragma unroll
      for (int u = 0; u < HYDRO_BATCH; ++u) {
        s[u] = f[u] = (TE)0;
        if (jb + u < r1) {
          s[u] = xh_ld<TE>(a.snw, (jb + u) * a.ld + c);
          if (PR) f[u] = xh_ld<TE>(a.pr, (jb + u) * a.ld + c);
        }
      }
#pragma unroll
      for (int u = 0; u < HYDRO_BATCH; ++u) {
        const int64_t j = jb + u;
        if (j >= r1) break;
        const double cur = (double)s[u];
        const double melt = (cur - prev) * -1.0;                         // :392 / :429
        const double total = PR ? (double)f[u] * a.per_day + melt : melt;  // :432
        prev = cur;
        ring[(int64_t)slot * XH_BLOCK] = total;
        slot = slot + 1 == W ? 0 : slot + 1;
        have = have < W ? have + 1 : W;
        if (j >= r0 && have == W) {
          int k = slot;
          double agg = ring[(int64_t)k * XH_BLOCK];
          for (int n = 1; n < W; ++n) {
            k = k + 1 == W ? 0 : k + 1;
            agg += ring[(int64_t)k * XH_BLOCK];
          }
          if (agg == agg) mx = (mx != mx || agg > mx) ? agg : mx;
        }
      }
    }
  }
  a.out[p * a.ld_out + c] = mx;
}

// ---- xh_antecedent_precip -------------------------------------------------------------------------------------------
struct ApiArgs {
  const void* pr;
  const double* weights;  // (window)
  double* out;
  int64_t T, C, ld, ld_out;
  double per_day;
  int window;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_api(ApiArgs a) {
  extern __shared__ double api_ring[];  // [window][XH_BLOCK] | weights[window]
  double* ring = api_ring + threadIdx.x;
  const int W = a.window;
  // the weights go to LDS once per workgroup: read from memory inside the window loop, every term waits for a scalar load
  double* wts = api_ring + (int64_t)W * XH_BLOCK;
  if ((int)threadIdx.x < W) wts[threadIdx.x] = a.weights[threadIdx.x];
  __syncthreads();
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const double nan = xh_nan64();
  for (int64_t t0 = (int64_t)blockIdx.y * API_TILE; t0 < a.T; t0 += (int64_t)gridDim.y * API_TILE) {
    const int64_t t1 = t0 + API_TILE < a.T ? t0 + API_TILE : a.T;
    const int64_t j0 = t0 - W + 1 > 0 ? t0 - W + 1 : 0;
    int slot = 0, have = 0;
    for (int64_t jb = j0; jb < t1; jb += HYDRO_BATCH) {
      TE f[HYDRO_BATCH];
#pragma unroll
      for (int u = 0; u < HYDRO_BATCH; ++u) f[u] = jb + u < t1 ? xh_ld<TE>(a.pr, (jb + u) * a.ld + c) : (TE)0;
#pragma unroll
      for (int u = 0; u < HYDRO_BATCH; ++u) {
        const int64_t j = jb + u;
        if (j >= t1) break;
        ring[(int64_t)slot * XH_BLOCK] = (double)f[u] * a.per_day;  // rate2amount (:698)
        slot = slot + 1 == W ? 0 : slot + 1;
        have = have < W ? have + 1 : W;
        if (j < t0) continue;
        double v = nan;
        if (have == W) {
          int k = slot;
          v = wts[0] * ring[(int64_t)k * XH_BLOCK];
          for (int n = 1; n < W; ++n) {
            k = k + 1 == W ? 0 : k + 1;
            v += wts[n] * ring[(int64_t)k * XH_BLOCK];
          }
        }
        a.out[j * a.ld_out + c] = v;
      }
    }
  }
}

// ---- xh_sen_slope ---------------------------------------------------------------------------------------------------
struct SenArgs {
  const void* x;
  const int64_t* period_of;  // (Y, K)
  double *slope_out, *p_out;
  int32_t* n_out;
  int64_t C, ld, ld_out;
  int Y, K, npad;  // npad: the power of two >= Y (Y - 1) / 2 (>= 1)
};

template <typename TE>
__global__ void __launch_bounds__(SEN_BLOCK) k_sen_slope(SenArgs a) {
  extern __shared__ double sen_lds[];  // vals[Y] | slopes[npad] | part[4][SEN_BLOCK]
  double* vals = sen_lds;
  double* sl = sen_lds + a.Y;
  double* part = sl + a.npad;
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int k = blockIdx.y;
  const int Y = a.Y;
  const double nan = xh_nan64(), inf = hydro_inf();

  int n_part = 0;
  for (int y = lane; y < Y; y += SEN_BLOCK) {
    const int64_t row = a.period_of[(int64_t)y * a.K + k];
    const double v = row >= 0 ? (double)xh_ld<TE>(a.x, row * a.ld + c) : nan;
    vals[y] = v;
    n_part += v == v ? 1 : 0;
  }
  const int pairs = Y * (Y - 1) / 2;
  for (int i = pairs + lane; i < a.npad; i += SEN_BLOCK) sl[i] = inf;
  __syncthreads();

  // the slopes (one division each) and the Mann-Kendall score; the pair (i, j) is slot i (2 Y - i - 1) / 2 + (j - i - 1)
  int s_part = 0, m_part = 0;
  for (int i = 0; i + 1 < Y; ++i) {
    const double xi = vals[i];
    const int base = i * (2 * Y - i - 1) / 2;
    for (int j = i + 1 + lane; j < Y; j += SEN_BLOCK) {
      const double d = vals[j] - xi;
      const double slope = d / (double)(j - i);
      const bool keep = slope == slope;  // NaN exactly when a value of the pair is (or their difference is)
      sl[base + (j - i - 1)] = keep ? slope : inf;
      m_part += keep ? 1 : 0;
      s_part += (d > 0 ? 1 : 0) - (d < 0 ? 1 : 0);
    }
  }
  // groups of equal values: the first member of a group of t adds t (t - 1) (2 t + 5)
  double tie_part = 0.0;
  for (int y = lane; y < Y; y += SEN_BLOCK) {
    const double v = vals[y];
    if (v != v) continue;
    int t = 0;
    bool first = true;
    for (int z = 0; z < Y; ++z) {
      const bool same = vals[z] == v;
      t += same ? 1 : 0;
      first = first && !(same && z < y);
    }
    if (first) tie_part += (double)t * (double)(t - 1) * (double)(2 * t + 5);
  }
  part[lane] = (double)n_part;
  part[SEN_BLOCK + lane] = (double)s_part;
  part[2 * SEN_BLOCK + lane] = (double)m_part;
  part[3 * SEN_BLOCK + lane] = tie_part;
  __syncthreads();

  // bitonic sort of sl[0 .. npad), ascending
  for (int kk = 2; kk <= a.npad; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = lane; i < a.npad; i += SEN_BLOCK) {
        const int o = i ^ jj;
        if (o > i) {
          const double u = sl[i], v = sl[o];
          const bool up = (i & kk) == 0;
          if (up ? u > v : u < v) sl[i] = v, sl[o] = u;
        }
      }
      __syncthreads();
    }
  }

  if (lane == 0) {
    double n = 0.0, s = 0.0, ties = 0.0;
    int m = 0;
#pragma unroll 4  // (unrolled whole, the 256 LDS reads of this loop take 256 VGPRs and the kernel drops to one wave per SIMD)
    for (int t = 0; t < SEN_BLOCK; ++t) {
      n += part[t], s += part[SEN_BLOCK + t], ties += part[3 * SEN_BLOCK + t];
      m += (int)part[2 * SEN_BLOCK + t];
    }
    double slope = nan, pv = nan;
    if (n >= 2) {
      if (m > 0) slope = (m & 1) ? sl[m / 2] : (sl[m / 2 - 1] + sl[m / 2]) / 2;
      const double var = (n * (n - 1) * (2 * n + 5) - ties) / 18;
      const double z = s > 0 ? (s - 1) / sqrt(var) : (s < 0 ? (s + 1) / sqrt(var) : 0.0);
      pv = 2 * (1 - erfc(-fabs(z) / sqrt(2.0)) / 2);
    }
    const int64_t o = (int64_t)k * a.ld_out + c;
    if (a.slope_out) a.slope_out[o] = slope;
    if (a.p_out) a.p_out[o] = pv;
    if (a.n_out) a.n_out[o] = (int32_t)n;
  }
}

// ---- host front end -------------------------------------------------------------------------------------------------
int hydro_window(const char* fn, int window) {
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "%s: window must be at least 1, got %d", fn, window);
  XH_REQUIRE(window <= XH_HYDRO_MAX_WINDOW, XH_ERR_LIMIT, "%s: windows of up to %d rows are served, got %d", fn, XH_HYDRO_MAX_WINDOW,
             window);
  return XH_OK;
}

}  // namespace

int xh_flow_period_stats(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* q, int64_t P, const int64_t* seg,
                         double* bfi_out, double* rbi_out, double* mean_out, double* sum_out, int32_t* valid_out, int64_t ld_out) {
  const char* fn = "xh_flow_period_stats";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (!rc) rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  XH_REQUIRE(q, XH_ERR_ARG, "%s: NULL field", fn);
  XH_REQUIRE(bfi_out || rbi_out || mean_out || sum_out || valid_out, XH_ERR_ARG, "%s: no output requested", fn);
  if (P == 0 || C == 0) return XH_OK;

  FlowArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (rc) return rc;
  a.q = q;
  a.bfi_out = bfi_out, a.rbi_out = rbi_out, a.mean_out = mean_out, a.sum_out = sum_out, a.valid_out = valid_out;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_flow<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_melt_period_max(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* snw, const void* pr, double per_day,
                       int window, int64_t P, const int64_t* seg, double* out, int64_t ld_out) {
  const char* fn = "xh_melt_period_max";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (!rc) rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  XH_REQUIRE(snw && out, XH_ERR_ARG, "%s: NULL argument", fn);
  rc = hydro_window(fn, window);
  if (rc) return rc;
  if (P == 0 || C == 0) return XH_OK;

  MeltArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (rc) return rc;
  a.snw = snw, a.pr = pr, a.out = out;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.per_day = per_day, a.window = window;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P), b(XH_BLOCK);
  const size_t lds = (size_t)window * XH_BLOCK * sizeof(double);
  xh_by_width(f64, [&](auto w) {
    if (pr) hipLaunchKernelGGL((k_melt<XH_WIDTH(w), true>), g, b, lds, ctx->stream, a);
    else hipLaunchKernelGGL((k_melt<XH_WIDTH(w), false>), g, b, lds, ctx->stream, a);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_antecedent_precip(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, double per_day, int window,
                         const double* weights, double* out, int64_t ld_out) {
  const char* fn = "xh_antecedent_precip";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, T, ld_out);
  if (rc) return rc;
  XH_REQUIRE(pr && out && weights, XH_ERR_ARG, "%s: NULL argument", fn);
  rc = hydro_window(fn, window);
  if (rc) return rc;
  if (T == 0 || C == 0) return XH_OK;

  ApiArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, weights, (size_t)window, &a.weights);
  if (rc) return rc;
  a.pr = pr, a.out = out;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.per_day = per_day, a.window = window;
  const int64_t tiles = cdiv64(T, API_TILE);
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(tiles > 65535 ? 65535 : tiles)), b(XH_BLOCK);
  const size_t lds = ((size_t)window * XH_BLOCK + (size_t)window) * sizeof(double);  // (the largest window: 256 bytes over 64 KiB)
  rc = xh_by_width(f64, [&](auto w) { return xh_launch_lds(k_api<XH_WIDTH(w)>, g, b, lds, ctx->stream, a); });
  if (rc) return rc;
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_sen_slope(xh_ctx* ctx, int64_t P, int64_t C, int64_t ld, int f64, const void* x, int64_t Y, int64_t K,
                 const int64_t* period_of, double* slope_out, double* p_out, int32_t* n_out, int64_t ld_out) {
  const char* fn = "xh_sen_slope";
  int rc = xh_check_pitched(fn, ctx, P, C, ld, K, ld_out);
  if (rc) return rc;
  XH_REQUIRE(Y >= 0 && K >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(x && period_of, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(slope_out || p_out, XH_ERR_ARG, "%s: no output requested (slope_out or p_out)", fn);
  XH_REQUIRE(K <= 65535, XH_ERR_LIMIT, "%s: at most 65535 seasons, got %lld", fn, (long long)K);
  XH_REQUIRE(Y <= XH_SEN_MAX_YEARS, XH_ERR_LIMIT, "%s: series of up to %d years are served, got %lld", fn, XH_SEN_MAX_YEARS, (long long)Y);
  XH_REQUIRE(C < ((int64_t)1 << 31), XH_ERR_LIMIT, "%s: too many cells", fn);
  for (int64_t i = 0; i < Y * K; ++i)
    XH_REQUIRE(period_of[i] >= -1 && period_of[i] < P, XH_ERR_ARG, "%s: period_of[%lld] = %lld outside the %lld rows of x", fn,
               (long long)i, (long long)period_of[i], (long long)P);
  if (K == 0 || C == 0) return XH_OK;

  SenArgs a{};
  size_t cur = 0;
  const int64_t none = -1;
  rc = Y > 0 ? xh_upload(ctx, &cur, period_of, (size_t)(Y * K), &a.period_of) : xh_upload(ctx, &cur, &none, 1, &a.period_of);
  if (rc) return rc;
  a.x = x, a.slope_out = slope_out, a.p_out = p_out, a.n_out = n_out;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.Y = (int)Y, a.K = (int)K;
  const int64_t pairs = Y * (Y - 1) / 2;
  a.npad = 1;
  while (a.npad < pairs) a.npad <<= 1;
  const size_t lds = ((size_t)Y + (size_t)a.npad + 4 * SEN_BLOCK) * sizeof(double);
  const dim3 g((unsigned)C, (unsigned)K), b(SEN_BLOCK);
  rc = xh_by_width(f64, [&](auto w) { return xh_launch_lds(k_sen_slope<XH_WIDTH(w)>, g, b, lds, ctx->stream, a); });
  if (rc) return rc;
  XH_LAUNCH_CHECK();
  return XH_OK;
}
