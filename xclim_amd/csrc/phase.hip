// phase.hip — the snow / rain partition of total precipitation by temperature and the period indices on it:
// snowfall_approximation and rain_approximation (indices/converters.py:1088-1373), precip_accumulation / precip_average with a
// phase, liquid_precip_ratio, winter_rain_ratio, high_precip_low_temp, rain_on_frozen_ground_days
// (indices/_multivariate.py:871-1171, :1797-1829) and first_snowfall, last_snowfall, snowfall_frequency, snowfall_intensity
// (indices/_threshold.py:1701-1967).  C ABI and the exact definition of every result: include/xclim_hip_phase.h.
//
// phase_split is the partition of ONE sample, shared by both kernels; the method is a template argument, so a kernel carries
// the arithmetic of its own method only (the tanh of the dai methods does not cost the binary walk a register).
//
// k_phase_period: one lane per (cell, period), cells along x (a wave reads 64 consecutive elements of a row), periods along y.
// The loads of PHASE_BATCH rows of both fields (and the row's season and day of year, one packed int32 that is uniform over the
// workgroup: a scalar load) are issued before the first of them is used, as in agro.hip.  The snow and rain amounts of a day
// live in registers; the prsn field of the reference never exists.  Only rain on frozen ground looks outside the period: its
// counter of frozen rows is warmed on the `window` rows of tas before the period's first row.
//
// k_phase_map: the element-wise form, VEC consecutive cells per lane (16-byte loads where the view allows them), rows
// blockIdx.y, blockIdx.y + gridDim.y, ...; outputs pitched like the inputs.
//
// The auer table and the dai coefficients are read from global memory thread by thread (824 and 768 bytes, cache resident);
// nothing is staged in LDS, so the kernels have no barrier.
#include <vector>

#include "../../include/xclim_hip_phase.h"
#include "hostargs.h"

namespace {

constexpr int PHASE_BATCH = 8;

struct PhaseParams {
  const double* tab;    // auer: K nodes then K values; dai: the coefficient table
  const uint8_t* land;  // (C) or NULL
  double thresh, upper, add_K, sub_C, step;
  int K, clip, land_all;
};

// np.interp on the auer table: the last node at or below x, found from a guess on the regular part and corrected on the table
__device__ __forceinline__ double auer_fraction(const PhaseParams& q, double x) {
  if (x != x) return x;
  const double* nodes = q.tab;
  const double* vals = q.tab + q.K;
  const int K = q.K;
  if (x < nodes[0]) return vals[0];
  if (x >= nodes[K - 1]) return vals[K - 1];
  int j = 0;
  if (K > 3 && x >= nodes[1]) {
    const double g = (x - nodes[1]) / q.step;
    j = g < (double)(K - 3) ? 1 + (int)g : K - 2;
  }
  while (j > 0 && nodes[j] > x) --j;
  while (j + 2 < K && nodes[j + 1] <= x) ++j;
  const double slope = (vals[j + 1] - vals[j]) / (nodes[j + 1] - nodes[j]);
  return slope * (x - nodes[j]) + vals[j];
}

__device__ __forceinline__ double dai_fraction(const PhaseParams& q, double t, int phase, int land, int season) {
  const double* k = q.tab + ((phase * 2 + land) * 4 + season) * 6;
  double f = k[0] * (tanh(k[1] * (t - k[2])) - k[3]) / 100;
  if (q.clip) f = (f - k[4]) / k[5];
  return f < 0 ? 0.0 : (f > 1 ? 1.0 : f);  // clip(0, 1) keeps NaN
}

template <int M>
__device__ __forceinline__ void phase_split(const PhaseParams& q, double pr, double tas, int season, int land, double& snow,
                                            double& rain) {
  if (M == XH_PHASE_BINARY) {
    snow = tas <= q.thresh ? pr : 0.0;
    rain = pr - snow;
  } else if (M == XH_PHASE_GIVEN) {
    snow = tas;
    rain = pr - snow;
  } else if (M == XH_PHASE_BROWN) {
    double f = tas;  // NaN
    if (tas <= q.thresh) f = 1.0;
    else if (tas >= q.upper) f = 0.0;
    else if (tas == tas) f = (0.0 - 1.0) / (q.upper - q.thresh) * (tas - q.thresh) + 1.0;
    snow = pr * f;
    rain = pr - snow;
  } else if (M == XH_PHASE_AUER) {
    snow = pr * auer_fraction(q, (tas + q.add_K) - q.thresh);
    rain = pr - snow;
  } else {
    const double t = tas - q.sub_C;
    snow = pr * dai_fraction(q, t, 0, land, season);
    rain = pr * dai_fraction(q, t, 1, land, season);
  }
}

// ---- xh_precip_phase_period -----------------------------------------------------------------------------------------
struct PeriodArgs {
  PhaseParams q;
  const void *pr, *tas;
  const int64_t* seg;   // (P + 1)
  const int32_t* meta;  // (T): season | doy << 8
  double* out[XH_PHASE_NOUT];
  int64_t C, ld, ld_out;
  double per_day, snow_low, snow_high, snow_thresh, hplt_pr, hplt_tas, rofg_pr, rofg_frz;
  int window;
};

template <typename TE, int M>
__global__ void __launch_bounds__(XH_BLOCK) k_phase_period(PeriodArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  const int land = a.q.land ? (a.q.land[c] != 0) : a.q.land_all;
  const double pd = a.per_day;
  const bool want_rofg = M != XH_PHASE_GIVEN && a.out[XH_PHASE_ROFG_DAYS] != nullptr;

  double s_pr = 0.0, s_solid = 0.0, s_liquid = 0.0, s_over = 0.0;
  int n_pr = 0, n_solid = 0, n_liquid = 0, n_tas = 0, n_days = 0, n_over = 0, n_hplt = 0, n_rofg = 0;
  int first = 0, last = 0;  // days of year; 0 = none
  int frozen = 0;           // rows with !(tas > frz) in a row, ending on the row before the current one
  if (want_rofg) {
    int64_t w0 = r0 - a.window;
    w0 = w0 < 0 ? 0 : w0;
    for (int64_t r = w0; r < r0; ++r) frozen = xh_ldw<TE>(a.tas, r * a.ld + c) > a.rofg_frz ? 0 : frozen + 1;
  }

  for (int64_t rb = r0; rb < r1; rb += PHASE_BATCH) {
    TE x[PHASE_BATCH], t[PHASE_BATCH];  // as loaded: a float32 batch is half the registers, widened at use
    int m[PHASE_BATCH];
#pragma unroll
    for (int u = 0; u < PHASE_BATCH; ++u) {
      const int64_t r = rb + u;
      x[u] = t[u] = (TE)0;
      m[u] = 0;
      if (r < r1) {
        x[u] = xh_ld<TE>(a.pr, r * a.ld + c);
        t[u] = xh_ld<TE>(a.tas, r * a.ld + c);
        m[u] = a.meta[r];
      }
    }
#pragma unroll
    for (int u = 0; u < PHASE_BATCH; ++u) {
      if (rb + u >= r1) break;
      const double prv = (double)x[u], tv = (double)t[u];
      double snow, rain;
      phase_split<M>(a.q, prv, tv, m[u] & 3, land, snow, rain);
      const double am = prv * pd, sm = snow * pd, lm = rain * pd;
      if (am == am) s_pr += am, ++n_pr;
      if (sm == sm) s_solid += sm, ++n_solid;
      if (lm == lm) s_liquid += lm, ++n_liquid;
      n_tas += tv == tv ? 1 : 0;
      n_days += (sm > a.snow_low && sm <= a.snow_high) ? 1 : 0;  // domain_count: compare(>) * compare(<=)
      if (sm >= a.snow_thresh) {
        s_over += sm, ++n_over;
        last = m[u] >> 8;
        first = first ? first : last;
      }
      if (M != XH_PHASE_GIVEN) {
        n_hplt += (prv >= a.hplt_pr && tv < a.hplt_tas) ? 1 : 0;
        if (want_rofg) {
          const bool warm = tv > a.rofg_frz;
          n_rofg += (warm && frozen >= a.window && prv > a.rofg_pr) ? 1 : 0;
          frozen = warm ? 0 : frozen + 1;
        }
      }
    }
  }

  const int64_t o = p * a.ld_out + c;
  const double nan = xh_nan64();
  if (a.out[XH_PHASE_PR_SUM]) a.out[XH_PHASE_PR_SUM][o] = s_pr;
  if (a.out[XH_PHASE_SOLID_SUM]) a.out[XH_PHASE_SOLID_SUM][o] = s_solid;
  if (a.out[XH_PHASE_LIQUID_SUM]) a.out[XH_PHASE_LIQUID_SUM][o] = s_liquid;
  if (a.out[XH_PHASE_PR_N]) a.out[XH_PHASE_PR_N][o] = (double)n_pr;
  if (a.out[XH_PHASE_SOLID_N]) a.out[XH_PHASE_SOLID_N][o] = (double)n_solid;
  if (a.out[XH_PHASE_LIQUID_N]) a.out[XH_PHASE_LIQUID_N][o] = (double)n_liquid;
  if (a.out[XH_PHASE_TAS_N]) a.out[XH_PHASE_TAS_N][o] = (double)n_tas;
  if (a.out[XH_PHASE_SNOW_DAYS]) a.out[XH_PHASE_SNOW_DAYS][o] = (double)n_days;
  if (a.out[XH_PHASE_SNOW_SUM_OVER]) a.out[XH_PHASE_SNOW_SUM_OVER][o] = s_over;
  if (a.out[XH_PHASE_SNOW_N_OVER]) a.out[XH_PHASE_SNOW_N_OVER][o] = (double)n_over;
  if (a.out[XH_PHASE_FIRST_SNOW]) a.out[XH_PHASE_FIRST_SNOW][o] = first ? (double)first : nan;
  if (a.out[XH_PHASE_LAST_SNOW]) a.out[XH_PHASE_LAST_SNOW][o] = last ? (double)last : nan;
  if (a.out[XH_PHASE_HPLT_DAYS]) a.out[XH_PHASE_HPLT_DAYS][o] = (double)n_hplt;
  if (a.out[XH_PHASE_ROFG_DAYS]) a.out[XH_PHASE_ROFG_DAYS][o] = (double)n_rofg;
}

// ---- xh_precip_phase_map --------------------------------------------------------------------------------------------
struct MapArgs {
  PhaseParams q;
  const void *pr, *tas;
  const uint8_t* season;  // (T)
  void *snow, *rain;
  int64_t T, C, ld, ld_out;
};

template <typename T, int N>
struct alignas(sizeof(T) * N) PhaseVec {
  T v[N];
};

// TE: the fields; TO: the outputs (TE for the binary select, double otherwise); VEC cells per lane
template <typename TE, typename TO, int M, int VEC>
__global__ void __launch_bounds__(XH_BLOCK) k_phase_map(MapArgs a) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= a.C) return;  // (C is a multiple of VEC when VEC > 1)
  int land[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) land[k] = a.q.land ? (a.q.land[c + k] != 0) : a.q.land_all;
  for (int64_t r = blockIdx.y; r < a.T; r += gridDim.y) {
    const int season = a.season[r] & 3;
    const PhaseVec<TE, VEC> x = *reinterpret_cast<const PhaseVec<TE, VEC>*>(static_cast<const TE*>(a.pr) + r * a.ld + c);
    const PhaseVec<TE, VEC> t = *reinterpret_cast<const PhaseVec<TE, VEC>*>(static_cast<const TE*>(a.tas) + r * a.ld + c);
    PhaseVec<TO, VEC> s, l;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      double snow, rain;
      phase_split<M>(a.q, (double)x.v[k], (double)t.v[k], season, land[k], snow, rain);
      s.v[k] = (TO)snow, l.v[k] = (TO)rain;
    }
    if (a.snow) *reinterpret_cast<PhaseVec<TO, VEC>*>(static_cast<TO*>(a.snow) + r * a.ld_out + c) = s;
    if (a.rain) *reinterpret_cast<PhaseVec<TO, VEC>*>(static_cast<TO*>(a.rain) + r * a.ld_out + c) = l;
  }
}

// ---- host front end -------------------------------------------------------------------------------------------------
// the checks of the partition's parameters, and its tables uploaded
int phase_params(const char* fn, xh_ctx* ctx, size_t* cur, int method, bool given_ok, const double* par, const double* tab,
                 int64_t ntab, const uint8_t* season, int64_t T, const uint8_t* land, PhaseParams* q, bool upload) {
  XH_REQUIRE(method >= XH_PHASE_BINARY && method <= XH_PHASE_GIVEN, XH_ERR_ARG, "%s: unknown method %d", fn, method);
  XH_REQUIRE(given_ok || method != XH_PHASE_GIVEN, XH_ERR_ARG, "%s: the given-snow method has no element-wise form", fn);
  XH_REQUIRE(par, XH_ERR_ARG, "%s: NULL parameters", fn);
  *q = PhaseParams{};
  q->land = land;
  q->thresh = par[0], q->upper = par[1], q->add_K = par[2], q->sub_C = par[3];
  q->clip = par[4] != 0.0, q->land_all = par[5] != 0.0;
  if (method == XH_PHASE_BROWN) XH_REQUIRE(par[1] > par[0], XH_ERR_ARG, "%s: brown needs upper > thresh", fn);
  if (season)
    for (int64_t r = 0; r < T; ++r) XH_REQUIRE(season[r] <= 3, XH_ERR_ARG, "%s: season[%lld] = %d outside 0 .. 3", fn, (long long)r, season[r]);
  int64_t n = 0;
  if (method == XH_PHASE_AUER) {
    XH_REQUIRE(tab && ntab >= 2, XH_ERR_ARG, "%s: auer needs a table of at least two nodes", fn);
    XH_REQUIRE(ntab <= XH_PHASE_MAX_NODES, XH_ERR_LIMIT, "%s: at most %d nodes, got %lld", fn, XH_PHASE_MAX_NODES, (long long)ntab);
    for (int64_t k = 0; k + 1 < ntab; ++k) XH_REQUIRE(tab[k] < tab[k + 1], XH_ERR_ARG, "%s: the nodes must be strictly increasing", fn);
    q->K = (int)ntab;
    q->step = ntab > 3 ? (tab[ntab - 2] - tab[1]) / (double)(ntab - 3) : 1.0;
    n = 2 * ntab;
  } else if (method == XH_PHASE_DAI_ANNUAL || method == XH_PHASE_DAI_SEASONAL) {
    XH_REQUIRE(tab && ntab == XH_PHASE_DAI_NTAB, XH_ERR_ARG, "%s: the dai methods need a table of %d coefficients", fn, XH_PHASE_DAI_NTAB);
    if (q->clip)
      for (int k = 0; k < XH_PHASE_DAI_NTAB / 6; ++k)
        XH_REQUIRE(tab[k * 6 + 5] != 0.0 && tab[k * 6 + 5] == tab[k * 6 + 5], XH_ERR_ARG, "%s: clip needs fmax != fmin", fn);
    n = ntab;
  }
  if (upload && n > 0) return xh_upload(ctx, cur, tab, (size_t)n, &q->tab);
  return XH_OK;
}

// f(std::integral_constant<int, M>{}) for the method
template <typename F>
void phase_by_method(int method, F&& f) {
  xh_pick<XH_PHASE_BINARY, XH_PHASE_BROWN, XH_PHASE_AUER, XH_PHASE_DAI_ANNUAL, XH_PHASE_DAI_SEASONAL, XH_PHASE_GIVEN>(method, f);
}

template <typename TE, typename TO, int M>
void launch_map(xh_ctx* ctx, const MapArgs& a, int vec, int64_t rows) {
  const unsigned gy = (unsigned)(rows < 1 ? 1 : (rows > 65535 ? 65535 : rows));
  const dim3 g((unsigned)cdiv64(cdiv64(a.C, vec), XH_BLOCK), gy), b(XH_BLOCK);
  if (vec == 4) hipLaunchKernelGGL((k_phase_map<TE, TO, M, 4>), g, b, 0, ctx->stream, a);
  else if (vec == 2) hipLaunchKernelGGL((k_phase_map<TE, TO, M, 2>), g, b, 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_phase_map<TE, TO, M, 1>), g, b, 0, ctx->stream, a);
}

}  // namespace

int xh_precip_phase_map(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, const void* tas, int method,
                        const double* par, const double* tab, int64_t ntab, const uint8_t* season, const uint8_t* land,
                        void* snow_out, void* rain_out, int64_t ld_out) {
  const char* fn = "xh_precip_phase_map";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, T, ld_out);
  if (rc) return rc;
  XH_REQUIRE(pr && tas, XH_ERR_ARG, "%s: NULL field", fn);
  XH_REQUIRE(snow_out || rain_out, XH_ERR_ARG, "%s: no output requested (snow_out or rain_out)", fn);
  const bool run = T > 0 && C > 0;
  MapArgs a{};
  size_t cur = 0;
  rc = phase_params(fn, ctx, &cur, method, false, par, tab, ntab, season, T, land, &a.q, run);
  if (rc) return rc;
  if (!run) return XH_OK;
  std::vector<uint8_t> zeros;
  if (!season) zeros.assign((size_t)T, 0);
  rc = xh_upload(ctx, &cur, season ? season : zeros.data(), (size_t)T, &a.season);
  if (rc) return rc;
  a.pr = pr, a.tas = tas, a.snow = snow_out, a.rain = rain_out;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  // cells per lane: 16-byte loads where both fields and both outputs allow them (the outputs of the fractional methods are
  // float64 whatever the fields are)
  const size_t esz = f64 ? 8 : 4, osz = method == XH_PHASE_BINARY ? esz : 8;
  const int width = f64 ? 2 : 4;
  int vec = xh_cells_per_lane(pr, C, ld, width, esz);
  if (xh_cells_per_lane(tas, C, ld, width, esz) != vec) vec = 1;
  if (snow_out && xh_cells_per_lane(snow_out, C, ld_out, width, osz) != vec) vec = 1;
  if (rain_out && xh_cells_per_lane(rain_out, C, ld_out, width, osz) != vec) vec = 1;
  xh_by_width(f64, [&](auto w) {
    using TE = XH_WIDTH(w);
    phase_by_method(method, [&](auto m) {
      constexpr int M = decltype(m)::value;
      if constexpr (M == XH_PHASE_BINARY) launch_map<TE, TE, M>(ctx, a, vec, T);
      else if constexpr (M != XH_PHASE_GIVEN) launch_map<TE, double, M>(ctx, a, vec, T);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_precip_phase_period(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, const void* tas, double per_day,
                           int64_t P, const int64_t* seg, const int32_t* doy, int method, const double* par, const double* tab,
                           int64_t ntab, const uint8_t* season, const uint8_t* land, const double* lim, int window, uint32_t mask,
                           void* const* outs, int64_t ld_out) {
  const char* fn = "xh_precip_phase_period";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(pr && tas, XH_ERR_ARG, "%s: NULL field", fn);
  XH_REQUIRE(lim && outs, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(mask != 0 && mask < (1u << XH_PHASE_NOUT), XH_ERR_ARG, "%s: mask must ask for at least one of the %d outputs", fn, XH_PHASE_NOUT);
  for (int k = 0; k < XH_PHASE_NOUT; ++k)
    XH_REQUIRE(!(mask & (1u << k)) || outs[k], XH_ERR_ARG, "%s: output %d is asked for and NULL", fn, k);
  XH_REQUIRE(method != XH_PHASE_GIVEN || !(mask & ((1u << XH_PHASE_HPLT_DAYS) | (1u << XH_PHASE_ROFG_DAYS))), XH_ERR_ARG,
             "%s: the given-snow method has no temperature for hplt_days / rofg_days", fn);
  XH_REQUIRE(window >= 1 && window <= (1 << 30), XH_ERR_ARG, "%s: window must be at least 1, got %d", fn, window);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  for (int64_t p = 0; p < P; ++p) XH_REQUIRE(seg[p + 1] - seg[p] < ((int64_t)1 << 30), XH_ERR_LIMIT, "%s: period too long", fn);
  const bool dates = (mask & ((1u << XH_PHASE_FIRST_SNOW) | (1u << XH_PHASE_LAST_SNOW))) != 0;
  XH_REQUIRE(!dates || doy, XH_ERR_ARG, "%s: first_snow / last_snow need doy", fn);
  if (dates)
    for (int64_t r = seg[0]; r < seg[P]; ++r)
      XH_REQUIRE(doy[r] >= 1 && doy[r] <= 366, XH_ERR_ARG, "%s: doy[%lld] = %d outside 1 .. 366", fn, (long long)r, doy[r]);
  const bool run = P > 0 && C > 0;
  PeriodArgs a{};
  size_t cur = 0;
  rc = phase_params(fn, ctx, &cur, method, true, par, tab, ntab, season, T, land, &a.q, run);
  if (rc) return rc;
  if (!run) return XH_OK;

  std::vector<int32_t> meta((size_t)(T > 0 ? T : 1), 0);
  for (int64_t r = 0; r < T; ++r) meta[(size_t)r] = (season ? (int32_t)season[r] : 0) | (dates && r >= seg[0] && r < seg[P] ? doy[r] << 8 : 0);
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc) rc = xh_upload(ctx, &cur, (const int32_t*)meta.data(), meta.size(), &a.meta);
  if (rc) return rc;
  a.pr = pr, a.tas = tas;
  for (int k = 0; k < XH_PHASE_NOUT; ++k) a.out[k] = (mask & (1u << k)) ? static_cast<double*>(outs[k]) : nullptr;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.per_day = per_day;
  a.snow_low = lim[0], a.snow_high = lim[1], a.snow_thresh = lim[2], a.hplt_pr = lim[3], a.hplt_tas = lim[4];
  a.rofg_pr = lim[5], a.rofg_frz = lim[6];
  a.window = window;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) {
    using TE = XH_WIDTH(w);
    phase_by_method(method, [&](auto m) { hipLaunchKernelGGL((k_phase_period<TE, decltype(m)::value>), g, b, 0, ctx->stream, a); });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
