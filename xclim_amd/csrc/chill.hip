// chill.hip — the winter-chill indices (indices/_agro.py) and Linvill's hourly temperature profile (indices/helpers.py).
//
// Reference: _accumulate_intermediate / _chill_portion_one_season (_agro.py:1436-1465: the Dynamic Model of Fishman et al.
// with the constants of Luedeling et al.), the Utah weights of chill_units (:1574-1592), and make_hourly_temperature with
// _compute_daytime_temperature / _compute_nighttime_temperature (helpers.py:977-1123).
//
// One lane owns one (cell, period): cells along x, periods along y.  A period restarts the recurrence at E = 0, so the
// periods are independent and a narrow band of many years still fills the machine.  The lane marches down the rows of its
// period; an unselected row (select_time(..., drop=True)) is skipped and the state carries across the gap.
//
// Arithmetic is float64 in the reference's order of operations (the build has -ffp-contract=off).  The hour step is ONE
// function, chill_step, for both entry points: k_chill_hourly feeds it the field, k_chill_daily the 24 hourly temperatures
// it builds per day in registers.  A NaN temperature makes E NaN to the end of the period; `E < 1` and `E >= 1` are then
// both false, so delta is 0 from there on (never NaN), exactly as np.where does in the reference.
// The Utah comparisons run in the dtype of the temperature they see (numpy compares a float32 field against the float32
// roundings of 1.4, 2.4 ...); the fused path compares in float64, because its hourly temperatures are float64.
#include "hostargs.h"

namespace {

// _chill_portion_one_season's constants (_agro.py:1445-1452)
constexpr double E0 = 4153.5;
constexpr double E1 = 12888.8;
constexpr double A0 = 139500;
constexpr double A1 = 2.567e18;
constexpr double SLP = 1.6;
constexpr double TETMLT = 277;
constexpr double AA = A0 / A1;
constexpr double EE = E1 - E0;

struct ChillState {
  double E;     // inter_E of the previous selected hour
  double xi;    // xi of the previous selected hour
  int started;  // 0 until the period's first selected hour, whose inter_E is 0 whatever its temperature
};

// One hour.  tK [K] advances the Dynamic Model and returns delta (:1454-1463); tC [degC] gives the Utah weight w
// (:1574-1586), with nanw set for a NaN temperature (the hour then contributes nothing, :1587).
// dyn / utah: which of the two models the launch asked for (uniform over the launch).
template <typename TU>
__device__ __forceinline__ double chill_step(double tK, TU tC, bool dyn, bool utah, ChillState& s, double& w, bool& nanw) {
  double delta = 0.0;
  if (dyn) {
    const double ftmprt = SLP * TETMLT * (tK - TETMLT) / tK;
    const double sr = exp(ftmprt);
    const double xi = sr / (1 + sr);
    double E = 0.0;
    if (s.started) {
      const double xs = AA * exp(EE / tK);
      const double ak1 = A1 * exp(-E1 / tK);
      const double S = s.E < 1 ? s.E : s.E - s.E * s.xi;
      E = xs - (xs - S) * exp(-ak1);
    }
    s.E = E;
    s.xi = xi;
    s.started = 1;
    delta = E >= 1 ? E * xi : 0.0;
  }

  nanw = tC != tC;
  w = 0.0;
  if (!utah) return delta;
  if (tC <= (TU)1.4 || (tC > (TU)12.4 && tC <= (TU)15.9)) w = 0.0;
  else if ((tC > (TU)1.4 && tC <= (TU)2.4) || (tC > (TU)9.1 && tC <= (TU)12.4)) w = 0.5;
  else if (tC > (TU)2.4 && tC <= (TU)9.1) w = 1.0;
  else if (tC > (TU)15.9 && tC <= (TU)17.9) w = -0.5;
  else w = -1.0;
  if (nanw) w = 0.0;
  return delta;
}

// The sums of one period: chill portions, chill units (per day with positive_only, :1589-1591) and the valid hours
struct ChillSums {
  double cp, cu, day;
  int32_t valid;
  __device__ __forceinline__ void add(double delta, double w, bool nanw, int positive_only) {
    cp += delta;
    valid += nanw ? 0 : 1;
    if (positive_only) day += w;
    else cu += w;
  }
  __device__ __forceinline__ void end_of_day(int positive_only) {
    if (positive_only && day > 0) cu += day;
    day = 0.0;
  }
};

struct ChillArgs {
  const void* tas;     // hourly: the field; daily: tasmin
  const void* tasmax;  // daily only
  const double* dl;    // daily only: (D, L)
  const int32_t* lat_idx;
  const int64_t* seg;
  const uint8_t* sel;  // NULL = every row
  double* cp_out;
  double* cu_out;
  int32_t* valid_out;
  double* row_out;  // hourly: delta_out (H, C); daily: hourly_out (24 D, C)
  bool dyn, utah;   // the Dynamic Model / the Utah model is asked for
  int64_t T, C, ld, ld_out, L;
  double add_K, sub_C;
  int rows_per_day, positive_only;
};

__device__ __forceinline__ void chill_store(const ChillArgs& a, int64_t p, int64_t c, const ChillSums& m) {
  const int64_t o = p * a.ld_out + c;
  if (a.cp_out) a.cp_out[o] = m.cp;
  if (a.cu_out) a.cu_out[o] = m.cu;
  if (a.valid_out) a.valid_out[o] = m.valid;
}

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_chill_hourly(ChillArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > a.T ? a.T : r1;
  ChillState s{0.0, 0.0, 0};
  ChillSums m{0.0, 0.0, 0.0, 0};
  const int64_t rpd = a.rows_per_day;
  for (int64_t r = r0; r < r1; ++r) {
    double delta = 0.0;
    if (!a.sel || a.sel[r]) {
      const TE t = xh_ld<TE>(a.tas, r * a.ld + c);
      double w;
      bool nanw;
      delta = chill_step<TE>((double)t + a.add_K, t - (TE)a.sub_C, a.dyn, a.utah, s, w, nanw);
      m.add(delta, w, nanw, a.positive_only);
    }
    if (a.row_out) a.row_out[r * a.ld_out + c] = delta;
    if (r % rpd == rpd - 1 || r == r1 - 1) m.end_of_day(a.positive_only);
  }
  chill_store(a, p, c, m);
}

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_chill_daily(ChillArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  int64_t d0 = a.seg[p], d1 = a.seg[p + 1];
  d0 = d0 < 0 ? 0 : d0;
  d1 = d1 > a.T ? a.T : d1;
  const int64_t li = a.lat_idx[c];
  const double pi = 3.141592653589793;  // np.pi
  ChillState s{0.0, 0.0, 0};
  ChillSums m{0.0, 0.0, 0.0, 0};
  for (int64_t d = d0; d < d1; ++d) {
    const bool sel = !a.sel || a.sel[d];
    if (!sel && !a.row_out) continue;
    const TE tn = xh_ld<TE>(a.tas, d * a.ld + c), tx = xh_ld<TE>(a.tasmax, d * a.ld + c);
    // helpers.py:1093-1106: the last day's next tasmin is its own (the appended copy of the last day)
    const double tnn = d + 1 < a.T ? (double)xh_ld<TE>(a.tas, (d + 1) * a.ld + c) : (double)tn;
    const double dl = a.dl[d * a.L + li];
    const TE range = tx - tn;  // in the field's dtype, as two DataArrays of it subtract
    const double rng = (double)range, tnd = (double)tn;
    const double den = dl + 4;
    const double sunset = rng * sin((pi * dl) / den) + tnd;           // helpers.py:1105
    const double slope = (sunset - tnn) / log(24 - (dl - 1));         // helpers.py:1035 with daylength - 1 (:1121)
    for (int h = 0; h < 24; ++h) {
      double t;
      if ((double)h < dl) {
        t = rng * sin((pi * (double)h) / den) + tnd;  // helpers.py:1004
      } else {
        double nh = (double)(h + 1) - dl;  // helpers.py:1112: clip(1) keeps NaN
        nh = nh < 1 ? 1.0 : nh;
        t = sunset - slope * log(nh);
      }
      if (a.row_out) a.row_out[(d * 24 + h) * a.ld_out + c] = t;
      if (sel) {
        double w;
        bool nanw;
        const double delta = chill_step<double>(t + a.add_K, t - a.sub_C, a.dyn, a.utah, s, w, nanw);
        m.add(delta, w, nanw, a.positive_only);
      }
    }
    m.end_of_day(a.positive_only);
  }
  if (a.cp_out || a.cu_out || a.valid_out) chill_store(a, p, c, m);
}

// seg is a DEVICE table here: its offsets cannot be walked on the host (the kernels clamp them to [0, T])
int chill_checks(const char* who, xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int64_t P, const void* seg, int64_t ld_out,
                 int64_t out_rows) {
  const int rc = xh_check_pitched(who, ctx, T, C, ld, out_rows, ld_out);
  if (rc) return rc;
  XH_REQUIRE(P >= 0, XH_ERR_ARG, "%s: negative shape", who);
  XH_REQUIRE(seg, XH_ERR_ARG, "%s: NULL period offsets", who);
  XH_REQUIRE(P <= XH_MAX_PERIODS, XH_ERR_LIMIT, "%s: at most 65535 periods, got %lld", who, (long long)P);
  return XH_OK;
}

}  // namespace

int xh_chill_hourly(xh_ctx* ctx, int64_t H, int64_t C, int64_t ld, int f64, const void* tas, int rows_per_day, int64_t P,
                    const int64_t* seg, const uint8_t* row_sel, double add_K, double sub_C, int positive_only, double* cp_out,
                    double* cu_out, int32_t* valid_out, double* delta_out, int64_t ld_out) {
  const int rc = chill_checks("xh_chill_hourly", ctx, H, C, ld, P, seg, ld_out, H > P ? H : P);
  if (rc != XH_OK) return rc;
  XH_REQUIRE(tas, XH_ERR_ARG, "xh_chill_hourly: NULL field");
  XH_REQUIRE(rows_per_day >= 1, XH_ERR_ARG, "xh_chill_hourly: rows_per_day must be positive, got %d", rows_per_day);
  XH_REQUIRE(cp_out || cu_out || valid_out || delta_out, XH_ERR_ARG, "xh_chill_hourly: no output requested");
  if (P == 0 || C == 0) return XH_OK;
  ChillArgs a{};
  a.tas = tas;
  a.seg = seg;
  a.sel = row_sel;
  a.cp_out = cp_out;
  a.cu_out = cu_out;
  a.valid_out = valid_out;
  a.row_out = delta_out;
  a.T = H;
  a.C = C;
  a.ld = ld;
  a.ld_out = ld_out;
  a.add_K = add_K;
  a.sub_C = sub_C;
  a.rows_per_day = rows_per_day;
  a.positive_only = positive_only != 0;
  a.dyn = cp_out || delta_out;
  a.utah = cu_out != nullptr;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_chill_hourly<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_chill_daily(xh_ctx* ctx, int64_t D, int64_t C, int64_t ld, int f64, const void* tasmin, const void* tasmax,
                   const double* dl, int64_t L, const int32_t* lat_idx, int64_t P, const int64_t* seg, const uint8_t* day_sel,
                   double add_K, double sub_C, int positive_only, double* cp_out, double* cu_out, int32_t* valid_out,
                   double* hourly_out, int64_t ld_out) {
  const int rc = chill_checks("xh_chill_daily", ctx, D, C, ld, P, seg, ld_out, 24 * D > P ? 24 * D : P);
  if (rc != XH_OK) return rc;
  XH_REQUIRE(tasmin && tasmax && dl && lat_idx, XH_ERR_ARG, "xh_chill_daily: NULL argument");
  XH_REQUIRE(L >= 1 && D * L < ((int64_t)1 << 40), XH_ERR_ARG, "xh_chill_daily: bad day-length table shape");
  XH_REQUIRE(cp_out || cu_out || valid_out || hourly_out, XH_ERR_ARG, "xh_chill_daily: no output requested");
  if (P == 0 || C == 0) return XH_OK;
  ChillArgs a{};
  a.tas = tasmin;
  a.tasmax = tasmax;
  a.dl = dl;
  a.lat_idx = lat_idx;
  a.seg = seg;
  a.sel = day_sel;
  a.cp_out = cp_out;
  a.cu_out = cu_out;
  a.valid_out = valid_out;
  a.row_out = hourly_out;
  a.T = D;
  a.C = C;
  a.ld = ld;
  a.ld_out = ld_out;
  a.L = L;
  a.add_K = add_K;
  a.sub_C = sub_C;
  a.rows_per_day = 24;
  a.positive_only = positive_only != 0;
  a.dyn = cp_out != nullptr;
  a.utah = cu_out != nullptr;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_chill_daily<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
