// agro.hip — the viticulture and agroclimatic heat-sum indices of indices/_agro.py: huglin_index (:151-263),
// biologically_effective_degree_days (:275-443), cool_night_index (:447-528), dryness_index (:532-724),
// latitude_temperature_index (:728-787), corn_heat_units (:69-142), qian_weighted_mean_average (:1245-1284) and
// effective_growing_degree_days (:1292-1384, with generic.py:1417-1511 aggregate_between_dates, :1556-1608
// first_day_threshold_reached and core/calendar.py:1004-1072 doy_to_days_since).
//
// The three period kernels have one lane per (cell, period): cells along x (consecutive lanes on consecutive cells, so a
// wave reads 64 consecutive elements of a row), periods along y.  The two element-wise kernels have one lane per cell and
// walk rows blockIdx.y, blockIdx.y + gridDim.y, ...
//
// Values are widened to float64 on load and all arithmetic is float64 in the reference's order of operations (the build has
// -ffp-contract=off).  A temperature goes to degC as `x - sub_C` right after widening, each field on its own, as
// convert_units_to does before the reference combines them.  ASSUMPTION: for float32 fields the reference subtracts 273.15
// and goes on in float32; this unit does not reproduce float32 arithmetic (README: status of the agroclimatic unit).
//
// k_agro_degree_sum issues the loads of AGRO_BATCH rows (every field, and the day factor) before it uses the first of them:
// the addresses depend on nothing that was loaded, so the batch is AGRO_BATCH * fields independent loads in flight per lane
// instead of one dependent load per row.  The entry point turns seg and day_sel into the RUNS of consecutive selected rows of
// every period on the host (one run for a season inside the period, two for one that wraps around its ends), and a lane walks
// the runs of its period: it reads no row outside the span from the first to the last selected row (nor the holes between
// runs), and the mask itself is never read on the device — a mask byte loaded per row would put a wait on every outstanding
// load into the batch.
//
// k_egdd walks its period TWICE.  The start of the season is a day of year that doy_to_days_since turns into a day number
// counted from the period's label, and for a start found in the last days of a "YS-JUL" period the reference's conversion
// wraps to a day number at the BEGINNING of the period (a day of year at or past the label's is taken to lie in the label's
// year).  A running sum frozen at the first frost cannot give that answer, since those days are long past when the start is
// found; so the first walk finds the two bounds and the second sums between them.  A period is at most 366 rows: the second
// walk reads what the first one left in the cache.
#include <vector>

#include "../../include/xclim_hip_agro.h"
#include "hostargs.h"

namespace {

constexpr int AGRO_BATCH = 8;

// ---- xh_agro_degree_sum ---------------------------------------------------------------------------------------------
struct DegArgs {
  const void *tas, *tasmin, *tasmax;
  const int64_t *run_off, *run_lo, *run_hi;  // (P + 1): the runs of every period; (R), (R): first and one-past-last row of a run
  const double *k_cell, *k_day, *k_period;
  const int32_t* lat_idx;
  double *hi_out, *bedd_out;
  int32_t* valid_out;
  int64_t C, ld, ld_out, L;
  double sub_C, thresh_hi, thresh_bedd, low_dtr, high_dtr, max_dd;
  int tr_adj;
};

template <typename TE, bool HI, bool BEDD>
__global__ void __launch_bounds__(XH_BLOCK) k_agro_degree_sum(DegArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t li = a.lat_idx ? a.lat_idx[c] : 0;
  const double kc = a.k_cell ? a.k_cell[c] : 1.0;
  double s_hi = 0.0, s_bedd = 0.0;
  int32_t valid = 0;
  for (int64_t k = a.run_off[p]; k < a.run_off[p + 1]; ++k) {
    const int64_t lo = a.run_lo[k], hi = a.run_hi[k];
    for (int64_t r0 = lo; r0 < hi; r0 += AGRO_BATCH) {
      TE tx[AGRO_BATCH], tg[AGRO_BATCH], tn[AGRO_BATCH];  // as loaded: a float32 batch is half the registers, widened at use
      double kd[AGRO_BATCH];
      bool on[AGRO_BATCH];
#pragma unroll
      for (int u = 0; u < AGRO_BATCH; ++u) {
        const int64_t r = r0 + u;
        on[u] = r < hi;
        tx[u] = tg[u] = tn[u] = (TE)0;
        kd[u] = kc;
        if (on[u]) {
          const int64_t i = r * a.ld + c;
          tx[u] = xh_ld<TE>(a.tasmax, i);
          if (HI) tg[u] = xh_ld<TE>(a.tas, i);
          if (BEDD) tn[u] = xh_ld<TE>(a.tasmin, i);
          if (a.k_day) kd[u] = a.k_day[r * a.L + li];
        }
      }
#pragma unroll
      for (int u = 0; u < AGRO_BATCH; ++u) {
        if (!on[u]) continue;
        const double x = (double)tx[u] - a.sub_C;
        bool present = x == x;
        if (HI) {
          const double g = (double)tg[u] - a.sub_C;
          present = present && g == g;
          double t = (g + x) / 2 - a.thresh_hi;  // _agro.py:257
          t = t < 0 ? 0.0 : t;                   // clip(min=0) keeps NaN
          t = t * kd[u];
          if (t == t) s_hi += t;
        }
        if (BEDD) {
          const double n = (double)tn[u] - a.sub_C;
          present = present && n == n;
          double adj = 0.0;
          if (a.tr_adj) {  // :411-416
            const double dtr = x - n;
            adj = 0.25 * (dtr > a.high_dtr ? dtr - a.high_dtr : (dtr < a.low_dtr ? dtr - a.low_dtr : 0.0));
          }
          double t = (n + x) / 2 - a.thresh_bedd;  // :435
          t = t < 0 ? 0.0 : t;
          t = t * kd[u] + adj;
          t = t > a.max_dd ? a.max_dd : t;  // clip(max=) keeps NaN
          if (t == t) s_bedd += t;
        }
        valid += present ? 1 : 0;
      }
    }
  }
  const int64_t o = p * a.ld_out + c;
  const double kp = a.k_period ? a.k_period[p * a.L + li] : 1.0;
  if (a.hi_out) a.hi_out[o] = a.k_period ? s_hi * kp : s_hi;
  if (a.bedd_out) a.bedd_out[o] = a.k_period ? s_bedd * kp : s_bedd;
  if (a.valid_out) a.valid_out[o] = valid;
}

// ---- xh_agro_monthly ------------------------------------------------------------------------------------------------
// dryness_index's month coefficients (:649-658), index = calendar month - 1
__constant__ double DI_K_NORTH[12] = {0, 0, 0, 0.1, 0.3, 0.5, 0.5, 0.5, 0.5, 0, 0, 0};
__constant__ double DI_K_SOUTH[12] = {0.5, 0.5, 0.5, 0, 0, 0, 0, 0, 0, 0.1, 0.3, 0.5};

struct MonArgs {
  const void *tasmin, *tas, *pr, *evspsblpot;
  const int64_t *month_off, *seg_months;  // (M + 1), (P + 1)
  const int32_t *month_cal, *month_days;  // (M), (M)
  const double* lat;                      // (C) or NULL
  double *cni_out, *mtwm_out, *di_out;
  int32_t* valid_out;
  int64_t M, C, ld, ld_out;
  double sub_C, per_day, wo;
  int hemisphere;  // 0 = by the cell's latitude, 1 = north, 2 = south
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_agro_monthly(MonArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t m0 = a.seg_months[p], m1 = a.seg_months[p + 1];
  const double nan = xh_nan64();
  const double lat = a.lat ? a.lat[c] : 0.0;
  const bool cni_north = a.hemisphere ? a.hemisphere == 1 : lat > 0;   // :513
  const bool di_north = a.hemisphere ? a.hemisphere == 1 : lat >= 0;  // :670
  const int cni_month = cni_north ? 9 : 3;
  double cni_s = 0.0, mtwm = nan, di = 0.0;
  int32_t cni_n = 0, valid = 0;
  // the months of the period: cool nights, the warmest month, and the rows that count as present
  for (int64_t m = m0; (a.tasmin || a.tas || a.valid_out) && m < m1; ++m) {
    const int64_t r0 = a.month_off[m], r1 = a.month_off[m + 1];
    const bool cni_m = a.cni_out && a.month_cal[m] == cni_month;
    double ts = 0.0;
    int32_t tn = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t i = r * a.ld + c;
      bool present = true;
      if (a.tasmin && (cni_m || a.valid_out)) {
        const double x = xh_ldw<TE>(a.tasmin, i) - a.sub_C;
        present = present && x == x;
        if (cni_m && x == x) cni_s += x, cni_n += 1;
      }
      if (a.tas) {
        const double x = xh_ldw<TE>(a.tas, i) - a.sub_C;
        present = present && x == x;
        if (x == x) ts += x, tn += 1;
      }
      if (a.valid_out && a.pr) {
        const double x = xh_ldw<TE>(a.pr, i), e = xh_ldw<TE>(a.evspsblpot, i);
        present = present && x == x && e == e;
      }
      valid += present ? 1 : 0;
    }
    if (a.mtwm_out && tn > 0) {
      const double mean = ts / (double)tn;  // :776, then max over the period's months (:777)
      mtwm = (mtwm != mtwm || mean > mtwm) ? mean : mtwm;
    }
  }
  // the dryness index: January - December of the period in the north, July before it - June in the south (:706-711)
  if (a.di_out) {
    int64_t d0 = di_north ? m0 : m0 - 6, d1 = di_north ? m1 : m1 - 6;
    d0 = d0 < 0 ? 0 : d0;
    d1 = d1 > a.M ? a.M : d1;
    const double* kt = di_north ? DI_K_NORTH : DI_K_SOUTH;
    for (int64_t m = d0; m < d1; ++m) {
      const int64_t r0 = a.month_off[m], r1 = a.month_off[m + 1];
      double E = 0.0, Pm = 0.0;
      for (int64_t r = r0; r < r1; ++r) {
        const int64_t i = r * a.ld + c;
        const double e = xh_ldw<TE>(a.evspsblpot, i) * a.per_day, x = xh_ldw<TE>(a.pr, i) * a.per_day;
        if (e == e) E += e;
        if (x == x) Pm += x;
      }
      const double k = kt[a.month_cal[m] - 1], N = (double)a.month_days[m];
      const double Pk = (k > 0 ? 1.0 : 0.0) * Pm;          // :690
      const double tv = E * k;                              // :693
      const double jpm = Pk / 5 > N ? N : Pk / 5;           // clip(max=daysinmonth)
      const double es = (E / N) * (1 - k) * jpm;            // :696-700
      const double term = Pk - tv - es;
      if (term == term) di += term;
    }
    di = a.wo + di;
  }
  const int64_t o = p * a.ld_out + c;
  if (a.cni_out) a.cni_out[o] = cni_n > 0 ? cni_s / (double)cni_n : nan;
  if (a.mtwm_out) a.mtwm_out[o] = mtwm;
  if (a.di_out) a.di_out[o] = di;
  if (a.valid_out) a.valid_out[o] = valid;
}

// ---- xh_egdd --------------------------------------------------------------------------------------------------------
struct EgddArgs {
  const void *tasmin, *tasmax;
  const int64_t* seg;          // (P + 1)
  const int32_t* doy;          // (T)
  const int64_t *start_from, *end_from, *day0;  // (P) each: first row the bound may lie on (-1 = none), days label -> first row
  const int32_t *label_doy, *label_days;        // (P) each: day of year of the label, days in the label's year
  double *egdd_out, *start_out, *end_out;
  int32_t* valid_out;
  int64_t T, C, ld, ld_out;
  double sub_C, thresh;
  int method;
};

// (_agro.py:1357 after :1352-1353: each field to degC first, then the mean)
template <typename TE>
__device__ __forceinline__ double egdd_tas(const EgddArgs& a, int64_t r, int64_t c, double& tn) {
  const int64_t i = r * a.ld + c;
  tn = xh_ldw<TE>(a.tasmin, i) - a.sub_C;
  return (tn + (xh_ldw<TE>(a.tasmax, i) - a.sub_C)) / 2;
}

// doy_to_days_since(da) with start=None (calendar.py:1050-1059): days since the period's label
__device__ __forceinline__ int64_t days_since(int64_t doy, int64_t label_doy, int64_t label_days) {
  return (doy >= label_doy ? doy : doy + label_days) - label_doy;
}

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_egdd(EgddArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  const int64_t sf = a.start_from[p], ef = a.end_from[p];
  const double nan = xh_nan64();
  const int window = a.method == 1 ? 5 : 1;
  int64_t start_row = -1, end_row = -1;
  int32_t valid = 0;
  int run = 0;
  // walk 1: the bounds.  w0 .. w4 hold tas of rows r - 2 .. r + 2 of the WHOLE series (NaN outside it)
  double w0 = nan, w1 = nan, w2 = nan, w3 = nan, w4 = nan, tn2 = nan, tn3 = nan, tn4 = nan, t;
  if (r0 < r1) {
    if (r0 - 2 >= 0) w1 = egdd_tas<TE>(a, r0 - 2, c, t);
    if (r0 - 1 >= 0) w2 = egdd_tas<TE>(a, r0 - 1, c, t);
    w3 = egdd_tas<TE>(a, r0, c, tn3);
    if (r0 + 1 < a.T) w4 = egdd_tas<TE>(a, r0 + 1, c, tn4);
  }
  for (int64_t r = r0; r < r1; ++r) {
    w0 = w1, w1 = w2, w2 = w3, w3 = w4, tn2 = tn3, tn3 = tn4;
    w4 = nan, tn4 = nan;
    if (r + 2 < a.T) w4 = egdd_tas<TE>(a, r + 2, c, tn4);
    valid += (w2 == w2) ? 1 : 0;  // NaN exactly when tasmin or tasmax is
    double v = w2;
    if (a.method == 1) v = (((w0 * 0.0625 + w1 * 0.25) + w2 * 0.375) + w3 * 0.25) + w4 * 0.0625;  // :1281-1282, left to right
    const bool cond = sf >= 0 && r >= sf && v > a.thresh;
    run = cond ? run + 1 : 0;
    if (start_row < 0 && run >= window) start_row = r - (window - 1);
    if (end_row < 0 && ef >= 0 && r >= ef && tn2 < 0) end_row = r;
  }
  // day of year of the bounds (:1361-1379) and their day numbers (generic.py:1477-1484)
  const int64_t ld_ = a.label_doy[p], ly = a.label_days[p];
  const int64_t start_doy = start_row >= 0 ? (int64_t)a.doy[start_row] + (a.method == 0 ? 10 : 0) : 0;
  const int64_t end_doy = end_row >= 0 ? (int64_t)a.doy[end_row] - 1 : 0;
  const int64_t start_d = days_since(start_doy, ld_, ly), end_d = days_since(end_doy, ld_, ly);
  const bool ok = start_row >= 0 && end_row >= 0 && start_d <= end_d;  // :1501
  double sum = 0.0;
  if (ok && a.egdd_out) {
    // walk 2: rows whose day number d = day0 + (r - r0) has start_d <= d <= end_d - 1 (:1496-1500)
    int64_t ra = r0 + (start_d - a.day0[p]), rb = r0 + (end_d - 1 - a.day0[p]) + 1;
    ra = ra < r0 ? r0 : ra;
    rb = rb > r1 ? r1 : rb;
    for (int64_t rr = ra; rr < rb; rr += AGRO_BATCH) {
      double v[AGRO_BATCH];
#pragma unroll
      for (int u = 0; u < AGRO_BATCH; ++u) v[u] = rr + u < rb ? egdd_tas<TE>(a, rr + u, c, t) : nan;
#pragma unroll
      for (int u = 0; u < AGRO_BATCH; ++u) {
        double d = v[u] - a.thresh;  // :1381
        d = d < 0 ? 0.0 : d;
        if (d == d) sum += d;
      }
    }
  }
  const int64_t o = p * a.ld_out + c;
  if (a.egdd_out) a.egdd_out[o] = ok ? sum : nan;
  if (a.start_out) a.start_out[o] = start_row >= 0 ? (double)start_doy : nan;
  if (a.end_out) a.end_out[o] = end_row >= 0 ? (double)end_doy : nan;
  if (a.valid_out) a.valid_out[o] = valid;
}

// ---- the element-wise pair ------------------------------------------------------------------------------------------
struct ElemArgs {
  const void *a, *b;
  double* out;
  int64_t T, C, ld, ld_out;
  double sub_C, thresh_a, thresh_b;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_corn_heat_units(ElemArgs e) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= e.C) return;
  for (int64_t r = blockIdx.y; r < e.T; r += gridDim.y) {
    const double tn = xh_ldw<TE>(e.a, r * e.ld + c) - e.sub_C, tx = xh_ldw<TE>(e.b, r * e.ld + c) - e.sub_C;
    const double dn = tn - e.thresh_a, dx = tx - e.thresh_b;
    // :129-139: each half is 0 where its own comparison is false, and a comparison with NaN is false
    const double yn = tn > e.thresh_a ? 1.8 * dn : 0.0;
    const double yx = tx > e.thresh_b ? 3.33 * dx - 0.084 * (dx * dx) : 0.0;
    e.out[r * e.ld_out + c] = (yn + yx) / 2;
  }
}

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_qian_wma(ElemArgs e) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= e.C) return;
  for (int64_t r = blockIdx.y; r < e.T; r += gridDim.y) {
    double v = xh_nan64();  // rolling(5, center=True).construct pads with NaN: NaN within 2 rows of either end
    if (r >= 2 && r + 2 < e.T) {
      const double w0 = xh_ldw<TE>(e.a, (r - 2) * e.ld + c), w1 = xh_ldw<TE>(e.a, (r - 1) * e.ld + c), w2 = xh_ldw<TE>(e.a, r * e.ld + c),
                   w3 = xh_ldw<TE>(e.a, (r + 1) * e.ld + c), w4 = xh_ldw<TE>(e.a, (r + 2) * e.ld + c);
      v = (((w0 * 0.0625 + w1 * 0.25) + w2 * 0.375) + w3 * 0.25) + w4 * 0.0625;
    }
    e.out[r * e.ld_out + c] = v;
  }
}

// ---- host front end -------------------------------------------------------------------------------------------------
dim3 agro_grid(int64_t C, int64_t rows) {
  return dim3((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(rows < 1 ? 1 : (rows > 65535 ? 65535 : rows)));
}

}  // namespace

int xh_agro_degree_sum(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, const void* tasmin,
                       const void* tasmax, int64_t P, const int64_t* seg, const uint8_t* day_sel, const double* k_cell,
                       const double* k_day, const double* k_period, int64_t L, const int32_t* lat_idx, double sub_C,
                       double thresh_hi, double thresh_bedd, int tr_adj, double low_dtr, double high_dtr, double max_dd,
                       double* hi_out, double* bedd_out, int32_t* valid_out, int64_t ld_out) {
  const char* fn = "xh_agro_degree_sum";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (!rc) rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  XH_REQUIRE(hi_out || bedd_out, XH_ERR_ARG, "%s: no output requested (hi_out or bedd_out)", fn);
  XH_REQUIRE(tasmax && (!hi_out || tas) && (!bedd_out || tasmin), XH_ERR_ARG, "%s: a field needed by the requested outputs is NULL", fn);
  XH_REQUIRE(!(k_cell && k_day), XH_ERR_ARG, "%s: at most one day factor (k_cell or k_day)", fn);
  XH_REQUIRE(!(k_day || k_period) || (lat_idx && L >= 1 && T * L < ((int64_t)1 << 40) && P * L < ((int64_t)1 << 40)), XH_ERR_ARG,
             "%s: k_day and k_period need lat_idx and L >= 1", fn);
  if (P == 0 || C == 0) return XH_OK;

  // the runs of consecutive selected rows of every period
  std::vector<int64_t> run_off((size_t)P + 1, 0), lo, hi;
  for (int64_t p = 0; p < P; ++p) {
    for (int64_t r = seg[p]; r < seg[p + 1];) {
      if (day_sel && !day_sel[r]) {
        ++r;
        continue;
      }
      int64_t e = day_sel ? r : seg[p + 1];
      while (e < seg[p + 1] && day_sel[e]) ++e;
      lo.push_back(r), hi.push_back(e);
      r = e;
    }
    run_off[(size_t)p + 1] = (int64_t)lo.size();
  }
  if (lo.empty()) lo.push_back(0), hi.push_back(0);  // (nothing selected anywhere: the tables still exist)
  DegArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, run_off.data(), run_off.size(), &a.run_off);
  if (!rc) rc = xh_upload(ctx, &cur, lo.data(), lo.size(), &a.run_lo);
  if (!rc) rc = xh_upload(ctx, &cur, hi.data(), hi.size(), &a.run_hi);
  if (rc) return rc;
  a.tas = hi_out ? tas : nullptr;
  a.tasmin = bedd_out ? tasmin : nullptr;
  a.tasmax = tasmax;
  a.k_cell = k_cell, a.k_day = k_day, a.k_period = k_period, a.lat_idx = (k_day || k_period) ? lat_idx : nullptr;
  a.hi_out = hi_out, a.bedd_out = bedd_out, a.valid_out = valid_out;
  a.C = C, a.ld = ld, a.ld_out = ld_out, a.L = L;
  a.sub_C = sub_C, a.thresh_hi = thresh_hi, a.thresh_bedd = thresh_bedd;
  a.low_dtr = low_dtr, a.high_dtr = high_dtr, a.max_dd = max_dd, a.tr_adj = tr_adj != 0;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) {
    if (hi_out && bedd_out) hipLaunchKernelGGL((k_agro_degree_sum<XH_WIDTH(w), true, true>), g, b, 0, ctx->stream, a);
    else if (hi_out) hipLaunchKernelGGL((k_agro_degree_sum<XH_WIDTH(w), true, false>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_agro_degree_sum<XH_WIDTH(w), false, true>), g, b, 0, ctx->stream, a);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_agro_monthly(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tasmin, const void* tas, const void* pr,
                    const void* evspsblpot, int64_t M, const int64_t* month_off, const int32_t* month_cal,
                    const int32_t* month_days, int64_t P, const int64_t* seg_months, const double* lat, int hemisphere,
                    double sub_C, double per_day, double wo, double* cni_out, double* mtwm_out, double* di_out,
                    int32_t* valid_out, int64_t ld_out) {
  const char* fn = "xh_agro_monthly";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), XH_ERR_ARG, "%s: bad month count", fn);
  XH_REQUIRE(month_cal && month_days, XH_ERR_ARG, "%s: NULL month table", fn);
  rc = xh_check_offsets(fn, seg_months, P, M, "month period");
  if (!rc) rc = xh_check_offsets(fn, month_off, M, T, "month", M);  // (the month count has its own check above)
  if (rc) return rc;
  for (int64_t m = 0; m < M; ++m)
    XH_REQUIRE(month_cal[m] >= 1 && month_cal[m] <= 12 && month_days[m] >= 1, XH_ERR_ARG, "%s: month %lld: calendar month %d, %d days", fn,
               (long long)m, month_cal[m], month_days[m]);
  XH_REQUIRE(cni_out || mtwm_out || di_out, XH_ERR_ARG, "%s: no output requested (cni_out, mtwm_out or di_out)", fn);
  XH_REQUIRE((!cni_out || tasmin) && (!mtwm_out || tas) && (!di_out || (pr && evspsblpot)), XH_ERR_ARG,
             "%s: a field needed by the requested outputs is NULL", fn);
  XH_REQUIRE(hemisphere >= 0 && hemisphere <= 2, XH_ERR_ARG, "%s: hemisphere must be 0 (by latitude), 1 (north) or 2 (south)", fn);
  XH_REQUIRE(hemisphere != 0 || lat || !(cni_out || di_out), XH_ERR_ARG, "%s: the hemisphere by cell needs lat", fn);
  if (P == 0 || C == 0) return XH_OK;

  MonArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, month_off, (size_t)M + 1, &a.month_off);
  if (!rc) rc = xh_upload(ctx, &cur, seg_months, (size_t)P + 1, &a.seg_months);
  if (!rc) rc = xh_upload(ctx, &cur, month_cal, (size_t)(M > 0 ? M : 1), &a.month_cal);
  if (!rc) rc = xh_upload(ctx, &cur, month_days, (size_t)(M > 0 ? M : 1), &a.month_days);
  if (rc) return rc;
  a.tasmin = cni_out ? tasmin : nullptr;
  a.tas = mtwm_out ? tas : nullptr;
  a.pr = di_out ? pr : nullptr;
  a.evspsblpot = di_out ? evspsblpot : nullptr;
  a.lat = hemisphere == 0 ? lat : nullptr;
  a.cni_out = cni_out, a.mtwm_out = mtwm_out, a.di_out = di_out, a.valid_out = valid_out;
  a.M = M, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.sub_C = sub_C, a.per_day = per_day, a.wo = wo, a.hemisphere = hemisphere;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_agro_monthly<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_egdd(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tasmin, const void* tasmax, int64_t P,
            const int64_t* seg, const int32_t* doy, const int64_t* start_from, const int64_t* end_from, const int64_t* day0,
            const int32_t* label_doy, const int32_t* label_days, int method, double sub_C, double thresh, double* egdd_out,
            double* start_out, double* end_out, int32_t* valid_out, int64_t ld_out) {
  const char* fn = "xh_egdd";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (!rc) rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  XH_REQUIRE(tasmin && tasmax, XH_ERR_ARG, "%s: NULL field", fn);
  XH_REQUIRE(doy && start_from && end_from && day0 && label_doy && label_days, XH_ERR_ARG, "%s: NULL table", fn);
  XH_REQUIRE(method == 0 || method == 1, XH_ERR_ARG, "%s: method must be 0 (bootsma) or 1 (qian), got %d", fn, method);
  XH_REQUIRE(egdd_out || start_out || end_out, XH_ERR_ARG, "%s: no output requested (egdd_out, start_out or end_out)", fn);
  for (int64_t p = 0; p < P; ++p) {
    XH_REQUIRE(start_from[p] == -1 || (start_from[p] >= seg[p] && start_from[p] < seg[p + 1]), XH_ERR_ARG,
               "%s: start_from[%lld] outside its period", fn, (long long)p);
    XH_REQUIRE(end_from[p] == -1 || (end_from[p] >= seg[p] && end_from[p] < seg[p + 1]), XH_ERR_ARG,
               "%s: end_from[%lld] outside its period", fn, (long long)p);
    XH_REQUIRE(day0[p] >= 0 && day0[p] <= 366 && label_doy[p] >= 1 && label_doy[p] <= 366 && label_days[p] >= 360 && label_days[p] <= 366,
               XH_ERR_ARG, "%s: label of period %lld out of range", fn, (long long)p);
  }
  for (int64_t t = 0; t < T; ++t) XH_REQUIRE(doy[t] >= 1 && doy[t] <= 366, XH_ERR_ARG, "%s: doy[%lld] = %d", fn, (long long)t, doy[t]);
  if (P == 0 || C == 0) return XH_OK;

  EgddArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc) rc = xh_upload(ctx, &cur, doy, (size_t)(T > 0 ? T : 1), &a.doy);
  if (!rc) rc = xh_upload(ctx, &cur, start_from, (size_t)P, &a.start_from);
  if (!rc) rc = xh_upload(ctx, &cur, end_from, (size_t)P, &a.end_from);
  if (!rc) rc = xh_upload(ctx, &cur, day0, (size_t)P, &a.day0);
  if (!rc) rc = xh_upload(ctx, &cur, label_doy, (size_t)P, &a.label_doy);
  if (!rc) rc = xh_upload(ctx, &cur, label_days, (size_t)P, &a.label_days);
  if (rc) return rc;
  a.tasmin = tasmin, a.tasmax = tasmax;
  a.egdd_out = egdd_out, a.start_out = start_out, a.end_out = end_out, a.valid_out = valid_out;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.sub_C = sub_C, a.thresh = thresh, a.method = method;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_egdd<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_corn_heat_units(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tasmin, const void* tasmax,
                       double sub_C, double thresh_tasmin, double thresh_tasmax, double* out, int64_t ld_out) {
  const char* fn = "xh_corn_heat_units";
  const int rc = xh_check_pitched(fn, ctx, T, C, ld, T, ld_out);
  if (rc) return rc;
  XH_REQUIRE(tasmin && tasmax && out, XH_ERR_ARG, "%s: NULL argument", fn);
  if (T == 0 || C == 0) return XH_OK;
  ElemArgs e{tasmin, tasmax, out, T, C, ld, ld_out, sub_C, thresh_tasmin, thresh_tasmax};
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_corn_heat_units<XH_WIDTH(w)>, agro_grid(C, T), dim3(XH_BLOCK), 0, ctx->stream, e); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_qian_wma(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, double* out, int64_t ld_out) {
  const char* fn = "xh_qian_wma";
  const int rc = xh_check_pitched(fn, ctx, T, C, ld, T, ld_out);
  if (rc) return rc;
  XH_REQUIRE(tas && out, XH_ERR_ARG, "%s: NULL argument", fn);
  if (T == 0 || C == 0) return XH_OK;
  ElemArgs e{tas, nullptr, out, T, C, ld, ld_out, 0.0, 0.0, 0.0};
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_qian_wma<XH_WIDTH(w)>, agro_grid(C, T), dim3(XH_BLOCK), 0, ctx->stream, e); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
