// pet.hip — potential evapotranspiration and the water budget (indices/converters.py:1890-2152, 2652-2740).
//
// Solar geometry (indices/helpers.py:60-63, 95-238, 241-525) depends only on (day, latitude): k_solar_table builds a float64
// table (R, L) of the extraterrestrial radiation Ra [J m-2 d-1] and / or the day length [h] over the L distinct latitudes,
// from one day angle per row computed on the host (xarray's decimal year).  Cells carry an int32 index into it.
//
// Daily methods (BR65, HG85, MB05, FAO_PM98) are element-wise: lanes along the cells, rows of a block spread over
// blockIdx.y.  The monthly methods (TW48, DA02) take one lane per cell that marches down the rows of each calendar month
// (NaN-skipping means, as xarray's resample().mean()); TW48 keeps the months of one year in registers for its heat index.
// Arithmetic is float64 in the reference's order after widening the fields; the means of float32 fields are float64 sums
// rounded once to float32 (the convention of stdidx.hip).  Results are kg m-2 s-1 (amount2rate, then the hydro context).
#include "hostargs.h"
#include "pyminmax.h"

#include <cmath>

namespace {

constexpr double PI = 3.141592653589793;  // np.pi

__device__ __forceinline__ double pymod(double a, double b) {  // numpy's float remainder (sign of the divisor)
  double m = fmod(a, b);
  if (m != 0.0 && ((b < 0.0) != (m < 0.0))) m += b;
  return m;
}

// _wrap_radians (helpers.py:60-63)
__device__ __forceinline__ double wrap(double x) { return pymod(x + PI, 2 * PI) - PI; }

// _sunlit_integral_of_cosine_of_solar_zenith_angle (helpers.py:353-397), average = False
__device__ double sunlit_integral(double decl, double lat, double hss, double hs, double he) {
  const double hsr = -hss;
  double num, den;
  const bool nan_ss = isnan(hss);
  if (nan_ss && (decl * lat) > 0) {
    num = sin(he) - sin(hs);
    den = he < hs ? he + 2 * PI - hs : he - hs;
  } else if (nan_ss && (decl * lat) < 0) {
    return 0.0;
  } else if ((hs > hss && he < hsr) || (hs < hsr && he < hsr) || (hs > hss && he > hss)) {
    return 0.0;
  } else if (hs > he && he >= hsr && hs >= hss) {
    num = sin(he) - sin(hsr);
    den = he - hsr;
  } else if (he < hs && hs >= hsr && hsr >= he) {
    num = sin(hss) - sin(hs);
    den = hss - hs;
  } else if (hss >= hs && hs > he && he >= hsr) {
    num = sin(hss) - sin(hs) + sin(he) - sin(hsr);
    den = hss - hs + he - hsr;
  } else {
    const double h1 = pymax(hsr, hs), h2 = pymin(hss, he);
    num = sin(h2) - sin(h1);
    den = h2 - h1;
  }
  return sin(decl) * sin(lat) * den + cos(decl) * cos(lat) * num;
}

// one (row, latitude): Ra = gsc * 86400 / (2 pi) * cosz_integral * dr (helpers.py:400-447), day length (:450-525)
__global__ void __launch_bounds__(XH_BLOCK) k_solar_table(int64_t R, int64_t L, const double* __restrict__ dang,
                                                          const double* __restrict__ lat_deg, double gsc_day,
                                                          double* __restrict__ ra, double* __restrict__ dl) {
  const int64_t i = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (i >= R * L) return;
  const int64_t r = i / L, l = i - r * L;
  const double da = dang[r];
  // solar_declination, spencer (helpers.py:155-163), wrapped
  const double sd = 0.006918 - 0.399912 * cos(da) + 0.070257 * sin(da) - 0.006758 * cos(2 * da) +
                    0.000907 * sin(2 * da) - 0.002697 * cos(3 * da) + 0.001480 * sin(3 * da);
  const double decl = wrap(sd);
  const double latr = lat_deg[l] * (PI / 180);
  if (ra) {
    // eccentricity_correction_factor, spencer (:230-237)
    const double dr = 1.0001100 + 0.034221 * cos(da) + 0.001280 * sin(da) + 0.000719 * cos(2 * da) + 0.000077 * sin(2 * da);
    const double lw = wrap(latr);
    const double tt = -tan(lw) * tan(decl);
    const double hss = fabs(tt) <= 1 ? acos(tt) : xh_nan64();
    const double cz = sunlit_integral(decl, lw, wrap(hss), wrap(-PI), wrap(PI - 1e-9));
    ra[i] = gsc_day * (1 / (2 * PI)) * cz * dr;
  }
  if (dl) dl[i] = (24 / PI) * acos(-tan(latr) * tan(decl));  // NaN in the polar day and night (no infill)
}

// per (month, latitude) from the daily table over whole months: kind 0 = mean of dl / 12 over non-NaN days (TW48),
// kind 1 = sum of Ra in MJ m-2 d-1 times 0.408 (DA02)
__global__ void __launch_bounds__(XH_BLOCK) k_month_table(int64_t M, int64_t L, const double* __restrict__ daily,
                                                          const int64_t* __restrict__ seg, int kind,
                                                          double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (i >= M * L) return;
  const int64_t m = i / L, l = i - m * L;
  double s = 0.0;
  int64_t n = 0;
  for (int64_t d = seg[m]; d < seg[m + 1]; ++d) {
    const double v = daily[d * L + l];
    if (kind == 0) {
      const double h = v / 12;
      if (!isnan(h)) {
        s += h;
        ++n;
      }
    } else {
      const double mj = v * 1e-6;
      if (!isnan(mj)) s += mj;
    }
  }
  out[i] = kind == 0 ? (n ? s / (double)n : xh_nan64()) : s * 0.408;
}

struct PetArgs {
  const void* tn;
  const void* tx;
  const void* tas;  // NULL = (tasmin + tasmax) / 2
  const void* hurs;
  const void* rsds;
  const void* rsus;
  const void* rlds;
  const void* rlus;
  const void* ws;
  const void* pr;
  const double* tab;     // daily: Ra (T, L); monthly: the (M, L) month table
  const int32_t* lidx;   // (C) row of each cell in the table
  const int64_t* seg;    // monthly: rows of each month (M + 1)
  const double* msec;    // monthly: seconds of each month (M)
  double* pet;           // NULL = not written
  double* wb;
  int64_t T, C, L, M, st, st_out;
  double peta, petb, wlog2, wlog10;
  int method, m0;  // m0: month of year (0..11) of the first month
};

enum { BR65 = 0, HG85 = 1, MB05 = 2, FAO = 3, TW48 = 4, DA02 = 5 };

__device__ __forceinline__ double clip0(double x) { return x < 0.0 ? 0.0 : x; }  // np.clip(x, 0, None): NaN stays

// pint's K -> degF: (K - offset) / scale with degF = 5/9 K, offset 233.15 + 200/9
__device__ __forceinline__ double k2f(double k) { return (k - (233.15 + 200.0 / 9)) / (5.0 / 9); }

// _saturation_vapor_pressure_over_water, sonntag90 (converters.py:416-423), T in K, Pa
__device__ __forceinline__ double svp(double t) {
  return 100 * exp(-6096.9385 / t + 16.635794 + -2.711193e-2 * t + 1.673952e-5 * (t * t) + 2.433502 * log(t));
}

template <typename TF>
__global__ void __launch_bounds__(XH_BLOCK) k_pet_daily(PetArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t li = a.method == FAO ? 0 : a.lidx[c];
  for (int64_t t = blockIdx.y; t < a.T; t += gridDim.y) {
    const int64_t i = t * a.st + c;
    double pet;
    if (a.method == BR65) {
      const double tn = k2f(xh_ldw<TF>(a.tn, i)), tx = k2f(xh_ldw<TF>(a.tx, i));
      const double re = a.tab[t * a.L + li] * (1e-4 / 4.184);  // J m-2 d-1 -> cal cm-2 day-1
      pet = clip0(0.094 * (-87.03 + 0.928 * tx + 0.933 * (tx - tn) + 0.0486 * re));
    } else if (a.method == HG85) {
      const double tn = xh_ldw<TF>(a.tn, i) - 273.15, tx = xh_ldw<TF>(a.tx, i) - 273.15;
      const double tm = a.tas ? xh_ldw<TF>(a.tas, i) - 273.15 : (tn + tx) / 2;
      const double ra = a.tab[t * a.L + li] * 1e-6 * 0.408;
      pet = clip0(0.0023 * ra * (tm + 17.8) * sqrt(tx - tn));
    } else if (a.method == MB05) {
      const double tm = a.tas ? xh_ldw<TF>(a.tas, i) - 273.15 : ((xh_ldw<TF>(a.tn, i) - 273.15) + (xh_ldw<TF>(a.tx, i) - 273.15)) / 2;
      const double tk = tm + 273.15;
      const double rl = a.tab[t * a.L + li] / (4185.5 * (751.78 - 0.5655 * tk));
      pet = rl * a.peta * tm + rl * a.petb;
    } else {  // FAO_PM98 (converters.py:2121-2145, fao_allen98 :1867-1874)
      const double tx = xh_ldw<TF>(a.tx, i) - 273.15, tn = xh_ldw<TF>(a.tn, i) - 273.15;
      const double hu = xh_ldw<TF>(a.hurs, i) / 100;
      const double w2 = xh_ldw<TF>(a.ws, i) * a.wlog2 / a.wlog10;
      const double tm = (tx + tn) / 2;
      const double es = (1.0 / 2) * (svp(tx + 273.15) + svp(tn + 273.15)) * 1e-3;
      const double ea = es * hu;
      const double dt = tm + 237.3;
      const double delta = 4098 * es / (dt * dt);
      const double rn = (xh_ldw<TF>(a.rsds, i) - xh_ldw<TF>(a.rsus, i) - (xh_ldw<TF>(a.rlus, i) - xh_ldw<TF>(a.rlds, i))) * 0.0864;
      const double gamma = 0.665e-03 * 101.325;
      const double a1 = 0.408 * delta * (rn - 0.0);
      const double a2 = gamma * 900 / (tm + 273.15) * w2 * (es - ea);
      const double a3 = delta + (gamma * (1 + 0.34 * w2));
      pet = (a1 + a2) / a3;
    }
    const double rate = pet / 86400;  // mm/d -> kg m-2 s-1
    const int64_t o = t * a.st_out + c;
    if (a.pet) a.pet[o] = rate;
    if (a.wb) a.wb[o] = xh_ldw<TF>(a.pr, i) - rate;
  }
}

// NaN-skipping mean of one month; float32 fields round the mean once, as xarray's float32 mean
template <bool F32>
__device__ __forceinline__ double mean_of(double s, int n) {
  const double m = n ? s / (double)n : xh_nan64();
  return F32 ? (double)(float)m : m;
}

template <typename TF>
__global__ void __launch_bounds__(XH_BLOCK) k_pet_monthly(PetArgs a) {
  constexpr bool F32 = sizeof(TF) == 4;
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t li = a.lidx[c];
  int64_t m = 0;
  while (m < a.M) {
    const int nm = (int)(m == 0 ? (12 - a.m0 < a.M ? 12 - a.m0 : a.M) : (a.M - m < 12 ? a.M - m : 12));
    if (a.method == DA02) {
      for (int j = 0; j < nm; ++j) {
        double sn = 0, sx = 0, st = 0, sp = 0, sw = 0;
        int nn = 0, nx = 0, nt = 0, np = 0, nw = 0;
        for (int64_t t = a.seg[m + j]; t < a.seg[m + j + 1]; ++t) {
          const int64_t i = t * a.st + c;
          const double tn = xh_ldw<TF>(a.tn, i) - 273.15, tx = xh_ldw<TF>(a.tx, i) - 273.15, p = xh_ldw<TF>(a.pr, i);
          const double tm = a.tas ? xh_ldw<TF>(a.tas, i) - 273.15 : (tn + tx) / 2;
          const double pm = p * 2629800.0;  // kg m-2 s-1 -> mm/month (pint's month: 365.25 / 12 days)
          if (!isnan(tn)) { sn += tn; ++nn; }
          if (!isnan(tx)) { sx += tx; ++nx; }
          if (!isnan(tm)) { st += tm; ++nt; }
          if (!isnan(pm)) { sp += pm; ++np; }
          if (!isnan(p)) { sw += p; ++nw; }
        }
        const double tnm = mean_of<F32>(sn, nn), txm = mean_of<F32>(sx, nx), tmm = mean_of<F32>(st, nt);
        const double pmm = mean_of<F32>(sp, np);
        double tr = txm - tnm;
        tr = tr > 0 ? tr : 0.0;  // tr.where(tr > 0, 0): NaN -> 0
        const double ab = tr - 0.0123 * pmm;
        const double p76 = pow(ab, 0.76);
        double pet = 0.0013 * a.tab[(m + j) * a.L + li] * (tmm + 17.0) * p76;
        pet = clip0(isnan(p76) ? 0.0 : pet);
        const double rate = pet / a.msec[m + j];
        const int64_t o = (m + j) * a.st_out + c;
        if (a.pet) a.pet[o] = rate;
        if (a.wb) a.wb[o] = mean_of<F32>(sw, nw) - rate;
      }
    } else {  // TW48: the year's monthly means stay in registers (compile-time slots)
      double tmv[12];
      double hi = 0.0;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        tmv[j] = 0.0;
        if (j < nm) {
          double s = 0;
          int n = 0;
          for (int64_t t = a.seg[m + j]; t < a.seg[m + j + 1]; ++t) {
            const int64_t i = t * a.st + c;
            const double tm = clip0(a.tas ? xh_ldw<TF>(a.tas, i) - 273.15
                                          : ((xh_ldw<TF>(a.tn, i) - 273.15) + (xh_ldw<TF>(a.tx, i) - 273.15)) / 2);
            if (!isnan(tm)) { s += tm; ++n; }
          }
          tmv[j] = mean_of<F32>(s, n);
          const double idm = pow(tmv[j] / 5, 1.514);
          if (!isnan(idm)) hi += idm;
        }
      }
      const double ex = 6.75e-7 * pow(hi, 3.0) - 7.71e-5 * (hi * hi) + 0.01791 * hi + 0.49239;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if (j < nm) {
          const double frac = pow(10 * tmv[j] / hi, ex);
          const double pet = 10 * (1.6 * a.tab[(m + j) * a.L + li] * frac);  // mm/month
          const double rate = pet / a.msec[m + j];
          const int64_t o = (m + j) * a.st_out + c;
          if (a.pet) a.pet[o] = rate;
          if (a.wb) {
            double sw = 0;
            int nw = 0;
            for (int64_t t = a.seg[m + j]; t < a.seg[m + j + 1]; ++t) {
              const double p = xh_ldw<TF>(a.pr, t * a.st + c);
              if (!isnan(p)) { sw += p; ++nw; }
            }
            a.wb[o] = mean_of<F32>(sw, nw) - rate;
          }
        }
      }
    }
    m += nm;
  }
}

}  // namespace

int xh_solar_table(xh_ctx* ctx, int64_t R, int64_t L, const double* day_angle, const double* lat_deg,
                   double solar_constant, double* ra_out, double* dl_out) {
  XH_REQUIRE(ctx && day_angle && lat_deg, XH_ERR_ARG, "xh_solar_table: NULL argument");
  XH_REQUIRE(R >= 0 && L >= 0, XH_ERR_ARG, "xh_solar_table: negative shape");
  XH_REQUIRE(ra_out || dl_out, XH_ERR_ARG, "xh_solar_table: no output requested");
  if (R == 0 || L == 0) return XH_OK;
  XH_REQUIRE(R * L < ((int64_t)1 << 40), XH_ERR_LIMIT, "xh_solar_table: table too large");
  const double gsc_day = solar_constant * 86400.0;  // W m-2 -> J m-2 d-1
  hipLaunchKernelGGL(k_solar_table, dim3((unsigned)cdiv64(R * L, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, R, L,
                     day_angle, lat_deg, gsc_day, ra_out, dl_out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_pet_month_table(xh_ctx* ctx, int64_t D, int64_t L, const double* daily, int64_t M, const int64_t* seg, int kind,
                       double* out) {
  XH_REQUIRE(ctx && daily && seg && out, XH_ERR_ARG, "xh_pet_month_table: NULL argument");
  XH_REQUIRE(D >= 0 && L >= 0 && M >= 0, XH_ERR_ARG, "xh_pet_month_table: negative shape");
  XH_REQUIRE(kind == 0 || kind == 1, XH_ERR_ARG, "xh_pet_month_table: kind must be 0 (day length) or 1 (Ra), got %d", kind);
  if (M == 0 || L == 0) return XH_OK;
  XH_REQUIRE(M * L < ((int64_t)1 << 40) && D * L < ((int64_t)1 << 40), XH_ERR_LIMIT, "xh_pet_month_table: table too large");
  hipLaunchKernelGGL(k_month_table, dim3((unsigned)cdiv64(M * L, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, M, L, daily,
                     seg, kind, out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_pet_daily(xh_ctx* ctx, int64_t T, int64_t C, int64_t st, int method, int f64, const void* tasmin,
                 const void* tasmax, const void* tas, const void* hurs, const void* rsds, const void* rsus,
                 const void* rlds, const void* rlus, const void* sfcwind, const void* pr, const double* ra, int64_t L,
                 const int32_t* lat_idx, double peta, double petb, double* pet_out, double* wb_out, int64_t st_out) {
  XH_REQUIRE(ctx, XH_ERR_ARG, "xh_pet_daily: NULL context");
  XH_REQUIRE(T >= 0 && C >= 0 && L >= 0, XH_ERR_ARG, "xh_pet_daily: negative shape");
  XH_REQUIRE(method >= 0 && method <= 3, XH_ERR_ARG, "xh_pet_daily: method must be 0..3 (BR65, HG85, MB05, FAO_PM98), got %d",
             method);
  XH_REQUIRE(st >= C && st_out >= C, XH_ERR_LAYOUT, "xh_pet_daily: needs time-major views (st >= C, st_out >= C)");
  XH_REQUIRE(pet_out || wb_out, XH_ERR_ARG, "xh_pet_daily: no output requested");
  const bool temps = method == MB05 ? (tas || (tasmin && tasmax)) : (tasmin && tasmax);
  XH_REQUIRE(temps && (method == FAO ? (hurs && rsds && rsus && rlds && rlus && sfcwind) : (ra && lat_idx && L > 0)) &&
                 (!wb_out || pr),
             XH_ERR_ARG, "xh_pet_daily: an input needed by the method or the outputs is NULL");
  if (T == 0 || C == 0) return XH_OK;
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40) && T * st_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT,
             "xh_pet_daily: field too large");
  PetArgs a{};
  a.tn = tasmin;
  a.tx = tasmax;
  a.tas = tas;
  a.hurs = hurs;
  a.rsds = rsds;
  a.rsus = rsus;
  a.rlds = rlds;
  a.rlus = rlus;
  a.ws = sfcwind;
  a.pr = pr;
  a.tab = ra;
  a.lidx = lat_idx;
  a.pet = pet_out;
  a.wb = wb_out;
  a.T = T;
  a.C = C;
  a.L = L;
  a.st = st;
  a.st_out = st_out;
  a.peta = peta;
  a.petb = petb;
  a.wlog2 = std::log(67.8 * 2 - 5.42);  // wind_speed_height_conversion 10 m -> 2 m (helpers.py:848), numpy's scalar log
  a.wlog10 = std::log(67.8 * 10 - 5.42);
  a.method = method;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(T < 4096 ? T : 4096));
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_pet_daily<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_pet_monthly(xh_ctx* ctx, int64_t T, int64_t C, int64_t st, int method, int f64, const void* tasmin,
                   const void* tasmax, const void* tas, const void* pr, int64_t M, int first_month, const int64_t* seg,
                   const double* month_table, const double* month_seconds, int64_t L, const int32_t* lat_idx,
                   double* pet_out, double* wb_out, int64_t st_out) {
  XH_REQUIRE(ctx, XH_ERR_ARG, "xh_pet_monthly: NULL context");
  XH_REQUIRE(T >= 0 && C >= 0 && L >= 0 && M >= 0, XH_ERR_ARG, "xh_pet_monthly: negative shape");
  XH_REQUIRE(method == TW48 || method == DA02, XH_ERR_ARG, "xh_pet_monthly: method must be 4 (TW48) or 5 (DA02), got %d",
             method);
  XH_REQUIRE(first_month >= 0 && first_month < 12, XH_ERR_ARG, "xh_pet_monthly: first_month must be 0..11, got %d",
             first_month);
  XH_REQUIRE(st >= C && st_out >= C, XH_ERR_LAYOUT, "xh_pet_monthly: needs time-major views (st >= C, st_out >= C)");
  XH_REQUIRE(pet_out || wb_out, XH_ERR_ARG, "xh_pet_monthly: no output requested");
  const bool temps = method == TW48 ? (tas || (tasmin && tasmax)) : (tasmin && tasmax && pr);
  XH_REQUIRE(temps && seg && month_table && month_seconds && lat_idx && L > 0 && (!wb_out || pr), XH_ERR_ARG,
             "xh_pet_monthly: an input needed by the method or the outputs is NULL");
  if (M == 0 || C == 0) return XH_OK;
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40) && M * st_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT,
             "xh_pet_monthly: field too large");
  PetArgs a{};
  a.tn = tasmin;
  a.tx = tasmax;
  a.tas = tas;
  a.pr = pr;
  a.tab = month_table;
  a.lidx = lat_idx;
  a.seg = seg;
  a.msec = month_seconds;
  a.pet = pet_out;
  a.wb = wb_out;
  a.T = T;
  a.C = C;
  a.L = L;
  a.M = M;
  a.st = st;
  a.st_out = st_out;
  a.method = method;
  a.m0 = first_month;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK));
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_pet_monthly<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
