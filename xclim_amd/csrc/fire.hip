// fire.hip — the Canadian Forest Fire Weather Index System (indices/fire/_cffwis.py) in one launch.
//
// Reference: _fire_weather_calc (_cffwis.py:655-880), the three moisture codes (:245-430), the four numpy indices
// (:435-527), _overwintering_drought_code (:530-568) and _fire_season (:570-652).  The reference loops over days in
// Python and calls a grid-wide ufunc per code per day; here one lane owns one cell, marches down the time-major (T, C)
// fields and keeps every piece of state (the three previous codes, the overwintering / dry-start carries, the season
// mask of the previous day and the season-window counters) in registers.
//
// Arithmetic follows the reference's dtypes on float32 fields:
//   * DC, DMC, FFMC and the overwintered DC are numba ufuncs: the float32 inputs are widened by the float64 literals, the
//     day's code is computed in float64, stored into the float32 output and the STORED value is the next day's start.
//   * ISI, BUI, FWI, DSR are numpy expressions on float32 arrays with python float constants (NEP 50: float32 arithmetic,
//     the constants rounded to float32).  Basic operations are float32 here too; exp / log / pow are evaluated in
//     float64 and rounded once (a correctly rounded float32 result in practice).
//   * Season thresholds and the dry-start precipitation threshold are numpy compares of float32 arrays against python
//     floats, i.e. float32 compares: the host passes them rounded to float32.
//   * The GFWED season means are numpy float32 means: a float32 sum in order, then a float32 divide (windows <= 7).
// Python's max / min (`max(a, b)` keeps a unless b > a) are kept as written: they propagate a NaN first argument.
#include "common.h"
#include "pyminmax.h"

namespace {

constexpr int GFWED_MAXWIN = 7;  // numpy sums windows shorter than 8 in order (pairwise summation beyond)

// Effective day length (hours) per month for the five latitude bands of the GFWED / cffdrs tables (Van Wagner 1987,
// Lawson & Armitage 2008): rows = month 1..12, columns = band 90S-30S, 30S-15S, 15S-15N, 15N-30N, 30N-90N.
__constant__ double c_day_length[12][5] = {
    {11.5, 10.1, 9.0, 7.9, 6.5},  {10.5, 9.6, 9.0, 8.4, 7.5},   {9.2, 9.1, 9.0, 8.9, 9.0},    {7.9, 8.5, 9.0, 9.5, 12.8},
    {6.8, 8.1, 9.0, 9.9, 13.9},   {6.2, 7.8, 9.0, 10.2, 13.9},  {6.5, 7.9, 9.0, 10.1, 12.4},  {7.4, 8.3, 9.0, 9.7, 10.9},
    {8.7, 8.9, 9.0, 9.1, 9.4},    {10.0, 9.4, 9.0, 8.6, 8.0},   {11.2, 9.9, 9.0, 8.1, 7.0},   {11.8, 10.2, 9.0, 7.8, 6.0}};
// Day-length adjustment of the drought code per month, three bands: 90S-15S, 15S-15N, 15N-90N.
__constant__ double c_day_length_factor[12][3] = {
    {6.4, 1.39, -1.6}, {5.0, 1.39, -1.6}, {2.4, 1.39, -1.6}, {0.4, 1.39, 0.9},  {-1.6, 1.39, 3.8}, {-1.6, 1.39, 5.8},
    {-1.6, 1.39, 6.4}, {-1.6, 1.39, 5.0}, {-1.6, 1.39, 2.4}, {0.9, 1.39, 0.4},  {3.8, 1.39, -1.6}, {5.8, 1.39, -1.6}};

__device__ __forceinline__ float f32exp(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float f32log(float x) { return (float)log((double)x); }
__device__ __forceinline__ float f32pow(float a, float b) { return (float)pow((double)a, (double)b); }
__device__ __forceinline__ bool isnan64(double x) { return x != x; }
__device__ __forceinline__ bool isnan32(float x) { return x != x; }

// Latitude bands of the two tables; -1 outside [-90, 90] (and for NaN), where the reference raises ValueError.
__device__ __forceinline__ int band5(double lat) {
  if (-30.0 > lat && lat >= -90.0) return 0;
  if (-15.0 > lat && lat >= -30.0) return 1;
  if (15.0 > lat && lat >= -15.0) return 2;
  if (30.0 > lat && lat >= 15.0) return 3;
  if (90.0 >= lat && lat >= 30.0) return 4;
  return -1;
}
__device__ __forceinline__ int band3(double lat) {
  if (-15.0 > lat && lat >= -90.0) return 0;
  if (15.0 > lat && lat >= -15.0) return 1;
  if (90.0 >= lat && lat >= 15.0) return 2;
  return -1;
}

// ---- the moisture codes, float64 (numba ufuncs of the reference) ------------------------------------------------
__device__ double ffmc_day(double t, double p, double w, double h, double ffmc0) {
  double mo = (147.2 * (101.0 - ffmc0)) / (59.5 + ffmc0);  // Eq. 1
  if (p > 0.5) {
    const double rf = p - 0.5;  // Eq. 2
    const double wet = 42.5 * rf * exp(-100.0 / (251.0 - mo)) * (1.0 - exp(-6.93 / rf));
    if (mo > 150.0)
      mo = (mo + wet) + (0.0015 * ((mo - 150.0) * (mo - 150.0))) * sqrt(rf);  // Eq. 3b
    else if (mo <= 150.0)
      mo = mo + wet;  // Eq. 3a
    mo = pymin(mo, 250.0);
  }
  const double e1 = exp((h - 100.0) / 10.0);
  const double dry = 0.18 * (21.1 - t) * (1.0 - 1.0 / exp(0.115 * h));
  const double ed = 0.942 * pow(h, 0.679) + (11.0 * e1) + dry;  // Eq. 4
  double m;
  if (mo < ed) {
    const double ew = 0.618 * pow(h, 0.753) + (10.0 * e1) + dry;  // Eq. 5
    if (mo < ew) {
      const double r = (100.0 - h) / 100.0;
      const double kl = 0.424 * (1.0 - pow(r, 1.7)) + (0.0694 * sqrt(w)) * (1.0 - pow(r, 8.0));  // Eq. 7a
      const double kw = kl * (0.581 * exp(0.0365 * t));                                       // Eq. 7b
      m = ew - (ew - mo) / pow(10.0, kw);                                                     // Eq. 9
    } else {
      m = mo;  // (mo == ew raises in the reference; both branches give mo there)
    }
  } else if (mo == ed) {
    m = mo;
  } else {
    const double r = h / 100.0;
    const double kl = 0.424 * (1.0 - pow(r, 1.7)) + (0.0694 * sqrt(w)) * (1.0 - pow(r, 8.0));  // Eq. 6a
    const double kw = kl * (0.581 * exp(0.0365 * t));                                       // Eq. 6b
    m = ed + (mo - ed) / pow(10.0, kw);                                                     // Eq. 8
  }
  double ffmc = (59.5 * (250.0 - m)) / (147.2 + m);  // Eq. 10
  if (ffmc > 101.0) ffmc = 101.0;
  else if (ffmc <= 0.0) ffmc = 0.0;
  return ffmc;
}

__device__ double dmc_day(double t, double p, double h, double dl, double dmc0) {
  if (isnan64(dmc0)) return dmc0;
  const double rk = t < -1.1 ? 0.0 : 1.894 * (t + 1.1) * (100.0 - h) * dl * 0.0001;  // Eqs. 16, 17
  double pr;
  if (p > 1.5) {
    const double rw = 0.92 * p - 1.27;                  // Eq. 11
    const double wmi = 20.0 + 280.0 / exp(0.023 * dmc0);  // Eq. 12 (cffdrs form)
    double b;
    if (dmc0 <= 33.0) b = 100.0 / (0.5 + 0.3 * dmc0);  // Eq. 13a
    else if (dmc0 <= 65.0) b = 14.0 - 1.3 * log(dmc0);  // Eq. 13b
    else b = 6.2 * log(dmc0) - 17.2;                    // Eq. 13c
    const double wmr = wmi + (1000.0 * rw) / (48.77 + b * rw);  // Eq. 14
    pr = 43.43 * (5.6348 - log(wmr - 20.0));                     // Eq. 15 (cffdrs form)
  } else {
    pr = dmc0;
  }
  pr = pymax(pr, 0.0);
  return pymax(pr + rk, 0.0);
}

__device__ double dc_day(double t, double p, double fl, double dc0) {
  t = pymax(t, -2.8);
  double pe = (0.36 * (t + 2.8) + fl) / 2.0;  // Eq. 22
  pe = pymax(pe, 0.0);
  if (p > 2.8) {
    const double rw = 0.83 * p - 1.27;                                // Eq. 18
    const double smi = 800.0 * exp(-dc0 / 400.0);                      // Eq. 19
    const double dr = dc0 - 400.0 * log(1.0 + ((3.937 * rw) / smi));  // Eqs. 20, 21
    if (dr > 0.0) return dr + pe;
    if (isnan64(dc0)) return dc0;
    return pe;
  }
  return dc0 + pe;
}

// ---- the numpy indices, float32 ---------------------------------------------------------------------------------
__device__ float isi_day(float ws, float ffmc) {
  const float mo = (147.2f * (101.0f - ffmc)) / (59.5f + ffmc);                                    // Eq. 1
  const float ff = (19.1152f * f32exp(mo * -0.1386f)) * (1.0f + f32pow(mo, 5.31f) / 49300000.0f);  // Eq. 25
  return ff * f32exp(0.05039f * ws);                                                               // Eq. 26
}

__device__ float bui_day(float dmc, float dc) {
  if (dmc == 0.0f && dc == 0.0f) return 0.0f;
  const float denom = dmc + 0.4f * dc;
  float bui;
  if (dmc <= 0.4f * dc) bui = ((0.8f * dc) * dmc) / denom;                                         // Eq. 27a
  else bui = dmc - (1.0f - (0.8f * dc) / denom) * (0.92f + f32pow(0.0114f * dmc, 1.7f));           // Eq. 27b
  return bui < 0.0f ? 0.0f : bui;  // np.clip(bui, 0, None) keeps NaN
}

__device__ float fwi_day(float isi, float bui) {
  float fwi;
  if (bui <= 80.0f) fwi = (0.1f * isi) * (0.626f * f32pow(bui, 0.809f) + 2.0f);                   // Eq. 28a
  else fwi = (0.1f * isi) * (1000.0f / (25.0f + 108.64f / f32exp(0.023f * bui)));                   // Eq. 28b
  if (fwi > 1.0f) fwi = f32exp(2.72f * f32pow(0.434f * f32log(fwi), 0.647f));                      // Eq. 30b
  return fwi;
}

__device__ __forceinline__ float dsr_day(float fwi) { return 0.0272f * f32pow(fwi, 1.77f); }

__device__ __forceinline__ double overwinter_dc(double dcf, double wpr, double a, double b, double min_dc) {
  if (isnan64(dcf) || isnan64(wpr)) return xh_nan64();
  const double qf = 800.0 * exp(-dcf / 400.0);
  const double qs = a * qf + b * (3.94 * wpr);
  return pymax(400.0 * log(800.0 / qs), min_dc);
}

struct FireArgs {
  const float* tas;
  const float* pr;
  const float* hurs;
  const float* ws;
  const float* snd;
  const uint8_t* mask;  // season_mask input (mode XH_FIRE_SEASON_MASK)
  const int32_t* month;  // (T) 1..12
  const double* lat;
  const float* dc0;  // (C), NULL = all NaN
  const float* dmc0;
  const float* ffmc0;
  const float* wpr0;
  float* out[7];  // DC DMC FFMC ISI BUI FWI DSR, NULL = not requested
  uint8_t* mask_out;
  float* wpr_out;
  int* err;
  int64_t T, C, st, st_mask, st_out;
  double p[XH_FIRE_NPARAM];
  int season, ndays_t, ndays_s, overwinter, dry, initial_start_up;
};

__global__ void __launch_bounds__(XH_BLOCK) k_fire_weather(FireArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const bool do_dc = a.out[0] != nullptr, do_dmc = a.out[1] != nullptr, do_ffmc = a.out[2] != nullptr;
  const bool do_isi = a.out[3] != nullptr, do_bui = a.out[4] != nullptr, do_fwi = a.out[5] != nullptr, do_dsr = a.out[6] != nullptr;
  const bool ow = a.overwinter && do_dc;
  const int season = a.season;
  const bool need_pr = do_dc || do_dmc || do_ffmc || a.dry;
  const bool need_tas = do_dc || do_dmc || do_ffmc || season >= XH_FIRE_SEASON_WF93;
  const bool need_snd = season == XH_FIRE_SEASON_LA08 || season == XH_FIRE_SEASON_GFWED;
  const bool need_h = do_dmc || do_ffmc;
  const bool need_w = do_ffmc || do_isi;

  const float dc_start = (float)a.p[XH_FIRE_DC_START], dmc_start = (float)a.p[XH_FIRE_DMC_START];
  const float ffmc_start = (float)a.p[XH_FIRE_FFMC_START];
  const float ts = (float)a.p[XH_FIRE_TEMP_START], te = (float)a.p[XH_FIRE_TEMP_END], sthr = (float)a.p[XH_FIRE_SNOW];
  const float pthr = (float)a.p[XH_FIRE_PREC];
  const float dcf = (float)a.p[XH_FIRE_DC_DRY], dmcf = (float)a.p[XH_FIRE_DMC_DRY];

  const double lat = a.lat ? a.lat[c] : 0.0;
  const int b5 = band5(lat), b3 = band3(lat);
  bool bad_lat = false;

  const float nan = xh_nan32();
  const float dc_in = a.dc0 ? a.dc0[c] : nan, dmc_in = a.dmc0 ? a.dmc0[c] : nan, ffmc_in = a.ffmc0 ? a.ffmc0[c] : nan;
  float dc_p = dc_in, dmc_p = dmc_in, ffmc_p = ffmc_in;
  if (season == XH_FIRE_SEASON_NONE) {
    if (isnan32(dc_p)) dc_p = dc_start;
    if (isnan32(dmc_p)) dmc_p = dmc_start;
    if (isnan32(ffmc_p)) ffmc_p = ffmc_start;
  }
  float ow_dc = dc_in, ow_dmc = dmc_in;
  if (ow) dc_p = nan;
  if (a.dry) {
    if (!a.overwinter) ow_dc = isnan32(dc_in) ? dc_start : dc_in;
    ow_dmc = isnan32(dmc_in) ? dmc_start : dmc_in;
  }
  float wpr = a.wpr0 ? a.wpr0[c] : 0.0f;

  // season state
  const int N = a.ndays_t, S = a.ndays_s;
  const int64_t t_first = season == XH_FIRE_SEASON_WF93 ? (int64_t)N + 1 : (int64_t)(N > S ? N : S);
  int run_hi = 0, run_lo = 0, run_snow = 0;  // consecutive days tas > ts / tas < te / snd <= sthr
  float ht[GFWED_MAXWIN], hs[GFWED_MAXWIN];
#pragma unroll
  for (int k = 0; k < GFWED_MAXWIN; ++k) ht[k] = hs[k] = 0.0f;
  bool m_prev = false;

  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t ro = t * a.st + c;
    const float tv = need_tas ? a.tas[ro] : 0.0f;
    const float pv = need_pr ? a.pr[ro] : 0.0f;
    const float hv = need_h ? a.hurs[ro] : 0.0f;
    const float wv = need_w ? a.ws[ro] : 0.0f;
    const float sv = need_snd ? a.snd[ro] : 0.0f;
    const int mth = a.month[t] - 1;

    if (season != XH_FIRE_SEASON_NONE) {
      bool m;
      if (season == XH_FIRE_SEASON_MASK) {
        m = a.mask[t * a.st_mask + c] != 0;
      } else {
        bool su, sd;
        if (season == XH_FIRE_SEASON_WF93) {  // the N days BEFORE today
          su = run_hi >= N;
          sd = run_lo >= N;
          run_hi = tv > ts ? min(run_hi + 1, 1 << 30) : 0;
          run_lo = tv < te ? min(run_lo + 1, 1 << 30) : 0;
        } else if (season == XH_FIRE_SEASON_LA08) {  // the days up to and including today
          run_snow = sv <= sthr ? min(run_snow + 1, 1 << 30) : 0;
          run_lo = tv < te ? min(run_lo + 1, 1 << 30) : 0;
          su = run_snow >= S;
          sd = sv > sthr || run_lo >= N;
        } else {  // GFWED: float32 means of the last N temperatures / S snow depths, today included
#pragma unroll
          for (int k = 0; k < GFWED_MAXWIN - 1; ++k) {
            ht[k] = ht[k + 1];
            hs[k] = hs[k + 1];
          }
          ht[GFWED_MAXWIN - 1] = tv;
          hs[GFWED_MAXWIN - 1] = sv;
          float st_ = 0.0f, ss_ = 0.0f;
#pragma unroll
          for (int k = 0; k < GFWED_MAXWIN; ++k) {
            if (k >= GFWED_MAXWIN - N) st_ += ht[k];
            if (k >= GFWED_MAXWIN - S) ss_ += hs[k];
          }
          const float mtemp = st_ / (float)N, msnow = ss_ / (float)S;
          su = mtemp > ts && msnow < sthr;
          sd = msnow >= sthr || mtemp < te;
        }
        m = t >= t_first ? ((m_prev || su) && !sd) : false;
      }
      if (a.mask_out) a.mask_out[t * a.st_out + c] = m ? 1 : 0;
      const int delta = t == 0 ? (a.initial_start_up ? (int)m : 0) : (int)m - (int)m_prev;
      const bool shut_down = delta == -1, winter = delta == 0 && !m, start_up = delta == 1;
      m_prev = m;
      const bool wet = pv > pthr;
      if (do_dc) {
        if (a.overwinter) {
          if (shut_down) {
            ow_dc = dc_p;
            wpr = pv;
          }
          if (winter) wpr = wpr + pv;
          if (start_up) {
            dc_p = isnan32(ow_dc) ? dc_start
                                  : (float)overwinter_dc(ow_dc, wpr, a.p[XH_FIRE_CARRY_OVER], a.p[XH_FIRE_WETTING_EFF],
                                                         a.p[XH_FIRE_DC_START]);
            ow_dc = nan;
            wpr = nan;
          }
        } else if (a.dry) {
          if (shut_down) ow_dc = dc_start;
          if (a.dry == XH_FIRE_DRY_GFWED) {
            if (start_up || winter) ow_dc = wet ? 0.0f : ow_dc + dcf;
          } else if (winter) {
            ow_dc = wet ? dc_start : ow_dc + dcf;
          }
          if (start_up) {
            dc_p = ow_dc;
            ow_dc = nan;
          }
        } else if (start_up) {
          dc_p = dc_start;
        }
        if (shut_down) dc_p = nan;
      }
      if (do_dmc) {
        if (a.dry) {
          if (shut_down) ow_dmc = dmc_start;
          if (a.dry == XH_FIRE_DRY_GFWED) {
            if (start_up || winter) ow_dmc = wet ? 0.0f : ow_dmc + dmcf;
          } else if (winter) {
            ow_dmc = wet ? dmc_start : ow_dmc + dmcf;
          }
          if (start_up) {
            dmc_p = ow_dmc;
            ow_dmc = nan;
          }
        } else if (start_up) {
          dmc_p = dmc_start;
        }
        if (shut_down) dmc_p = nan;
      }
      if (do_ffmc) {
        if (start_up) ffmc_p = ffmc_start;
        if (shut_down) ffmc_p = nan;
      }
    }

    const int64_t oo = t * a.st_out + c;
    float dc = nan, dmc = nan, ffmc = nan, isi = nan, bui = nan, fwi = nan;
    if (do_dc) {
      bad_lat |= b3 < 0;
      const double fl = b3 < 0 ? (double)nan : c_day_length_factor[mth][b3];
      dc = (float)dc_day((double)tv, (double)pv, fl, (double)dc_p);
      a.out[0][oo] = dc;
      dc_p = dc;
    }
    if (do_dmc) {
      bad_lat |= b5 < 0 && !isnan32(dmc_p);
      const double dl = b5 < 0 ? (double)nan : c_day_length[mth][b5];
      dmc = (float)dmc_day((double)tv, (double)pv, (double)hv, dl, (double)dmc_p);
      a.out[1][oo] = dmc;
      dmc_p = dmc;
    }
    if (do_ffmc) {
      ffmc = (float)ffmc_day((double)tv, (double)pv, (double)wv, (double)hv, (double)ffmc_p);
      a.out[2][oo] = ffmc;
      ffmc_p = ffmc;
    }
    if (do_isi) {
      isi = isi_day(wv, ffmc);
      a.out[3][oo] = isi;
    }
    if (do_bui) {
      bui = bui_day(dmc, dc);
      a.out[4][oo] = bui;
    }
    if (do_fwi) {
      fwi = fwi_day(isi, bui);
      a.out[5][oo] = fwi;
    }
    if (do_dsr) a.out[6][oo] = dsr_day(fwi);
  }
  if (a.wpr_out) a.wpr_out[c] = wpr;
  if (bad_lat) atomicOr(a.err, 1);
}

__global__ void __launch_bounds__(XH_BLOCK)
k_overwintering_dc(const float* __restrict__ last_dc, const float* __restrict__ wpr, int64_t n, double ca, double wb,
                   double min_dc, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (i < n) out[i] = (float)overwinter_dc((double)last_dc[i], (double)wpr[i], ca, wb, min_dc);
}

}  // namespace

int xh_fire_weather(xh_ctx* ctx, int64_t T, int64_t C, int64_t st, const float* tas, const float* pr, const float* hurs,
                    const float* sfcwind, const float* snd, const int32_t* month, const double* lat, const float* dc0,
                    const float* dmc0, const float* ffmc0, const float* winter_pr, const uint8_t* season_mask,
                    int64_t st_mask, int season_method, int temp_condition_days, int snow_condition_days, int overwintering,
                    int dry_start, int initial_start_up, const double* params, float* const* outputs, int64_t st_out,
                    uint8_t* season_mask_out, float* winter_pr_out) {
  XH_REQUIRE(ctx && params && outputs, XH_ERR_ARG, "xh_fire_weather: NULL argument");
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "xh_fire_weather: negative shape");
  XH_REQUIRE(st >= C && st_out >= C, XH_ERR_LAYOUT, "xh_fire_weather: needs time-major views (st >= C, st_out >= C)");
  XH_REQUIRE(season_method >= XH_FIRE_SEASON_NONE && season_method <= XH_FIRE_SEASON_GFWED, XH_ERR_ARG,
             "xh_fire_weather: unknown season method %d", season_method);
  XH_REQUIRE(dry_start >= XH_FIRE_DRY_NONE && dry_start <= XH_FIRE_DRY_GFWED_SNOW, XH_ERR_ARG,
             "xh_fire_weather: unknown dry start %d", dry_start);
  if (dry_start == XH_FIRE_DRY_GFWED_SNOW) return XH_ERR_NOTIMPL;  // the 60-day snow-cover window is not implemented
  XH_REQUIRE(temp_condition_days >= 0 && snow_condition_days >= 0, XH_ERR_ARG,
             "xh_fire_weather: negative condition days");
  if (season_method == XH_FIRE_SEASON_GFWED && (temp_condition_days > GFWED_MAXWIN || snow_condition_days > GFWED_MAXWIN))
    return XH_ERR_NOTIMPL;  // numpy's pairwise summation of longer windows is not reproduced
  XH_REQUIRE(!overwintering || season_method != XH_FIRE_SEASON_NONE, XH_ERR_ARG,
             "xh_fire_weather: overwintering needs a season method or mask");
  const bool dc = outputs[0], dmc = outputs[1], ffmc = outputs[2], isi = outputs[3], bui = outputs[4], fwi = outputs[5],
             dsr = outputs[6];
  XH_REQUIRE((!isi || ffmc) && (!bui || (dc && dmc)) && (!fwi || (isi && bui)) && (!dsr || fwi), XH_ERR_ARG,
             "xh_fire_weather: an index needs the codes it is computed from (ISI <- FFMC, BUI <- DC + DMC, FWI <- ISI + "
             "BUI, DSR <- FWI)");
  const bool need_tas = dc || dmc || ffmc || season_method >= XH_FIRE_SEASON_WF93;
  const bool need_snd = season_method == XH_FIRE_SEASON_LA08 || season_method == XH_FIRE_SEASON_GFWED;
  XH_REQUIRE((!need_tas || tas) && (!(dc || dmc || ffmc || dry_start) || pr) && (!(dmc || ffmc) || hurs) &&
                 (!(ffmc || isi) || sfcwind) && (!need_snd || snd) && (!(dc || dmc) || (month && lat)),
             XH_ERR_ARG, "xh_fire_weather: an input needed by the requested outputs is NULL");
  XH_REQUIRE(season_method != XH_FIRE_SEASON_MASK || season_mask, XH_ERR_ARG, "xh_fire_weather: season mode 'mask' needs the mask");
  XH_REQUIRE(season_method != XH_FIRE_SEASON_MASK || st_mask >= C, XH_ERR_LAYOUT,
             "xh_fire_weather: the season mask needs time-major rows (st_mask >= C)");
  XH_REQUIRE(!season_mask_out || season_method != XH_FIRE_SEASON_NONE, XH_ERR_ARG,
             "xh_fire_weather: no season mask without a season method");
  if (T == 0 || C == 0) {
    if (winter_pr_out && C > 0) {
      if (winter_pr) XH_CHECK_HIP(hipMemcpyAsync(winter_pr_out, winter_pr, (size_t)C * 4, hipMemcpyDeviceToDevice, ctx->stream));
      else XH_CHECK_HIP(hipMemsetAsync(winter_pr_out, 0, (size_t)C * 4, ctx->stream));
    }
    return XH_OK;
  }
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "xh_fire_weather: field too large");

  FireArgs a{};
  a.tas = tas;
  a.pr = pr;
  a.hurs = hurs;
  a.ws = sfcwind;
  a.snd = snd;
  a.mask = season_mask;
  a.dc0 = dc0;
  a.dmc0 = dmc0;
  a.ffmc0 = ffmc0;
  a.wpr0 = winter_pr;
  for (int k = 0; k < 7; ++k) a.out[k] = outputs[k];
  a.mask_out = season_mask_out;
  a.wpr_out = winter_pr_out;
  a.T = T;
  a.C = C;
  a.st = st;
  a.st_mask = st_mask;
  a.st_out = st_out;
  for (int k = 0; k < XH_FIRE_NPARAM; ++k) a.p[k] = params[k];
  a.season = season_method;
  a.ndays_t = temp_condition_days;
  a.ndays_s = snow_condition_days;
  a.overwinter = overwintering != 0;
  a.dry = dry_start;
  a.initial_start_up = initial_start_up != 0;

  // the month of every row and the latitude-error word go through the scratch ring
  size_t cur = 0;
  void* d = nullptr;
  int32_t* mt = (int32_t*)malloc(sizeof(int32_t) * (size_t)T);
  XH_REQUIRE(mt, XH_ERR_HIP, "xh_fire_weather: out of host memory");
  for (int64_t t = 0; t < T; ++t) {
    const int32_t m = month ? month[t] : 1;
    if (m < 1 || m > 12) {
      free(mt);
      xh_set_error("xh_fire_weather: month[%lld] = %d outside 1..12", (long long)t, (int)m);
      return XH_ERR_ARG;
    }
    mt[t] = m;
  }
  int rc = xh_scratch_upload(ctx, &cur, mt, sizeof(int32_t) * (size_t)T, &d);
  free(mt);
  if (rc) return rc;
  a.month = (const int32_t*)d;
  const int zero = 0;
  rc = xh_scratch_upload(ctx, &cur, &zero, sizeof(int), &d);
  if (rc) return rc;
  a.err = (int*)d;
  // a latitude is only read by DC / DMC
  XH_REQUIRE(lat || !(dc || dmc), XH_ERR_ARG, "xh_fire_weather: lat NULL");
  a.lat = lat;

  hipLaunchKernelGGL(k_fire_weather, dim3((unsigned)cdiv64(C, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  if (dc || dmc) {
    int err = 0;
    XH_CHECK_HIP(hipMemcpyAsync(&err, a.err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    XH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    XH_REQUIRE(err == 0, XH_ERR_ARG, "Invalid lat specified.");
  }
  return XH_OK;
}

int xh_overwintering_dc(xh_ctx* ctx, const float* last_dc, const float* winter_pr, int64_t n, double carry_over_fraction,
                        double wetting_efficiency_fraction, double min_dc, float* out) {
  XH_REQUIRE(ctx && last_dc && winter_pr && out, XH_ERR_ARG, "xh_overwintering_dc: NULL argument");
  XH_REQUIRE(n >= 0, XH_ERR_ARG, "xh_overwintering_dc: negative size");
  if (n == 0) return XH_OK;
  hipLaunchKernelGGL(k_overwintering_dc, dim3((unsigned)cdiv64(n, XH_BLOCK)), dim3(XH_BLOCK), 0, ctx->stream, last_dc, winter_pr,
                     n, carry_over_fraction, wetting_efficiency_fraction, min_dc, out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}
