// ffdi.hip — the McArthur Forest Fire Danger system (indices/fire/_ffdi.py) in one launch.
//
// Reference: the two numba gufuncs _keetch_byram_drought_index (_ffdi.py:38-89) and _griffiths_drought_factor (:92-183),
// and the numpy expression of mcarthur_forest_fire_danger_index (:359-402).  One lane owns one cell and marches down the
// time-major (T, C) fields; any subset of KBDI -> DF -> FFDI runs in the same pass, a stage feeding the next from registers.
//
// Arithmetic is float64 in the reference's evaluation order (the gufuncs widen every input).  Python's min / max keep a
// NaN first argument (pyminmax.h): one NaN rain or temperature day makes the rest of a cell's KBDI NaN, as in numba.
// The DF window of 20 days is 20 registers shifted by one per day, so that the event scan of every day uses compile-time
// indices only (a runtime-indexed register array would live in scratch).  N ** 1.3 comes from a host table (Python's pow).
// FFDI follows numpy on the given dtypes (NEP 50): float32 tasmax / hurs / sfcWind give a float32 exponent with float32
// constants, a float32 DF gives a float32 power; exp / pow are evaluated in float64 and rounded once.
#include "hostargs.h"
#include "pyminmax.h"

namespace {

constexpr int WL = 20;  // the DF window (_ffdi.py:118)

struct FfdiArgs {
  const void* pr;
  const void* tas;
  const void* hurs;
  const void* ws;
  const void* smd;
  const void* df;
  const double* pa;
  const double* k0;  // NULL = 0
  double* out_k;     // NULL = stage not run
  double* out_df;
  double* out_ff;
  int64_t T, C, st, st_out;
  double n13[WL];  // n13[k] = (k + 1) ** 1.3
  int lim;
};

// KBDI of one day (_ffdi.py:67-89); rr and k are carried
__device__ __forceinline__ double kbdi_day(double p, double t, double den, double& rr, double k) {
  double r;
  if (p <= 0.0) {
    r = p;
    rr = 5.0;
  } else {
    r = pymin(p, rr);
    rr -= r;
  }
  const double peff = p - r;
  const double et = 1e-3 * (203.2 - k) * (0.968 * exp(0.0875 * t + 1.5552) - 8.3) / den;
  k += et - peff;
  return pymin(pymax(k, 0.0), 203.2);
}

// DF of the window ending today (_ffdi.py:121-181); w[0] is the oldest day
template <typename TP>
__device__ __forceinline__ double df_day(const TP (&w)[WL], double smd, int lim, const double (&n13)[WL]) {
  bool run = false;  // conseq != 0
  double pmax = 0.0, P = 0.0, x = 1.0, nn = n13[0];  // nn = N ** 1.3 of the current event
#pragma unroll
  for (int iw = 0; iw < WL; ++iw) {
    const double v = (double)w[iw];
    const bool event = v > 2.0;
    if (event) {
      run = true;
      P = P + v;
      if (v >= pmax) {
        nn = n13[WL - 1 - iw];  // N = WL - iw
        pmax = v;
      }
    }
    if ((!event && run) || (event && iw == WL - 1)) {
      const double xe = nn / (nn + P - 2.0);
      x = pymin(xe, x);
      run = false;
      P = 0.0;
      pmax = 0.0;
    }
  }
  if (lim == 0) {
    const double xlim = smd < 20 ? 1 / (1 + 0.1135 * smd) : 75 / (270.525 - 1.267 * smd);
    x = pymin(x, xlim);
  }
  double dfw = 10.5 * (1 - exp(-(smd + 30) / 40)) * (41 * (x * x) + x) / (40 * (x * x) + x + 1);
  if (lim == 1) {
    double dflim;
    if (smd < 25.0) dflim = 6.0;
    else if (smd >= 25.0 && smd < 42.0) dflim = 7.0;
    else if (smd >= 42.0 && smd < 65.0) dflim = 8.0;
    else if (smd >= 65.0 && smd < 100.0) dflim = 9.0;
    else dflim = 10.0;
    dfw = pymin(dfw, dflim);
  }
  return pymin(dfw, 10.0);
}

// FFDI (_ffdi.py:399): df ** 0.987 * exp(0.0338 * tasmax - 0.0345 * hurs + 0.0234 * sfcWind + 0.243147) on numpy's dtypes
template <typename TT, bool DF32>
__device__ __forceinline__ double ffdi_day(double df, TT t, TT h, TT w) {
  double e;
  if constexpr (sizeof(TT) == 4) {
    // numpy rounds the python float constants to float32 (not the decimal literals directly)
    const float s = (float)0.0338 * t - (float)0.0345 * h + (float)0.0234 * w + (float)0.243147;
    e = (double)(float)exp((double)s);
  } else {
    e = exp(0.0338 * t - 0.0345 * h + 0.0234 * w + 0.243147);
  }
  if constexpr (DF32) {
    const float pw = (float)pow(df, (double)(float)0.987);
    if constexpr (sizeof(TT) == 4) return (double)(pw * (float)e);
    else return (double)pw * e;
  } else {
    return pow(df, 0.987) * e;
  }
}

// TP: pr; TT: tasmax, hurs, sfcWind; TS: smd and the DF input
template <typename TP, typename TT, typename TS>
__global__ void __launch_bounds__(XH_BLOCK) k_mcarthur(FfdiArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const bool do_k = a.out_k != nullptr, do_d = a.out_df != nullptr, do_f = a.out_ff != nullptr;
  const bool need_p = do_k || do_d, need_t = do_k || do_f;
  const double nan = xh_nan64();

  double den = 1.0, k = 0.0, rr = 5.0;
  if (do_k) {
    den = 1 + 10.88 * exp(-0.00173 * a.pa[c]);  // per cell: the same operations as the daily expression
    k = a.k0 ? a.k0[c] : 0.0;
  }
  TP w[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) w[i] = (TP)0;

  for (int64_t t = 0; t < a.T; ++t) {
    const int64_t ro = t * a.st + c, oo = t * a.st_out + c;
    const TP pv = need_p ? xh_ld<TP>(a.pr, ro) : (TP)0;
    const TT tv = need_t ? xh_ld<TT>(a.tas, ro) : (TT)0;
    if (do_k) {
      k = kbdi_day((double)pv, (double)tv, den, rr, k);
      a.out_k[oo] = k;
    }
    double dfv = nan;
    if (do_d) {
#pragma unroll
      for (int i = 0; i < WL - 1; ++i) w[i] = w[i + 1];
      w[WL - 1] = pv;
      if (t >= WL - 1) dfv = df_day(w, do_k ? k : (double)xh_ld<TS>(a.smd, ro), a.lim, a.n13);
      a.out_df[oo] = dfv;
    }
    if (do_f) {
      const TT hv = xh_ld<TT>(a.hurs, ro), wv = xh_ld<TT>(a.ws, ro);
      double f;
      if (!do_d && sizeof(TS) == 4) f = ffdi_day<TT, true>((double)xh_ld<TS>(a.df, ro), tv, hv, wv);
      else f = ffdi_day<TT, false>(do_d ? dfv : (double)xh_ld<TS>(a.df, ro), tv, hv, wv);
      a.out_ff[oo] = f;
    }
  }
}

}  // namespace

int xh_mcarthur(xh_ctx* ctx, int64_t T, int64_t C, int64_t st, int pr_f64, int tas_f64, int smd_f64, const void* pr,
                const void* tasmax, const void* hurs, const void* sfcwind, const void* smd, const void* df,
                const double* pr_annual, const double* kbdi0, int lim, const double* n13, double* kbdi_out,
                double* df_out, double* ffdi_out, int64_t st_out) {
  XH_REQUIRE(ctx && n13, XH_ERR_ARG, "xh_mcarthur: NULL argument");
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "xh_mcarthur: negative shape");
  XH_REQUIRE(st >= C && st_out >= C, XH_ERR_LAYOUT, "xh_mcarthur: needs time-major views (st >= C, st_out >= C)");
  XH_REQUIRE(kbdi_out || df_out || ffdi_out, XH_ERR_ARG, "xh_mcarthur: no output requested");
  XH_REQUIRE(lim == 0 || lim == 1, XH_ERR_ARG, "xh_mcarthur: lim must be 0 (xlim) or 1 (discrete), got %d", lim);
  const bool k = kbdi_out, d = df_out, f = ffdi_out;
  XH_REQUIRE((!(k || d) || pr) && (!(k || f) || tasmax) && (!k || pr_annual) && (!(d && !k) || smd) &&
                 (!f || (hurs && sfcwind)) && (!(f && !d) || df),
             XH_ERR_ARG, "xh_mcarthur: an input needed by the requested outputs is NULL");
  if (T == 0 || C == 0) return XH_OK;
  XH_REQUIRE(T * st + C < ((int64_t)1 << 40) && T * st_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT,
             "xh_mcarthur: field too large");

  FfdiArgs a{};
  a.pr = pr;
  a.tas = tasmax;
  a.hurs = hurs;
  a.ws = sfcwind;
  a.smd = smd;
  a.df = df;
  a.pa = pr_annual;
  a.k0 = kbdi0;
  a.out_k = kbdi_out;
  a.out_df = df_out;
  a.out_ff = ffdi_out;
  a.T = T;
  a.C = C;
  a.st = st;
  a.st_out = st_out;
  for (int i = 0; i < WL; ++i) a.n13[i] = n13[i];
  a.lim = lim;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK));
  xh_by_width(pr_f64, [&](auto wp) {
    xh_by_width(tas_f64, [&](auto wt) {
      xh_by_width(smd_f64, [&](auto ws) {
        hipLaunchKernelGGL((k_mcarthur<XH_WIDTH(wp), XH_WIDTH(wt), XH_WIDTH(ws)>), g, dim3(XH_BLOCK), 0, ctx->stream, a);
      });
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
