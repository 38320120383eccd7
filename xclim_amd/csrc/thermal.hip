// thermal.hip — saturation vapour pressure, and UTCI with the mean radiant temperature and the cosine of the solar zenith angle
// (indices/converters.py:390-603, 2155-2635; indices/helpers.py:60-397).  C ABI: include/units/xclim_hip_thermal.h.
//
// k_thermal is element-wise with the shape of k_pet_daily: lanes along the cells, the rows of a block spread over blockIdx.y.  A
// lane keeps sin, cos and tan of its latitude and its longitude in registers across its rows; what depends on the row alone
// (declination, UTC hour angle, interval, time correction, sun distance) is a float64 table built on the host and read with
// wave-uniform addresses.  Per sample, in registers: the sunlit-average (or instant) cosine of the zenith angle, the direct
// fraction, fp, i_star and the fourth root of the radiation bracket, ITS-90 e_sat, and the UTCI polynomial nested by variable
// (utci_poly.h).  Nothing intermediate is stored: seven fields in, up to three out.
//
// Order of operations follows the reference where it decides a comparison (every test of the ten-branch integral, the clamps
// at 0.85 and 0.9, cos 89.5 deg, 0.001, the validity box).  Where it only rounds differently the device takes the cheaper form
// and the tests bound the difference stage by stage: _wrap_radians by one fma instead of fmod (exact: see wrap), tan(dec) from
// the host table, x ** 0.25 as two square roots, the polynomial by Horner.
//
// One lane per cell and scalar loads at every size: a wave's 64 loads of a field are one contiguous 256 B (float32) or 512 B
// (float64) segment.  No 16-byte variant: a year of 1440 x 720 cells takes 17 times its read-plus-write floor, and the counter run
// (profiles/r23/pmc_valu_k_thermal.csv) shows 1278 VALU instructions per sample with the VALU busy 49 % of the time, so the kernel
// waits on instruction latency, not on how its loads are issued; there is no size switch.
#include "esat.h"
#include "hostargs.h"
#include "pyminmax.h"
#include "utci_poly.h"

#include <cmath>

namespace {

constexpr double PI = 3.141592653589793;  // np.pi
constexpr double TWO_PI = 2 * PI;

// _wrap_radians (helpers.py:60-63): ((x + pi) % (2 pi)) - pi with numpy's remainder (sign of the divisor).  The remainder is
// x - q 2 pi for the integer q = floor(x / 2 pi), and it is a float64 (fmod is exact), so one fma from the right q gives it without
// a rounding; q from a rounded product can be off by one next to a multiple of 2 pi, which the two corrections (exact for the
// same reason) take back.
__device__ __forceinline__ double wrap(double x) {
  const double y = x + PI;
  const double q = floor(y * (1 / TWO_PI));
  double m = fma(-q, TWO_PI, y);
  if (m < 0.0) m += TWO_PI;
  if (m >= TWO_PI) m -= TWO_PI;
  return m - PI;
}

struct ThermalArgs {
  const void* tas;
  const void* hurs;
  const void* ws;
  const void* mrt_in;
  const void* rsds;
  const void* rsus;
  const void* rlds;
  const void* rlus;
  const double* rows;  // (XH_THERMAL_NROW, R)
  const double* lat;   // (C) wrapped, rad
  const double* lon;   // (C) rad
  void* utci;
  double* mrt;
  double* csza;
  int64_t R, C, ld, ld_out;
  int mode, stat, flags;
};

// _sunlit_integral_of_cosine_of_solar_zenith_angle (helpers.py:353-397) with average = True.  sd_sl = sin dec sin lat,
// cd_cl = cos dec cos lat; day / night: the signs of dec * lat, read where the sunset hour angle is NaN.
__device__ __forceinline__ double sunlit_average(double sd_sl, double cd_cl, bool day, bool night, double hss, double hs, double he) {
  const double hsr = -hss;
  const bool nan_ss = isnan(hss);
  double num, den;
  if (nan_ss && day) {
    num = sin(he) - sin(hs);
    den = he < hs ? he + 2 * PI - hs : he - hs;
  } else if (nan_ss && night) {
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
  return (sd_sl * den + cd_cl * num) / den;
}

template <typename TF>
__global__ void __launch_bounds__(XH_BLOCK) k_thermal(ThermalArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const bool need_mrt = a.utci || a.mrt;  // false: csza_out alone, and the radiation fields may be NULL
  const bool need_sun = (need_mrt && !a.mrt_in) || a.csza;
  double lat = 0, sl = 0, cl = 0, tl = 0, lon = 0;
  if (need_sun) {
    lat = a.lat[c];
    sl = sin(lat);
    cl = cos(lat);
    tl = tan(lat);
    if (a.mode == XH_THERMAL_SUBDAILY) lon = a.lon[c];
  }
  const double cos895 = 0.008726535498373897;  // np.cos(89.5 / 180 * np.pi)
  const int64_t R = a.R;
  for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
    const int64_t i = r * a.ld + c, o = r * a.ld_out + c;
    double csza = 0, mrt = 0;
    if (need_sun) {
      const double sd = a.rows[XH_THERMAL_SIN_DEC * R + r], cd = a.rows[XH_THERMAL_COS_DEC * R + r];
      double hs, he = 0;
      if (a.mode == XH_THERMAL_SUBDAILY) {
        hs = a.rows[XH_THERMAL_H_UTC * R + r] + lon;
        he = hs + a.rows[XH_THERMAL_INTERVAL * R + r];
      } else {
        hs = a.stat == XH_THERMAL_INSTANT ? 0.0 : -PI;
        he = PI - 1e-9;
      }
      if (a.stat == XH_THERMAL_INSTANT) {
        const double v = sd * sl + cd * cl * cos(hs + a.rows[XH_THERMAL_TCORR * R + r]);
        csza = v < 0.0 ? 0.0 : v;  // clip(0, None): NaN stays
      } else {
        const double tt = -tl * a.rows[XH_THERMAL_TAN_DEC * R + r];
        const double hss = fabs(tt) <= 1 ? acos(tt) : xh_nan64();
        const double dl = sd * lat;  // the sign of dec * lat: |dec| < pi / 2
        csza = sunlit_average(sd * sl, cd * cl, dl > 0, dl < 0, wrap(hss), wrap(hs), wrap(he));
      }
      if (a.csza) a.csza[o] = csza;
    }
    if (a.mrt_in) {
      mrt = xh_ldw<TF>(a.mrt_in, i);
    } else if (need_mrt) {
      // _fdir_ratio (converters.py:2525-2534) and mean_radiant_temperature (:2615-2633)
      const double rsds = xh_ldw<TF>(a.rsds, i), rsus = xh_ldw<TF>(a.rsus, i);
      const double rlds = xh_ldw<TF>(a.rlds, i), rlus = xh_ldw<TF>(a.rlus, i);
      double s_star = rsds * (1 / (1367 * csza * a.rows[XH_THERMAL_INV_D2 * R + r]));
      s_star = s_star > 0.85 ? 0.85 : s_star;
      double fdir = exp(3 - 1.34 * s_star - 1.65 * (1 / s_star));
      fdir = fdir > 0.9 ? 0.9 : fdir;
      fdir = (fdir <= 0 || csza <= cos895 || rsds <= 0) ? 0.0 : fdir;
      const double direct = fdir * rsds;
      const double diffuse = rsds - direct;
      const double gamma = asin(csza);
      const double fp = 0.308 * cos(gamma * 0.988 - (gamma * gamma / 50000));
      const double i_star = csza > 0.001 ? direct / csza : 0.0;
      const double s = (1 / 5.67e-8) * (0.5 * rlds + 0.5 * rlus + (0.7 / 0.97) * (0.5 * diffuse + 0.5 * rsus + fp * i_star));
      mrt = sqrt(sqrt(s));
      if (a.mrt) a.mrt[o] = mrt;
    }
    if (a.utci) {
      // universal_thermal_climate_index (converters.py:2462-2489)
      const double tk = xh_ldw<TF>(a.tas, i);
      const double e_sat = xh_esat_its90_water(tk);
      const double ta = tk - 273.15;
      double va = xh_ldw<TF>(a.ws, i);
      if ((a.flags & XH_THERMAL_WIND_CAP_MIN) && va < 0.5) va = 0.5;
      const double dt = (mrt - 273.15) - ta;
      const double pa = (e_sat * 1e-3) * (xh_ldw<TF>(a.hurs, i) * 1e-2);
      double u = xh_utci::utci(ta, va, dt, pa);
      if ((a.flags & XH_THERMAL_MASK_INVALID) && !(-50.0 < ta && ta < 50.0 && -30 < dt && dt < 30 && 0.5 <= va && va < 17.0)) u = xh_nan64();
      reinterpret_cast<TF*>(a.utci)[o] = (TF)u;
    }
  }
}

template <typename TF>
__global__ void __launch_bounds__(XH_BLOCK) k_esat(const void* __restrict__ tas, int64_t R, int64_t C, int64_t ld, int method, int kase,
                                                   double t_ice, double t_water, double power, TF* __restrict__ out, int64_t ld_out) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= C) return;
  for (int64_t r = blockIdx.y; r < R; r += gridDim.y)
    out[r * ld_out + c] = (TF)xh_esat_of(xh_ldw<TF>(tas, r * ld + c), method, kase, t_ice, t_water, power);
}

}  // namespace

int xh_esat(xh_ctx* ctx, const void* tas, int64_t R, int64_t C, int64_t ld, int f64, int method, int kase, double ice_thresh,
            double water_thresh, double interp_power, void* out, int64_t ld_out) {
  const char* fn = "xh_esat";
  const int rc = xh_check_pitched(fn, ctx, R, C, ld, R, ld_out);
  if (rc) return rc;
  XH_REQUIRE(method >= 0 && method < XH_ESAT_NMETHODS, XH_ERR_ARG, "%s: method must be 0..%d, got %d", fn, XH_ESAT_NMETHODS - 1, method);
  XH_REQUIRE(kase >= XH_ESAT_WATER && kase <= XH_ESAT_INTERP, XH_ERR_ARG, "%s: case must be 0..2, got %d", fn, kase);
  if (R == 0 || C == 0) return XH_OK;
  XH_REQUIRE(tas && out, XH_ERR_ARG, "%s: NULL argument", fn);
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(R < 4096 ? R : 4096));
  xh_by_width(f64, [&](auto w) {
    using TF = XH_WIDTH(w);
    hipLaunchKernelGGL(k_esat<TF>, g, dim3(XH_BLOCK), 0, ctx->stream, tas, R, C, ld, method, kase, ice_thresh, water_thresh, interp_power,
                       static_cast<TF*>(out), ld_out);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_thermal_comfort(xh_ctx* ctx, int64_t R, int64_t C, int64_t ld, int f64, const void* tas, const void* hurs,
                       const void* sfcwind, const void* mrt_in, const void* rsds, const void* rsus, const void* rlds,
                       const void* rlus, const double* rows, const double* lat, const double* lon, int mode, int stat, int flags,
                       void* utci_out, double* mrt_out, double* csza_out, int64_t ld_out) {
  const char* fn = "xh_thermal_comfort";
  const int rc = xh_check_pitched(fn, ctx, R, C, ld, R, ld_out);
  if (rc) return rc;
  XH_REQUIRE(R >= 1 && C >= 1, XH_ERR_ARG, "%s: needs R >= 1 and C >= 1", fn);
  XH_REQUIRE(mode == XH_THERMAL_DAILY || mode == XH_THERMAL_SUBDAILY, XH_ERR_ARG, "%s: mode must be 0 (daily) or 1 (sub-daily), got %d", fn, mode);
  XH_REQUIRE(stat == XH_THERMAL_SUNLIT || stat == XH_THERMAL_INSTANT, XH_ERR_ARG, "%s: stat must be 0 (sunlit) or 1 (instant), got %d", fn, stat);
  XH_REQUIRE((flags & ~(XH_THERMAL_MASK_INVALID | XH_THERMAL_WIND_CAP_MIN)) == 0, XH_ERR_ARG, "%s: unknown flag bits in %d", fn, flags);
  XH_REQUIRE(utci_out || mrt_out || csza_out, XH_ERR_ARG, "%s: no output requested", fn);
  XH_REQUIRE(!(mrt_in && mrt_out), XH_ERR_ARG, "%s: mrt_out with mrt_in given", fn);
  XH_REQUIRE(!utci_out || (tas && hurs && sfcwind), XH_ERR_ARG, "%s: utci_out needs tas, hurs and sfcwind", fn);
  const bool radiation = !mrt_in && (utci_out || mrt_out);
  XH_REQUIRE(!radiation || (rsds && rsus && rlds && rlus), XH_ERR_ARG, "%s: without mrt_in, rsds, rsus, rlds and rlus are needed", fn);
  const bool sun = radiation || csza_out;
  XH_REQUIRE(!sun || (rows && lat && (mode == XH_THERMAL_DAILY || lon)), XH_ERR_ARG,
             "%s: the solar tables (rows, lat, and lon for sub-daily rows) are needed", fn);
  ThermalArgs a{};
  a.tas = tas;
  a.hurs = hurs;
  a.ws = sfcwind;
  a.mrt_in = mrt_in;
  a.rsds = rsds;
  a.rsus = rsus;
  a.rlds = rlds;
  a.rlus = rlus;
  a.rows = rows;
  a.lat = lat;
  a.lon = lon;
  a.utci = utci_out;
  a.mrt = mrt_out;
  a.csza = csza_out;
  a.R = R;
  a.C = C;
  a.ld = ld;
  a.ld_out = ld_out;
  a.mode = mode;
  a.stat = stat;
  a.flags = flags;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(R < 4096 ? R : 4096));
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_thermal<XH_WIDTH(w)>, g, dim3(XH_BLOCK), 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
