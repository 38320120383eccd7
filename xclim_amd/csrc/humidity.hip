// humidity.hip — the humidity, heat-stress and wind conversions of indices/converters.py: humidex (:75-172), heat_index (:175-223),
// uas_vas_to_sfcwind and sfcwind_to_uas_vas (:272-387), vapor_pressure, vapor_pressure_deficit, relative_humidity,
// specific_humidity, specific_humidity_from_dewpoint, dewpoint_from_specific_humidity (:606-1084), wind_chill_index (:1659-1744)
// and wind_power_potential (:2797-2902).  C ABI and the exact definition of every result: include/units/xclim_hip_humidity.h.
//
// Both kernels are element-wise and have the shape of k_phase_map (phase.hip): VEC consecutive cells per lane, 16-byte loads and
// stores where every given field and requested output allows them and one element per lane otherwise (tails, views off the
// 16-byte grid), rows blockIdx.y, blockIdx.y + gridDim.y, ...  Every field is read once, every requested output comes from that
// one read, and nothing intermediate is written: (tas, tdps, ps) -> (hurs, huss, humidex, heat_index) is seven field passes
// where the single-output launches make twelve.  The set of given fields and requested outputs is a kernel argument, so every
// branch on it is uniform over the launch: an absent field costs no load and an output that is not asked for no arithmetic and
// no store.  No LDS, no atomics, no barrier.
//
// All arithmetic is float64 on the widened values in the reference's order of operations (the unit is compiled with
// -ffp-contract=off like every other), e_sat comes from esat.h.  Where the reference calls pow with an integer exponent
// (v ** 3 of the power curve) the device multiplies; 10 ** x and v ** 0.16 are pow.
#include "../../include/units/xclim_hip_humidity.h"
#include "esat.h"
#include "hostargs.h"

#include <cmath>

namespace {

enum { F_TAS = 0, F_TDPS, F_HURS, F_HUSS, F_PS, F_N };

template <typename T, int N>
struct alignas(sizeof(T) * N) HVec {
  T v[N];
};

__device__ __forceinline__ double vapor_pressure(double huss, double ps) {
  const double eps = 0.62198;
  return ps * huss / (eps + (1 - eps) * huss);
}

// hurs.clip(lo, hi) of np.clip (a NaN stays) and hurs.where((x <= hi) & (x >= lo))
__device__ __forceinline__ double invalid_rule(double x, double lo, double hi, int rule) {
  if (rule == XH_INVALID_CLIP) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
  }
  if (rule == XH_INVALID_MASK) return (x <= hi && x >= lo) ? x : xh_nan64();
  return x;
}

// x % 360.0 as numpy takes it: the sign of the divisor
__device__ __forceinline__ double mod360(double x) {
  double m = fmod(x, 360.0);
  if (m != 0.0) {
    if (m < 0.0) m += 360.0;
  } else {
    m = 0.0;
  }
  return m;
}

struct AmArgs {
  const void* in[F_N];
  void* out[XH_AM_NOUT];
  int64_t R, C, ld, ld_out;
  double t_ice, t_water, power;
  double dew_a, dew_b, dew_c;
  int celsius, method, kase, rh_method, invalid_rh, invalid_q;
};

// one sample: x the five fields as loaded (widened), o the nine results.  What a branch tests is uniform over the launch.
__device__ __forceinline__ void am_sample(const AmArgs& a, const double* x, double* o) {
  const bool has_tdps = a.in[F_TDPS] != nullptr, has_hurs = a.in[F_HURS] != nullptr;
  const bool want_rh_dependent = a.out[XH_AM_VPD] || a.out[XH_AM_HUSS] || a.out[XH_AM_HEAT_INDEX] || (a.out[XH_AM_HUMIDEX] && !has_tdps);
  const bool want_rh = a.out[XH_AM_HURS] || (want_rh_dependent && !has_hurs);
  const bool rh_esat = want_rh && a.rh_method == XH_RH_ESAT;
  const double tas = x[F_TAS], ps = x[F_PS];
  const double tas_k = a.celsius ? tas + 273.15 : tas, tas_c = a.celsius ? tas : tas - 273.15;
  const double tdps_k = a.celsius ? x[F_TDPS] + 273.15 : x[F_TDPS];

  double es_t = 0, es_d = 0;
  if (a.out[XH_AM_ESAT] || a.out[XH_AM_VPD] || a.out[XH_AM_HUSS] || rh_esat) es_t = xh_esat_of(tas_k, a.method, a.kase, a.t_ice, a.t_water, a.power);
  if (a.out[XH_AM_HUSS_DEW] || (rh_esat && has_tdps)) es_d = xh_esat_of(tdps_k, a.method, a.kase, a.t_ice, a.t_water, a.power);
  if (a.out[XH_AM_ESAT]) o[XH_AM_ESAT] = es_t;
  if (a.out[XH_AM_VP]) o[XH_AM_VP] = vapor_pressure(x[F_HUSS], ps);

  double rh = x[F_HURS];
  if (want_rh) {  // relative_humidity (:806-841)
    double h;
    if (a.rh_method == XH_RH_BOHREN98) {
      h = 100 * exp(-2.501e6 * (tas_k - tdps_k) / (461.5 * tas_k * tdps_k));
    } else if (has_tdps) {
      h = 100 * es_d / es_t;
    } else {
      h = 100 * vapor_pressure(x[F_HUSS], ps) / es_t;
    }
    h = invalid_rule(h, 0.0, 100.0, a.invalid_rh);
    if (a.out[XH_AM_HURS]) o[XH_AM_HURS] = h;
    if (!has_hurs) rh = h;
  }
  if (a.out[XH_AM_VPD]) o[XH_AM_VPD] = (1 - (rh / 100)) * es_t;
  if (a.out[XH_AM_HUSS]) {  // specific_humidity (:929-948); the conversion of % to 1 is one multiplication
    const double w_sat = 0.62198 * es_t / (ps - es_t);
    const double w = w_sat * (rh * 0.01);
    double q = w / (1 + w);
    if (a.invalid_q != XH_INVALID_NONE) q = invalid_rule(q, 0.0, w_sat / (1 + w_sat), a.invalid_q);
    o[XH_AM_HUSS] = q;
  }
  if (a.out[XH_AM_HUSS_DEW]) o[XH_AM_HUSS_DEW] = 0.62198 * es_d / (ps - es_d * (1 - 0.62198));
  if (a.out[XH_AM_TDPS]) {  // dewpoint_from_specific_humidity (:1076-1084)
    const double q = x[F_HUSS] > 0 ? x[F_HUSS] : xh_nan64();
    const double f = log(vapor_pressure(q, ps) / a.dew_a) / a.dew_b;
    o[XH_AM_TDPS] = (-273.16 - a.dew_c * f) / (f - 1);
  }
  if (a.out[XH_AM_HUMIDEX]) {  // humidex (:146-172): the delta is the same number in K and in degC
    double e;
    if (has_tdps) e = 6.112 * exp(5417.7530 * (1 / 273.16 - 1.0 / tdps_k));
    else e = rh / 100 * 6.112 * pow(10.0, 7.5 * tas_c / (tas_c + 237.7));
    o[XH_AM_HUMIDEX] = 5.0 / 9 * (e - 10) + tas;
  }
  if (a.out[XH_AM_HEAT_INDEX]) {  // heat_index (:206-223)
    const double t = tas_c > 20 ? tas_c : xh_nan64(), r = rh;
    const double hi = -8.78469475556 + 1.61139411 * t + 2.33854883889 * r - 0.14611605 * t * r - 0.012308094 * t * t -
                      0.0164248277778 * r * r + 0.002211732 * t * t * r + 0.00072546 * t * r * r - 0.000003582 * t * t * r * r;
    o[XH_AM_HEAT_INDEX] = a.celsius ? hi : hi + 273.15;
  }
}

template <typename TE, int VEC>
__global__ void __launch_bounds__(XH_BLOCK) k_air_moisture(AmArgs a) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= a.C) return;  // (C is a multiple of VEC when VEC > 1)
  using V = HVec<TE, VEC>;
  for (int64_t r = blockIdx.y; r < a.R; r += gridDim.y) {
    const int64_t i = r * a.ld + c, j = r * a.ld_out + c;
    V x[F_N];
#pragma unroll
    for (int f = 0; f < F_N; ++f) {
      x[f] = V{};
      if (a.in[f]) x[f] = *reinterpret_cast<const V*>(static_cast<const TE*>(a.in[f]) + i);
    }
    V y[XH_AM_NOUT];
    // the cells of the lane by a constant index each (a loop the compiler declines to unroll would index x and y in scratch)
    auto cell = [&](auto kc) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k < VEC) {
        double xs[F_N], o[XH_AM_NOUT];
#pragma unroll
        for (int f = 0; f < F_N; ++f) xs[f] = (double)x[f].v[k];
#pragma unroll
        for (int n = 0; n < XH_AM_NOUT; ++n) o[n] = 0.0;
        am_sample(a, xs, o);
#pragma unroll
        for (int n = 0; n < XH_AM_NOUT; ++n) y[n].v[k] = (TE)o[n];
      }
    };
    cell(std::integral_constant<int, 0>{}), cell(std::integral_constant<int, 1>{});
    cell(std::integral_constant<int, 2>{}), cell(std::integral_constant<int, 3>{});
#pragma unroll
    for (int n = 0; n < XH_AM_NOUT; ++n)
      if (a.out[n]) *reinterpret_cast<V*>(static_cast<TE*>(a.out[n]) + j) = y[n];
  }
}

// ---- xh_wind_map ----------------------------------------------------------------------------------------------------
struct WindArgs {
  const void *a, *b;
  void *out0, *out1;
  int64_t R, C, ld, ld_out;
  double p0, p1, p2;  // the calm threshold; cut_in, rated, cut_out (as they are compared)
  double ci3, den;    // cut_in ** 3 and rated ** 3 - cut_in ** 3 of the unrounded parameters
  int flags;
};

template <typename TE, int OP>
__device__ __forceinline__ void wind_sample(const WindArgs& w, double a, double b, double& o0, double& o1) {
  constexpr double PI = 3.141592653589793;
  if (OP == XH_WIND_FROM_UV) {
    o0 = hypot(a, b);
    double d = mod360(270 - atan2(b, a) * (180.0 / PI));
    d = rint(d) == 0 ? 360.0 : d;
    o1 = (double)(TE)o0 < w.p0 ? 0.0 : d;
  } else if (OP == XH_WIND_TO_UV) {
    const double m = mod360(-b + 270) * (PI / 180.0);
    o0 = a * cos(m);
    o1 = a * sin(m);
  } else if (OP == XH_WIND_CHILL) {
    const double t = (w.flags & XH_WIND_CELSIUS) ? a : a - 273.15;
    const double v = (w.flags & XH_WIND_KMH) ? b : b * 3.6;
    const double V = pow(v, 0.16);
    double W = 13.12 + 0.6215 * t - 11.37 * V + 0.3965 * t * V;
    const bool us = (w.flags & XH_WIND_US) != 0;
    if (!us && v < 5) W = t + v * (-1.59 + 0.1345 * t) / 5;
    if (w.flags & XH_WIND_MASK_INVALID) {
      const bool valid = us ? (v > 4.828032 && t <= 10) : t <= 0;
      W = valid ? W : xh_nan64();
    }
    o0 = W;
  } else {
    double v = a;
    if (w.b) v = a * pow(b / 1.225, 1.0 / 3);
    if (v < w.p0) o0 = 0.0;
    else if (v < w.p1) o0 = (v * v * v - w.ci3) / w.den;
    else if (v < w.p2) o0 = 1.0;
    else o0 = 0.0;  // (a NaN speed too, as _wind_power_factor returns it)
  }
}

template <typename TE, int VEC, int OP>
__global__ void __launch_bounds__(XH_BLOCK) k_wind_map(WindArgs w) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= w.C) return;
  using V = HVec<TE, VEC>;
  for (int64_t r = blockIdx.y; r < w.R; r += gridDim.y) {
    const int64_t i = r * w.ld + c, j = r * w.ld_out + c;
    const V a = *reinterpret_cast<const V*>(static_cast<const TE*>(w.a) + i);
    V b = V{};
    if (w.b) b = *reinterpret_cast<const V*>(static_cast<const TE*>(w.b) + i);
    V y0, y1;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      double o0 = 0.0, o1 = 0.0;
      wind_sample<TE, OP>(w, (double)a.v[k], (double)b.v[k], o0, o1);
      y0.v[k] = (TE)o0, y1.v[k] = (TE)o1;
    }
    if (w.out0) *reinterpret_cast<V*>(static_cast<TE*>(w.out0) + j) = y0;
    if (w.out1) *reinterpret_cast<V*>(static_cast<TE*>(w.out1) + j) = y1;
  }
}

dim3 map_grid(int64_t R, int64_t C, int vec) {
  return dim3((unsigned)cdiv64(cdiv64(C, vec), XH_BLOCK), (unsigned)(R < 4096 ? R : 4096));
}

}  // namespace

int xh_air_moisture(xh_ctx* ctx, int64_t R, int64_t C, int64_t ld, int f64, const void* tas, const void* tdps, const void* hurs,
                    const void* huss, const void* ps, int celsius, int method, int kase, double ice_thresh, double water_thresh,
                    double interp_power, int rh_method, int invalid_rh, int invalid_q, int dew_method, int dew_ice,
                    void* const* outs, int64_t ld_out) {
  const char* fn = "xh_air_moisture";
  const int rc = xh_check_pitched(fn, ctx, R, C, ld, R, ld_out);
  if (rc) return rc;
  XH_REQUIRE(outs, XH_ERR_ARG, "%s: NULL outs", fn);
  XH_REQUIRE(method >= 0 && method < XH_ESAT_NMETHODS, XH_ERR_ARG, "%s: method must be 0..%d, got %d", fn, XH_ESAT_NMETHODS - 1, method);
  XH_REQUIRE(kase >= XH_ESAT_WATER && kase <= XH_ESAT_INTERP, XH_ERR_ARG, "%s: case must be 0..2, got %d", fn, kase);
  XH_REQUIRE(rh_method == XH_RH_ESAT || rh_method == XH_RH_BOHREN98, XH_ERR_ARG, "%s: rh_method must be 0 or 1, got %d", fn, rh_method);
  XH_REQUIRE(invalid_rh >= XH_INVALID_NONE && invalid_rh <= XH_INVALID_MASK && invalid_q >= XH_INVALID_NONE && invalid_q <= XH_INVALID_MASK,
             XH_ERR_ARG, "%s: invalid_rh and invalid_q must be 0..2, got %d and %d", fn, invalid_rh, invalid_q);
  XH_REQUIRE(dew_method >= XH_DEW_TETENS30 && dew_method <= XH_DEW_AERK96, XH_ERR_ARG, "%s: dew_method must be 0..3, got %d", fn, dew_method);
  AmArgs a{};
  a.in[F_TAS] = tas, a.in[F_TDPS] = tdps, a.in[F_HURS] = hurs, a.in[F_HUSS] = huss, a.in[F_PS] = ps;
  bool any = false;
  for (int n = 0; n < XH_AM_NOUT; ++n) a.out[n] = outs[n], any = any || outs[n];
  XH_REQUIRE(any, XH_ERR_ARG, "%s: no output requested", fn);
  // what each output needs; "rh" is the field hurs or this launch's relative humidity
  const bool rh_computable = tas && (rh_method == XH_RH_BOHREN98 ? tdps != nullptr : (tdps || (huss && ps)));
  const bool rh = hurs || rh_computable;
  XH_REQUIRE(!a.out[XH_AM_ESAT] || tas, XH_ERR_ARG, "%s: e_sat needs tas", fn);
  XH_REQUIRE(!a.out[XH_AM_VP] || (huss && ps), XH_ERR_ARG, "%s: vapor_pressure needs huss and ps", fn);
  XH_REQUIRE(!a.out[XH_AM_VPD] || (tas && rh), XH_ERR_ARG, "%s: vapor_pressure_deficit needs tas and hurs (given or computable)", fn);
  XH_REQUIRE(!a.out[XH_AM_HURS] || rh_computable, XH_ERR_ARG,
             "%s: relative_humidity needs tas and tdps, or tas, huss and ps (bohren98: tas and tdps)", fn);
  XH_REQUIRE(!a.out[XH_AM_HUSS] || (tas && ps && rh), XH_ERR_ARG, "%s: specific_humidity needs tas, ps and hurs (given or computable)", fn);
  XH_REQUIRE(!a.out[XH_AM_HUSS_DEW] || (tdps && ps), XH_ERR_ARG, "%s: specific_humidity_from_dewpoint needs tdps and ps", fn);
  XH_REQUIRE(!a.out[XH_AM_TDPS] || (huss && ps), XH_ERR_ARG, "%s: dewpoint_from_specific_humidity needs huss and ps", fn);
  XH_REQUIRE(!a.out[XH_AM_HUMIDEX] || (tas && (tdps || rh)), XH_ERR_ARG, "%s: humidex needs tas and tdps, or tas and hurs (given or computable)", fn);
  XH_REQUIRE(!a.out[XH_AM_HEAT_INDEX] || (tas && rh), XH_ERR_ARG, "%s: heat_index needs tas and hurs (given or computable)", fn);
  if (R == 0 || C == 0) return XH_OK;

  // ESAT_FORMULAS_COEFFICIENTS (converters.py:390-395), water then ice
  static const double magnus[4][2][3] = {{{610.78, 17.269388, -35.86}, {610.78, 21.8745584, -7.66}},
                                         {{611.2, 17.62, -30.04}, {611.2, 22.46, -0.54}},
                                         {{611.21, 17.502, -32.19}, {611.15, 22.542, 0.32}},
                                         {{610.94, 17.625, -30.12}, {611.21, 22.587, 0.7}}};
  const double* m = magnus[dew_method][dew_ice ? 1 : 0];
  a.dew_a = m[0], a.dew_b = m[1], a.dew_c = m[2];
  a.R = R, a.C = C, a.ld = ld, a.ld_out = ld_out;
  // numpy >= 2 compares a float32 field with the threshold rounded to float32; a field in degC is compared after the offset,
  // which the device adds in float64
  const bool round32 = !f64 && !celsius;
  a.t_ice = round32 ? (double)(float)ice_thresh : ice_thresh;
  a.t_water = round32 ? (double)(float)water_thresh : water_thresh;
  a.power = interp_power;
  a.celsius = celsius != 0, a.method = method, a.kase = kase, a.rh_method = rh_method, a.invalid_rh = invalid_rh, a.invalid_q = invalid_q;

  const size_t esz = f64 ? 8 : 4;
  const int width = f64 ? 2 : 4;
  int vec = width;
  for (int f = 0; f < F_N; ++f)
    if (a.in[f] && xh_cells_per_lane(a.in[f], C, ld, width, esz) != width) vec = 1;
  for (int n = 0; n < XH_AM_NOUT; ++n)
    if (a.out[n] && xh_cells_per_lane(a.out[n], C, ld_out, width, esz) != width) vec = 1;
  const dim3 g = map_grid(R, C, vec), b(XH_BLOCK);
  if (f64) {
    if (vec == 2) hipLaunchKernelGGL((k_air_moisture<double, 2>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_air_moisture<double, 1>), g, b, 0, ctx->stream, a);
  } else {
    if (vec == 4) hipLaunchKernelGGL((k_air_moisture<float, 4>), g, b, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_air_moisture<float, 1>), g, b, 0, ctx->stream, a);
  }
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_wind_map(xh_ctx* ctx, int op, int64_t R, int64_t C, int64_t ld, int f64, const void* a, const void* b, const double* par,
                int flags, void* out0, void* out1, int64_t ld_out) {
  const char* fn = "xh_wind_map";
  const int rc = xh_check_pitched(fn, ctx, R, C, ld, R, ld_out);
  if (rc) return rc;
  XH_REQUIRE(op >= 0 && op < XH_WIND_NOPS, XH_ERR_ARG, "%s: op must be 0..%d, got %d", fn, XH_WIND_NOPS - 1, op);
  XH_REQUIRE((flags & ~(XH_WIND_CELSIUS | XH_WIND_KMH | XH_WIND_US | XH_WIND_MASK_INVALID)) == 0, XH_ERR_ARG, "%s: unknown flag bits in %d", fn, flags);
  XH_REQUIRE(a && (b || op == XH_WIND_POWER), XH_ERR_ARG, "%s: NULL field", fn);
  const bool two = op == XH_WIND_FROM_UV || op == XH_WIND_TO_UV;
  XH_REQUIRE(out0 || (two && out1), XH_ERR_ARG, "%s: no output requested", fn);
  XH_REQUIRE(two || !out1, XH_ERR_ARG, "%s: this operation has one output", fn);
  XH_REQUIRE(par || op == XH_WIND_TO_UV || op == XH_WIND_CHILL, XH_ERR_ARG, "%s: NULL parameters", fn);
  WindArgs w{};
  if (op == XH_WIND_FROM_UV) {
    XH_REQUIRE(par[0] == par[0], XH_ERR_ARG, "%s: the calm threshold is NaN", fn);
    w.p0 = f64 ? par[0] : (double)(float)par[0];
  } else if (op == XH_WIND_POWER) {
    XH_REQUIRE(par[0] < par[1], XH_ERR_ARG, "%s: needs cut_in < rated", fn);
    XH_REQUIRE(par[2] == par[2], XH_ERR_ARG, "%s: cut_out is NaN", fn);
    w.ci3 = std::pow(par[0], 3.0);
    w.den = std::pow(par[1], 3.0) - w.ci3;
    w.p0 = f64 ? par[0] : (double)(float)par[0];
    w.p1 = f64 ? par[1] : (double)(float)par[1];
    w.p2 = f64 ? par[2] : (double)(float)par[2];
  }
  if (R == 0 || C == 0) return XH_OK;
  w.a = a, w.b = b, w.out0 = out0, w.out1 = out1;
  w.R = R, w.C = C, w.ld = ld, w.ld_out = ld_out, w.flags = flags;
  const size_t esz = f64 ? 8 : 4;
  const int width = f64 ? 2 : 4;
  int vec = xh_cells_per_lane(a, C, ld, width, esz);
  if (b && xh_cells_per_lane(b, C, ld, width, esz) != width) vec = 1;
  if (out0 && xh_cells_per_lane(out0, C, ld_out, width, esz) != width) vec = 1;
  if (out1 && xh_cells_per_lane(out1, C, ld_out, width, esz) != width) vec = 1;
  const dim3 g = map_grid(R, C, vec), blk(XH_BLOCK);
  xh_pick<XH_WIND_FROM_UV, XH_WIND_TO_UV, XH_WIND_CHILL, XH_WIND_POWER>(op, [&](auto o) {
    constexpr int OP = decltype(o)::value;
    if (f64) {
      if (vec == 2) hipLaunchKernelGGL((k_wind_map<double, 2, OP>), g, blk, 0, ctx->stream, w);
      else hipLaunchKernelGGL((k_wind_map<double, 1, OP>), g, blk, 0, ctx->stream, w);
    } else {
      if (vec == 4) hipLaunchKernelGGL((k_wind_map<float, 4, OP>), g, blk, 0, ctx->stream, w);
      else hipLaunchKernelGGL((k_wind_map<float, 1, OP>), g, blk, 0, ctx->stream, w);
    }
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
