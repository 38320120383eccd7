// humidity_driver — xh_air_moisture and xh_wind_map of the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE ONLY).
// A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_humidity_cpu.py links it with humidity.hip
// and sim_runtime.cpp, everything compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field and every output is a malloc block of EXACTLY R * C elements, so that an access one element outside lands in a
// redzone; a field the call does not need and an output it does not ask for are NULL, so that a touch of either faults.  The
// cases: 3 rows by 1, 3, 4, 5, 65 and 130 cells (the 16-byte path where C allows it, the scalar path otherwise), float32 and
// float64, every single output with just the fields it needs, the full set from all five fields, the fused launch from
// (tas, tdps, ps), every e_sat method and case, both rh methods, the three invalid rules, K and degC; the four wind operations with
// each output subset, with and without the density field.  Checked without a reference: the return code, every requested output
// written (the blocks start as 0x7B), a relative humidity under "clip" inside [0, 100], a power factor inside [0, 1], and the
// argument errors.
#include "driver_common.h"
#include "units/xclim_hip_humidity.h"
#include "units/xclim_hip_thermal.h"

const char* const kProgram = "humidity_driver";

namespace {

template <typename TE>
bool poisoned(const TE* p, int64_t n) {
  TE pat;
  memset(&pat, 0x7B, sizeof(TE));
  for (int64_t i = 0; i < n; ++i)
    if (memcmp(&p[i], &pat, sizeof(TE)) == 0) return true;
  return false;
}

enum { TAS = 1, TDPS = 2, HURS = 4, HUSS = 8, PS = 16 };

// one launch: the fields of `in` (a bit set), the outputs of `outs` (a bit set over XH_AM_*)
template <typename TE>
void moisture(int64_t R, int64_t C, int in, int outs, int celsius, int method, int kase, int rh_method, int rule) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const double t0 = celsius ? -40.0 : 233.15;
  TE* tas = (in & TAS) ? field<TE>(R, C, 1u, t0, 85.0) : nullptr;
  TE* tdps = (in & TDPS) ? field<TE>(R, C, 2u, t0, 70.0) : nullptr;
  TE* hurs = (in & HURS) ? field<TE>(R, C, 3u, -5.0, 115.0) : nullptr;
  TE* huss = (in & HUSS) ? field<TE>(R, C, 4u, -0.001, 0.03) : nullptr;
  TE* ps = (in & PS) ? field<TE>(R, C, 5u, 60000.0, 45000.0) : nullptr;
  void* o[XH_AM_NOUT];
  for (int n = 0; n < XH_AM_NOUT; ++n) o[n] = (outs >> n & 1) ? (void*)block<TE>(R * C) : nullptr;
  ok(xh_air_moisture(ctx, R, C, C, sizeof(TE) == 8, tas, tdps, hurs, huss, ps, celsius, method, kase, 250.16, 273.16, 2.0, rh_method, rule, rule,
                     method % 4, kase == XH_ESAT_BINARY, o, C),
     "xh_air_moisture");
  for (int n = 0; n < XH_AM_NOUT; ++n)
    if (o[n] && poisoned((TE*)o[n], R * C)) fail("xh_air_moisture: an output element was not written");
  if (o[XH_AM_HURS] && rule == XH_INVALID_CLIP)
    for (int64_t i = 0; i < R * C; ++i) {
      const double h = (double)((TE*)o[XH_AM_HURS])[i];
      if (!isnan(h) && !(h >= 0.0 && h <= 100.0)) fail("xh_air_moisture: a clipped relative humidity outside [0, 100]");
    }
  free(tas), free(tdps), free(hurs), free(huss), free(ps);
  for (int n = 0; n < XH_AM_NOUT; ++n) free(o[n]);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void wind(int64_t R, int64_t C, int op, int outs, bool with_b, int flags) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* a = field<TE>(R, C, 6u, op == XH_WIND_CHILL ? 240.0 : -3.0, op == XH_WIND_CHILL ? 50.0 : 33.0);
  TE* b = with_b ? field<TE>(R, C, 7u, 0.1, op == XH_WIND_TO_UV ? 360.0 : 2.0) : nullptr;
  const double par[XH_WIND_NPAR] = {op == XH_WIND_FROM_UV ? 0.5 : 3.5, 13.0, 25.0};
  TE* o0 = (outs & 1) ? block<TE>(R * C) : nullptr;
  TE* o1 = (outs & 2) ? block<TE>(R * C) : nullptr;
  ok(xh_wind_map(ctx, op, R, C, C, sizeof(TE) == 8, a, b, par, flags, o0, o1, C), "xh_wind_map");
  if ((o0 && poisoned(o0, R * C)) || (o1 && poisoned(o1, R * C))) fail("xh_wind_map: an output element was not written");
  if (op == XH_WIND_POWER)
    for (int64_t i = 0; i < R * C; ++i)
      if (!((double)o0[i] >= 0.0 && (double)o0[i] <= 1.0)) fail("xh_wind_map: a power factor outside [0, 1]");
  free(a), free(b), free(o0), free(o1);
  xh_destroy(ctx);
  ++g_cases;
}

void refusals() {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  double* x = block<double>(12);
  void* o[XH_AM_NOUT] = {};
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("no output was taken");
  o[XH_AM_HURS] = x;
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, 0, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("hurs without tdps or ps was taken");
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, 0, 0, x, x, 0, 0, 0, 0, 0, 0, XH_RH_BOHREN98, 0, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("bohren98 without tdps was taken");
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, x, 0, 0, 0, 0, XH_ESAT_NMETHODS, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("an unknown method was taken");
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("an unknown invalid rule was taken");
  if (xh_air_moisture(ctx, 3, 4, 3, 1, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 4) != XH_ERR_LAYOUT) fail("ld < C was taken");
  o[XH_AM_HURS] = nullptr, o[XH_AM_HEAT_INDEX] = x;
  if (xh_air_moisture(ctx, 3, 4, 4, 1, x, 0, 0, 0, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, o, 4) != XH_ERR_ARG) fail("heat_index without hurs was taken");
  const double par[XH_WIND_NPAR] = {13.0, 3.5, 25.0};
  if (xh_wind_map(ctx, XH_WIND_POWER, 3, 4, 4, 1, x, 0, par, 0, x, 0, 4) != XH_ERR_ARG) fail("cut_in >= rated was taken");
  if (xh_wind_map(ctx, XH_WIND_FROM_UV, 3, 4, 4, 1, x, 0, par, 0, x, 0, 4) != XH_ERR_ARG) fail("a NULL vas was taken");
  if (xh_wind_map(ctx, XH_WIND_CHILL, 3, 4, 4, 1, x, x, 0, 0, x, x, 4) != XH_ERR_ARG) fail("a second wind chill output was taken");
  if (xh_wind_map(ctx, XH_WIND_NOPS, 3, 4, 4, 1, x, x, par, 0, x, 0, 4) != XH_ERR_ARG) fail("an unknown operation was taken");
  if (xh_wind_map(ctx, XH_WIND_TO_UV, 3, 4, 4, 1, x, x, 0, 16, x, 0, 4) != XH_ERR_ARG) fail("an unknown flag was taken");
  free(x);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_cases() {
  const int need[XH_AM_NOUT] = {TAS, HUSS | PS, TAS | HURS, TAS | TDPS, TAS | HURS | PS, TDPS | PS, HUSS | PS, TAS | TDPS, TAS | HURS};
  const int64_t R = 3;
  for (int64_t C : {(int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)65, (int64_t)130}) {
    for (int n = 0; n < XH_AM_NOUT; ++n) moisture<TE>(R, C, need[n], 1 << n, n & 1, XH_ESAT_SONNTAG90, XH_ESAT_WATER, XH_RH_ESAT, n % 3);
    moisture<TE>(R, C, TAS | TDPS | HURS | HUSS | PS, (1 << XH_AM_NOUT) - 1, 0, XH_ESAT_ECMWF, XH_ESAT_INTERP, XH_RH_ESAT, XH_INVALID_CLIP);
    const int fused = 1 << XH_AM_HURS | 1 << XH_AM_HUSS | 1 << XH_AM_HUMIDEX | 1 << XH_AM_HEAT_INDEX;
    moisture<TE>(R, C, TAS | TDPS | PS, fused, 0, XH_ESAT_SONNTAG90, XH_ESAT_WATER, XH_RH_ESAT, XH_INVALID_CLIP);
    moisture<TE>(R, C, TAS | TDPS | PS, fused, 1, XH_ESAT_WMO08, XH_ESAT_BINARY, XH_RH_BOHREN98, XH_INVALID_MASK);
    moisture<TE>(R, C, TAS | HUSS | PS, 1 << XH_AM_HURS | 1 << XH_AM_VPD | 1 << XH_AM_HUMIDEX, 0, XH_ESAT_ITS90, XH_ESAT_BINARY, XH_RH_ESAT, XH_INVALID_NONE);
    for (int outs = 1; outs < 4; ++outs) {
      wind<TE>(R, C, XH_WIND_FROM_UV, outs, true, 0);
      wind<TE>(R, C, XH_WIND_TO_UV, outs, true, 0);
    }
    for (int flags : {0, XH_WIND_US, XH_WIND_MASK_INVALID, XH_WIND_US | XH_WIND_MASK_INVALID | XH_WIND_KMH}) wind<TE>(R, C, XH_WIND_CHILL, 1, true, flags);
    wind<TE>(R, C, XH_WIND_POWER, 1, true, 0);
    wind<TE>(R, C, XH_WIND_POWER, 1, false, 0);
  }
  for (int m = 0; m < XH_ESAT_NMETHODS; ++m)
    for (int k = XH_ESAT_WATER; k <= XH_ESAT_INTERP; ++k)
      moisture<TE>(R, 130, TAS | TDPS | PS, 1 << XH_AM_HURS | 1 << XH_AM_HUSS_DEW | 1 << XH_AM_ESAT, 0, m, k, XH_RH_ESAT, XH_INVALID_CLIP);
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  refusals();
  printf("%d cases clean\n", g_cases);
  return 0;
}
