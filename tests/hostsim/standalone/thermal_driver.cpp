// thermal_driver — xh_thermal_comfort and xh_esat of the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE ONLY).
// A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_thermal_cpu.py links it with thermal.hip
// and sim_runtime.cpp, everything compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY R * C elements, the row table one of exactly XH_THERMAL_NROW * R, the cell tables of
// exactly C and every output of exactly R * C, so that an access one element outside lands in a redzone.  A field the call does
// not need is passed as NULL, so that a read of it faults.  The cases: both modes and both stats on 1, 65 and 130 cells, 3 and 24
// rows, float32 and float64, every non-empty subset of the three outputs with the radiation fields, UTCI with mrt given (no
// tables at all), csza alone (no field at all), and xh_esat with every method in the three cases.  Checked without a reference:
// the return code, every requested output written (the blocks start as 0x7B), csza inside [0, 1], and the argument errors.
#include "driver_common.h"
#include "units/xclim_hip_thermal.h"

const char* const kProgram = "thermal_driver";

namespace {

const double PI = 3.141592653589793;

template <typename TE>
bool poisoned(const TE* p, int64_t n) {
  TE pat;
  memset(&pat, 0x7B, sizeof(TE));
  for (int64_t i = 0; i < n; ++i)
    if (memcmp(&p[i], &pat, sizeof(TE)) == 0) return true;
  return false;
}

template <typename TE>
void comfort(int64_t R, int64_t C, int mode, int stat, int outs, bool mrt_given) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const bool want_u = outs & 1, want_m = outs & 2, want_c = outs & 4;
  const bool radiation = !mrt_given && (want_u || want_m), sun = radiation || want_c;
  TE* tas = want_u ? field<TE>(R, C, 1u, 250.0, 60.0) : nullptr;
  TE* hurs = want_u ? field<TE>(R, C, 2u, 5.0, 90.0) : nullptr;
  TE* ws = want_u ? field<TE>(R, C, 3u, 0.0, 18.0) : nullptr;
  TE* mrt_in = mrt_given ? field<TE>(R, C, 4u, 250.0, 70.0) : nullptr;
  TE* rsds = radiation ? field<TE>(R, C, 5u, -5.0, 900.0) : nullptr;
  TE* rsus = radiation ? field<TE>(R, C, 6u, 0.0, 200.0) : nullptr;
  TE* rlds = radiation ? field<TE>(R, C, 7u, 150.0, 300.0) : nullptr;
  TE* rlus = radiation ? field<TE>(R, C, 8u, 200.0, 300.0) : nullptr;
  std::vector<double> rows((size_t)(XH_THERMAL_NROW * R)), lat((size_t)C), lon((size_t)C);
  for (int64_t r = 0; r < R; ++r) {
    const double dec = 0.409 * cos(0.3 * (double)r);
    rows[XH_THERMAL_SIN_DEC * R + r] = sin(dec);
    rows[XH_THERMAL_COS_DEC * R + r] = cos(dec);
    rows[XH_THERMAL_TAN_DEC * R + r] = tan(dec);
    rows[XH_THERMAL_H_UTC * R + r] = ((double)(r % 24) / 24) * 2 * PI + PI;
    rows[XH_THERMAL_INTERVAL * R + r] = 2 * PI / 24;
    rows[XH_THERMAL_TCORR * R + r] = 0.01;
    rows[XH_THERMAL_INV_D2 * R + r] = 0.97;
  }
  for (int64_t c = 0; c < C; ++c) {
    lat[c] = C > 1 ? (-89.0 + 178.0 * (double)c / (double)(C - 1)) * PI / 180 : 1.15;
    lon[c] = (-180.0 + 7.0 * (double)c) * PI / 180;
  }
  double* d_rows = sun ? exact(rows) : nullptr;
  double* d_lat = sun ? exact(lat) : nullptr;
  double* d_lon = sun && mode == XH_THERMAL_SUBDAILY ? exact(lon) : nullptr;
  TE* utci = want_u ? block<TE>(R * C) : nullptr;
  double* mrt = want_m ? block<double>(R * C) : nullptr;
  double* csza = want_c ? block<double>(R * C) : nullptr;
  ok(xh_thermal_comfort(ctx, R, C, C, sizeof(TE) == 8, tas, hurs, ws, mrt_in, rsds, rsus, rlds, rlus, d_rows, d_lat, d_lon, mode, stat,
                        XH_THERMAL_MASK_INVALID | (R > 3 ? XH_THERMAL_WIND_CAP_MIN : 0), utci, mrt, csza, C),
     "xh_thermal_comfort");
  if ((want_u && poisoned(utci, R * C)) || (want_m && poisoned(mrt, R * C)) || (want_c && poisoned(csza, R * C))) fail("an output element was not written");
  if (want_c)
    for (int64_t i = 0; i < R * C; ++i)
      if (!(csza[i] >= 0.0 && csza[i] <= 1.0 + 1e-12)) fail("a cosine outside [0, 1]");
  free(tas), free(hurs), free(ws), free(mrt_in), free(rsds), free(rsus), free(rlds), free(rlus);
  free(d_rows), free(d_lat), free(d_lon), free(utci), free(mrt), free(csza);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void esat(int64_t R, int64_t C) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* tas = field<TE>(R, C, 9u, 200.0, 130.0);
  for (int m = 0; m < XH_ESAT_NMETHODS; ++m)
    for (int k = XH_ESAT_WATER; k <= XH_ESAT_INTERP; ++k) {
      TE* out = block<TE>(R * C);
      ok(xh_esat(ctx, tas, R, C, C, sizeof(TE) == 8, m, k, 250.16, 273.16, 2.0, out, C), "xh_esat");
      if (poisoned(out, R * C)) fail("xh_esat: an output element was not written");
      for (int64_t i = 0; i < R * C; ++i)
        if (!isnan((double)tas[i]) && !((double)out[i] > 0.0)) fail("xh_esat: a saturation pressure that is not positive");
      free(out);
      ++g_cases;
    }
  if (xh_esat(ctx, tas, R, C, C, sizeof(TE) == 8, XH_ESAT_NMETHODS, 0, 0, 0, 0, tas, C) != XH_ERR_ARG) fail("xh_esat took an unknown method");
  if (xh_esat(ctx, tas, R, C, C - 1, sizeof(TE) == 8, 0, 0, 0, 0, 0, tas, C) != XH_ERR_LAYOUT && C > 0) fail("xh_esat took ld < C");
  free(tas);
  xh_destroy(ctx);
}

void refusals() {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  double* x = block<double>(12);
  if (xh_thermal_comfort(ctx, 3, 4, 4, 1, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, x, 0, 4) != XH_ERR_ARG) fail("mrt_out with mrt_in was taken");
  if (xh_thermal_comfort(ctx, 3, 4, 4, 1, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, 0, 0, 4) != XH_ERR_ARG) fail("utci without mrt or radiation was taken");
  if (xh_thermal_comfort(ctx, 3, 4, 4, 1, 0, 0, 0, 0, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, x, 0, 4) != XH_ERR_ARG) fail("mrt without the solar tables was taken");
  if (xh_thermal_comfort(ctx, 3, 4, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, x, x, 0, 1, 0, 0, 0, 0, x, 4) != XH_ERR_ARG) fail("sub-daily rows without lon were taken");
  if (xh_thermal_comfort(ctx, 3, 4, 4, 1, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4) != XH_ERR_ARG) fail("no output was taken");
  if (xh_thermal_comfort(ctx, 0, 4, 4, 1, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, 0, 0, 4) != XH_ERR_ARG) fail("R = 0 was taken");
  if (xh_thermal_comfort(ctx, 3, 4, 3, 1, x, x, x, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, x, 0, 0, 4) != XH_ERR_LAYOUT) fail("ld < C was taken");
  free(x);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_cases() {
  const int64_t cells[] = {1, 65, 130};
  for (int64_t C : cells)
    for (int64_t R : {(int64_t)3, (int64_t)24}) {
      for (int mode = XH_THERMAL_DAILY; mode <= XH_THERMAL_SUBDAILY; ++mode)
        for (int stat = XH_THERMAL_SUNLIT; stat <= XH_THERMAL_INSTANT; ++stat)
          for (int outs = 1; outs < 8; ++outs) comfort<TE>(R, C, mode, stat, outs, false);
      comfort<TE>(R, C, XH_THERMAL_DAILY, XH_THERMAL_SUNLIT, 1, true);       // utci from mrt: no table at all
      comfort<TE>(R, C, XH_THERMAL_SUBDAILY, XH_THERMAL_SUNLIT, 1 | 4, true);   // ... and the cosine next to it
      esat<TE>(R, C);
    }
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  refusals();
  printf("%d cases clean\n", g_cases);
  return 0;
}
