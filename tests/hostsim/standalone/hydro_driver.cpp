// hydro_driver — the four entry points of hydro.hip on the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE
// ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_units_cpu.py links it with
// hydro.hip (on fibers: k_sen_slope sorts in LDS behind barriers) and sim_runtime.cpp, everything compiled with -g -O1
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every output one of exactly its rows * C and every table one of
// exactly its length, so that a read one row before the first, one element past the last row or one entry past a table lands
// in a redzone; the dynamic LDS of a launch is a heap block of exactly its size.  The cases: periods that start on row 0 and
// end on row T - 1 (the 7-day window, the melt window and the API halo reach outside the series there), empty periods,
// series of 1, 5, 400 and 800 rows, windows 1, 3, 7, 31 and 32 (all five at 65 cells, 3 and 32 everywhere), Sen series of 0, 1,
// 2, 3, 30, 64 and 181 years with absent years; float32 and float64; 1, 65 and 260 cells (1, 5 and 9 for the Sen slope: a workgroup of 64 fibers per series).  The program checks the return codes and a few properties that need no
// reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "xclim_hip_hydro.h"

const char* const kProgram = "hydro_driver";

namespace {

template <typename TE>
void run_fields(int64_t T, int64_t C, const std::vector<int64_t>& seg, bool every_window) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  const int64_t P = (int64_t)seg.size() - 1;
  TE* q = field<TE>(T, C, 11u, 5.0, 90.0);
  TE* snw = field<TE>(T, C, 12u, 0.0, 120.0);
  TE* pr = field<TE>(T, C, 13u, 0.0, 2e-4);
  int64_t* hseg = exact(seg);

  double *bfi = block<double>(P * C), *rbi = block<double>(P * C), *mean = block<double>(P * C), *sum = block<double>(P * C);
  int32_t* valid = block<int32_t>(P * C);
  ok(xh_flow_period_stats(ctx, T, C, C, f64, q, P, hseg, bfi, rbi, mean, sum, valid, C), "xh_flow_period_stats");
  ok(xh_flow_period_stats(ctx, T, C, C, f64, q, P, hseg, nullptr, rbi, nullptr, nullptr, nullptr, C), "xh_flow_period_stats (rbi)");
  for (int64_t p = 0; p < P; ++p)
    for (int64_t c = 0; c < C; ++c) {
      const int64_t o = p * C + c, rows = seg[(size_t)p + 1] - seg[(size_t)p];
      if (valid[o] < 0 || valid[o] > rows) fail("valid outside the rows of the period");
      if (valid[o] > 0 && !(mean[o] >= 5.0 && mean[o] <= 95.0)) fail("mean outside the range of the field");
      if (valid[o] == 0 && (!isnan(mean[o]) || !isnan(bfi[o]) || sum[o] != 0.0)) fail("an empty period with a value");
      if (!isnan(bfi[o]) && !(bfi[o] > 0.0 && bfi[o] < 3.0)) fail("bfi out of range");
      if (!isnan(rbi[o]) && rbi[o] < 0.0) fail("rbi negative");
    }
  ++g_cases;

  static const int windows[] = {1, 3, 7, 31, XH_HYDRO_MAX_WINDOW};
  double* mx = block<double>(P * C);
  double* api = block<double>(T * C);
  for (int w : windows) {
    if (!every_window && w != 3 && w != XH_HYDRO_MAX_WINDOW) continue;
    for (int with_pr = 0; with_pr < 2; ++with_pr) {
      ok(xh_melt_period_max(ctx, T, C, C, f64, snw, with_pr ? pr : nullptr, 86400.0, w, P, hseg, mx, C), "xh_melt_period_max");
      for (int64_t i = 0; i < P * C; ++i)
        if (!isnan(mx[i]) && !(fabs(mx[i]) <= 120.0 * w + 20.0 * w)) fail("melt maximum out of range");
      for (int64_t p = 0; p < P; ++p)
        if (seg[(size_t)p + 1] <= w)   // every row of the period has i - w + 1 < 1
          for (int64_t c = 0; c < C; ++c)
            if (!isnan(mx[p * C + c])) fail("a melt maximum before the first full window");
      ++g_cases;
    }
    std::vector<double> wt((size_t)w);
    for (int k = 0; k < w; ++k) wt[(size_t)k] = pow(0.935, w - 1 - k);
    double* hw = exact(wt);
    ok(xh_antecedent_precip(ctx, T, C, C, f64, pr, 86400.0, w, hw, api, C), "xh_antecedent_precip");
    for (int64_t i = 0; i < T; ++i)
      for (int64_t c = 0; c < C; ++c) {
        const double v = api[i * C + c];
        if (i < w - 1 && !isnan(v)) fail("an API value before the window is full");
        if (!isnan(v) && !(v >= 0.0 && v <= 2e-4 * 86400.0 * w)) fail("API out of range");
      }
    free(hw);
    ++g_cases;
  }
  free(q), free(snw), free(pr), free(hseg), free(bfi), free(rbi), free(mean), free(sum), free(valid), free(mx), free(api);
  xh_destroy(ctx);
}

template <typename TE>
void run_sen(int64_t Y, int64_t K, int64_t C) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  // season k of year y is row y * K + k; the first year of season 0 and every seventh year of the last season are absent
  const int64_t P = Y * K;
  std::vector<int64_t> po((size_t)(Y * K));
  for (int64_t y = 0; y < Y; ++y)
    for (int64_t k = 0; k < K; ++k) po[(size_t)(y * K + k)] = ((k == 0 && y == 0) || (k == K - 1 && y % 7 == 3)) ? -1 : y * K + k;
  int64_t* hpo = exact(po);
  TE* x = field<TE>(P, C, 21u, 0.0, 10.0);
  for (int64_t r = 0; r < P; ++r)
    for (int64_t c = 0; c < C; ++c)
      if (x[r * C + c] == x[r * C + c]) x[r * C + c] += (TE)(0.5 * (double)(r / (K > 0 ? K : 1)));   // a trend
  double *slope = block<double>(K * C), *pv = block<double>(K * C);
  int32_t* n = block<int32_t>(K * C);
  ok(xh_sen_slope(ctx, P, C, C, f64, x, Y, K, hpo, slope, pv, n, C), "xh_sen_slope");
  ok(xh_sen_slope(ctx, P, C, C, f64, x, Y, K, hpo, slope, nullptr, nullptr, C), "xh_sen_slope (slope)");
  for (int64_t i = 0; i < K * C; ++i) {
    if (n[i] < 0 || n[i] > Y) fail("n outside the years");
    if ((n[i] < 2) != (isnan(slope[i]) != 0) || (n[i] < 2) != (isnan(pv[i]) != 0)) fail("NaN exactly below two values");
    if (n[i] >= 2 && !(pv[i] >= 0.0 && pv[i] <= 1.0)) fail("p outside [0, 1]");
    if (n[i] >= 2 && !(fabs(slope[i]) <= 10.5)) fail("slope out of range");
  }
  free(hpo), free(x), free(slope), free(pv), free(n);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all() {
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)260}) {
    const int64_t T = C == 260 ? 400 : 800;                            // (two workgroups of cells: half the rows)
    run_fields<TE>(T, C, {0, 0, T / 2, T / 2, T - 69, T, T}, C == 65);     // periods on row 0 and on row T - 1, empty ones between
    run_fields<TE>(5, C, {0, 5}, true);                                // a series shorter than the 7-day window
    run_fields<TE>(1, C, {0, 1}, C == 65);
    if (C == 260) continue;
    run_fields<TE>(T, C, {0, 10, 15, 45, T}, false);                   // periods shorter than the windows
    for (int64_t Y : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)64}) run_sen<TE>(Y, 2, C == 65 ? 9 : C);
  }
  run_sen<TE>(XH_SEN_MAX_YEARS, 1, 3);
  run_sen<TE>(30, 4, 5);
}

}  // namespace

int main() {
  all<float>();
  all<double>();
  printf("hydro_driver: %d cases clean\n", g_cases);
  return 0;
}
