// compound_driver — the four entry points of compound.hip on the host simulation under the compiler's sanitizers (TEST
// INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_compound_cpu.py
// links it with compound.hip (compiled like the fiber units: the ring of k_blowing_snow is dynamic LDS) and sim_runtime.cpp,
// everything compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every table one of exactly ndoy * C, every output one of exactly
// P * C and every host table one of exactly its length, so that a read one row before the first, one element past the last row
// (the 16-byte lanes of xh_compound_doy_days on a row whose length is no multiple of the lane) or one entry past a table lands in
// a redzone; the dynamic LDS of a launch is a heap block of exactly its size, so a ring slot past the ring does too.  The cases:
// 1, 65, 130 and 132 cells (132: whole 16-byte lanes; 130: the partial last group; 65: the one-cell walk), float32 and float64,
// every one of the 15 output sets with the tables it does not need NULL, periods that start on row 0 and end on row T - 1, empty
// periods, a one-row series; the start row on the first and on the last row of a period and absent; windows 1, 2 and
// XH_BS_MAX_WINDOW with and without flags, periods shorter than the window.  The program checks the return codes and a few
// properties that need no reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "units/xclim_hip_compound.h"

const char* const kProgram = "compound_driver";

namespace {

template <typename TE>
void run(int64_t T, int64_t C, const std::vector<int64_t>& seg) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  const int64_t P = (int64_t)seg.size() - 1, ndoy = 366;
  TE* tas = field<TE>(T, C, 11u + (unsigned)T, 270.0, 30.0);
  TE* pr = field<TE>(T, C, 12u + (unsigned)C, 0.0, 2e-4);
  double* tab[4];
  for (int k = 0; k < 4; ++k) tab[k] = field<double>(ndoy, C, 20u + (unsigned)k, k < 2 ? 278.0 + 8.0 * k : 4e-5 * (k - 1), k < 2 ? 6.0 : 4e-5);
  std::vector<int32_t> tidx((size_t)T), doy((size_t)T);
  for (int64_t t = 0; t < T; ++t) doy[(size_t)t] = (int32_t)((t + 300) % 366) + 1, tidx[(size_t)t] = doy[(size_t)t] - 1;
  int64_t* hseg = exact(seg);
  int32_t *hti = exact(tidx), *hdy = exact(doy);
  double* out[4];
  for (int k = 0; k < 4; ++k) out[k] = block<double>(P * C);
  double* one = block<double>(P * C);

  // ---- xh_compound_doy_days: all four, then every other set against them
  ok(xh_compound_doy_days(ctx, T, C, C, f64, tas, pr, ndoy, C, tab[0], tab[1], tab[2], tab[3], hti, P, hseg, out[0], out[1], out[2], out[3], C),
     "xh_compound_doy_days");
  for (int64_t p = 0; p < P; ++p)
    for (int64_t c = 0; c < C; ++c) {
      const double n = (double)(seg[(size_t)p + 1] - seg[(size_t)p]);
      double sum = 0;
      for (int k = 0; k < 4; ++k) {
        const double v = out[k][p * C + c];
        if (!(v >= 0 && v <= n && v == floor(v))) fail("a count outside 0 .. the rows of the period");
        sum += v;
      }
      if (sum > n) fail("the four exclusive counts exceed the rows of the period");
    }
  for (int mask = 1; mask < 15; ++mask) {
    const bool need[4] = {(mask & 9) != 0, (mask & 6) != 0, (mask & 3) != 0, (mask & 12) != 0};
    for (int k = 0; k < 4; ++k) {   // one requested output at a time into `one`, the others of the set into scratch blocks
      if (!(mask >> k & 1)) continue;
      double* scratch[4] = {nullptr, nullptr, nullptr, nullptr};
      std::vector<double*> made;
      for (int j = 0; j < 4; ++j)
        if ((mask >> j & 1) && j != k) made.push_back(scratch[j] = block<double>(P * C));
      scratch[k] = one;
      ok(xh_compound_doy_days(ctx, T, C, C, f64, tas, pr, ndoy, C, need[0] ? tab[0] : nullptr, need[1] ? tab[1] : nullptr, need[2] ? tab[2] : nullptr,
                              need[3] ? tab[3] : nullptr, hti, P, hseg, scratch[0], scratch[1], scratch[2], scratch[3], C),
         "xh_compound_doy_days (subset)");
      if (memcmp(one, out[k], sizeof(double) * (size_t)(P * C)) != 0) fail("an output of a subset differs from the fused launch");
      for (double* m : made) free(m);
    }
    ++g_cases;
  }

  // ---- xh_degree_exceedance_date: the start on the first row, on the last row, absent
  std::vector<double> never((size_t)(P > 0 ? P : 1), 300.0);
  double* hnv = exact(never);
  for (int where = 0; where < 3; ++where) {
    std::vector<int64_t> start((size_t)(P > 0 ? P : 1), -1);
    for (int64_t p = 0; p < P; ++p) {
      const int64_t r0 = seg[(size_t)p], r1 = seg[(size_t)p + 1];
      if (r1 > r0 && where < 2) start[(size_t)p] = where == 0 ? r0 : r1 - 1;
    }
    int64_t* hst = exact(start);
    for (int below = 0; below < 2; ++below) {
      ok(xh_degree_exceedance_date(ctx, T, C, C, f64, tas, 280.0, below, 150.0, P, hseg, hst, hnv, hdy, one, C), "xh_degree_exceedance_date");
      for (int64_t i = 0; i < P * C; ++i) {
        const double v = one[i];
        if (!isnan(v) && !(v >= 1 && v <= 366 && v == floor(v))) fail("a date outside 1 .. 366");
        if (where == 2 && !isnan(v)) fail("a date in a period without the start date");
      }
      ++g_cases;
    }
    free(hst);
  }

  // ---- xh_blowing_snow_days
  std::vector<uint8_t> fl((size_t)(T > 0 ? T : 1));
  for (int64_t t = 0; t < T; ++t) fl[(size_t)t] = (uint8_t)((t / 45) % 2);
  uint8_t* hfl = exact(fl);
  for (int w : {1, 2, XH_BS_MAX_WINDOW}) {
    ok(xh_blowing_snow_days(ctx, T, C, C, f64, tas, pr, 1.0, 5e-5, w, P, hseg, nullptr, out[0], C), "xh_blowing_snow_days");
    ok(xh_blowing_snow_days(ctx, T, C, C, f64, tas, pr, 1.0, 5e-5, w, P, hseg, hfl, one, C), "xh_blowing_snow_days (flags)");
    for (int64_t p = 0; p < P; ++p)
      for (int64_t c = 0; c < C; ++c) {
        const double all = out[0][p * C + c], sel = one[p * C + c], n = (double)(seg[(size_t)p + 1] - seg[(size_t)p]);
        if (!(all >= 0 && all <= n) || !(sel >= 0 && sel <= all)) fail("a blowing-snow count outside its bounds");
        if (seg[(size_t)p + 1] <= w && all != 0) fail("a count on rows without a full window");
      }
    ++g_cases;
  }

  // ---- xh_pair_period_sum
  ok(xh_pair_period_sum(ctx, T, C, C, f64, pr, pr, 86400.0, P, hseg, one, C), "xh_pair_period_sum");
  for (int64_t i = 0; i < P * C; ++i)
    if (!(one[i] >= 0)) fail("a sum of amounts that is negative or NaN");
  ++g_cases;

  free(tas), free(pr), free(hseg), free(hti), free(hdy), free(one), free(hnv), free(hfl);
  for (int k = 0; k < 4; ++k) free(tab[k]), free(out[k]);
  xh_destroy(ctx);
}

template <typename TE>
void all() {
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)130, (int64_t)132}) {
    const int64_t T = 800;
    run<TE>(T, C, {0, 0, T / 2, T / 2, T - 69, T, T});   // periods on row 0 and on row T - 1, empty ones between
    run<TE>(T, C, {0, T});
    run<TE>(40, C, {0, 1, 3, 10, 40});                   // periods shorter than the windows
    run<TE>(1, C, {0, 1});
  }
}

}  // namespace

int main() {
  all<float>();
  all<double>();
  printf("compound_driver: %d cases clean\n", g_cases);
  return 0;
}
