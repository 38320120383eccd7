// bioclim_driver — xh_bioclim of the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE ONLY).
// A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_units_cpu.py links it with
// bioclim.hip and sim_runtime.cpp, everything compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements and every output one of exactly P * C, so that a read one row before
// the first (the lead-in of a period's first quarter is where it would hide) or one element past the last row (the last bin of
// one day) lands in a redzone.  The cases: a daily series that starts on 1999-03-15 and runs 1002 days (143 bins of seven days
// and one of a single day) with years from January and from July; a series of 80 days, shorter than a quarter; a monthly
// series with W = 3; float32 and float64; every output requested, and the quarter outputs alone.  The program checks the
// return code and two properties that need no reference (the quarters of the short series are NaN, their step indices -1);
// a sanitizer report aborts it.
#include "driver_common.h"

const char* const kProgram = "bioclim_driver";

namespace {

template <typename TE>
void run(int64_t T, int64_t C, const std::vector<int64_t>& step_off, const std::vector<int64_t>& seg_rows, int binned, int W,
         bool quarters_only, bool expect_no_quarter) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int64_t S = (int64_t)step_off.size() - 1, P = (int64_t)seg_rows.size() - 1;
  std::vector<int64_t> seg_steps(P + 1);
  for (int64_t p = 0; p <= P; ++p) {   // a step belongs to the period of its first row
    int64_t s = 0;
    while (s < S && step_off[s] < seg_rows[p]) ++s;
    seg_steps[p] = s;
  }
  std::vector<double> factor((size_t)T, 86400.0);
  TE* tas = field<TE>(T, C, 1u, 270.0, 30.0);
  TE* tn = field<TE>(T, C, 2u, 265.0, 20.0);
  TE* tx = field<TE>(T, C, 3u, 285.0, 20.0);
  TE* pr = field<TE>(T, C, 4u, 0.0, 1e-4);
  double* out[19];
  int32_t *which[4], *count[4];
  const bool is_quarter[19] = {0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1};
  for (int k = 0; k < 19; ++k) out[k] = (!quarters_only || is_quarter[k]) ? (double*)malloc(sizeof(double) * (size_t)(P * C)) : nullptr;
  for (int k = 0; k < 4; ++k) {
    which[k] = (int32_t*)malloc(sizeof(int32_t) * (size_t)(P * C));
    count[k] = quarters_only ? nullptr : (int32_t*)malloc(sizeof(int32_t) * (size_t)(P * C));
  }
  const int rc = xh_bioclim(ctx, T, C, C, sizeof(TE) == 8, tas, quarters_only ? nullptr : tn, quarters_only ? nullptr : tx, pr, S,
                            step_off.data(), factor.data(), binned, P, seg_rows.data(), seg_steps.data(), W, 0.0, 86400.0, 1e-5, out,
                            which, count, C);
  if (rc != XH_OK) {
    fprintf(stderr, "bioclim_driver: xh_bioclim returned %d: %s\n", rc, xh_last_error());
    exit(3);
  }
  if (expect_no_quarter)
    for (int64_t i = 0; i < P * C; ++i)
      if (!isnan(out[9][i]) || !isnan(out[15][i]) || which[0][i] != -1 || which[3][i] != -1) {
        fprintf(stderr, "bioclim_driver: a quarter in a series shorter than one\n");
        exit(4);
      }
  for (int k = 0; k < 19; ++k) free(out[k]);
  for (int k = 0; k < 4; ++k) free(which[k]), free(count[k]);
  free(tas), free(tn), free(tx), free(pr);
  xh_destroy(ctx);
  ++g_cases;
}

std::vector<int64_t> bins(int64_t T, int64_t n) {
  std::vector<int64_t> so;
  for (int64_t r = 0; r < T; r += n) so.push_back(r);
  so.push_back(T);
  return so;
}

template <typename TE>
void all_cases() {
  for (int q = 0; q < 2; ++q) {
    // 1999-03-15 + 1002 days: 2000-01-01 is row 292, 2001-01-01 row 658; 1999-07-01 row 108, 2000-07-01 row 474, 2001-07-01 row 839
    run<TE>(1002, 5, bins(1002, 7), {0, 292, 658, 1002}, 1, 13, q == 1, false);
    run<TE>(1002, 5, bins(1002, 7), {0, 108, 474, 839, 1002}, 1, 13, q == 1, false);
    run<TE>(1002, 260, bins(1002, 7), {0, 108, 474, 839, 1002}, 1, 13, q == 1, false);
    // 2001-02-01 + 80 days: eleven bins of seven days and one of three, no quarter
    run<TE>(80, 5, bins(80, 7), {0, 80}, 1, 13, q == 1, true);
    // 30 months from 2000-03: years of 10, 12 and 8 rows, W = 3
    run<TE>(30, 5, bins(30, 1), {0, 10, 22, 30}, 0, 3, q == 1, false);
  }
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  printf("%d cases clean\n", g_cases);
  return 0;
}
