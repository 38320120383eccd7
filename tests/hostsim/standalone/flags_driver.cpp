// flags_driver — the two entry points of dataflags.hip on the host simulation under the compiler's sanitizers (TEST
// INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_flags_cpu.py links
// it with dataflags.hip (unchanged, thread by thread) and sim_runtime.cpp, everything compiled with -g -O1
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every table one of exactly its rows * C, every output one of exactly
// K * P * C (or K * P) bytes and every host table one of exactly its length, so that a read one row before the first, one element
// past the last row, a store into a period that does not exist or one entry past a table lands in a redzone.  The cases: runs of
// equal values that touch row 0 and row T - 1 and runs longer than a period; every row a period of its own (P = T: a run that
// reaches n stores into the n - 1 periods behind it); empty periods at both ends; the windows of xh_doy_bounds on the first and the
// last days of the series (rows before row 0 and after row T - 1), windows with and without a kernel of their own and one longer
// than the series; 1, 65 and 260 cells; float32 and float64.  The program checks the return codes and properties that need no
// reference (the reduced flags are the `any` over the cells, the period flags the `any` over the rows of the element-wise ones,
// every row belongs to a run of one); a sanitizer report aborts it.
#include "driver_common.h"
#include "xclim_hip_flags.h"

const char* const kProgram = "flags_driver";

namespace {

// a seasonal series with noise on a coarse grid (so that values repeat by chance), planted runs on row 0 and on row T - 1 and
// about one NaN in 97
template <typename TE>
TE* series(int64_t T, int64_t C, unsigned seed) {
  TE* p = (TE*)malloc(sizeof(TE) * (size_t)(T * C > 0 ? T * C : 1));   // EXACTLY the field
  unsigned s = seed;
  for (int64_t t = 0; t < T; ++t)
    for (int64_t c = 0; c < C; ++c) {
      s = s * 1664525u + 1013904223u;
      const double v = 280.0 + 10.0 * sin(6.283185307179586 * (double)t / 365.25) + (double)((s >> 10) % 9) * 0.5;
      p[t * C + c] = (s >> 8) % 97 == 0 ? (TE)NAN : (TE)v;
    }
  for (int64_t c = 0; c < C; ++c) {
    const int64_t n = 3 + c % 6;
    for (int64_t t = 0; t < n && t < T; ++t) p[t * C + c] = (TE)291.0;             // a run on row 0
    for (int64_t t = T - n < 0 ? 0 : T - n; t < T; ++t) p[t * C + c] = (TE)250.0;  // a run that ends on row T - 1
    if (c % 5 == 2)
      for (int64_t t = T / 3; t < T / 3 + T / 2; ++t) p[t * C + c] = (TE)300.0;    // a run longer than a period
  }
  return p;
}

template <typename TE>
void run(int64_t T, int64_t C, const std::vector<int64_t>& seg, int window) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  const int64_t P = (int64_t)seg.size() - 1;
  TE *x = series<TE>(T, C, 17u + (unsigned)T), *y0 = series<TE>(T, C, 5u), *y1 = series<TE>(T, C, 9u);

  // the bound tables: two years of up to 366 days, the second possibly cut; day d of year y is row y * 366 + d
  const int nyears = 2, ndoy = (int)(T < 366 ? T : 366);
  std::vector<int32_t> tb((size_t)nyears * (size_t)ndoy, -1), ti((size_t)T);
  for (int64_t t = 0; t < T; ++t) {
    if (t / ndoy < nyears) tb[(size_t)((t / ndoy) * ndoy + t % ndoy)] = (int32_t)t;
    ti[(size_t)t] = (int32_t)(t % ndoy);
  }
  int32_t *htb = exact(tb), *hti = exact(ti);
  TE *lo = block<TE>((int64_t)ndoy * C), *hi = block<TE>((int64_t)ndoy * C);
  ok(xh_doy_bounds(ctx, T, C, C, f64, x, htb, nyears, ndoy, window, 3.0, lo, hi, C), "xh_doy_bounds");
  for (int64_t i = 0; i < (int64_t)ndoy * C; ++i) {
    if (isnan(lo[i]) != isnan(hi[i])) fail("one bound without the other");
    if (!isnan(lo[i]) && !(lo[i] <= hi[i])) fail("bounds out of order");
  }

  const std::vector<xh_flag_check> chk = {
      {XH_FLAG_CMP, XH_OP_GT, 0, 0, 289.0, 0.0},     {XH_FLAG_OUTSIDE, 0, 0, 0, 272.0, 292.0}, {XH_FLAG_PAIR, XH_OP_LT, 0, 0, 0.0, 0.0},
      {XH_FLAG_PAIR, XH_OP_NE, 0, 1, 0.0, 0.0},      {XH_FLAG_REPEAT, -1, 1, 0, 0.0, 0.0},     {XH_FLAG_REPEAT, -1, 3, 0, 0.0, 0.0},
      {XH_FLAG_REPEAT, XH_OP_GE, 8, 0, 291.0, 0.0},  {XH_FLAG_REPEAT, -1, (int32_t)(T > 1 ? T / 2 : 1), 0, 0.0, 0.0}, {XH_FLAG_CLIM, 0, 0, 0, 0.0, 0.0},
      {XH_FLAG_REPEAT, XH_OP_LT, 2, 0, 260.0, 0.0}};
  const int K = (int)chk.size();
  xh_flag_check* hchk = exact(chk);
  int64_t* hseg = exact(seg);
  std::vector<int64_t> rows((size_t)T + 1);
  for (int64_t t = 0; t <= T; ++t) rows[(size_t)t] = t;
  int64_t* hrows = exact(rows);

  uint8_t *per = block<uint8_t>((int64_t)K * P * C), *red = block<uint8_t>((int64_t)K * P);
  uint8_t *elem = block<uint8_t>((int64_t)K * T * C), *ered = block<uint8_t>((int64_t)K * T);
  ok(xh_data_flags(ctx, T, C, C, f64, x, y0, C, y1, C, K, hchk, P, hseg, hti, ndoy, lo, hi, C, 0, per, C), "xh_data_flags (periods)");
  ok(xh_data_flags(ctx, T, C, C, f64, x, y0, C, y1, C, K, hchk, P, hseg, hti, ndoy, lo, hi, C, 1, red, C), "xh_data_flags (periods, reduced)");
  ok(xh_data_flags(ctx, T, C, C, f64, x, y0, C, y1, C, K, hchk, T, hrows, hti, ndoy, lo, hi, C, 0, elem, C), "xh_data_flags (rows)");
  ok(xh_data_flags(ctx, T, C, C, f64, x, y0, C, y1, C, K, hchk, T, hrows, hti, ndoy, lo, hi, C, 1, ered, C), "xh_data_flags (rows, reduced)");
  for (int k = 0; k < K; ++k) {
    for (int64_t t = 0; t < T; ++t) {
      uint8_t any = 0;
      for (int64_t c = 0; c < C; ++c) {
        const uint8_t f = elem[((int64_t)k * T + t) * C + c];
        if (f > 1) fail("a flag that is neither 0 nor 1");
        if (k == 4 && f != 1) fail("a row that belongs to no run of one");
        any |= f;
      }
      if (ered[(int64_t)k * T + t] != any) fail("the reduced row flag is not the `any` over the cells");
    }
    for (int64_t p = 0; p < P; ++p) {
      uint8_t all = 0;
      for (int64_t c = 0; c < C; ++c) {
        uint8_t any = 0;
        for (int64_t t = seg[(size_t)p]; t < seg[(size_t)p + 1]; ++t) any |= elem[((int64_t)k * T + t) * C + c];
        if (per[((int64_t)k * P + p) * C + c] != any) fail("the period flag is not the `any` over its rows");
        all |= any;
      }
      if (red[(int64_t)k * P + p] != all) fail("the reduced period flag is not the `any` over the cells");
    }
  }
  const int64_t n0 = 3;   // the planted runs: at least three rows from row 0 and up to row T - 1 in every cell
  if (T >= 2 * n0)
    for (int64_t c = 0; c < C; ++c)
      for (int64_t t = 0; t < n0; ++t)
        if (!elem[(5 * T + t) * C + c] || !elem[(5 * T + T - 1 - t) * C + c]) fail("a planted run at an end of the series is not flagged");
  ++g_cases;
  free(x), free(y0), free(y1), free(htb), free(hti), free(lo), free(hi), free(hchk), free(hseg), free(hrows);
  free(per), free(red), free(elem), free(ered);
  xh_destroy(ctx);
}

template <typename TE>
void all() {
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)260}) {
    const int64_t T = C == 260 ? 400 : 800;
    run<TE>(T, C, {0, 0, T / 2, T / 2, T - 69, T, T}, 5);   // periods on row 0 and on row T - 1, empty ones at both ends and between
    run<TE>(T, C, {0, T}, C == 65 ? 3 : 7);
    run<TE>(T, C, {0, 1, 2, T - 1, T}, C == 1 ? 4 : 15);     // one-row periods at both ends; windows without a kernel of their own
    run<TE>(40, C, {0, 10, 40}, 101);                         // a window longer than the series
    run<TE>(1, C, {0, 1}, 5);
  }
}

}  // namespace

int main() {
  all<float>();
  all<double>();
  printf("flags_driver: %d cases clean\n", g_cases);
  return 0;
}
