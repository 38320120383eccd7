// phase_driver — the two entry points of phase.hip on the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE
// ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_phase_cpu.py links it with
// phase.hip (thread by thread: the kernels keep their tables in global memory and have no barrier) and sim_runtime.cpp, everything
// compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every output one of exactly its rows * C, every table one of exactly
// its length and the land bytes one of exactly C, so that a read one row before the first (the warm-up of rain on frozen ground at
// row 0), one element past the last row or one entry past a table (the auer nodes, the dai coefficients, the season and
// day-of-year rows) lands in a redzone.  The cases: a one-row series, periods on row 0 and on row T - 1, empty periods, one row
// per period, the frozen-ground warm-up at row 0 and across a period boundary with windows 1, 7 and one longer than the series,
// every method, 1, 65 and 260 cells (the 16-byte and the scalar paths of the map), float32 and float64, all outputs and each
// alone.  The program checks the return codes and a few properties that need no reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "xclim_hip_phase.h"

const char* const kProgram = "phase_driver";

namespace {

// the auer table of the reference: -273.15, 100 nodes from 0 in steps of 0.06, 6, 1e10; values that fall from 1 to 0
std::vector<double> auer_table() {
  std::vector<double> t(206);
  t[0] = -273.15, t[101] = 6.0, t[102] = 1e10;
  for (int k = 0; k < 100; ++k) t[(size_t)k + 1] = 0.06 * k;
  for (int k = 0; k < 103; ++k) t[(size_t)103 + k] = k == 0 ? 1.0 : (k >= 101 ? 0.0 : 1.0 - (double)k / 101.0);
  return t;
}

std::vector<double> dai_table() {
  std::vector<double> t(XH_PHASE_DAI_NTAB);
  for (int s = 0; s < XH_PHASE_DAI_NTAB / 6; ++s) {
    const bool rain = s >= 8;
    const double k[6] = {-48.0 + 0.1 * s, rain ? -0.7 : 0.7, 1.0 + 0.05 * s, 1.02, rain ? 0.1 : 0.2, rain ? 0.8 : 0.6};
    for (int j = 0; j < 6; ++j) t[(size_t)s * 6 + j] = k[j];
  }
  return t;
}

template <typename TE>
void run(int64_t T, int64_t C, const std::vector<int64_t>& seg, int window) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  const int64_t P = (int64_t)seg.size() - 1;
  TE* pr = field<TE>(T, C, 17u + (unsigned)(T * 3 + C), 0.0, 6.0);
  TE* tas = field<TE>(T, C, 5u + (unsigned)(T + C), -4.0, 9.0);   // degC: both sides of every threshold
  std::vector<int32_t> dy((size_t)T);
  std::vector<uint8_t> se((size_t)T), la((size_t)C);
  for (int64_t r = 0; r < T; ++r) dy[(size_t)r] = (int32_t)(r % 366) + 1, se[(size_t)r] = (uint8_t)((r / 90) % 4);
  for (int64_t c = 0; c < C; ++c) la[(size_t)c] = (uint8_t)(c % 3 != 0);
  int64_t* hseg = exact(seg);
  int32_t* hdy = exact(dy);
  uint8_t *hse = exact(se), *hla = exact(la);
  const std::vector<double> auer = auer_table(), dai = dai_table();
  double *hauer = exact(auer), *hdai = exact(dai);
  // thresh, upper, add_K, sub_C, clip, land; auer with thresh = -1 and add_K = 0: dtas = tas + 1 lies on both sides of the nodes
  const std::vector<double> par = {0.5, 2.5, 0.0, 0.0, 1.0, 1.0}, par_auer = {-1.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lim = {0.3, 1e9, 0.9, 0.5, 1.0, 0.5, 0.0};
  double *hpar_all = exact(par), *hpar_auer = exact(par_auer), *hlim = exact(lim);
  double* out[XH_PHASE_NOUT];
  for (int k = 0; k < XH_PHASE_NOUT; ++k) out[k] = block<double>(P * C);
  std::vector<void*> ptrs(out, out + XH_PHASE_NOUT);
  void** houts = exact(ptrs);

  for (int method = XH_PHASE_BINARY; method <= XH_PHASE_GIVEN; ++method) {
    const bool is_auer = method == XH_PHASE_AUER, is_dai = method == XH_PHASE_DAI_ANNUAL || method == XH_PHASE_DAI_SEASONAL;
    const double* hpar = is_auer ? hpar_auer : hpar_all;
    const double* tab = is_auer ? hauer : (is_dai ? hdai : nullptr);
    const int64_t ntab = is_auer ? 103 : (is_dai ? XH_PHASE_DAI_NTAB : 0);
    const uint8_t* season = method == XH_PHASE_DAI_SEASONAL ? hse : nullptr;
    const uint8_t* land = is_dai && C > 1 ? hla : nullptr;
    const uint32_t all = method == XH_PHASE_GIVEN ? (1u << XH_PHASE_HPLT_DAYS) - 1 : (1u << XH_PHASE_NOUT) - 1;
    // all outputs, then each alone
    for (int k = -1; k < XH_PHASE_NOUT; ++k) {
      const uint32_t mask = k < 0 ? all : (1u << k);
      if (!(mask & all)) continue;
      for (int j = 0; j < XH_PHASE_NOUT; ++j) memset(out[j], 0x7B, sizeof(double) * (size_t)(P * C > 0 ? P * C : 1));
      ok(xh_precip_phase_period(ctx, T, C, C, f64, pr, tas, 1.0, P, hseg, hdy, method, hpar, tab, ntab, season, land, hlim, window, mask, houts,
                                C),
         "xh_precip_phase_period");
      for (int j = 0; j < XH_PHASE_NOUT; ++j)
        for (int64_t i = 0; i < P * C; ++i) {
          const double v = out[j][i];
          const bool date = j == XH_PHASE_FIRST_SNOW || j == XH_PHASE_LAST_SNOW;
          if (!(mask & (1u << j))) {
            uint64_t bits;
            memcpy(&bits, &v, 8);
            if (bits != 0x7B7B7B7B7B7B7B7BULL) fail("an output that was not asked for was written");
          } else if (date ? !(v != v || (v >= 1 && v <= 366)) : !(v == v && v < 1e12)) {
            fail("an output is out of range");
          } else if (j >= XH_PHASE_PR_N && j <= XH_PHASE_SNOW_DAYS && (v < 0 || v > (double)(seg[(size_t)(i / C) + 1] - seg[(size_t)(i / C)]))) {
            fail("a count exceeds the rows of its period");
          }
        }
      ++g_cases;
    }
    if (method == XH_PHASE_GIVEN) continue;
    // the map: both outputs, then each alone
    const size_t osz = method == XH_PHASE_BINARY ? sizeof(TE) : sizeof(double);
    for (int which = 0; which < 3; ++which) {
      void* snow = which != 2 ? malloc(osz * (size_t)(T * C)) : nullptr;   // EXACTLY (T, C)
      void* rain = which != 1 ? malloc(osz * (size_t)(T * C)) : nullptr;
      ok(xh_precip_phase_map(ctx, T, C, C, f64, pr, tas, method, hpar, tab, ntab, season, land, snow, rain, C), "xh_precip_phase_map");
      if (method == XH_PHASE_BINARY && snow && rain)
        for (int64_t i = 0; i < T * C; ++i) {
          const TE s = ((TE*)snow)[i], l = ((TE*)rain)[i], x = pr[i];
          if (x == x && !((s == x && l == 0) || (s == 0 && l == x))) fail("binary: a sample is neither all snow nor all rain");
        }
      free(snow), free(rain);
      ++g_cases;
    }
  }
  for (int k = 0; k < XH_PHASE_NOUT; ++k) free(out[k]);
  free(pr), free(tas), free(hseg), free(hdy), free(hse), free(hla), free(hauer), free(hdai), free(hpar_all), free(hpar_auer), free(hlim), free(houts);
  xh_destroy(ctx);
}

template <typename TE>
void all_shapes() {
  run<TE>(1, 1, {0, 1}, 7);                                    // a one-row series
  run<TE>(1, 65, {0, 0, 1, 1}, 1);
  run<TE>(40, 65, {0, 13, 13, 40}, 7);                         // periods on row 0 and on row T - 1, an empty one; warm-up at row 0
  run<TE>(40, 260, {0, 3, 40}, 7);                             // a first period shorter than the window: the warm-up stops at row 0
  run<TE>(23, 260, {2, 9, 21}, 50);                            // rows outside every period; a window longer than the series
  std::vector<int64_t> each(18);
  for (int64_t r = 0; r < 18; ++r) each[(size_t)r] = r;
  run<TE>(17, 4, each, 2);                                     // one row per period (16-byte loads of the map: 4 cells)
  run<TE>(400, 1, {0, 200, 400}, 7);
}

}  // namespace

int main() {
  all_shapes<float>();
  all_shapes<double>();
  printf("phase_driver: %d cases clean\n", g_cases);
  return 0;
}
