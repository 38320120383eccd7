// rain_driver — the two entry points of rainseason.hip on the host simulation under the compiler's sanitizers (TEST
// INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_units_cpu.py links
// it with rainseason.hip (compiled like the fiber units: its ring is dynamic LDS) and sim_runtime.cpp, everything compiled with -g
// -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every output one of exactly its rows * C and every table one of
// exactly its length, so that a read one row before the first, one element past the last row or one entry past a table lands in
// a redzone; the dynamic LDS of a launch is a heap block of exactly its size, so a ring slot past the ring does too.  The
// cases: periods that start on row 0 and end on row T - 1, empty periods, periods shorter than every window, all four method
// combinations, every sum window at 1 and at XH_RAIN_MAX_WINDOW (all three at once: the largest ring), per-day windows of 33 and
// 400 rows (the second read of the decision row, a lag longer than the period), float32 and float64, 1, 65 and 260 cells, each
// output alone; the zones with windows 1, 30 and one longer than the series, two edges and XH_ZONES_MAX_EDGES.  The program
// checks the return codes and a few properties that need no reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "xclim_hip_rain.h"

const char* const kProgram = "rain_driver";

namespace {

// (this driver's own field, not the uniform one of driver_common.h)  wet spells of a few rows, long moist stretches, dry stretches and a few NaN, in mm per day
template <typename TE>
TE* field(int64_t T, int64_t C, unsigned seed) {
  TE* p = (TE*)malloc(sizeof(TE) * (size_t)(T * C > 0 ? T * C : 1));   // EXACTLY the field
  unsigned s = seed;
  for (int64_t c = 0; c < C; ++c) {
    int left = 0;
    double level = 0.0;
    for (int64_t t = 0; t < T; ++t) {
      s = s * 1664525u + 1013904223u;
      if (left == 0) {
        const unsigned k = (s >> 10) % 10;
        level = k < 2 ? 12.0 : (k < 7 ? 1.5 : 0.0);
        left = 1 + (int)((s >> 16) % (k < 2 ? 4 : 45));
      }
      --left;
      p[t * C + c] = (s >> 8) % 211 == 0 ? (TE)NAN : (TE)level;
    }
  }
  return p;
}

struct Windows {
  int ww, wnd, wd, ts, we, te;
};

template <typename TE>
void run_rain(int64_t T, int64_t C, const std::vector<int64_t>& seg, const std::vector<Windows>& sets) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  const int64_t P = (int64_t)seg.size() - 1;
  TE* pr = field<TE>(T, C, 31u + (unsigned)T);
  std::vector<uint8_t> fl((size_t)T);
  std::vector<int32_t> dy((size_t)T);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t r0 = seg[(size_t)p], n = seg[(size_t)p + 1] - r0;
    for (int64_t i = 0; i < n; ++i) {   // the start window: the last five sixths of the period; the bounds inside it
      uint8_t f = 0;
      if (i >= n / 6) f |= XH_RAIN_START_WINDOW;
      if (i >= n / 6 && i < n / 6 + (2 * n) / 3 + 1) f |= XH_RAIN_START_BOUNDS;
      if (i >= n / 3) f |= XH_RAIN_END_BOUNDS;
      fl[(size_t)(r0 + i)] = f;
    }
  }
  for (int64_t t = 0; t < T; ++t) dy[(size_t)t] = (int32_t)(t % 366) + 1;
  int64_t* hseg = exact(seg);
  uint8_t* hfl = exact(fl);
  int32_t* hdy = exact(dy);
  double *st = block<double>(P * C), *en = block<double>(P * C), *ln = block<double>(P * C), *one = block<double>(P * C);
  for (const Windows& w : sets) {
    ok(xh_rain_season(ctx, T, C, C, f64, pr, 1.0, P, hseg, hfl, hdy, 25.0, w.ww, w.wnd, 1.0, w.wd, w.ts, 0.0, w.we, w.te, st, en, ln, C),
       "xh_rain_season");
    for (int64_t p = 0; p < P; ++p)
      for (int64_t c = 0; c < C; ++c) {
        const int64_t o = p * C + c, n = seg[(size_t)p + 1] - seg[(size_t)p];
        const bool has = !isnan(st[o]);
        if (has != !isnan(ln[o])) fail("a length without a start, or a start without a length");
        if (!has && !isnan(en[o])) fail("an end without a start");
        if (has && !(st[o] >= 1 && st[o] <= 366)) fail("start outside 1 .. 366");
        if (has && !(ln[o] >= 1 && ln[o] <= (double)n)) fail("length outside the period");
        if (n == 0 && has) fail("a start in an empty period");
        if (!isnan(en[o]) && !(en[o] >= 1 && en[o] <= 366)) fail("end outside 1 .. 366");
      }
    // each output alone equals the launch with all three
    ok(xh_rain_season(ctx, T, C, C, f64, pr, 1.0, P, hseg, hfl, hdy, 25.0, w.ww, w.wnd, 1.0, w.wd, w.ts, 0.0, w.we, w.te, one, nullptr, nullptr, C),
       "xh_rain_season (start)");
    if (memcmp(one, st, sizeof(double) * (size_t)(P * C)) != 0) fail("start alone differs");
    ok(xh_rain_season(ctx, T, C, C, f64, pr, 1.0, P, hseg, hfl, hdy, 25.0, w.ww, w.wnd, 1.0, w.wd, w.ts, 0.0, w.we, w.te, nullptr, one, nullptr, C),
       "xh_rain_season (end)");
    if (memcmp(one, en, sizeof(double) * (size_t)(P * C)) != 0) fail("end alone differs");
    ok(xh_rain_season(ctx, T, C, C, f64, pr, 1.0, P, hseg, hfl, hdy, 25.0, w.ww, w.wnd, 1.0, w.wd, w.ts, 0.0, w.we, w.te, nullptr, nullptr, one, C),
       "xh_rain_season (length)");
    if (memcmp(one, ln, sizeof(double) * (size_t)(P * C)) != 0) fail("length alone differs");
    ++g_cases;
  }
  free(pr), free(hseg), free(hfl), free(hdy), free(st), free(en), free(ln), free(one);
  xh_destroy(ctx);
}

template <typename TE>
void run_zones(int64_t P, int64_t C, int nedges) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  TE* x = (TE*)malloc(sizeof(TE) * (size_t)(P * C > 0 ? P * C : 1));
  unsigned s = 77u;
  for (int64_t i = 0; i < P * C; ++i) {
    s = s * 1664525u + 1013904223u;
    x[i] = (s >> 8) % 53 == 0 ? (TE)NAN : (TE)(-30.0 + 60.0 * (double)(s >> 8) / (double)(1u << 24));
  }
  std::vector<double> e((size_t)nedges);
  for (int k = 0; k < nedges; ++k) e[(size_t)k] = -20.0 + 40.0 * k / (nedges - 1);
  double* he = exact(e);
  double* out = block<double>(P * C);
  for (int w : {1, 2, 30, (int)P + 3}) {
    ok(xh_rolling_zones(ctx, P, C, C, f64, x, w, nedges, he, out, C), "xh_rolling_zones");
    for (int64_t t = 0; t < P; ++t)
      for (int64_t c = 0; c < C; ++c) {
        const double z = out[t * C + c];
        if (t < w - 1 && !isnan(z)) fail("a zone before the window is full");
        if (!isnan(z) && !(z >= 0 && z <= nedges - 2 && z == floor(z))) fail("zone outside 0 .. nedges - 2");
      }
    ++g_cases;
  }
  free(x), free(he), free(out);
  xh_destroy(ctx);
}

template <typename TE>
void all() {
  const int M = XH_RAIN_MAX_WINDOW;
  const std::vector<Windows> methods = {{3, 30, 7, 0, 20, 0}, {3, 10, 7, 1, 5, 0}, {3, 10, 7, 0, 5, 1}, {3, 10, 7, 1, 5, 1}};
  const std::vector<Windows> limits = {{1, 0, 1, 1, 1, 1}, {M, 5, M, 1, M, 1}, {M, 5, M, 0, M, 0}, {2, 3, 33, 0, 33, 0}, {3, 30, 400, 0, 400, 0},
                                       {1, 0, 1, 0, 1, 0}, {M, 0, 1, 1, 2, 1}, {1, 2, M, 1, 1, 0}};
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)260}) {
    const int64_t T = C == 260 ? 400 : 800;
    run_rain<TE>(T, C, {0, 0, T / 2, T / 2, T - 69, T, T}, methods);       // periods on row 0 and on row T - 1, empty ones between
    run_rain<TE>(T, C, {0, T / 2, T}, limits);
    run_rain<TE>(40, C, {0, 1, 3, 10, 40}, C == 65 ? limits : methods);      // periods shorter than the windows
    run_rain<TE>(1, C, {0, 1}, methods);
    run_zones<TE>(31, C, 27);
    run_zones<TE>(C == 1 ? 1 : 5, C, C == 65 ? XH_ZONES_MAX_EDGES : 2);
  }
}

}  // namespace

int main() {
  all<float>();
  all<double>();
  printf("rain_driver: %d cases clean\n", g_cases);
  return 0;
}
