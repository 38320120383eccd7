// grid_driver — the three entry points of grid.hip on the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE
// ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_grid_cpu.py links it with grid.hip
// (compiled like the fiber units: the lanes of a workgroup talk through shuffles and LDS) and sim_runtime.cpp, everything compiled
// with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY its elements, the weights one of exactly C, every output one of exactly its length and
// every index list and host table one of exactly its entries, so that a read one element past the last row (the 16-byte lanes of
// xh_grid_masked_dot on the partial last group, the last chunk of a row that is no multiple of XH_GRID_CHUNK), one weight past
// the weights, one row before the first window of the filter or one index past a list lands in a redzone.  Every lane of a
// workgroup is a fiber with a stack of its own here, which the sanitizer makes expensive, so the cases are few and chosen: the
// fused launch on XH_GRID_ROWS + 1 rows of 1, 63, 64, 65, XH_GRID_CHUNK - 1, XH_GRID_CHUNK, XH_GRID_CHUNK + 1 and 2 *
// XH_GRID_CHUNK + 3 float32 cells (float64: 65, XH_GRID_CHUNK + 1 and 2 * XH_GRID_CHUNK + 3), on 1 and XH_GRID_ROWS - 1 rows of
// the smallest and the largest; at 65 and XH_GRID_CHUNK + 1 cells each output alone against the fused launch and the rows one at
// a time against the whole field, bit for bit; the box mean in both layouts with 1 .. 3 levels, 1, 63, 65 and 130 longitudes, 1,
// 3 and 65 latitudes from index lists that are not contiguous; the filter with 1, 2, 61 and XH_GRID_MAX_WINDOW weights on 62 and
// 130 rows, and XH_GRID_MAX_WINDOW + 1 answering XH_ERR_LIMIT.  The program checks the return codes and a few properties that
// need no reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "units/xclim_hip_grid.h"

const char* const kProgram = "grid_driver";

namespace {

bool same_bits(const double* a, const double* b, int64_t n) { return memcmp(a, b, sizeof(double) * (size_t)n) == 0; }

template <typename TE>
void run_dot(xh_ctx* ctx, int64_t T, int64_t C, bool parts) {
  const int f64 = sizeof(TE) == 8;
  TE* x = field<TE>(T, C, 31u + (unsigned)(T * 7 + C), 0.0, 100.0);
  double* w = field<double>(1, C, 5u + (unsigned)C, 1.0, 1e6);
  double wsum = 0;
  for (int64_t c = 0; c < C; ++c) {
    if (isnan(w[c])) w[c] = 2.0;
    wsum += w[c];
  }
  double *dot = block<double>(T), *msum = block<double>(T), *one = block<double>(T), *row = block<double>(1);
  ok(xh_grid_masked_dot(ctx, T, C, C, f64, x, w, 15.0, dot, msum), "xh_grid_masked_dot");
  for (int64_t t = 0; t < T; ++t) {
    if (!(msum[t] >= 0 && msum[t] <= wsum * (1 + 1e-12))) fail("an extent outside 0 .. the sum of the weights");
    if (!(dot[t] >= 0 && dot[t] <= 100.0 * msum[t] * (1 + 1e-12))) fail("an area outside 0 .. 100 x the extent");
  }
  if (parts) {
    ok(xh_grid_masked_dot(ctx, T, C, C, f64, x, w, 15.0, one, nullptr), "xh_grid_masked_dot (dot)");
    if (!same_bits(one, dot, T)) fail("the dot alone differs from the fused launch");
    ok(xh_grid_masked_dot(ctx, T, C, C, f64, x, w, 15.0, nullptr, one), "xh_grid_masked_dot (msum)");
    if (!same_bits(one, msum, T)) fail("the masked sum alone differs from the fused launch");
    for (int64_t t = 0; t < T; ++t) {   // a one-row field of exactly C elements
      TE* xr = block<TE>(C);
      memcpy(xr, x + t * C, sizeof(TE) * (size_t)C);
      ok(xh_grid_masked_dot(ctx, 1, C, C, f64, xr, w, 15.0, row, nullptr), "xh_grid_masked_dot (one row)");
      if (!same_bits(row, dot + t, 1)) fail("a row launched alone differs from the row of the whole field");
      free(xr);
    }
    g_cases += 3;
  }
  ++g_cases;
  free(x), free(w), free(dot), free(msum), free(one), free(row);
}

std::vector<int32_t> every_other(int64_t n, int64_t count) {   // `count` indices below n that are not contiguous
  std::vector<int32_t> v;
  for (int64_t i = 0; i < count; ++i) v.push_back((int32_t)((i * 2 + (i % 3 == 0 ? 1 : 0)) % n));
  return v;
}

template <typename TE>
void run_box(xh_ctx* ctx, bool y_fast, int64_t nz, int64_t ny, int64_t nx) {
  const int f64 = sizeof(TE) == 8;
  const int64_t T = 3, Z = nz + 1, Y = 2 * ny + 1, X = 2 * nx + 1;
  const int64_t ld = Z * Y * X, sz = Y * X, sy = y_fast ? 1 : X, sx = y_fast ? Y : 1;
  TE* u = field<TE>(T, ld, 77u + (unsigned)(nz * 5 + ny * 3 + nx), -20.0, 50.0);
  int32_t *iz = exact(every_other(Z, nz)), *iy = exact(every_other(Y, ny)), *ix = exact(every_other(X, nx));
  double* zm = block<double>(T * ny);
  ok(xh_grid_box_mean(ctx, T, ld, Z, Y, X, sz, sy, sx, f64, u, nz, iz, ny, iy, nx, ix, zm, ny), "xh_grid_box_mean");
  for (int64_t i = 0; i < T * ny; ++i)
    if (!isnan(zm[i]) && !(zm[i] >= -20.0 && zm[i] <= 30.0)) fail("a mean outside the range of its samples");
  ++g_cases;
  free(u), free(iz), free(iy), free(ix), free(zm);
}

void run_filter(xh_ctx* ctx, int64_t T, int64_t ny, int W, bool alone) {
  double* zm = field<double>(T, ny, 91u + (unsigned)(T + ny + W), -5.0, 20.0);
  std::vector<double> wv((size_t)W);
  for (int k = 0; k < W; ++k) wv[(size_t)k] = 1.0 / (1.0 + k);
  double* wts = exact(wv);
  double *f = block<double>(T * ny), *smax = block<double>(T), *only = block<double>(T);
  int32_t* jmax = block<int32_t>(T);
  ok(xh_grid_filter_argmax(ctx, T, ny, zm, ny, W, wts, f, ny, smax, jmax), "xh_grid_filter_argmax");
  for (int64_t t = 0; t < T; ++t) {
    const bool inside = t - W / 2 >= 0 && t - W / 2 + W <= T;
    if (jmax[t] < -1 || jmax[t] >= ny) fail("an index outside -1 .. ny - 1");
    if (jmax[t] >= 0 ? !(smax[t] == f[t * ny + jmax[t]]) : !isnan(smax[t])) fail("the maximum is not the value at its index");
    for (int64_t j = 0; j < ny; ++j) {
      const double v = f[t * ny + j];
      if (!inside && !isnan(v)) fail("a filtered value on a row whose window leaves the series");
      if (!isnan(v) && (v > smax[t] || (v == smax[t] && j < jmax[t]))) fail("a larger or an earlier equal value than the maximum");
    }
  }
  if (alone) {
    ok(xh_grid_filter_argmax(ctx, T, ny, zm, ny, W, wts, nullptr, 0, only, nullptr), "xh_grid_filter_argmax (smax)");
    if (!same_bits(only, smax, T)) fail("the maximum alone differs from the launch with all outputs");
  }
  ++g_cases;
  free(zm), free(wts), free(f), free(smax), free(only), free(jmax);
}

template <typename TE>
void all(xh_ctx* ctx) {
  const int64_t K = XH_GRID_CHUNK, R = XH_GRID_ROWS;
  const std::vector<int64_t> cells = sizeof(TE) == 4 ? std::vector<int64_t>{1, 63, 64, 65, K - 1, K, K + 1, 2 * K + 3}
                                                     : std::vector<int64_t>{65, K + 1, 2 * K + 3};
  for (int64_t C : cells) run_dot<TE>(ctx, R + 1, C, C == 65 || C == K + 1);
  for (int64_t C : {cells.front(), cells.back()})
    for (int64_t T : {(int64_t)1, R - 1}) run_dot<TE>(ctx, T, C, false);
  const int64_t box[4][3] = {{1, 1, 1}, {2, 3, 63}, {3, 65, 65}, {3, 3, 130}};   // (nz, ny, nx)
  for (int y_fast = 0; y_fast < 2; ++y_fast)
    for (const auto& b : box) run_box<TE>(ctx, y_fast != 0, b[0], b[1], b[2]);
}

}  // namespace

int main() {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  all<float>(ctx);
  all<double>(ctx);
  run_filter(ctx, 62, 1, 61, true);
  run_filter(ctx, 62, 65, 1, false);
  run_filter(ctx, 130, 3, 2, false);
  run_filter(ctx, 130, 65, XH_GRID_MAX_WINDOW, false);
  {
    double z = 0, w[XH_GRID_MAX_WINDOW + 1] = {0}, s = 7.0;
    if (xh_grid_filter_argmax(ctx, 1, 1, &z, 1, XH_GRID_MAX_WINDOW + 1, w, nullptr, 0, &s, nullptr) != XH_ERR_LIMIT)
      fail("a filter beyond XH_GRID_MAX_WINDOW is not refused with XH_ERR_LIMIT");
    if (s != 7.0) fail("a refused call wrote an output");
    ++g_cases;
  }
  xh_destroy(ctx);
  printf("grid_driver: %d cases clean\n", g_cases);
  return 0;
}
