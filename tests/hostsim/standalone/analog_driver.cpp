// analog_driver — the entry point of analog.hip on the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE
// ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_analog_cpu.py links it with
// analog.hip (on fibers: the kernel copies the target table to LDS behind one barrier) and sim_runtime.cpp, everything compiled
// with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY m * C elements, the target one of exactly n * d, the output one of exactly its rows *
// C, every table one of exactly its length; the work buffer and the LDS table are heap blocks of the sizes the entry point asks
// for.  So a read one row past a field, a slot past a lane's arrays (Prim's keys and sides, the KS counters, kldiv's list) or an
// entry past the target table lands in a redzone.  The cases: every method on 1, 65 and 260 cells, float32 and float64, with a
// NaN cell and a constant cell among them; one and six indices for kolmogorov_smirnov; m = 4; n > m; every limit of the header
// (512 + 512 points, 10 indices, k = 32, 16 values of k) on 2 cells; one past each limit.  The program checks the return codes
// and a few properties that need no reference; a sanitizer report aborts it.
#include "driver_common.h"
#include "ext/xclim_hip_analog.h"

const char* const kProgram = "analog_driver";

namespace {

const uint64_t kPoison = 0x7B7B7B7B7B7B7B7BULL;

bool poison(double v) {
  uint64_t bits;
  memcpy(&bits, &v, 8);
  return bits == kPoison;
}

// a field without NaN (driver_common's field() plants them), then NaN in sample 1 of cell 1 and a constant cell 2 where asked
template <typename TE>
TE* candidates(int64_t m, int64_t C, unsigned seed, bool edges) {
  TE* p = field<TE>(m, C, seed, -1.5, 3.6);
  for (int64_t i = 0; i < m * C; ++i)
    if (p[i] != p[i]) p[i] = (TE)0.25;
  if (edges && C > 2 && m > 1) {
    p[1 * C + 1] = (TE)NAN;
    for (int64_t i = 0; i < m; ++i) p[i * C + 2] = (TE)0.625;
  }
  return p;
}

template <typename TE>
void run(int64_t n, int64_t m, int d, int64_t C, const std::vector<int32_t>& ks, int only = -1) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int f64 = sizeof(TE) == 8;
  double* x = field<double>(n, d, 3u + (unsigned)(n * 7 + d), -1.0, 2.0);
  for (int64_t i = 0; i < n * d; ++i)
    if (x[i] != x[i]) x[i] = 0.125;
  std::vector<void*> fields;
  for (int j = 0; j < d; ++j) fields.push_back(candidates<TE>(m, C, 11u + (unsigned)(j * 131 + m + C), j == 0));
  void** y = exact(fields);
  std::vector<double> vi((size_t)d * d, 0.0);
  for (int j = 0; j < d; ++j) vi[(size_t)j * d + j] = 1.0 + 0.1 * j;
  const std::vector<double> one = {1e-12};
  double *hvi = exact(vi), *hone = exact(one);
  int32_t* hk = exact(ks);

  for (int method = 0; method < XH_ANALOG_NMETHODS; ++method) {
    if (only >= 0 && method != only) continue;
    if (method == XH_ANALOG_KOLMOGOROV_SMIRNOV && d > XH_ANALOG_KS_MAX_D) continue;
    const bool kl = method == XH_ANALOG_KLDIV;
    const int64_t rows = kl ? (int64_t)ks.size() : 1;
    const double* par = method == XH_ANALOG_MAHALANOBIS ? hvi : (method == XH_ANALOG_ZECH_ASLAN || method == XH_ANALOG_SZEKELY_RIZZO ? hone : nullptr);
    const int64_t npar = method == XH_ANALOG_MAHALANOBIS ? (int64_t)d * d : (par ? 1 : 0);
    double* out = block<double>(rows * C);   // EXACTLY (rows, C)
    ok(xh_analog(ctx, method, n, m, d, x, C, C, f64, y, par, npar, kl ? hk : nullptr, kl ? rows : 0, out, C), "xh_analog");
    for (int64_t i = 0; i < rows * C; ++i) {
      const double v = out[i];
      const int64_t c = i % C;
      if (poison(v)) fail("an output element was not written");
      if (C > 2 && m > 1 && c == 1 && v == v) fail("a cell with a NaN sample is not NaN");
      const bool counts = method == XH_ANALOG_NEAREST_NEIGHBOR || method == XH_ANALOG_FRIEDMAN_RAFSKY || method == XH_ANALOG_KOLMOGOROV_SMIRNOV;
      if (counts && v == v && !(v >= 0.0 && v <= 1.0)) fail("a quotient of counts lies outside [0, 1]");
      if ((method == XH_ANALOG_SEUCLIDEAN || method == XH_ANALOG_MAHALANOBIS) && n > 1 && !(C > 2 && m > 1 && c == 1) && !(v >= 0.0)) fail("a distance is negative or NaN");
      if (kl && (n < 5 || m < 5) && v == v) fail("kldiv of fewer than five points is not NaN");
    }
    free(out);
    ++g_cases;
  }
  for (void* f : fields) free(f);
  free(x), free(y), free(hvi), free(hone), free(hk);
  xh_destroy(ctx);
}

// one past a limit: XH_ERR_LIMIT and an output that keeps its bytes
void refused(int method, int64_t n, int64_t m, int d, const std::vector<int32_t>& ks) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int64_t C = 2;
  double* x = block<double>(n * d, 0);
  std::vector<void*> fields;
  for (int j = 0; j < d; ++j) fields.push_back(block<double>(m * C, 0));
  void** y = exact(fields);
  std::vector<double> vi((size_t)d * d, 1.0);
  double* par = exact(vi);
  int32_t* hk = exact(ks);
  const bool kl = method == XH_ANALOG_KLDIV;
  const int64_t rows = kl ? (int64_t)ks.size() : 1;
  const int64_t npar = method == XH_ANALOG_MAHALANOBIS ? (int64_t)d * d : (method == XH_ANALOG_ZECH_ASLAN || method == XH_ANALOG_SZEKELY_RIZZO ? 1 : 0);
  double* out = block<double>(rows * C);
  if (xh_analog(ctx, method, n, m, d, x, C, C, 1, y, par, npar, kl ? hk : nullptr, kl ? rows : 0, out, C) != XH_ERR_LIMIT) fail("one past a limit is not XH_ERR_LIMIT");
  for (int64_t i = 0; i < rows * C; ++i)
    if (!poison(out[i])) fail("a refused call wrote its output");
  for (void* f : fields) free(f);
  free(x), free(y), free(par), free(hk), free(out);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_shapes() {
  const std::vector<int32_t> k3 = {1, 2, 15}, k1 = {1};
  for (int64_t C : {1, 65, 260}) run<TE>(21, 33, 3, C, k3);
  run<TE>(25, 30, 1, 65, k1);                                  // one index
  run<TE>(12, 15, 6, 65, k1);                                  // the most indices of kolmogorov_smirnov
  run<TE>(21, 4, 3, 65, k3);                                   // m = 4: kldiv answers NaN
  run<TE>(40, 17, 2, 65, k3);                                  // n > m
  run<TE>(1, 1, 1, 3, k1);                                     // one point each
  // the limits: the largest per-lane arrays and the largest target table
  std::vector<int32_t> k16(XH_ANALOG_MAX_NK);
  for (int q = 0; q < XH_ANALOG_MAX_NK; ++q) k16[(size_t)q] = q == 0 ? XH_ANALOG_MAX_K : q;
  run<TE>(XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_D, 2, k16, XH_ANALOG_KLDIV);
  run<TE>(XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_D, 2, k1, XH_ANALOG_MAHALANOBIS);
  run<TE>(XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_SAMPLE, 2, 2, k1, XH_ANALOG_FRIEDMAN_RAFSKY);
  run<TE>(XH_ANALOG_MAX_SAMPLE, XH_ANALOG_MAX_SAMPLE, XH_ANALOG_KS_MAX_D, 2, k1, XH_ANALOG_KOLMOGOROV_SMIRNOV);
  run<TE>(183, 183, XH_ANALOG_MAX_D, 2, k1, XH_ANALOG_NEAREST_NEIGHBOR);
  run<TE>(183, 183, XH_ANALOG_MAX_D, 2, k1, XH_ANALOG_ZECH_ASLAN);
  run<TE>(183, 183, XH_ANALOG_MAX_D, 2, k1, XH_ANALOG_SZEKELY_RIZZO);
}

}  // namespace

int main() {
  all_shapes<float>();
  all_shapes<double>();
  const std::vector<int32_t> k1 = {1};
  for (int method = 0; method < XH_ANALOG_NMETHODS; ++method) {
    refused(method, XH_ANALOG_MAX_SAMPLE + 1, 5, 1, k1);
    refused(method, 5, XH_ANALOG_MAX_SAMPLE + 1, 1, k1);
    refused(method, 5, 5, XH_ANALOG_MAX_D + 1, k1);
  }
  refused(XH_ANALOG_KOLMOGOROV_SMIRNOV, 5, 5, XH_ANALOG_KS_MAX_D + 1, k1);
  refused(XH_ANALOG_KLDIV, 5, 5, 1, {XH_ANALOG_MAX_K + 1});
  refused(XH_ANALOG_KLDIV, 5, 5, 1, std::vector<int32_t>(XH_ANALOG_MAX_NK + 1, 1));
  printf("analog_driver: %d cases clean\n", g_cases);
  return 0;
}
