// partition_driver — xh_partition_smooth, xh_partition_components and xh_ensemble_stats of the host simulation under the compiler's
// sanitizers (TEST INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.
// tests/test_hostsim_partition_cpu.py links it with partition.hip and sim_runtime.cpp, everything compiled with -g -O1
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY its elements (y and sm_in T * N * C, the basis T * (deg + 1)), every output of exactly
// its own (sm and roll T * N * C, n_valid and status N * C, the flag 1, out (K + 2) * T * C, g T * C, the statistics 4 * E), so that
// an access one element outside lands in a redzone.  Optional outputs are NULL in turn, so that a write to one faults.  The cases:
// 1, 65 and 130 cells, float32 and float64 (about one NaN in 97 values), T = 10, 12 and 60, every degree, both windows, a given sm,
// the three baselines; member cubes 2 x 3, 2 x 3 x 2 and 2 x 2 x 2 x 2 with every rule and weight and both variability rules; the
// statistics with and without weights.  Checked without a reference: the return code, every output written (the blocks start as
// 0x7B), variances that are not negative, the total as the sum of its planes, max >= mean >= min, and the argument errors.
#include "driver_common.h"
#include "units/xclim_hip_partition.h"

const char* const kProgram = "partition_driver";

namespace {

template <typename TE>
bool poisoned(const TE* p, int64_t n) {
  TE pat;
  memset(&pat, 0x7B, sizeof(TE));
  for (int64_t i = 0; i < n; ++i)
    if (memcmp(&p[i], &pat, sizeof(TE)) == 0) return true;
  return false;
}

// an orthonormal polynomial basis (T, np) by Gram-Schmidt on the powers of the centred abscissa
std::vector<double> basis(int64_t T, int np) {
  std::vector<double> q((size_t)(T * np));
  for (int k = 0; k < np; ++k) {
    for (int64_t t = 0; t < T; ++t) q[t * np + k] = pow(T > 1 ? 2.0 * t / (T - 1) - 1.0 : 0.0, k);
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < k; ++j) {
        double dot = 0.0;
        for (int64_t t = 0; t < T; ++t) dot += q[t * np + k] * q[t * np + j];
        for (int64_t t = 0; t < T; ++t) q[t * np + k] -= dot * q[t * np + j];
      }
    double nrm = 0.0;
    for (int64_t t = 0; t < T; ++t) nrm += q[t * np + k] * q[t * np + k];
    for (int64_t t = 0; t < T; ++t) q[t * np + k] /= sqrt(nrm);
  }
  return q;
}

template <typename TE>
void smooth(int64_t T, int64_t N, int64_t C, int deg, int window, int base, bool given, int nulls) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* y = field<TE>(T * N, C, 51u + (unsigned)deg, 10.0, 3.0);
  TE* s_in = given ? field<TE>(T * N, C, 52u, 10.0, 1.0) : nullptr;
  std::vector<double> q = basis(T, deg + 1);
  double* h_q = given ? nullptr : exact(q);
  const bool want_sm = !(nulls & 1), want_roll = !(nulls & 2) || !want_sm;
  double* sm = want_sm ? block<double>(T * N * C) : nullptr;
  double* roll = want_roll ? block<double>(T * N * C) : nullptr;
  int32_t* nv = (nulls & 4) ? nullptr : block<int32_t>(N * C);
  uint8_t* st = (nulls & 8) ? nullptr : block<uint8_t>(N * C);
  uint8_t* flag = (nulls & 16) ? nullptr : block<uint8_t>(1);
  const int stat = window == 10 ? XH_PT_ROLL_MEAN : XH_PT_ROLL_VAR;
  ok(xh_partition_smooth(ctx, y, s_in, T, N, C, N * C, C, sizeof(TE) == 8, h_q, given ? 0 : deg, window, stat, base, 1, T < 6 ? T : 6, sm, roll, N * C,
                         C, nv, st, C, flag),
     "xh_partition_smooth");
  if ((sm && poisoned(sm, T * N * C)) || (roll && poisoned(roll, T * N * C)) || (nv && poisoned(nv, N * C))) fail("an output was not written");
  if (flag && *flag > 1) fail("a flag that is neither 0 nor 1");
  if (st)
    for (int64_t i = 0; i < N * C; ++i)
      if (st[i] > XH_PT_ILLPOSED) fail("a status byte outside the three values");
  if (roll && window == 11)
    for (int64_t i = 0; i < T * N * C; ++i)
      if (!isnan(roll[i]) && !(roll[i] >= 0.0)) fail("a negative rolling variance");
  if (roll)
    for (int64_t t = 0; t < T; ++t)
      if ((t < window / 2 || t > T - 1 - (window - 1) / 2) && !isnan(roll[t * N * C])) fail("a rolling value of an incomplete window");
  free(y), free(s_in), free(h_q), free(sm), free(roll), free(nv), free(st), free(flag);
  xh_destroy(ctx);
  ++g_cases;
}

void components(int64_t T, const std::vector<int64_t>& members, int64_t C, int variab, bool with_g) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  std::vector<int64_t> dims(members);
  dims.resize(XH_PT_MAX_AXES, 1);
  int64_t N = 1;
  for (int64_t d : dims) N *= d;
  double* sm = field<double>(T * N, C, 61u, -1.0, 2.0);
  double* roll = field<double>(T * N, C, 62u, 0.0, 1.0);
  std::vector<int32_t> comps;
  const int nax = (int)members.size(), w_axis = nax - 1;
  for (int ax = 0; ax < nax; ++ax) {   // every rule with every weight it may carry
    comps.insert(comps.end(), {ax, XH_PT_VAR_THEN_MEAN, ax == w_axis ? XH_PT_W_USER : XH_PT_W_COUNT});
    comps.insert(comps.end(), {ax, XH_PT_MEAN_THEN_VAR, ax == w_axis ? XH_PT_W_NONE : XH_PT_W_USER});
  }
  const int K = (int)comps.size() / 3;
  std::vector<double> w((size_t)dims[w_axis]);
  for (size_t k = 0; k < w.size(); ++k) w[k] = (double)k;   // (the first weight is 0)
  std::vector<int64_t> hd(dims);
  std::vector<int32_t> order = {3, 1, 0, 2};
  int64_t* h_dims = exact(hd);
  int32_t* h_comps = exact(comps);
  double* h_w = exact(w);
  int32_t* h_order = exact(order);
  double* out = block<double>((K + 2) * T * C);
  double* g = with_g ? block<double>(T * C) : nullptr;
  ok(xh_partition_components(ctx, sm, roll, T, h_dims, C, N * C, C, h_comps, K, h_w, w_axis, variab, T / 2, h_order, out, C, g),
     "xh_partition_components");
  if (poisoned(out, (K + 2) * T * C) || (g && poisoned(g, T * C))) fail("a component was not written");
  for (int64_t i = 0; i < T * C; ++i) {
    double total = out[i];
    for (int k = 1; k <= K; ++k) {
      if (!isnan(out[k * T * C + i]) && !(out[k * T * C + i] >= 0.0)) fail("a negative variance component");
      total += out[k * T * C + i];
    }
    const double got = out[(K + 1) * T * C + i];
    if (!(isnan(total) ? isnan(got) : got == total)) fail("the total is not the sum of its planes in their order");
  }
  free(sm), free(roll), free(h_dims), free(h_comps), free(h_w), free(h_order), free(out), free(g);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void stats(int64_t R, int64_t E, bool weighted, int min_members) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* x = field<TE>(R, E, 71u, 270.0, 20.0);
  std::vector<double> w((size_t)R);
  for (int64_t r = 0; r < R; ++r) w[r] = 0.5 * (double)r;
  double* h_w = weighted ? exact(w) : nullptr;
  double* out = block<double>(XH_ES_NSTAT * E);
  ok(xh_ensemble_stats(ctx, x, R, E, E, sizeof(TE) == 8, h_w, min_members, out, E), "xh_ensemble_stats");
  if (poisoned(out, XH_ES_NSTAT * E)) fail("a statistic was not written");
  for (int64_t e = 0; e < E; ++e) {
    const double mean = out[XH_ES_MEAN * E + e], sd = out[XH_ES_STD * E + e], mx = out[XH_ES_MAX * E + e], mn = out[XH_ES_MIN * E + e];
    if (isnan(mx) != isnan(mn)) fail("max and min disagree on NaN");
    if (!isnan(mean) && !(mn <= mean && mean <= mx && sd >= 0.0)) fail("a mean outside [min, max], or a negative deviation");
  }
  free(x), free(h_w), free(out);
  xh_destroy(ctx);
  ++g_cases;
}

void refusals() {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  double* x = block<double>(64);
  std::vector<double> q = basis(4, 2);
  int64_t dims[4] = {2, 2, 1, 1}, big[4] = {65, 1, 1, 1}, many[4] = {64, 64, 2, 1};
  int32_t order[4] = {0, 1, 2, 3}, twice[4] = {0, 0, 2, 3};
  int32_t count_mean[3] = {0, XH_PT_MEAN_THEN_VAR, XH_PT_W_COUNT}, user[3] = {0, XH_PT_VAR_THEN_MEAN, XH_PT_W_USER};
  if (xh_partition_smooth(ctx, x, 0, 513, 1, 1, 1, 1, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, 0, 0, 0, x, x, 1, 1, 0, 0, 1, 0) != XH_ERR_LIMIT) fail("513 years were taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 1, 9, XH_PT_ROLL_MEAN, 0, 0, 0, x, x, 8, 4, 0, 0, 4, 0) != XH_ERR_ARG) fail("a window of 9 was taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 1, 10, XH_PT_ROLL_VAR, 0, 0, 0, x, x, 8, 4, 0, 0, 4, 0) != XH_ERR_ARG) fail("the variance over 10 rows was taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 5, 11, XH_PT_ROLL_VAR, 0, 0, 0, x, x, 8, 4, 0, 0, 4, 0) != XH_ERR_ARG) fail("degree 5 was taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, 0, 0, 0, 0, 0, 8, 4, 0, 0, 4, 0) != XH_ERR_ARG) fail("sm and roll both NULL were taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, XH_PT_BASE_SUB, 2, 5, x, x, 8, 4, 0, 0, 4, 0) != XH_ERR_ARG) fail("baseline rows beyond T were taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 7, 4, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, 0, 0, 0, x, x, 8, 4, 0, 0, 4, 0) != XH_ERR_LAYOUT) fail("overlapping series were taken");
  if (xh_partition_smooth(ctx, x, 0, 4, 2, 4, 8, 4, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, 0, 0, 0, x, x, 8, 4, 0, 0, 3, 0) != XH_ERR_LAYOUT) fail("ld_nc < C was taken");
  if (xh_partition_smooth(ctx, 0, 0, 4, 2, 0, 8, 4, 1, q.data(), 1, 11, XH_PT_ROLL_VAR, 0, 0, 0, x, 0, 8, 4, 0, 0, 4, 0) != XH_OK) fail("C = 0 was refused");
  if (xh_partition_components(ctx, x, x, 2, big, 1, 65, 1, 0, 0, 0, 0, 0, 0, order, x, 1, 0) != XH_ERR_LIMIT) fail("an axis of 65 was taken");
  if (xh_partition_components(ctx, x, x, 1, many, 1, 8192, 1, 0, 0, 0, 0, 0, 0, order, x, 1, 0) != XH_ERR_LIMIT) fail("8192 members were taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 16, 4, count_mean, 1, 0, 0, 0, 0, order, x, 4, 0) != XH_ERR_ARG) fail("count weights on MEAN_THEN_VAR were taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 16, 4, user, 1, 0, 0, 0, 0, order, x, 4, 0) != XH_ERR_ARG) fail("user weights without weights were taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 16, 4, 0, 0, 0, 0, XH_PT_VARIAB_HS, 0, order, x, 4, 0) != XH_ERR_ARG) fail("HS without weights was taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 16, 4, 0, 0, 0, 0, 0, 0, twice, x, 4, 0) != XH_ERR_ARG) fail("an order that is no permutation was taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 16, 4, 0, 9, 0, 0, 0, 0, order, x, 4, 0) != XH_ERR_ARG) fail("nine components were taken");
  if (xh_partition_components(ctx, x, x, 2, dims, 4, 15, 4, 0, 0, 0, 0, 0, 0, order, x, 4, 0) != XH_ERR_LAYOUT) fail("overlapping members were taken");
  if (xh_partition_components(ctx, 0, 0, 2, dims, 0, 16, 4, 0, 0, 0, 0, 0, 0, order, 0, 4, 0) != XH_OK) fail("C = 0 was refused");
  if (xh_ensemble_stats(ctx, x, 0, 4, 4, 1, 0, 1, x, 4) != XH_ERR_ARG) fail("no realization was taken");
  if (xh_ensemble_stats(ctx, x, 2, 4, 3, 1, 0, 1, x, 4) != XH_ERR_LAYOUT) fail("ld < E was taken");
  if (xh_ensemble_stats(ctx, 0, 2, 0, 4, 1, 0, 1, 0, 4) != XH_OK) fail("E = 0 was refused");
  free(x);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_cases() {
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)130}) {
    for (int deg = 0; deg <= XH_PT_MAX_DEG; ++deg)
      for (int window = 10; window <= 11; ++window) smooth<TE>(60, 6, C, deg, window, XH_PT_BASE_NONE, false, 0);
    for (int64_t T : {(int64_t)10, (int64_t)12})
      for (int window = 10; window <= 11; ++window) smooth<TE>(T, 12, C, 4, window, XH_PT_BASE_SUB, false, 0);
    for (int base = XH_PT_BASE_NONE; base <= XH_PT_BASE_DIV; ++base) smooth<TE>(60, 6, C, 0, 10, base, true, 0);
    for (int nulls : {1, 2, 4, 8, 16, 28, 29, 30}) smooth<TE>(60, 6, C, 4, 11, XH_PT_BASE_DIV, false, nulls);
    for (bool weighted : {false, true})
      for (int min_members : {1, 2, 5}) stats<TE>(5, C, weighted, min_members);
  }
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)130})
    for (int variab = XH_PT_VARIAB_MEAN_ALL; variab <= XH_PT_VARIAB_HS; ++variab) {
      components(14, {2, 3}, C, variab, true);
      components(14, {2, 3, 2}, C, variab, false);
      components(14, {2, 2, 2, 2}, C, variab, true);
    }
  refusals();
  printf("%d cases clean\n", g_cases);
  return 0;
}
