// robust_driver — xh_change_test, xh_ar6_gamma, xh_robust_fractions and xh_robust_coefficient of the host simulation under the compiler's
// sanitizers (TEST INFRASTRUCTURE ONLY).  A program of its own: no Python in the process, nothing preloaded.
// tests/test_hostsim_robust_cpu.py links it with robust.hip and sim_runtime.cpp, everything compiled with -g -O1
// -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY its elements (fut R * T1 * C, ref R * T2 * C or T2 * C), every output of exactly R * C
// (7 * C, C), so that an access one element outside lands in a redzone.  Outputs a call does not write are NULL, so that a write
// faults.  The cases: the five tests on 1, 65 and 130 cells, series of 8 / 12 (the exact table), 30 / 30 (LDS) and 40 / 30 (the
// work buffer), float32 and float64 (about one NaN in 97 values), a ref with and without realizations; the fractions with every
// combination of masks and thresholds; the coefficient; gamma on 3, 50 and 60 years, both degrees, with and
// without blocks.  Checked without a reference: the return code,
// every output written (the blocks start as 0x7B), p-values and fractions inside [0, 1], and the argument errors.
#include "driver_common.h"
#include "units/xclim_hip_robust.h"

const char* const kProgram = "robust_driver";

namespace {

template <typename TE>
bool poisoned(const TE* p, int64_t n) {
  TE pat;
  memset(&pat, 0x7B, sizeof(TE));
  for (int64_t i = 0; i < n; ++i)
    if (memcmp(&p[i], &pat, sizeof(TE)) == 0) return true;
  return false;
}

template <typename TE>
void change(int64_t R, int64_t T1, int64_t T2, int64_t C, int test, bool ref_has_r) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* fut = field<TE>(R * T1, C, 11u, 273.0, 3.0);
  TE* ref = field<TE>((ref_has_r ? R : 1) * T2, C, 12u, 272.5, 3.0);
  const bool table = test == XH_CT_MWU && (T1 <= 8 || T2 <= 8);
  std::vector<double> sf((size_t)(T1 * T2 + 1));
  for (size_t k = 0; k < sf.size(); ++k) sf[k] = 1.0 - (double)k / (double)sf.size();
  double* h_sf = table ? exact(sf) : nullptr;
  const bool full = test != XH_CT_MOMENTS;
  double* delta = block<double>(R * C);
  double* mean_ref = block<double>(R * C);
  int32_t* n1 = block<int32_t>(R * C);
  int32_t* n2 = block<int32_t>(R * C);
  double* stat = full ? block<double>(R * C) : nullptr;
  double* df = full ? block<double>(R * C) : nullptr;
  double* p = full ? block<double>(R * C) : nullptr;
  uint8_t* status = full ? block<uint8_t>(R * C) : nullptr;
  ok(xh_change_test(ctx, fut, ref, R, T1, T2, C, C, T1 * C, C, ref_has_r ? T2 * C : 0, sizeof(TE) == 8, test, h_sf, table ? T1 * T2 + 1 : 0,
                    delta, mean_ref, n1, n2, stat, df, p, status, C),
     "xh_change_test");
  if (poisoned(delta, R * C) || poisoned(mean_ref, R * C) || poisoned(n1, R * C) || poisoned(n2, R * C)) fail("a moment was not written");
  if (full) {
    if (poisoned(stat, R * C) || poisoned(df, R * C) || poisoned(p, R * C)) fail("a test output was not written");
    for (int64_t i = 0; i < R * C; ++i) {
      if (status[i] > XH_CT_EXACT_PENDING) fail("a status byte outside the three values");
      if (status[i] == XH_CT_DONE && !(p[i] >= 0.0 && p[i] <= 1.0)) fail("a p-value outside [0, 1]");
      if (status[i] != XH_CT_DONE && !isnan(p[i])) fail("a p-value next to a status that is not DONE");
    }
  }
  free(fut), free(ref), free(h_sf), free(delta), free(mean_ref), free(n1), free(n2), free(stat), free(df), free(p), free(status);
  xh_destroy(ctx);
  ++g_cases;
}

void fractions(int64_t R, int64_t C, int masks, int kind, int strict) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  double* delta = field<double>(R, C, 21u, -1.0, 2.0);
  double* mean_ref = kind == XH_RF_THRESH_REL ? field<double>(R, C, 22u, 1.0, 1.0) : nullptr;
  uint8_t* changed = (masks & 1) && kind == XH_RF_THRESH_NONE ? block<uint8_t>(R * C, 1) : nullptr;
  uint8_t* valid = (masks & 2) ? block<uint8_t>(R * C, 1) : nullptr;
  if (valid) valid[0] = 0;
  std::vector<double> w((size_t)R);
  for (int64_t r = 0; r < R; ++r) w[r] = 0.5 + (double)r;
  double* h_w = exact(w);
  double* out = block<double>(XH_RF_NFRAC * C);
  ok(xh_robust_fractions(ctx, delta, changed, valid, mean_ref, R, C, C, h_w, strict, kind, 0.3, out, C), "xh_robust_fractions");
  if (poisoned(out, XH_RF_NFRAC * C)) fail("a fraction was not written");
  for (int64_t i = 0; i < XH_RF_NFRAC * C; ++i)
    if (!(out[i] >= 0.0 && out[i] <= (i / C == XH_RF_VALID ? 1e9 : 1.0 + 1e-12))) fail("a fraction outside [0, 1]");
  free(delta), free(mean_ref), free(changed), free(valid), free(h_w), free(out);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void coefficient(int64_t R, int64_t T1, int64_t T2, int64_t C, bool parts) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* fut = field<TE>(R * T1, C, 31u, 274.0, 3.0);
  TE* ref = field<TE>(T2, C, 32u, 272.0, 3.0);
  double* out = block<double>(C);
  double* a1 = parts ? block<double>(C) : nullptr;
  double* a2 = parts ? block<double>(C) : nullptr;
  ok(xh_robust_coefficient(ctx, fut, ref, R, T1, T2, C, C, T1 * C, C, sizeof(TE) == 8, out, a1, a2), "xh_robust_coefficient");
  if (poisoned(out, C) || (parts && (poisoned(a1, C) || poisoned(a2, C)))) fail("a coefficient was not written");
  for (int64_t c = 0; c < C; ++c)
    if (!isnan(out[c]) && !(out[c] <= 1.0)) fail("a coefficient above 1");
  free(fut), free(ref), free(out), free(a1), free(a2);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void gamma(int64_t R, int64_t T, int64_t C, int deg, bool blocks) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  TE* y = field<TE>(R * T, C, 41u, 270.0, 8.0);
  std::vector<double> x((size_t)T);
  for (int64_t t = 0; t < T; ++t) x[t] = 365.0 * (double)t;
  std::vector<int64_t> seg;
  for (int64_t t = 0; t < T; t += 20) seg.push_back(t);
  seg.push_back(T);
  double* h_x = exact(x);
  int64_t* h_seg = blocks ? exact(seg) : nullptr;
  double* out = block<double>(R * C);
  ok(xh_ar6_gamma(ctx, y, R, T, C, C, T * C, sizeof(TE) == 8, h_x, deg, h_seg, blocks ? (int64_t)seg.size() - 1 : 0, 1.645, out, C), "xh_ar6_gamma");
  if (poisoned(out, R * C)) fail("a gamma was not written");
  for (int64_t i = 0; i < R * C; ++i)
    if (!isnan(out[i]) && !(out[i] >= 0.0)) fail("a negative gamma");
  free(y), free(h_x), free(h_seg), free(out);
  xh_destroy(ctx);
  ++g_cases;
}

void refusals() {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  double* x = block<double>(4 * 16);
  int32_t* n = block<int32_t>(16);
  uint8_t* s = block<uint8_t>(16);
  if (xh_change_test(ctx, x, x, 1, 513, 4, 1, 1, 513, 1, 4, 1, XH_CT_TTEST, 0, 0, x, x, n, n, x, x, x, s, 1) != XH_ERR_LIMIT) fail("T1 = 513 was taken");
  if (xh_change_test(ctx, x, x, 1, 4, 4, 4, 3, 16, 4, 16, 1, XH_CT_TTEST, 0, 0, x, x, n, n, x, x, x, s, 4) != XH_ERR_LAYOUT) fail("ld < C was taken");
  if (xh_change_test(ctx, x, x, 1, 4, 4, 4, 4, 16, 4, 16, 1, XH_CT_NTESTS, 0, 0, x, x, n, n, x, x, x, s, 4) != XH_ERR_ARG) fail("an unknown test was taken");
  if (xh_change_test(ctx, x, x, 1, 4, 4, 4, 4, 16, 4, 16, 1, XH_CT_MWU, 0, 0, x, x, n, n, x, x, x, s, 4) != XH_ERR_ARG) fail("MWU without its table was taken");
  if (xh_change_test(ctx, x, x, 1, 4, 4, 4, 4, 16, 4, 16, 1, XH_CT_TTEST, 0, 0, x, x, n, n, x, x, 0, s, 4) != XH_ERR_ARG) fail("a test without pvals was taken");
  if (xh_change_test(ctx, x, x, 1, 4, 4, 0, 4, 16, 4, 16, 1, XH_CT_TTEST, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4) != XH_OK) fail("C = 0 was refused");
  if (xh_robust_fractions(ctx, x, s, 0, 0, 2, 4, 4, x, 1, XH_RF_THRESH_ABS, 1.0, x, 4) != XH_ERR_ARG) fail("a threshold next to `changed` was taken");
  if (xh_robust_fractions(ctx, x, 0, 0, 0, 2, 4, 4, x, 1, XH_RF_THRESH_REL, 1.0, x, 4) != XH_ERR_ARG) fail("rel_thresh without mean_ref was taken");
  if (xh_robust_fractions(ctx, x, 0, 0, 0, 2, 4, 3, x, 1, 0, 0.0, x, 4) != XH_ERR_LAYOUT) fail("ld < C was taken");
  if (xh_robust_coefficient(ctx, x, x, 16, 512, 4, 1, 1, 512, 1, 1, x, 0, 0) != XH_ERR_LIMIT) fail("a pool of 8208 values was taken");
  int64_t bad_seg[3] = {0, 5, 3};
  if (xh_ar6_gamma(ctx, x, 1, 4, 4, 4, 16, 1, x, 3, 0, 0, 1.0, x, 4) != XH_ERR_ARG) fail("deg = 3 was taken");
  if (xh_ar6_gamma(ctx, x, 1, 4, 4, 4, 16, 1, x, 1, bad_seg, 2, 1.0, x, 4) != XH_ERR_ARG) fail("block offsets beyond the years were taken");
  if (xh_ar6_gamma(ctx, x, 1, 513, 1, 1, 513, 1, x, 1, 0, 0, 1.0, x, 1) != XH_ERR_LIMIT) fail("513 years were taken");
  free(x), free(n), free(s);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_cases() {
  const int64_t cells[] = {1, 65, 130};
  const int64_t lens[][2] = {{8, 12}, {30, 30}, {40, 30}};
  for (int64_t C : cells)
    for (auto& l : lens)
      for (int test = 0; test < XH_CT_NTESTS; ++test) {
        change<TE>(3, l[0], l[1], C, test, true);
        change<TE>(3, l[0], l[1], C, test, false);
      }
  for (int64_t C : cells)
    for (int64_t T : {(int64_t)3, (int64_t)50, (int64_t)60})
      for (int deg = 1; deg <= 2; ++deg) {
        gamma<TE>(3, T, C, deg, false);
        gamma<TE>(3, T, C, deg, true);
      }
  for (int64_t C : cells) {
    coefficient<TE>(4, 12, 9, C, false);
    coefficient<TE>(3, 40, 70, C, true);
  }
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  for (int64_t C : {(int64_t)1, (int64_t)65, (int64_t)130})
    for (int masks = 0; masks < 4; ++masks)
      for (int kind = XH_RF_THRESH_NONE; kind <= XH_RF_THRESH_REL; ++kind)
        for (int strict = 0; strict < 2; ++strict) fractions(5, C, masks, kind, strict);
  refusals();
  printf("%d cases clean\n", g_cases);
  return 0;
}
