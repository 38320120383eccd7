// agro_driver — the five entry points of agro.hip on the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE
// ONLY).  A program of its own: no Python in the process, nothing preloaded.  tests/test_hostsim_units_cpu.py links it with
// agro.hip and sim_runtime.cpp, everything compiled with -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// Every field is a malloc block of EXACTLY T * C elements, every output one of exactly its rows * C and every table one of
// exactly its length, so that a read one row before the first, one element past the last row or one entry past a table lands
// in a redzone.  The cases: the daily series that starts on 1999-03-15 and runs 1002 days, with years from January and from
// July; a series of ONE row; a series of four rows (shorter than the Qian stencil); the Qian stencil at both series ends
// (xh_qian_wma, and the "qian" start of xh_egdd on periods that touch row 0 and row T - 1); a series that ends on 31 October,
// so that the season span ends on the last row; float32 and float64; 5 and 260 cells.  The program checks the return codes
// and a few properties that need no reference (the ends of the Qian mean are NaN, sums are not negative, counts stay within
// the rows selected); a sanitizer report aborts it.
#include "driver_common.h"
#include "xclim_hip_agro.h"

const char* const kProgram = "agro_driver";

namespace {

struct Axis {   // a daily standard-calendar axis and the host tables the entry points take
  std::vector<int> year, month, day, doy;
  int64_t T;
  static bool leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
  static int mlen(int y, int m) {
    static const int n[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return n[m - 1] + (m == 2 && leap(y));
  }
  Axis(int y, int m, int d, int64_t n) : T(n) {
    int dy = d;
    for (int k = 1; k < m; ++k) dy += mlen(y, k);
    for (int64_t i = 0; i < n; ++i) {
      year.push_back(y), month.push_back(m), day.push_back(d), doy.push_back(dy);
      ++d, ++dy;
      if (d > mlen(y, m)) {
        d = 1, ++m;
        if (m > 12) m = 1, ++y, dy = 1;
      }
    }
  }
  // first row of every year that starts in month `anchor`
  std::vector<int64_t> years(int anchor) const {
    std::vector<int64_t> seg{0};
    for (int64_t i = 1; i < T; ++i)
      if (month[i] == anchor && day[i] == 1) seg.push_back(i);
    seg.push_back(T);
    return seg;
  }
};

template <typename TE>
void run(const Axis& ax, int64_t C, int anchor) {
  xh_ctx* ctx = nullptr;
  if (xh_create(0, &ctx) != XH_OK) exit(2);
  const int64_t T = ax.T;
  const int f64 = sizeof(TE) == 8;
  const std::vector<int64_t> seg = ax.years(anchor);
  const int64_t P = (int64_t)seg.size() - 1;
  TE* tas = field<TE>(T, C, 1u, 270.0, 30.0);
  TE* tn = field<TE>(T, C, 2u, 262.0, 25.0);
  TE* tx = field<TE>(T, C, 3u, 280.0, 25.0);
  TE* pr = field<TE>(T, C, 4u, 0.0, 1e-4);
  TE* ev = field<TE>(T, C, 5u, 0.0, 5e-5);

  // --- degree sums: the season April - October, three kinds of factor
  std::vector<uint8_t> sel((size_t)T);
  int64_t nsel_max = 0;
  for (int64_t i = 0; i < T; ++i) sel[(size_t)i] = ax.month[(size_t)i] >= 4 && ax.month[(size_t)i] <= 10, nsel_max += sel[(size_t)i];
  int64_t* h_seg = exact(seg);
  uint8_t* h_sel = exact(sel);
  const int64_t L = 3;
  double* k_cell = block<double>(C);
  double* k_day = block<double>(T * L);
  double* k_per = block<double>(P * L);
  int32_t* li = block<int32_t>(C);
  for (int64_t c = 0; c < C; ++c) k_cell[c] = 1.0 + 0.01 * (double)(c % 7), li[c] = (int32_t)(c % L);
  for (int64_t i = 0; i < T * L; ++i) k_day[i] = i % 53 == 0 ? NAN : 0.9 + 0.001 * (double)(i % 200);
  for (int64_t i = 0; i < P * L; ++i) k_per[i] = 1.0 + 0.1 * (double)i;
  double* hi = block<double>(P * C);
  double* bedd = block<double>(P * C);
  int32_t* valid = block<int32_t>(P * C);
  for (int kind = 0; kind < 4; ++kind) {
    ok(xh_agro_degree_sum(ctx, T, C, C, f64, kind == 3 ? nullptr : tas, tn, tx, P, h_seg, kind == 2 ? nullptr : h_sel,
                          kind == 0 ? k_cell : nullptr, kind == 1 ? k_day : nullptr, kind == 2 ? k_per : nullptr, L, kind ? li : nullptr,
                          273.15, 10.0, 10.0, kind != 3, 10.0, 13.0, 9.0, kind == 3 ? nullptr : hi, bedd, valid, C),
       "xh_agro_degree_sum");
    for (int64_t i = 0; i < P * C; ++i) {
      if (kind != 3 && !(hi[i] >= 0)) fail("a negative or NaN Huglin sum");
      if (valid[i] < 0 || valid[i] > (kind == 2 ? T : nsel_max)) fail("a count beyond the rows selected");
    }
  }

  // --- the monthly entry point: every output, the hemisphere by cell and forced
  std::vector<int64_t> mo{0}, sm;
  std::vector<int32_t> mc, md;
  for (int64_t i = 0; i < T; ++i) {
    if (i > 0 && ax.month[(size_t)i] != ax.month[(size_t)i - 1]) mo.push_back(i);
    if (i == 0 || ax.month[(size_t)i] != ax.month[(size_t)i - 1])
      mc.push_back(ax.month[(size_t)i]), md.push_back(Axis::mlen(ax.year[(size_t)i], ax.month[(size_t)i]));
  }
  mo.push_back(T);
  const int64_t M = (int64_t)mc.size();
  for (int64_t p = 0; p <= P; ++p) {
    int64_t m = 0;
    while (m < M && mo[(size_t)m] < seg[(size_t)p]) ++m;
    sm.push_back(m);
  }
  int64_t *h_mo = exact(mo), *h_sm = exact(sm);
  int32_t *h_mc = exact(mc), *h_md = exact(md);
  double* lat = block<double>(C);
  for (int64_t c = 0; c < C; ++c) lat[c] = c % 2 ? -35.0 - (double)(c % 20) : 30.0 + (double)(c % 20);
  double *cni = block<double>(P * C), *mtwm = block<double>(P * C), *di = block<double>(P * C);
  for (int hemi = 0; hemi < 3; ++hemi) {
    ok(xh_agro_monthly(ctx, T, C, C, f64, tn, tas, pr, ev, M, h_mo, h_mc, h_md, P, h_sm, hemi ? nullptr : lat, hemi, 273.15, 86400.0, 200.0,
                       cni, mtwm, di, valid, C),
       "xh_agro_monthly");
    for (int64_t i = 0; i < P * C; ++i)
      if (valid[i] < 0 || valid[i] > T || isnan(di[i])) fail("xh_agro_monthly: a count out of range or a NaN dryness index");
  }
  ok(xh_agro_monthly(ctx, T, C, C, f64, nullptr, nullptr, pr, ev, M, h_mo, h_mc, h_md, P, h_sm, lat, 0, 0.0, 1.0, 0.0, nullptr, nullptr, di,
                     nullptr, C),
     "xh_agro_monthly (di alone)");

  // --- xh_egdd, both methods: the first period touches row 0, the last one row T - 1
  std::vector<int32_t> doy(ax.doy.begin(), ax.doy.end()), ldoy((size_t)P), ldays((size_t)P);
  std::vector<int64_t> sf((size_t)P, -1), ef((size_t)P, -1), day0((size_t)P, 0);
  for (int64_t p = 0; p < P; ++p) {
    const int64_t a = seg[(size_t)p], b = seg[(size_t)p + 1];
    const int ly = ax.month[(size_t)a] >= anchor ? ax.year[(size_t)a] : ax.year[(size_t)a] - 1;   // the label's year
    int d = 1;
    for (int k = 1; k < anchor; ++k) d += Axis::mlen(ly, k);
    ldoy[(size_t)p] = d, ldays[(size_t)p] = 365 + Axis::leap(ly);
    int64_t back = 0;   // days from the label to the first row: walk the label forward
    for (int y = ly, m = anchor, dd = 1; !(y == ax.year[(size_t)a] && m == ax.month[(size_t)a] && dd == ax.day[(size_t)a]); ++back) {
      if (++dd > Axis::mlen(y, m)) {
        dd = 1;
        if (++m > 12) m = 1, ++y;
      }
    }
    day0[(size_t)p] = back;
    for (int64_t i = a; i < b; ++i) {
      if (ax.month[(size_t)i] == 1 && ax.day[(size_t)i] == 1) sf[(size_t)p] = i;
      if (ax.month[(size_t)i] == 7 && ax.day[(size_t)i] == 1) ef[(size_t)p] = i;
    }
  }
  int32_t *h_doy = exact(doy), *h_ldoy = exact(ldoy), *h_ldays = exact(ldays);
  int64_t *h_sf = exact(sf), *h_ef = exact(ef), *h_day0 = exact(day0);
  double *eg = block<double>(P * C), *st = block<double>(P * C), *en = block<double>(P * C);
  for (int method = 0; method < 2; ++method) {
    ok(xh_egdd(ctx, T, C, C, f64, tn, tx, P, h_seg, h_doy, h_sf, h_ef, h_day0, h_ldoy, h_ldays, method, 273.15, 5.0, eg, st, en, valid, C),
       "xh_egdd");
    for (int64_t i = 0; i < P * C; ++i)
      if (eg[i] < 0 || valid[i] < 0 || valid[i] > T || (!isnan(st[i]) && (st[i] < 1 || st[i] > 376))) fail("xh_egdd: a value out of range");
  }

  // --- the element-wise pair: the Qian mean is NaN within two rows of either end, wherever the series ends
  double *chu = block<double>(T * C), *q = block<double>(T * C);
  ok(xh_corn_heat_units(ctx, T, C, C, f64, tn, tx, 273.15, 4.44, 10.0, chu, C), "xh_corn_heat_units");
  ok(xh_qian_wma(ctx, T, C, C, f64, tas, q, C), "xh_qian_wma");
  for (int64_t r = 0; r < T; ++r)
    for (int64_t c = 0; c < C; ++c) {
      if (isnan(chu[r * C + c])) fail("corn heat units are never NaN");
      if ((r < 2 || r + 2 >= T) && !isnan(q[r * C + c])) fail("a Qian mean within two rows of an end of the series");
    }

  for (void* p : {(void*)tas, (void*)tn, (void*)tx, (void*)pr, (void*)ev, (void*)h_seg, (void*)h_sel, (void*)k_cell, (void*)k_day, (void*)k_per,
                  (void*)li, (void*)hi, (void*)bedd, (void*)valid, (void*)h_mo, (void*)h_sm, (void*)h_mc, (void*)h_md, (void*)lat, (void*)cni,
                  (void*)mtwm, (void*)di, (void*)h_doy, (void*)h_ldoy, (void*)h_ldays, (void*)h_sf, (void*)h_ef, (void*)h_day0, (void*)eg,
                  (void*)st, (void*)en, (void*)chu, (void*)q})
    free(p);
  xh_destroy(ctx);
  ++g_cases;
}

template <typename TE>
void all_cases() {
  const Axis midyear(1999, 3, 15, 1002), one(2000, 6, 28, 1), four(2000, 12, 30, 4), october(2000, 1, 1, 305);
  if (october.month.back() != 10 || october.day.back() != 31) fail("the October axis does not end on 31 October");
  for (int anchor : {1, 7}) {
    run<TE>(midyear, 5, anchor);
    run<TE>(one, 5, anchor);
    run<TE>(four, 5, anchor);      // (30 December - 2 January: two January years of two rows each)
    run<TE>(october, 5, anchor);   // the season span ends on the last row of the series
  }
  run<TE>(midyear, 260, 7);
}

}  // namespace

int main() {
  all_cases<float>();
  all_cases<double>();
  printf("%d cases clean\n", g_cases);
  return 0;
}
