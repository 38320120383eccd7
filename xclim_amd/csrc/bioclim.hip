// bioclim.hip — the nineteen ANUCLIM bioclimatic variables (indices/_anuclim.py:66-625) in one launch.
//
// Reference: _to_quarter (:562-625: a daily series binned into 7-day steps from its first day, rolling(13) — or rolling(3) on
// monthly steps — mean of tas, sum of pr), select_resample_op for the extreme quarters, _from_other_arg (:527-559: the value
// of one quarter series at the nanargmax / nanargmin of the other), _anuclim_coeff_var (:520-524), prcptot (:446-470),
// prcptot_wetdry_period (:474-517), isothermality (:66-101) over daily_temperature_range and extreme_temperature_range.
//
// One lane owns one (cell, period): cells along x, periods along y.  The lane walks the STEPS of its period with a lead-in of
// W - 1 steps before it (the first quarters of a year reach back into the previous one), and inside each step the rows of the
// step.  The last W step values of tas and pr live in registers as a window that SHIFTS by one per step (2 (W - 1) register
// pair moves per step of up to seven rows): every quarter is then summed from rt[0] .. rt[W - 1] in step order with static
// indices, no running update.  BIO1-BIO7 and BIO12-BIO15 are reductions over the SOURCE ROWS of the period, which the same
// walk passes (a step that straddles the period's edge contributes only its rows inside it).
//
// Arithmetic is float64 in the reference's order (the build has -ffp-contract=off), except tasmax - tasmin and BIO7, which
// are taken in the fields' dtype as numpy does.  The two coefficients of variation are Welford accumulations: one pass, and
// no cancellation on a field whose spread is a thousandth of its mean.
#include "hostargs.h"

namespace {

constexpr int NBIO = 19;

struct BioArgs {
  const void *tas, *tasmin, *tasmax, *pr;  // NULL = not read by this launch
  const int64_t* step_off;                 // (S + 1)
  const double* factor;                    // (T)
  const int64_t* seg_rows;                 // (P + 1)
  const int64_t* seg_steps;                // (P + 1)
  double* out[NBIO];
  int32_t* which[4];  // wettest, driest, warmest, coldest
  int32_t* count[4];  // tas, tasmin, tasmax, pr
  int64_t C, ld, ld_out;
  double kelvin, cv_scale, thresh;
  int binned;
  bool quarters;  // any output that reads a quarter series
};

// Welford's single pass: mean and the sum of squared deviations of the values seen so far
struct Welford {
  double n, mean, m2;
  __device__ __forceinline__ void add(double x) {
    n += 1.0;
    const double d = x - mean;
    mean += d / n;
    m2 += d * (x - mean);
  }
  // 100 * (std / mean), ddof = 0 (:520-524 and the factor of :152 / :209)
  __device__ __forceinline__ double cv100() const { return n > 0 ? 100 * (sqrt(m2 / n) / mean) : xh_nan64(); }
};

// the first extreme of a criterion (NaN skipped) and the other series' value at the same step
struct Pick {
  double crit, other;
  int32_t idx;
  template <bool MAX>
  __device__ __forceinline__ void see(double c, double o, int64_t k) {
    if (c == c && (idx < 0 || (MAX ? c > crit : c < crit))) {
      crit = c;
      other = o;
      idx = (int32_t)k;
    }
  }
};

// the reductions over the source rows of the period
template <typename TE>
struct RowAcc {
  double s1, sd, s12, p13, p14;  // sum of tas, of tasmax - tasmin, of the amounts over thresh; extreme amounts
  TE tx, tn;                     // max of tasmax, min of tasmin
  int32_t n1, nd, ntx, ntn, npr;
  Welford wt, wp;
};

template <typename TE>
__device__ __forceinline__ void bio_row(const BioArgs& a, int64_t r, int64_t c, bool inp, RowAcc<TE>& m, double& ts, int& tn,
                                        double& ps, int& pn) {
  const int64_t i = r * a.ld + c;
  if (a.tas) {
    const double x = (double)xh_ld<TE>(a.tas, i);
    if (x == x) {
      ts += x;
      tn += 1;
      if (inp) {
        m.s1 += x;
        m.n1 += 1;
        m.wt.add(x + a.kelvin);
      }
    }
  }
  if (a.pr) {
    const double x = (double)xh_ld<TE>(a.pr, i);
    const double amt = x * a.factor[r];
    if (x == x) {
      ps += amt;
      pn += 1;
      if (inp) {
        m.p13 = (m.npr == 0 || amt > m.p13) ? amt : m.p13;
        m.p14 = (m.npr == 0 || amt < m.p14) ? amt : m.p14;
        m.npr += 1;
        m.wp.add(x * a.cv_scale);
        if (x >= a.thresh) m.s12 += amt;
      }
    }
  }
  if (inp && (a.tasmin || a.tasmax)) {
    const TE nan = (TE)xh_nan64();
    const TE l = a.tasmin ? xh_ld<TE>(a.tasmin, i) : nan, h = a.tasmax ? xh_ld<TE>(a.tasmax, i) : nan;
    if (h == h) {
      m.tx = (m.ntx == 0 || h > m.tx) ? h : m.tx;
      m.ntx += 1;
    }
    if (l == l) {
      m.tn = (m.ntn == 0 || l < m.tn) ? l : m.tn;
      m.ntn += 1;
    }
    const TE d = h - l;  // in the fields' dtype
    if (d == d) {
      m.sd += (double)d;
      m.nd += 1;
    }
  }
}

template <typename TE, int W>
__global__ void __launch_bounds__(XH_BLOCK) k_bioclim(BioArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t rows0 = a.seg_rows[p], rows1 = a.seg_rows[p + 1];
  const int64_t s0 = a.seg_steps[p], s1 = a.seg_steps[p + 1];
  const double nan = xh_nan64();
  RowAcc<TE> m{};
  Pick wet{0.0, nan, -1}, dry{0.0, nan, -1}, warm{0.0, nan, -1}, cold{0.0, nan, -1};

  if (!a.quarters) {
    double ts = 0.0, ps = 0.0;
    int tn = 0, pn = 0;
    for (int64_t r = rows0; r < rows1; ++r) bio_row<TE>(a, r, c, true, m, ts, tn, ps, pn);
  } else {
    const int64_t sl = s0 - (W - 1) < 0 ? 0 : s0 - (W - 1);
    double rt[W], rp[W];
#pragma unroll
    for (int j = 0; j < W; ++j) rt[j] = nan, rp[j] = nan;
    for (int64_t s = sl; s < s1; ++s) {
      const int64_t r0 = a.step_off[s], r1 = a.step_off[s + 1];
      double ts = 0.0, ps = 0.0;
      int tn = 0, pn = 0;
      for (int64_t r = r0; r < r1; ++r) bio_row<TE>(a, r, c, r >= rows0 && r < rows1, m, ts, tn, ps, pn);
#pragma unroll
      for (int j = 0; j + 1 < W; ++j) rt[j] = rt[j + 1], rp[j] = rp[j + 1];
      rt[W - 1] = tn > 0 ? ts / (double)tn : nan;           // tg_mean(freq="7D"): the mean of the present days
      rp[W - 1] = pn > 0 ? ps : (a.binned ? 0.0 : nan);     // precip_accumulation(freq="7D"): an empty bin sums to 0
      if (s >= s0 && s >= W - 1) {
        double qt = rt[0], qp = rp[0];
#pragma unroll
        for (int j = 1; j < W; ++j) qt += rt[j], qp += rp[j];
        qt = qt / (double)W;
        wet.see<true>(qp, qt, s);
        dry.see<false>(qp, qt, s);
        warm.see<true>(qt, qp, s);
        cold.see<false>(qt, qp, s);
      }
    }
  }

  const int64_t o = p * a.ld_out + c;
  auto put = [&](int k, double v) {
    if (a.out[k - 1]) a.out[k - 1][o] = v;
  };
  const double b2 = m.nd > 0 ? m.sd / (double)m.nd : nan;
  const double b7 = (m.ntx > 0 && m.ntn > 0) ? (double)(TE)(m.tx - m.tn) : nan;
  put(1, m.n1 > 0 ? m.s1 / (double)m.n1 : nan);
  put(2, b2);
  put(3, b2 / b7 * 100);
  put(4, m.wt.cv100());
  put(5, m.ntx > 0 ? (double)m.tx : nan);
  put(6, m.ntn > 0 ? (double)m.tn : nan);
  put(7, b7);
  put(8, wet.idx >= 0 ? wet.other : nan);
  put(9, dry.idx >= 0 ? dry.other : nan);
  put(10, warm.idx >= 0 ? warm.crit : nan);
  put(11, cold.idx >= 0 ? cold.crit : nan);
  put(12, m.s12);
  put(13, m.npr > 0 ? m.p13 : nan);
  put(14, m.npr > 0 ? m.p14 : nan);
  put(15, m.wp.cv100());
  put(16, wet.idx >= 0 ? wet.crit : nan);
  put(17, dry.idx >= 0 ? dry.crit : nan);
  put(18, warm.idx >= 0 ? warm.other : nan);
  put(19, cold.idx >= 0 ? cold.other : nan);
  if (a.which[0]) a.which[0][o] = wet.idx;
  if (a.which[1]) a.which[1][o] = dry.idx;
  if (a.which[2]) a.which[2][o] = warm.idx;
  if (a.which[3]) a.which[3][o] = cold.idx;
  if (a.count[0]) a.count[0][o] = m.n1;
  if (a.count[1]) a.count[1][o] = m.ntn;
  if (a.count[2]) a.count[2][o] = m.ntx;
  if (a.count[3]) a.count[3][o] = m.npr;
}

// which of the nineteen read a field, and which read a quarter series (bit k = BIO k)
constexpr unsigned B(int k) { return 1u << k; }
constexpr unsigned USES_TAS = B(1) | B(4) | B(8) | B(9) | B(10) | B(11) | B(18) | B(19);
constexpr unsigned USES_TASMIN = B(2) | B(3) | B(6) | B(7);
constexpr unsigned USES_TASMAX = B(2) | B(3) | B(5) | B(7);
constexpr unsigned USES_PR = B(8) | B(9) | B(12) | B(13) | B(14) | B(15) | B(16) | B(17) | B(18) | B(19);
constexpr unsigned USES_QUARTERS = B(8) | B(9) | B(10) | B(11) | B(16) | B(17) | B(18) | B(19);

}  // namespace

int xh_bioclim(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, const void* tasmin, const void* tasmax,
               const void* pr, int64_t S, const int64_t* step_off, const double* factor, int binned, int64_t P,
               const int64_t* seg_rows, const int64_t* seg_steps, int W, double kelvin_offset, double cv_scale, double thresh,
               double* const* outputs, int32_t* const* which_out, int32_t* const* count_out, int64_t ld_out) {
  const char* fn = "xh_bioclim";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(step_off && factor && seg_rows && seg_steps, XH_ERR_ARG, "%s: NULL table", fn);
  XH_REQUIRE(W == 3 || W == 13, XH_ERR_ARG, "%s: the window is 13 steps (daily, weekly) or 3 (monthly), got %d", fn, W);
  // the steps partition rows [step_off[0], step_off[S]) of the field; the periods: rows and steps non-decreasing in range, and
  // (below) the walk of a period (its steps and the lead-in) passes its rows
  rc = xh_check_offsets(fn, step_off, S, T, "step", INT32_MAX);
  if (!rc) rc = xh_check_offsets(fn, seg_rows, P, T, "period");
  if (!rc) rc = xh_check_offsets(fn, seg_steps, P, S, "period step");
  if (rc) return rc;
  unsigned want = 0;
  bool any = false;
  if (outputs)
    for (int k = 1; k <= NBIO; ++k) want |= outputs[k - 1] ? 1u << k : 0u;
  for (int k = 0; k < 4; ++k) any = any || (which_out && which_out[k]) || (count_out && count_out[k]);
  XH_REQUIRE(want || any, XH_ERR_ARG, "%s: no output requested", fn);
  const bool w_wetdry = which_out && (which_out[0] || which_out[1]), w_warmcold = which_out && (which_out[2] || which_out[3]);
  const bool quarters = (want & USES_QUARTERS) || w_wetdry || w_warmcold;
  const bool rd_tas = (want & USES_TAS) || w_warmcold || (count_out && count_out[0]);
  const bool rd_tn = (want & USES_TASMIN) || (count_out && count_out[1]);
  const bool rd_tx = (want & USES_TASMAX) || (count_out && count_out[2]);
  const bool rd_pr = (want & USES_PR) || w_wetdry || (count_out && count_out[3]);
  XH_REQUIRE((!rd_tas || tas) && (!rd_tn || tasmin) && (!rd_tx || tasmax) && (!rd_pr || pr), XH_ERR_ARG,
             "%s: a field needed by the requested outputs is NULL", fn);
  if (quarters)
    for (int64_t p = 0; p < P; ++p) {
      if (seg_rows[p] == seg_rows[p + 1]) continue;
      const int64_t sl = seg_steps[p] - (W - 1) < 0 ? 0 : seg_steps[p] - (W - 1);
      XH_REQUIRE(step_off[sl] <= seg_rows[p] && step_off[seg_steps[p + 1]] >= seg_rows[p + 1], XH_ERR_ARG,
                 "%s: the steps of period %lld and its lead-in do not cover its rows", fn, (long long)p);
    }
  if (P == 0 || C == 0) return XH_OK;

  BioArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, step_off, (size_t)S + 1, &a.step_off);
  if (!rc) rc = xh_upload(ctx, &cur, factor, (size_t)(T > 0 ? T : 1), &a.factor);
  if (!rc) rc = xh_upload(ctx, &cur, seg_rows, (size_t)P + 1, &a.seg_rows);
  if (!rc) rc = xh_upload(ctx, &cur, seg_steps, (size_t)P + 1, &a.seg_steps);
  if (rc) return rc;
  a.tas = rd_tas ? tas : nullptr;
  a.tasmin = rd_tn ? tasmin : nullptr;
  a.tasmax = rd_tx ? tasmax : nullptr;
  a.pr = rd_pr ? pr : nullptr;
  for (int k = 0; k < NBIO; ++k) a.out[k] = outputs ? outputs[k] : nullptr;
  for (int k = 0; k < 4; ++k) {
    a.which[k] = which_out ? which_out[k] : nullptr;
    a.count[k] = count_out ? count_out[k] : nullptr;
  }
  a.C = C;
  a.ld = ld;
  a.ld_out = ld_out;
  a.kelvin = kelvin_offset;
  a.cv_scale = cv_scale;
  a.thresh = thresh;
  a.binned = binned != 0;
  a.quarters = quarters;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P);
  const bool launched = xh_pick<3, 13>(W, [&](auto Wc) {
    xh_by_width(f64, [&](auto w) {
      hipLaunchKernelGGL((k_bioclim<XH_WIDTH(w), decltype(Wc)::value>), g, dim3(XH_BLOCK), 0, ctx->stream, a);
    });
  });
  XH_REQUIRE(launched, XH_ERR_ARG, "%s: no kernel for a window of %d steps", fn, W);
  XH_LAUNCH_CHECK();
  return XH_OK;
}
