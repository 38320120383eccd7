// compound.hip — the compound percentile-day counts (cold_and_dry_days, warm_and_dry_days, warm_and_wet_days, cold_and_wet_days:
// indices/_multivariate.py:162-423), degree_days_exceedance_date (indices/_threshold.py:3215-3310), blowing_snow
// (_multivariate.py:1833-1884) and the period sum of water_cycle_intensity (:1888-1918).  C ABI and the exact definition of every
// result: include/units/xclim_hip_compound.h.
//
// k_compound_days: the reference expands two per-doy tables to (T, cells) float64 with resample_doy, compares, takes the
// conjunction and resamples — four times over for the four indices of one (tas, pr) pair.  Here a lane owns 16 bytes of a field
// row (4 float32 or 2 float64 cells) and walks the rows of one period: per row one 16-byte load of tas, one of pr and one or two
// per table, R rows issued before the first is used; the table row of a field row is a scalar load (the row index is uniform
// over the workgroup).  The access pattern is the one k_tcount_year (reduce.hip) settled on: the fields are read once and their
// loads are non-temporal; the table loads are plain, and the grid puts the periods on the fast axis, so that the workgroups that
// are resident together walk the SAME cells in different periods (years) and find the table rows of their tile in L2 / the
// Infinity Cache.  The set of outputs is a template argument: a table no output needs is not loaded, an output that is absent is
// not counted.  The cells of a last partial group, and every cell of a view whose pointers or pitches are not 16-byte aligned,
// take the same walk one cell at a time.  No (T, cells) threshold or mask field exists anywhere.
//
// k_degree_exceedance, k_blowing_snow, k_pair_sum: one lane per (cell, period), cells along x (a wave reads 64 consecutive
// elements of a row), periods along y, 8 rows loaded before the first is used (the lane of k_degree_exceedance stops reading
// at its date).  The window of k_blowing_snow is a ring of `window` float64 differences per lane in LDS (ring[slot * BS_BLOCK +
// lane]: a lane reads and writes its own column only, so the ring needs no barrier), warmed on the window - 1 rows before the
// period.
//
// All arithmetic is float64 on the widened fields, in the reference's order (-ffp-contract=off).
#include "../../include/units/xclim_hip_compound.h"
#include "../../include/xclim_hip_hydro.h"
#include "hostargs.h"

static_assert(XH_BS_MAX_WINDOW == XH_HYDRO_MAX_WINDOW, "the sum windows of the daily units share one limit");

namespace {

constexpr int CD_BLOCK = 256;
constexpr int BS_BLOCK = 128;
constexpr int PL_BATCH = 8;   // rows in flight of the one-cell-per-lane kernels (16 in k_degree_exceedance measured slower)

// ---- xh_compound_doy_days --------------------------------------------------------------------------------------------
struct CdArgs {
  const void *tas, *pr;
  const double* tab[4];  // tas_lo, tas_hi, pr_lo, pr_hi
  double* out[XH_CD_NOUT];
  const int32_t* tidx;   // (T)
  const int64_t* seg;    // (P + 1)
  int64_t C, ld, ld_tab, ld_out;
  int P, period_fast;
};

#if defined(__clang__)
typedef float cd_f4 __attribute__((ext_vector_type(4)));
typedef double cd_d2 __attribute__((ext_vector_type(2)));
#endif

// VEC cells of a field row, read once: a non-temporal 16-byte load where VEC > 1
template <typename TE, int VEC>
__device__ __forceinline__ void cd_field(const TE* __restrict__ p, TE (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = p[0];
  } else {
#if defined(__clang__)
    if constexpr (sizeof(TE) == 4) {
      const cd_f4 t = __builtin_nontemporal_load(reinterpret_cast<const cd_f4*>(p));
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      const cd_d2 t = __builtin_nontemporal_load(reinterpret_cast<const cd_d2*>(p));
      v[0] = t.x, v[1] = t.y;
    }
#else
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = p[i];
#endif
  }
}

// VEC cells of a table row: plain 16-byte loads (the row is read again by the next year's workgroup)
template <int VEC>
__device__ __forceinline__ void cd_table(const double* __restrict__ p, double (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 2) {
      const double2 t = *reinterpret_cast<const double2*>(p + i);
      v[i] = t.x, v[i + 1] = t.y;
    }
  }
}

template <typename TE, int VEC, int OUTS>
__device__ __forceinline__ void cd_walk(const CdArgs& a, int p, int64_t c) {
  constexpr bool TLO = (OUTS & (XH_CD_COLD_DRY | XH_CD_COLD_WET)) != 0, THI = (OUTS & (XH_CD_WARM_DRY | XH_CD_WARM_WET)) != 0;
  constexpr bool PLO = (OUTS & (XH_CD_COLD_DRY | XH_CD_WARM_DRY)) != 0, PHI = (OUTS & (XH_CD_WARM_WET | XH_CD_COLD_WET)) != 0;
  constexpr int NT = (TLO ? 1 : 0) + (THI ? 1 : 0) + (PLO ? 1 : 0) + (PHI ? 1 : 0);
  constexpr int R = NT <= 2 ? 4 : 2;   // rows in flight: 2 + 2 NT 16-byte loads of float32 cells per row
  const int64_t t0 = a.seg[p], t1 = a.seg[p + 1];
  const TE* __restrict__ tas = static_cast<const TE*>(a.tas) + c;
  const TE* __restrict__ pr = static_cast<const TE*>(a.pr) + c;
  int cnt[XH_CD_NOUT][VEC];
#pragma unroll
  for (int o = 0; o < XH_CD_NOUT; ++o)
#pragma unroll
    for (int i = 0; i < VEC; ++i) cnt[o][i] = 0;

  auto tally = [&](const TE (&xt)[VEC], const TE (&xp)[VEC], const double (&tl)[VEC], const double (&th)[VEC],
                   const double (&pl)[VEC], const double (&ph)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const double x = (double)xt[i], q = (double)xp[i];
      const bool cold = TLO && x < tl[i], warm = THI && x > th[i], dry = PLO && q < pl[i], wet = PHI && q > ph[i];
      if (OUTS & XH_CD_COLD_DRY) cnt[0][i] += cold && dry ? 1 : 0;
      if (OUTS & XH_CD_WARM_DRY) cnt[1][i] += warm && dry ? 1 : 0;
      if (OUTS & XH_CD_WARM_WET) cnt[2][i] += warm && wet ? 1 : 0;
      if (OUTS & XH_CD_COLD_WET) cnt[3][i] += cold && wet ? 1 : 0;
    }
  };
  auto tables = [&](int64_t row, double (&tl)[VEC], double (&th)[VEC], double (&pl)[VEC], double (&ph)[VEC]) {
    const int64_t o = row * a.ld_tab + c;
    if (TLO) cd_table<VEC>(a.tab[0] + o, tl);
    if (THI) cd_table<VEC>(a.tab[1] + o, th);
    if (PLO) cd_table<VEC>(a.tab[2] + o, pl);
    if (PHI) cd_table<VEC>(a.tab[3] + o, ph);
  };

  int64_t t = t0;
  for (; t + R <= t1; t += R) {
    int64_t row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) row[r] = (int64_t)a.tidx[t + r];
    TE xt[R][VEC], xp[R][VEC];
    double tl[R][VEC] = {}, th[R][VEC] = {}, pl[R][VEC] = {}, ph[R][VEC] = {};
#pragma unroll
    for (int r = 0; r < R; ++r) {
      cd_field<TE, VEC>(tas + (t + r) * a.ld, xt[r]);
      cd_field<TE, VEC>(pr + (t + r) * a.ld, xp[r]);
      tables(row[r], tl[r], th[r], pl[r], ph[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) tally(xt[r], xp[r], tl[r], th[r], pl[r], ph[r]);
  }
  for (; t < t1; ++t) {  // the rows that are left, one by one
    TE xt[VEC], xp[VEC];
    double tl[VEC] = {}, th[VEC] = {}, pl[VEC] = {}, ph[VEC] = {};
    cd_field<TE, VEC>(tas + t * a.ld, xt);
    cd_field<TE, VEC>(pr + t * a.ld, xp);
    tables((int64_t)a.tidx[t], tl, th, pl, ph);
    tally(xt, xp, tl, th, pl, ph);
  }
  const int64_t o = (int64_t)p * a.ld_out + c;
#pragma unroll
  for (int k = 0; k < XH_CD_NOUT; ++k) {
    if (OUTS & (1 << k)) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) a.out[k][o + i] = (double)cnt[k][i];
    }
  }
}

template <typename TE, int VEC, int OUTS>
__global__ void __launch_bounds__(CD_BLOCK) k_compound_days(CdArgs a) {
  const unsigned tile = a.period_fast ? blockIdx.y : blockIdx.x;
  const int pstart = a.period_fast ? blockIdx.x : blockIdx.y, pstep = a.period_fast ? gridDim.x : gridDim.y;
  const int64_t c = ((int64_t)tile * CD_BLOCK + threadIdx.x) * VEC;
  if (c >= a.C) return;
  for (int p = pstart; p < a.P; p += pstep) {
    if (VEC == 1 || c + VEC <= a.C) {
      cd_walk<TE, VEC, OUTS>(a, p, c);
    } else {  // the last, partial group of the row
      for (int64_t cc = c; cc < a.C; ++cc) cd_walk<TE, 1, OUTS>(a, p, cc);
    }
  }
}

// ---- xh_degree_exceedance_date ---------------------------------------------------------------------------------------
struct DxArgs {
  const void* tas;
  const int64_t *seg, *start;  // (P + 1), (P)
  const double* never;         // (P)
  const int32_t* doy;          // (T)
  double* out;
  int64_t C, ld, ld_out;
  double thresh, sum_thresh;
  int below;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_degree_exceedance(DxArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1], s0 = a.start[p];
  const double st = a.sum_thresh;
  double res = xh_nan64();
  // The reference's find_boundary_run (run_length.py:600-610) gives NaN when argmax == argmin, that is also when EVERY row of
  // the period is above the threshold.  The running sum never decreases, so that is the case exactly when the period's first
  // row is above it: with a negative threshold (rows before the start hold 0), or with the exceedance on row seg[p] itself.
  if (s0 >= 0 && r1 > r0 && !(0.0 > st)) {
    if (st == st) res = a.never[p];
    double s = 0.0;
    bool found = false;
    for (int64_t tb = s0; tb < r1 && !found; tb += PL_BATCH) {
      TE x[PL_BATCH];
#pragma unroll
      for (int u = 0; u < PL_BATCH; ++u) x[u] = tb + u < r1 ? xh_ld<TE>(a.tas, (tb + u) * a.ld + c) : (TE)0;
#pragma unroll
      for (int u = 0; u < PL_BATCH; ++u) {
        if (tb + u < r1 && !found) {
          const double v = (double)x[u];
          const double d = a.below ? a.thresh - v : v - a.thresh;
          s += d > 0.0 ? d : 0.0;  // clip(0); a NaN row adds 0, as xarray's cumsum skips it
          if (s > st) {
            res = tb + u > r0 ? (double)a.doy[tb + u] : xh_nan64();
            found = true;
          }
        }
      }
    }
  }
  a.out[p * a.ld_out + c] = res;
}

// ---- xh_blowing_snow_days --------------------------------------------------------------------------------------------
struct BsArgs {
  const void *snd, *wind;
  const int64_t* seg;    // (P + 1)
  const uint8_t* flags;  // (T) or NULL
  double* out;
  int64_t C, ld, ld_out;
  double snd_thresh, wind_thresh;
  int window;
};

template <typename TE>
__global__ void __launch_bounds__(BS_BLOCK) k_blowing_snow(BsArgs a) {
  extern __shared__ double bs_ring[];  // [window][BS_BLOCK]
  double* ring = bs_ring + threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * BS_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  const int W = a.window;
  int64_t i0 = r0 - (W - 1);  // the first row whose difference a window of the period holds
  if (i0 < 1) i0 = 1;
  int cnt = 0;
  if (i0 < r1) {
    double prev = xh_ldw<TE>(a.snd, (i0 - 1) * a.ld + c);
    int slot = 0;
    for (int64_t tb = i0; tb < r1; tb += PL_BATCH) {
      TE xs[PL_BATCH], xw[PL_BATCH];
      int fl[PL_BATCH];
#pragma unroll
      for (int u = 0; u < PL_BATCH; ++u) {
        const int64_t t = tb + u;
        xs[u] = xw[u] = (TE)0;
        fl[u] = 0;
        if (t < r1) {
          xs[u] = xh_ld<TE>(a.snd, t * a.ld + c);
          if (t >= r0) {
            xw[u] = xh_ld<TE>(a.wind, t * a.ld + c);
            fl[u] = a.flags ? (int)a.flags[t] : 1;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PL_BATCH; ++u) {
        const int64_t t = tb + u;
        if (t >= r1) break;
        const double cur = (double)xs[u];
        ring[(int64_t)slot * BS_BLOCK] = cur - prev;
        prev = cur;
        if (t >= r0 && t >= W) {  // the ring holds d[t - W + 1] .. d[t]; the oldest follows the newest
          int k = slot + 1 == W ? 0 : slot + 1;
          double s = ring[(int64_t)k * BS_BLOCK];
          for (int m = 1; m < W; ++m) {
            k = k + 1 == W ? 0 : k + 1;
            s += ring[(int64_t)k * BS_BLOCK];
          }
          cnt += (s >= a.snd_thresh && (double)xw[u] >= a.wind_thresh && fl[u] != 0) ? 1 : 0;
        }
        slot = slot + 1 == W ? 0 : slot + 1;
      }
    }
  }
  a.out[p * a.ld_out + c] = (double)cnt;
}

// ---- xh_pair_period_sum ----------------------------------------------------------------------------------------------
struct PsArgs {
  const void *a, *b;
  const int64_t* seg;
  double* out;
  int64_t C, ld, ld_out;
  double scale;
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_pair_sum(PsArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p], r1 = a.seg[p + 1];
  double s = 0.0;
  for (int64_t tb = r0; tb < r1; tb += PL_BATCH) {
    TE xa[PL_BATCH], xb[PL_BATCH];
#pragma unroll
    for (int u = 0; u < PL_BATCH; ++u) {
      const bool in = tb + u < r1;
      xa[u] = in ? xh_ld<TE>(a.a, (tb + u) * a.ld + c) : (TE)xh_nan64();
      xb[u] = in ? xh_ld<TE>(a.b, (tb + u) * a.ld + c) : (TE)xh_nan64();
    }
#pragma unroll
    for (int u = 0; u < PL_BATCH; ++u) {
      const double v = ((double)xa[u] + (double)xb[u]) * a.scale;
      s += v == v ? v : 0.0;
    }
  }
  a.out[p * a.ld_out + c] = s;
}

// 16-byte loads of VEC elements of esz bytes from p with row pitch ld
bool aligned16(const void* p, int64_t ld, size_t esz) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld * (int64_t)esz) % 16 == 0; }

template <typename TE, int VEC>
void launch_compound_days(int outs, dim3 g, hipStream_t stream, const CdArgs& a) {
  xh_pick<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15>(outs, [&](auto O) {
    hipLaunchKernelGGL((k_compound_days<TE, VEC, decltype(O)::value>), g, dim3(CD_BLOCK), 0, stream, a);
  });
}

}  // namespace

int xh_compound_doy_days(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, const void* pr, int64_t ndoy,
                         int64_t ld_tab, const double* tas_lo, const double* tas_hi, const double* pr_lo, const double* pr_hi,
                         const int32_t* tidx, int64_t P, const int64_t* seg, double* cold_dry, double* warm_dry, double* warm_wet,
                         double* cold_wet, int64_t ld_out) {
  const char* fn = "xh_compound_doy_days";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(tas && pr && tidx, XH_ERR_ARG, "%s: NULL argument", fn);
  const int outs = (cold_dry ? XH_CD_COLD_DRY : 0) | (warm_dry ? XH_CD_WARM_DRY : 0) | (warm_wet ? XH_CD_WARM_WET : 0) |
                   (cold_wet ? XH_CD_COLD_WET : 0);
  XH_REQUIRE(outs, XH_ERR_ARG, "%s: no output requested", fn);
  XH_REQUIRE(ndoy >= 1 && ndoy <= 0x7FFFFFFF, XH_ERR_ARG, "%s: ndoy must be at least 1, got %lld", fn, (long long)ndoy);
  rc = xh_check_rows(fn, ld_tab, C, "ld_tab");
  if (rc) return rc;
  XH_REQUIRE(ndoy * ld_tab + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: table too large", fn);
  const bool need[4] = {(outs & (XH_CD_COLD_DRY | XH_CD_COLD_WET)) != 0, (outs & (XH_CD_WARM_DRY | XH_CD_WARM_WET)) != 0,
                        (outs & (XH_CD_COLD_DRY | XH_CD_WARM_DRY)) != 0, (outs & (XH_CD_WARM_WET | XH_CD_COLD_WET)) != 0};
  const double* tab[4] = {tas_lo, tas_hi, pr_lo, pr_hi};
  static const char* const names[4] = {"tas_lo", "tas_hi", "pr_lo", "pr_hi"};
  for (int k = 0; k < 4; ++k) XH_REQUIRE(!need[k] || tab[k], XH_ERR_ARG, "%s: a requested output needs the table %s", fn, names[k]);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  for (int64_t r = seg[0]; r < seg[P]; ++r)
    XH_REQUIRE(tidx[r] >= 0 && tidx[r] < ndoy, XH_ERR_ARG, "%s: tidx[%lld] = %d outside the table (ndoy = %lld)", fn, (long long)r,
               tidx[r], (long long)ndoy);
  if (P == 0 || C == 0) return XH_OK;

  CdArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc) rc = xh_upload(ctx, &cur, tidx, (size_t)T, &a.tidx);
  if (rc) return rc;
  a.tas = tas, a.pr = pr;
  const size_t esz = f64 ? 8 : 4;
  bool wide = aligned16(tas, ld, esz) && aligned16(pr, ld, esz);
  for (int k = 0; k < 4; ++k) {
    a.tab[k] = need[k] ? tab[k] : nullptr;
    if (need[k]) wide = wide && aligned16(tab[k], ld_tab, 8);
  }
  a.out[0] = cold_dry, a.out[1] = warm_dry, a.out[2] = warm_wet, a.out[3] = cold_wet;
  a.C = C, a.ld = ld, a.ld_tab = ld_tab, a.ld_out = ld_out, a.P = (int)P;
  const int vec = wide ? (f64 ? 2 : 4) : 1;
  const unsigned tiles = (unsigned)cdiv64(cdiv64(C, vec), CD_BLOCK);
  a.period_fast = (P > 1 && tiles <= 65535u) ? 1 : 0;
  const dim3 g = a.period_fast ? dim3(xh_period_blocks((int)P), tiles) : dim3(tiles, xh_period_blocks((int)P));
  if (f64) {
    if (wide) launch_compound_days<double, 2>(outs, g, ctx->stream, a);
    else launch_compound_days<double, 1>(outs, g, ctx->stream, a);
  } else {
    if (wide) launch_compound_days<float, 4>(outs, g, ctx->stream, a);
    else launch_compound_days<float, 1>(outs, g, ctx->stream, a);
  }
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_degree_exceedance_date(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* tas, double thresh, int below,
                              double sum_thresh, int64_t P, const int64_t* seg, const int64_t* start, const double* never,
                              const int32_t* doy, double* out, int64_t ld_out) {
  const char* fn = "xh_degree_exceedance_date";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(tas && start && never && doy && out, XH_ERR_ARG, "%s: NULL argument", fn);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  for (int64_t p = 0; p < P; ++p)
    XH_REQUIRE(start[p] == -1 || (start[p] >= seg[p] && start[p] < seg[p + 1]), XH_ERR_ARG,
               "%s: start[%lld] = %lld is neither -1 nor a row of its period", fn, (long long)p, (long long)start[p]);
  for (int64_t r = seg[0]; r < seg[P]; ++r)
    XH_REQUIRE(doy[r] >= 1 && doy[r] <= 366, XH_ERR_ARG, "%s: doy[%lld] = %d outside 1 .. 366", fn, (long long)r, doy[r]);
  if (P == 0 || C == 0) return XH_OK;

  DxArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc) rc = xh_upload(ctx, &cur, start, (size_t)P, &a.start);
  if (!rc) rc = xh_upload(ctx, &cur, never, (size_t)P, &a.never);
  if (!rc) rc = xh_upload(ctx, &cur, doy, (size_t)T, &a.doy);
  if (rc) return rc;
  a.tas = tas, a.out = out;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.thresh = thresh, a.sum_thresh = sum_thresh, a.below = below != 0;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_degree_exceedance<XH_WIDTH(w)>, g, b, 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_blowing_snow_days(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* snd, const void* sfcWind,
                         double snd_thresh, double wind_thresh, int window, int64_t P, const int64_t* seg, const uint8_t* flags,
                         double* out, int64_t ld_out) {
  const char* fn = "xh_blowing_snow_days";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(snd && sfcWind && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "%s: window must be at least 1, got %d", fn, window);
  XH_REQUIRE(window <= XH_BS_MAX_WINDOW, XH_ERR_LIMIT, "%s: windows of up to %d rows are served, got %d", fn, XH_BS_MAX_WINDOW, window);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  if (P == 0 || C == 0) return XH_OK;

  BsArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc && flags) rc = xh_upload(ctx, &cur, flags, (size_t)(T > 0 ? T : 1), &a.flags);
  if (rc) return rc;
  a.snd = snd, a.wind = sfcWind, a.out = out;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.snd_thresh = snd_thresh, a.wind_thresh = wind_thresh, a.window = window;
  const size_t lds = (size_t)window * BS_BLOCK * sizeof(double);  // at most 32 768 bytes
  const dim3 g((unsigned)cdiv64(C, BS_BLOCK), (unsigned)P), b(BS_BLOCK);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_blowing_snow<XH_WIDTH(w)>, g, b, lds, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_pair_period_sum(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* a_field, const void* b_field, double scale,
                       int64_t P, const int64_t* seg, double* out, int64_t ld_out) {
  const char* fn = "xh_pair_period_sum";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(a_field && b_field && out, XH_ERR_ARG, "%s: NULL argument", fn);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  if (P == 0 || C == 0) return XH_OK;

  PsArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (rc) return rc;
  a.a = a_field, a.b = b_field, a.out = out;
  a.C = C, a.ld = ld, a.ld_out = ld_out, a.scale = scale;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)P), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_pair_sum<XH_WIDTH(w)>, g, b, 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
