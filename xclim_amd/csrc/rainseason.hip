// rainseason.hip — rain_season (indices/_agro.py:796-980) and the rolling mean + zone lookup of hardiness_zones (:1388-1433,
// get_zones of indices/generic.py:1698-1706).  C ABI and the exact definition of every result: include/xclim_hip_rain.h.
//
// k_rain_season: one lane per (cell, period), cells along x (a wave reads 64 consecutive elements of a row), periods along y.
// The reference's chain — select_time, rolling sums, runs_with_holes, rle, argmax / argmin, a masked copy, a second rle or
// rolling sum, argmax / argmin again — is ONE forward walk of the period:
//
//   * the load FRONT is row f; it decides whether a dry sequence of window_dry_start (wd) rows begins at row i = f - (wd - 1),
//     which is all a stop marker needs ("per_day": a counter of dry rows ending at f; "total": the sum of rows i .. f);
//   * the DECISION row i trails the front by wd - 1 rows: its wet-window sum, its event value, the length of the event run it
//     belongs to and whether that run has reached window_not_dry_start + window_wet_start rows;
//   * at most one candidate start is alive at a time (event runs do not overlap), so the search for the END runs speculatively
//     from the row after the first row of the current in-bounds run and is reset when a new candidate replaces a failed one;
//     once a candidate is confirmed the end search simply goes on.  Every row is decided once; nothing is walked twice.
//
// The rows between i - max(ww, we) + 1 and f live in a ring in LDS, one column per lane (ring[slot * RAIN_BLOCK + lane]) in the
// FIELD's dtype: a lane reads and writes its own column only, so the ring needs no barrier.  A "per_day" dry window longer than
// the ring allows has no lag in the ring: the decision row is read a second time from memory instead (REREAD).  The three date
// selections and the day of year arrive as one int32 per row that the entry point packs on the host (flags | doy << 8): the
// index is uniform over the workgroup, so these are scalar loads, eight per batch, issued with the batch's field loads.
// Loads are issued RAIN_BATCH rows at a time before the first of them is used.
//
// All arithmetic is float64 on the widened field: a[i] = (double)pr[i] * per_day, and a window is added in row order from its
// first term (ASSUMPTION, README: where xarray runs on bottleneck its running sum rounds differently).
//
// k_rolling_zones: one lane per cell walks the periods; the window is re-read from the (P, C) field, which is small and
// cache-resident, so any window is served; the bin edges travel as kernel arguments.
#include <vector>

#include "../../include/xclim_hip_hydro.h"
#include "../../include/xclim_hip_rain.h"
#include "hostargs.h"

static_assert(XH_RAIN_MAX_WINDOW == XH_HYDRO_MAX_WINDOW, "the sum windows of the daily units share one limit");

namespace {

constexpr int RAIN_BLOCK = 128;
constexpr int RAIN_BATCH = 8;

struct RainArgs {
  const void* pr;
  const int64_t* seg;   // (P + 1)
  const int32_t* meta;  // (T): flags | doy << 8
  double *start_out, *end_out, *length_out;
  int64_t C, ld, ld_out;
  double per_day, tw, td, te;
  int ww, wd, we, nrun;  // nrun = window_not_dry_start + window_wet_start
  int total_start, total_end;
  int ring;              // rows of the ring
};

template <typename TE, bool REREAD>
__global__ void __launch_bounds__(RAIN_BLOCK) k_rain_season(RainArgs a) {
  extern __shared__ double rain_ring[];  // TE [ring][RAIN_BLOCK]
  TE* ring = reinterpret_cast<TE*>(rain_ring) + threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * RAIN_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int64_t p = blockIdx.y;
  const int64_t r0 = a.seg[p];
  const int n = (int)(a.seg[p + 1] - r0);
  const double nan = xh_nan64();
  const int ww = a.ww, wd = a.wd, we = a.we, R = a.ring;
  const int L = wd - 1;            // rows the decision trails the front by
  const int Lr = REREAD ? 0 : L;   // ... of which the ring holds this many ahead of the decision row
  const double pd = a.per_day;

  int sf = 0;                      // the ring slot of the front row
  int dc = 0;                      // "per_day": dry rows in a row, ending at the front
  int ev = 0, run_len = 0, run_start = 0;
  bool run_inb = false, confirmed = false;
  int cand = -1, start = -1, n_true = 0, n_inb = 0;
  int d2 = 0, e_first = -1, e_ntrue = 0, n_inb2 = 0;
  bool d2_inb = false;

  for (int fb = 0; fb < n + L; fb += RAIN_BATCH) {
    TE xf[RAIN_BATCH], xd[RAIN_BATCH];
    int mf[RAIN_BATCH], md[RAIN_BATCH];
#pragma unroll
    for (int u = 0; u < RAIN_BATCH; ++u) {
      const int f = fb + u, i = f - L;
      xf[u] = xd[u] = (TE)nan;
      mf[u] = md[u] = 0;
      if (f < n) {
        xf[u] = xh_ld<TE>(a.pr, (r0 + f) * a.ld + c);
        mf[u] = a.meta[r0 + f];
      }
      if (i >= 0 && i < n) {
        md[u] = a.meta[r0 + i];
        if (REREAD) xd[u] = xh_ld<TE>(a.pr, (r0 + i) * a.ld + c);
      }
    }
#pragma unroll
    for (int u = 0; u < RAIN_BATCH; ++u) {
      const int f = fb + u, i = f - L;
      if (f >= n + L) break;
      int si = sf - Lr;            // the ring slot of the decision row
      if (si < 0) si += R;

      // ---- the front: does a dry sequence of wd rows begin at row i?
      bool stop = false;
      if (f < n) {
        const TE raw = (mf[u] & XH_RAIN_START_WINDOW) ? xf[u] : (TE)nan;
        if (!REREAD) ring[(int64_t)sf * RAIN_BLOCK] = raw;
        if (!a.total_start) {
          dc = (double)raw * pd <= a.td ? dc + 1 : 0;
          stop = dc >= wd;
        } else if (i >= 0) {
          int k = si;
          double s = (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          for (int m = 1; m < wd; ++m) {
            k = k + 1 == R ? 0 : k + 1;
            s += (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          }
          stop = s <= a.td;
        }
      } else {
        dc = 0;
      }

      // ---- the decision row
      if (i >= 0) {
        if (REREAD) ring[(int64_t)si * RAIN_BLOCK] = (md[u] & XH_RAIN_START_WINDOW) ? xd[u] : (TE)nan;
        bool wet = false;
        if (i >= ww - 1) {
          int k = si - (ww - 1);
          if (k < 0) k += R;
          double s = (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          for (int m = 1; m < ww; ++m) {
            k = k + 1 == R ? 0 : k + 1;
            s += (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          }
          wet = s >= a.tw;
        }
        const int was = ev;
        ev = stop ? 0 : (wet ? 1 : ev);
        const bool inb = (md[u] & XH_RAIN_START_BOUNDS) != 0, inb2 = (md[u] & XH_RAIN_END_BOUNDS) != 0;
        n_inb += inb ? 1 : 0;
        n_inb2 += inb2 ? 1 : 0;
        if (ev && !was) {          // an event run begins: in bounds and without a start yet, it is the candidate
          run_start = i, run_len = 0, run_inb = inb;
          if (!confirmed && inb) cand = i, e_first = -1, e_ntrue = 0, d2 = 0;
        }
        if (!ev && was && !confirmed) cand = -1;
        if (ev) {
          ++run_len;
          if (run_len == a.nrun && run_inb) {   // run_positions[run_start] is true
            ++n_true;
            if (!confirmed) confirmed = true, start = run_start;
          }
        }
        // the end search, on the rows after the candidate
        if (!a.total_end) {
          if (cand >= 0 && i > cand) {
            if ((double)ring[(int64_t)si * RAIN_BLOCK] * pd <= a.te) {
              if (d2 == 0) d2_inb = inb2;
              ++d2;
              if (d2 == we && d2_inb) {
                ++e_ntrue;
                if (e_first < 0) e_first = i - we + 1;
              }
            } else {
              d2 = 0;
            }
          }
        } else if (i >= we - 1) {
          int k = si - (we - 1);
          if (k < 0) k += R;
          double s = (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          for (int m = 1; m < we; ++m) {
            k = k + 1 == R ? 0 : k + 1;
            s += (double)ring[(int64_t)k * RAIN_BLOCK] * pd;
          }
          if (cand >= 0 && i - we + 1 > cand && s <= a.te && inb2) {
            ++e_ntrue;
            if (e_first < 0) e_first = i;
          }
        }
      }
      sf = sf + 1 == R ? 0 : sf + 1;
    }
  }

  // _get_first_run: none when no row in bounds is marked, and none when every one is (argmax == argmin)
  const bool has_start = confirmed && n_true < n_inb;
  const bool has_end = has_start && e_ntrue > 0 && e_ntrue < n_inb2;
  const int64_t o = p * a.ld_out + c;
  if (a.start_out) a.start_out[o] = has_start ? (double)(a.meta[r0 + start] >> 8) : nan;
  if (a.end_out) a.end_out[o] = has_end ? (double)(a.meta[r0 + e_first] >> 8) : nan;
  if (a.length_out) a.length_out[o] = has_start ? (double)((has_end ? e_first : n) - start) : nan;
}

// ---- xh_rolling_zones -----------------------------------------------------------------------------------------------
struct ZoneArgs {
  const void* x;
  double* out;
  int64_t P, C, ld, ld_out;
  int window, nedges;
  double edges[XH_ZONES_MAX_EDGES];
};

template <typename TE>
__global__ void __launch_bounds__(XH_BLOCK) k_rolling_zones(ZoneArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const double nan = xh_nan64();
  const int W = a.window;
  for (int64_t t = 0; t < a.P; ++t) {
    double zone = nan;
    if (t >= W - 1) {
      double s = (double)xh_ld<TE>(a.x, (t - W + 1) * a.ld + c);
      for (int k = 1; k < W; ++k) s += (double)xh_ld<TE>(a.x, (t - W + 1 + k) * a.ld + c);
      const double mean = s / (double)W;
      int cnt = 0;  // np.digitize(mean, edges): the edges <= mean (none for a NaN mean)
      for (int k = 0; k < a.nedges; ++k) cnt += a.edges[k] <= mean ? 1 : 0;
      int z = cnt - 1;
      if (mean == a.edges[a.nedges - 1]) z = a.nedges - 2;  // the last zone is closed on the right
      if (z >= 0 && z < a.nedges - 1) zone = (double)z;
    }
    a.out[t * a.ld_out + c] = zone;
  }
}

}  // namespace

int xh_rain_season(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* pr, double per_day, int64_t P,
                   const int64_t* seg, const uint8_t* flags, const int32_t* doy, double thresh_wet_start, int window_wet_start,
                   int window_not_dry_start, double thresh_dry_start, int window_dry_start, int total_dry_start, double thresh_dry_end,
                   int window_dry_end, int total_dry_end, double* start_out, double* end_out, double* length_out, int64_t ld_out) {
  const char* fn = "xh_rain_season";
  int rc = xh_check_pitched(fn, ctx, T, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(pr && seg && flags && doy, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(start_out || end_out || length_out, XH_ERR_ARG, "%s: no output requested", fn);
  XH_REQUIRE(window_wet_start >= 1 && window_dry_start >= 1 && window_dry_end >= 1 && window_not_dry_start >= 0, XH_ERR_ARG,
             "%s: windows must be at least 1 (window_not_dry_start at least 0)", fn);
  XH_REQUIRE(window_not_dry_start <= (1 << 30) && window_dry_start <= (1 << 30) && window_dry_end <= (1 << 30), XH_ERR_LIMIT,
             "%s: window too long", fn);
  XH_REQUIRE(window_wet_start <= XH_RAIN_MAX_WINDOW && (!total_dry_start || window_dry_start <= XH_RAIN_MAX_WINDOW) &&
                 (!total_dry_end || window_dry_end <= XH_RAIN_MAX_WINDOW),
             XH_ERR_LIMIT, "%s: sum windows of up to %d rows are served, got %d, %d, %d", fn, XH_RAIN_MAX_WINDOW, window_wet_start,
             window_dry_start, window_dry_end);
  rc = xh_check_offsets(fn, seg, P, T, "period");
  if (rc) return rc;
  for (int64_t p = 0; p < P; ++p) {
    XH_REQUIRE(seg[p + 1] - seg[p] < ((int64_t)1 << 30), XH_ERR_LIMIT, "%s: period too long", fn);
    for (int64_t r = seg[p]; r + 1 < seg[p + 1]; ++r)   // P is the amounts on every row the end search looks at
      XH_REQUIRE(!(flags[r] & XH_RAIN_START_WINDOW) || (flags[r + 1] & XH_RAIN_START_WINDOW), XH_ERR_ARG,
                 "%s: the rows inside the start window must be the last rows of their period (row %lld)", fn, (long long)r);
  }
  for (int64_t r = seg[0]; r < seg[P]; ++r)
    XH_REQUIRE(doy[r] >= 1 && doy[r] <= 366, XH_ERR_ARG, "%s: doy[%lld] = %d outside 1 .. 366", fn, (long long)r, doy[r]);
  if (P == 0 || C == 0) return XH_OK;

  std::vector<int32_t> meta((size_t)(T > 0 ? T : 1), 0);
  for (int64_t r = seg[0]; r < seg[P]; ++r) meta[(size_t)r] = (int32_t)flags[r] | (doy[r] << 8);

  RainArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc) rc = xh_upload(ctx, &cur, (const int32_t*)meta.data(), meta.size(), &a.meta);
  if (rc) return rc;
  a.pr = pr, a.start_out = start_out, a.end_out = end_out, a.length_out = length_out;
  a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.per_day = per_day, a.tw = thresh_wet_start, a.td = thresh_dry_start, a.te = thresh_dry_end;
  a.ww = window_wet_start, a.wd = window_dry_start, a.we = window_dry_end, a.nrun = window_not_dry_start + window_wet_start;
  a.total_start = total_dry_start != 0, a.total_end = total_dry_end != 0;
  const bool reread = !a.total_start && window_dry_start > XH_RAIN_MAX_WINDOW;
  const int behind = a.total_end && window_dry_end > window_wet_start ? window_dry_end : window_wet_start;
  a.ring = (reread ? 0 : window_dry_start - 1) + behind;
  const size_t lds = ((size_t)a.ring * RAIN_BLOCK * (f64 ? 8 : 4) + 7) & ~(size_t)7;  // at most 63 * 128 * 8 = 64 512 bytes
  const dim3 g((unsigned)cdiv64(C, RAIN_BLOCK), (unsigned)P), b(RAIN_BLOCK);
  xh_by_width(f64, [&](auto w) {
    if (reread) hipLaunchKernelGGL((k_rain_season<XH_WIDTH(w), true>), g, b, lds, ctx->stream, a);
    else hipLaunchKernelGGL((k_rain_season<XH_WIDTH(w), false>), g, b, lds, ctx->stream, a);
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_rolling_zones(xh_ctx* ctx, int64_t P, int64_t C, int64_t ld, int f64, const void* x, int window, int64_t nedges,
                     const double* edges, double* out, int64_t ld_out) {
  const char* fn = "xh_rolling_zones";
  int rc = xh_check_pitched(fn, ctx, P, C, ld, P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(x && edges && out, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "%s: window must be at least 1, got %d", fn, window);
  XH_REQUIRE(nedges >= 2, XH_ERR_ARG, "%s: at least two bin edges, got %lld", fn, (long long)nedges);
  XH_REQUIRE(nedges <= XH_ZONES_MAX_EDGES, XH_ERR_LIMIT, "%s: at most %d bin edges, got %lld", fn, XH_ZONES_MAX_EDGES, (long long)nedges);
  for (int64_t k = 0; k + 1 < nedges; ++k)
    XH_REQUIRE(edges[k] < edges[k + 1], XH_ERR_ARG, "%s: the bin edges must be strictly increasing", fn);
  if (P == 0 || C == 0) return XH_OK;

  ZoneArgs a{};
  a.x = x, a.out = out;
  a.P = P, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.window = window, a.nedges = (int)nedges;
  for (int64_t k = 0; k < nedges; ++k) a.edges[k] = edges[k];
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK)), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) { hipLaunchKernelGGL(k_rolling_zones<XH_WIDTH(w)>, g, b, 0, ctx->stream, a); });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
