// dataflags.hip — the checks of xclim.core.dataflags.data_flags (core/dataflags.py:581-746) on one variable in ONE launch, and
// the bound tables of its climatology check.  C ABI and the exact definition of every result: include/xclim_hip_flags.h.
//
// k_data_flags: one lane per cell, consecutive lanes on consecutive cells (a wave reads 64 consecutive elements of a row), one
// forward walk of the whole series.  The variable, up to two companions and, for the climatology check, the two bound rows of
// the step's day of year are loaded FLAGS_BATCH rows at a time before the first of them is used; the list of checks travels as
// kernel arguments and is evaluated on every sample, so every field is read once however many checks there are and no (T, C)
// mask is ever written.  Within a batch the checks are the OUTER loop and the rows the inner one: the kind and the operands of a
// check are scalar loads from the kernel arguments, made once per batch instead of once per sample.
//
//   * One run tracker per lane (the previous value, the run length, the row where the run began) serves every REPEAT check.
//   * The flags of the current period are bits of one register; they are stored when the walk crosses seg[p + 1].
//   * A run that reaches n_k at row t flags rows t - n_k + 1 .. t: the periods from that of row t - n_k + 1 up to the one before
//     the current have been stored already, so the lane stores a 1 into ITS OWN column of those periods (a plain store: no
//     other lane writes there).
//   * reduce_cells: the entry point zeroes out[K, P] and a lane whose period flag is set stores the byte 1.  Every writer
//     writes the same value: no atomics, no wave votes, and the kernel runs thread by thread on the host simulation.
//
// k_doy_bounds: one lane per (cell, day of year), the two passes of k_doy_mean_std (reduce2.hip) on a float32 or float64 field
// with a row pitch; sums in float64, the bounds rounded in the field's dtype.  Loads are unconditional (clamped row, validity
// applied afterwards), so the samples of a window are in flight together.
#include "../../include/xclim_hip_flags.h"
#include "hostargs.h"

namespace {

constexpr int FLAGS_BLOCK = 64;
constexpr int FLAGS_BATCH = 8;

struct FlagArgs {
  const void *x, *y0, *y1, *lo, *hi;
  const int64_t* seg;    // (P + 1)
  const int32_t* tidx;   // (T), CLIM only
  uint8_t* out;
  int64_t T, C, P, ld, ld_y0, ld_y1, ld_tab, ld_out;
  int K, reduce_cells;
  xh_flag_check chk[XH_FLAGS_MAX_CHECKS];
};

// PAIRS: a PAIR check is present (an absent companion aliases x, so both are always loaded); CLIM, REPEAT: such a check is present
template <typename TE, bool PAIRS, bool CLIM, bool REPEAT>
__global__ void __launch_bounds__(FLAGS_BLOCK) k_data_flags(FlagArgs a) {
  const int64_t c = (int64_t)blockIdx.x * FLAGS_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int K = a.K;
  const int64_t T = a.T, P = a.P;

  auto store = [&](int k, int64_t p, uint8_t bit) {
    if (a.reduce_cells) {
      if (bit) a.out[(int64_t)k * P + p] = 1;
    } else {
      a.out[((int64_t)k * P + p) * a.ld_out + c] = bit;
    }
  };
  auto flush = [&](int64_t p, uint32_t mask) {
    for (int k = 0; k < K; ++k) store(k, p, (uint8_t)((mask >> k) & 1u));
  };

  int64_t p = 0, next = a.seg[1];
  uint32_t mask = 0;
  TE prev = (TE)0;
  int32_t run_len = 0;   // (T < 2^31: checked by the entry point)

  for (int64_t tb = 0; tb < T; tb += FLAGS_BATCH) {
    TE xv[FLAGS_BATCH], y0v[FLAGS_BATCH], y1v[FLAGS_BATCH], lov[FLAGS_BATCH], hiv[FLAGS_BATCH];
#pragma unroll
    for (int u = 0; u < FLAGS_BATCH; ++u) {
      const int64_t t = tb + u < T ? tb + u : T - 1;   // (clamped: the loads of a batch are unconditional)
      xv[u] = xh_ld<TE>(a.x, t * a.ld + c);
      if (PAIRS) {
        y0v[u] = xh_ld<TE>(a.y0, t * a.ld_y0 + c);
        y1v[u] = xh_ld<TE>(a.y1, t * a.ld_y1 + c);
      }
      if (CLIM) {
        const int64_t d = a.tidx[t];
        lov[u] = xh_ld<TE>(a.lo, d * a.ld_tab + c);
        hiv[u] = xh_ld<TE>(a.hi, d * a.ld_tab + c);
      }
    }
    // the flags of the batch's rows, check by check: a check's kind and operands are read once per batch, not once per sample
    uint32_t bits[FLAGS_BATCH], reach[FLAGS_BATCH];   // reach: the REPEAT checks whose run has reached n on this very row
    int32_t rl[FLAGS_BATCH];                           // the length of the run the row ends
#pragma unroll
    for (int u = 0; u < FLAGS_BATCH; ++u) {
      bits[u] = reach[u] = 0u;
      rl[u] = 0;
      if (REPEAT) {   // (the clamped rows past T - 1 go on counting: nothing reads the tracker after them)
        run_len = (tb + u > 0 && xv[u] == prev) ? run_len + 1 : 1;
        prev = xv[u];
        rl[u] = run_len;
      }
    }
    for (int k = 0; k < K; ++k) {
      const xh_flag_check q = a.chk[k];
      const uint32_t bit = 1u << k;
      switch (q.kind) {
        case XH_FLAG_CMP:
#pragma unroll
          for (int u = 0; u < FLAGS_BATCH; ++u) bits[u] |= xh_cmp_f64((double)xv[u], q.op, q.a) ? bit : 0u;
          break;
        case XH_FLAG_OUTSIDE:
#pragma unroll
          for (int u = 0; u < FLAGS_BATCH; ++u) bits[u] |= ((double)xv[u] < q.a || (double)xv[u] > q.b) ? bit : 0u;
          break;
        case XH_FLAG_PAIR:
          if (PAIRS) {
#pragma unroll
            for (int u = 0; u < FLAGS_BATCH; ++u)
              bits[u] |= xh_cmp_f64((double)xv[u], q.op, (double)(q.other ? y1v[u] : y0v[u])) ? bit : 0u;
          }
          break;
        case XH_FLAG_REPEAT:
          if (REPEAT) {
#pragma unroll
            for (int u = 0; u < FLAGS_BATCH; ++u) {
              const bool f = rl[u] >= q.n && (q.op < 0 || xh_cmp_f64((double)xv[u], q.op, q.a));
              bits[u] |= f ? bit : 0u;
              reach[u] |= (f && rl[u] == q.n) ? bit : 0u;
            }
          }
          break;
        default:  // XH_FLAG_CLIM
          if (CLIM) {
#pragma unroll
            for (int u = 0; u < FLAGS_BATCH; ++u) bits[u] |= !(lov[u] < xv[u] && xv[u] < hiv[u]) ? bit : 0u;
          }
          break;
      }
    }
    // the rows in order: the periods they close, the mask of their own period, the periods a run reaches back into
#pragma unroll
    for (int u = 0; u < FLAGS_BATCH; ++u) {
      const int64_t t = tb + u;
      if (t >= T) break;
      while (t >= next) {   // (seg[P] == T > t: p + 1 stays below P)
        flush(p, mask);
        mask = 0;
        ++p;
        next = a.seg[p + 1];
      }
      mask |= bits[u];
      if (REPEAT && reach[u]) {   // a run has just become suspicious: its rows in the periods stored already
        const int64_t run_start = t - rl[u] + 1;
        for (int k = 0; k < K; ++k) {
          if (!((reach[u] >> k) & 1u)) continue;
          for (int64_t s = p - 1; s >= 0 && a.seg[s + 1] > run_start; --s)
            if (a.seg[s] < a.seg[s + 1]) store(k, s, 1);
        }
      }
    }
  }
  flush(p, mask);
  for (int64_t s = p + 1; s < P; ++s) flush(s, 0u);   // empty periods after the last row
}

struct BoundArgs {
  const void* x;
  const int32_t* tbase;  // (nyears, ndoy)
  void *lo, *hi;
  int64_t T, C, ld, ld_out;
  int nyears, ndoy, window;
  double n;
};

template <typename TE, int W>
__global__ void __launch_bounds__(XH_BLOCK) k_doy_bounds(BoundArgs a) {
  const int64_t c = (int64_t)blockIdx.x * XH_BLOCK + threadIdx.x;
  if (c >= a.C) return;
  const int w = W > 0 ? W : a.window;   // W == 0: run-time window
  const int half = w / 2;
  const int64_t T = a.T;
  const TE nan = sizeof(TE) == 8 ? (TE)xh_nan64() : (TE)xh_nan32();
  for (int d = blockIdx.y; d < a.ndoy; d += gridDim.y) {
    double s = 0.0;
    int m = 0;
    auto pass = [&](auto&& f) {
      for (int y = 0; y < a.nyears; ++y) {
        const int64_t tb = a.tbase[(int64_t)y * a.ndoy + d];
        if (W > 0) {
          TE v[W > 0 ? W : 1];
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const int64_t t = tb - half + k;
            v[k] = xh_ld<TE>(a.x, (t < 0 ? 0 : (t >= T ? T - 1 : t)) * a.ld + c);
          }
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const int64_t t = tb - half + k;
            if (tb >= 0 && t >= 0 && t < T && v[k] == v[k]) f((double)v[k]);
          }
        } else {
          for (int k = 0; k < w; ++k) {
            const int64_t t = tb - half + k;
            const TE v = xh_ld<TE>(a.x, (t < 0 ? 0 : (t >= T ? T - 1 : t)) * a.ld + c);
            if (tb >= 0 && t >= 0 && t < T && v == v) f((double)v);
          }
        }
      }
    };
    pass([&](double v) { s += v; ++m; });
    const double mean = m > 0 ? s / (double)m : 0.0;
    double s2 = 0.0;
    pass([&](double v) { const double dv = v - mean; s2 += dv * dv; });
    TE lo = nan, hi = nan;
    if (m > 0) {
      const TE mu = (TE)mean, sig = (TE)sqrt(s2 / (double)m);
      const TE spread = (TE)a.n * sig;
      lo = mu - spread;
      hi = mu + spread;
    }
    reinterpret_cast<TE*>(a.lo)[(int64_t)d * a.ld_out + c] = lo;
    reinterpret_cast<TE*>(a.hi)[(int64_t)d * a.ld_out + c] = hi;
  }
}

}  // namespace

int xh_data_flags(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const void* y0, int64_t ld_y0,
                  const void* y1, int64_t ld_y1, int K, const xh_flag_check* checks, int64_t P, const int64_t* seg,
                  const int32_t* tidx, int64_t D, const void* lo, const void* hi, int64_t ld_tab, int reduce_cells, uint8_t* out,
                  int64_t ld_out) {
  const char* fn = "xh_data_flags";
  XH_REQUIRE(K >= 0 && P >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(K <= XH_FLAGS_MAX_CHECKS, XH_ERR_LIMIT, "%s: at most %d checks, got %d", fn, XH_FLAGS_MAX_CHECKS, K);
  int rc = xh_check_pitched(fn, ctx, T, C, ld, (int64_t)K * P, ld_out);
  if (rc) return rc;
  XH_REQUIRE(x && out && (checks || K == 0), XH_ERR_ARG, "%s: NULL argument", fn);
  bool pairs = false, clim = false, repeat = false;
  for (int k = 0; k < K; ++k) {
    const xh_flag_check& q = checks[k];
    XH_REQUIRE(q.kind >= XH_FLAG_CMP && q.kind <= XH_FLAG_CLIM, XH_ERR_ARG, "%s: check %d: unknown kind %d", fn, k, q.kind);
    const bool has_op = q.kind == XH_FLAG_CMP || q.kind == XH_FLAG_PAIR || q.kind == XH_FLAG_REPEAT;
    XH_REQUIRE(!has_op || (q.op >= XH_OP_GT && q.op <= XH_OP_NE) || (q.kind == XH_FLAG_REPEAT && q.op == -1), XH_ERR_ARG,
               "%s: check %d: unknown operator %d", fn, k, q.op);
    if (q.kind == XH_FLAG_REPEAT) {
      XH_REQUIRE(q.n >= 1, XH_ERR_ARG, "%s: check %d: runs of at least 1 row, got n = %d", fn, k, q.n);
      repeat = true;
    }
    if (q.kind == XH_FLAG_PAIR) {
      XH_REQUIRE(q.other == 0 || q.other == 1, XH_ERR_ARG, "%s: check %d: companion %d is neither 0 nor 1", fn, k, q.other);
      XH_REQUIRE(q.other ? y1 != nullptr : y0 != nullptr, XH_ERR_ARG, "%s: check %d: companion y%d is NULL", fn, k, q.other);
      pairs = true;
    }
    if (q.kind == XH_FLAG_CLIM) clim = true;
  }
  for (int j = 0; j < 2; ++j) {
    if (!(j ? y1 : y0)) continue;
    const int64_t ldy = j ? ld_y1 : ld_y0;
    rc = xh_check_rows(fn, ldy, C, j ? "ld_y1" : "ld_y0");
    if (rc) return rc;
    XH_REQUIRE(T * ldy + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  }
  XH_REQUIRE(T < INT32_MAX, XH_ERR_LIMIT, "%s: series too long", fn);
  rc = xh_check_offsets(fn, seg, P, T, "period", INT64_MAX);
  if (rc) return rc;
  XH_REQUIRE(seg[0] == 0 && seg[P] == T, XH_ERR_ARG, "%s: the periods must cover [0, T]: seg[0] = %lld, seg[P] = %lld, T = %lld", fn,
             (long long)seg[0], (long long)seg[P], (long long)T);
  if (clim) {
    XH_REQUIRE(tidx && lo && hi, XH_ERR_ARG, "%s: the climatology check needs tidx and both bound tables", fn);
    XH_REQUIRE(D >= 1 && D <= INT32_MAX, XH_ERR_ARG, "%s: bound tables of %lld rows", fn, (long long)D);
    rc = xh_check_rows(fn, ld_tab, C, "ld_tab");
    if (!rc) rc = xh_check_tidx(fn, tidx, T, (int)D);
    if (rc) return rc;
    XH_REQUIRE(D * ld_tab + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: bound tables too large", fn);
  }
  if (T == 0 || C == 0 || P == 0 || K == 0) return XH_OK;

  FlagArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, seg, (size_t)P + 1, &a.seg);
  if (!rc && clim) rc = xh_upload(ctx, &cur, tidx, (size_t)T, &a.tidx);
  if (rc) return rc;
  a.x = x, a.out = out;
  a.y0 = y0 ? y0 : x, a.ld_y0 = y0 ? ld_y0 : ld;   // (an absent companion is never compared: it aliases x)
  a.y1 = y1 ? y1 : x, a.ld_y1 = y1 ? ld_y1 : ld;
  a.lo = lo, a.hi = hi, a.ld_tab = ld_tab;
  a.T = T, a.C = C, a.P = P, a.ld = ld, a.ld_out = ld_out;
  a.K = K, a.reduce_cells = reduce_cells != 0;
  for (int k = 0; k < K; ++k) a.chk[k] = checks[k];
  if (a.reduce_cells) XH_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)K * (size_t)P, ctx->stream));
  const dim3 g((unsigned)cdiv64(C, FLAGS_BLOCK)), b(FLAGS_BLOCK);
  xh_by_width(f64, [&](auto w) {
    using TE = XH_WIDTH(w);
    xh_pick<0, 1, 2, 3, 4, 5, 6, 7>((pairs ? 1 : 0) | (clim ? 2 : 0) | (repeat ? 4 : 0), [&](auto V) {
      constexpr int v = decltype(V)::value;
      hipLaunchKernelGGL((k_data_flags<TE, (v & 1) != 0, (v & 2) != 0, (v & 4) != 0>), g, b, 0, ctx->stream, a);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_doy_bounds(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const int32_t* tbase, int nyears, int ndoy,
                  int window, double n, void* lo, void* hi, int64_t ld_out) {
  const char* fn = "xh_doy_bounds";
  XH_REQUIRE(ndoy >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  int rc = xh_check_pitched(fn, ctx, T, C, ld, ndoy, ld_out);
  if (rc) return rc;
  XH_REQUIRE(x && tbase && lo && hi, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(nyears >= 1 && window >= 1, XH_ERR_ARG, "%s: at least one year and a window of at least 1, got %d and %d", fn, nyears,
             window);
  XH_REQUIRE(T <= INT32_MAX, XH_ERR_LIMIT, "%s: series too long", fn);
  for (int64_t i = 0; i < (int64_t)nyears * ndoy; ++i)
    XH_REQUIRE(tbase[i] >= -1 && tbase[i] < T, XH_ERR_ARG, "%s: tbase[%lld] = %d outside [-1, T)", fn, (long long)i, tbase[i]);
  if (T == 0 || C == 0 || ndoy == 0) return XH_OK;

  BoundArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, tbase, (size_t)nyears * (size_t)ndoy, &a.tbase);
  if (rc) return rc;
  a.x = x, a.lo = lo, a.hi = hi;
  a.T = T, a.C = C, a.ld = ld, a.ld_out = ld_out;
  a.nyears = nyears, a.ndoy = ndoy, a.window = window, a.n = n;
  const dim3 g((unsigned)cdiv64(C, XH_BLOCK), (unsigned)(ndoy > 1024 ? 1024 : ndoy)), b(XH_BLOCK);
  xh_by_width(f64, [&](auto w) {
    using TE = XH_WIDTH(w);
    xh_pick<5, 3, 7, 0>((window == 5 || window == 3 || window == 7) ? window : 0,
                        [&](auto W) { hipLaunchKernelGGL((k_doy_bounds<TE, decltype(W)::value>), g, b, 0, ctx->stream, a); });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
