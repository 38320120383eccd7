// hostargs.h — the host-side front end of an entry point.  Two families: the STREAMING one takes a time-major field
// (x, T, C, st, sc), usually with a period table seg_off[P + 1], and marches it one cell or cell group per lane: the argument
// checks, the tables it uploads, cells per lane, the (cells, periods) grid, and run-time integers turned into template
// arguments.  The PITCHED one takes (ctx, T, C, ld, f64, fields..., P, seg, ..., outs..., ld_out) with float32 or float64 fields
// behind const void* and one lane per (cell, period): its shape checks, its host offset tables, the element width turned into a
// template argument, and launches with dynamic LDS.  Host code only.  Every check answers through XH_REQUIRE with the entry
// point's name `fn` first; nothing here touches the device before the checks of its own call have passed.
#pragma once

#include <type_traits>

#include "common.h"

// the field: non-NULL, a shape that is not negative, cells contiguous and rows that do not overlap
static inline int xh_check_field(const char* fn, xh_ctx* ctx, const void* x, int64_t T, int64_t C, int64_t st, int64_t sc) {
  XH_REQUIRE(ctx && x, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(sc == 1 && st >= C, XH_ERR_LAYOUT, "%s: streaming kernels need a time-major view (sc == 1, st >= C); got st=%lld sc=%lld",
             fn, (long long)st, (long long)sc);
  return XH_OK;
}

// two fields read in step (their cell stride is 1 by contract: these entry points take no sc)
static inline int xh_check_fields2(const char* fn, xh_ctx* ctx, const void* a, const void* b, int64_t T, int64_t C, int64_t st_a,
                                   int64_t st_b) {
  XH_REQUIRE(ctx && a && b, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(st_a >= C && st_b >= C, XH_ERR_LAYOUT, "%s: needs time-major views (row strides >= C); got %lld and %lld", fn,
             (long long)st_a, (long long)st_b);
  return XH_OK;
}

// rows of an output (or of a second input) at least as long as the row
static inline int xh_check_rows(const char* fn, int64_t stride, int64_t C, const char* what) {
  XH_REQUIRE(stride >= C, XH_ERR_LAYOUT, "%s: needs time-major rows of at least the row width (%s)", fn, what);
  return XH_OK;
}

// the segment table: P >= 1 periods, offsets non-decreasing inside [0, T]
static inline int xh_check_segments(const char* fn, const int64_t* seg_off, int P, int64_t T) {
  XH_REQUIRE(seg_off && P >= 1, XH_ERR_ARG, "%s: seg_off NULL or P < 1", fn);
  for (int p = 0; p < P; ++p)
    XH_REQUIRE(seg_off[p] <= seg_off[p + 1] && seg_off[p] >= 0 && seg_off[p + 1] <= T, XH_ERR_ARG,
               "%s: seg_off must be non-decreasing within [0, T]", fn);
  return XH_OK;
}

// a host table copied to the context's scratch ring, typed
template <typename TE>
static inline int xh_upload(xh_ctx* ctx, size_t* cur, const TE* host, size_t n, const TE** dev) {
  void* d = nullptr;
  const int rc = xh_scratch_upload(ctx, cur, host, sizeof(TE) * n, &d);
  if (rc) return rc;
  *dev = static_cast<const TE*>(d);
  return XH_OK;
}

// check, then upload
static inline int xh_upload_segments(const char* fn, xh_ctx* ctx, size_t* cur, const int64_t* seg_off, int P, int64_t T,
                                     const int64_t** d_seg) {
  const int rc = xh_check_segments(fn, seg_off, P, T);
  return rc ? rc : xh_upload(ctx, cur, seg_off, (size_t)P + 1, d_seg);
}

// the day-of-year index of every step: inside the table of D rows
static inline int xh_check_tidx(const char* fn, const int32_t* tidx, int64_t T, int D) {
  XH_REQUIRE(tidx, XH_ERR_ARG, "%s: tidx is NULL", fn);
  for (int64_t t = 0; t < T; ++t)
    XH_REQUIRE(tidx[t] >= 0 && tidx[t] < D, XH_ERR_ARG, "%s: tidx[%lld] = %d outside the table (D = %d)", fn, (long long)t,
               tidx[t], D);
  return XH_OK;
}
static inline int xh_upload_tidx(const char* fn, xh_ctx* ctx, size_t* cur, const int32_t* tidx, int64_t T, int D,
                                 const int32_t** d_tidx) {
  const int rc = xh_check_tidx(fn, tidx, T, D);
  return rc ? rc : xh_upload(ctx, cur, tidx, (size_t)T, d_tidx);
}

// cells per lane: `width` when the view allows vector loads of `width` elements of `esz` bytes, else 1
// (4 x float32 and 2 x float64 are 16-byte loads, 2 x float32 the 8-byte loads of a mixed pair)
static inline int xh_cells_per_lane(const void* p, int64_t C, int64_t st, int width, size_t esz) {
  return ((reinterpret_cast<uintptr_t>(p) & (width * esz - 1)) == 0 && (C % width) == 0 && (st % width) == 0) ? width : 1;
}
static inline int xh_pick_vec(const void* p, int64_t C, int64_t st) { return xh_cells_per_lane(p, C, st, 4, 4); }
static inline int xh_pick_vec64(const void* p, int64_t C, int64_t st, size_t esz = 8) { return xh_cells_per_lane(p, C, st, 2, esz); }

// periods along the second grid axis: a block walks p, p + gridDim.y, ...
static inline unsigned xh_period_blocks(int P) { return (unsigned)(P < 1 ? 1 : (P > 4096 ? 4096 : P)); }
static inline dim3 xh_period_grid(int64_t C, int vec, int P) {
  return dim3((unsigned)cdiv64(cdiv64(C, vec), XH_BLOCK), xh_period_blocks(P));
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; false when none does
template <int... Vs, typename F>
static inline bool xh_pick(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- the pitched family ---------------------------------------------------------------------------------------------
// the shape: a context, nothing negative, rows of the fields (ld) and of the outputs (ld_out) at least the row width, and both
// index ranges below 2^40
static inline int xh_check_pitched(const char* fn, xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int64_t out_rows, int64_t ld_out) {
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(T >= 0 && C >= 0 && out_rows >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  int rc = xh_check_rows(fn, ld, C, "ld");
  if (!rc) rc = xh_check_rows(fn, ld_out, C, "ld_out");
  if (rc) return rc;
  XH_REQUIRE(T * ld + C < ((int64_t)1 << 40) && out_rows * ld_out + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  return XH_OK;
}

// a HOST offset table seg[P + 1] (`what`: "period", "month" ...): non-NULL, at most max_P entries (periods lie along the
// second grid axis: 65535), offsets non-decreasing within [0, rows]
constexpr int64_t XH_MAX_PERIODS = 65535;
static inline int xh_check_offsets(const char* fn, const int64_t* seg, int64_t P, int64_t rows, const char* what,
                                   int64_t max_P = XH_MAX_PERIODS) {
  XH_REQUIRE(seg, XH_ERR_ARG, "%s: NULL %s offsets", fn, what);
  XH_REQUIRE(P >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(P <= max_P, XH_ERR_LIMIT, "%s: at most %lld %ss, got %lld", fn, (long long)max_P, what, (long long)P);
  XH_REQUIRE(seg[0] >= 0 && seg[P] <= rows, XH_ERR_ARG, "%s: %s offsets outside [0, %lld]", fn, what, (long long)rows);
  for (int64_t p = 0; p < P; ++p) XH_REQUIRE(seg[p] <= seg[p + 1], XH_ERR_ARG, "%s: %s offsets must be non-decreasing", fn, what);
  return XH_OK;
}

// f(tag) with XH_WIDTH(tag) = double when f64, float otherwise; returns what f returns
template <typename TE>
struct xh_width {
  using type = TE;
};
#define XH_WIDTH(tag) typename decltype(tag)::type
template <typename F>
static inline auto xh_by_width(int f64, F&& f) {
  if (f64) return f(xh_width<double>{});
  return f(xh_width<float>{});
}

// a launch with dynamic LDS: more than 64 KiB has to be allowed per kernel first
template <typename A>
static inline int xh_launch_lds(void (*kernel)(A), dim3 g, dim3 b, size_t lds, hipStream_t stream, const A& a) {
  if (lds > 64 * 1024) XH_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, g, b, lds, stream, a);
  return XH_OK;
}
