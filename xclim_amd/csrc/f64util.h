// f64util.h — helpers shared by the float64 FIELD twins (f64run.hip, f64red.hip): the 2-element vector loads, the
// double-buffered row marches, argument checks, the segment upload and the choice of two cells per lane.
#pragma once

#include "common.h"

namespace {

template <typename TE, int VEC>
struct VR {
  TE v[VEC];
};

template <int VEC, typename TE>
__device__ __forceinline__ VR<TE, VEC> ldv(const TE* __restrict__ p) {
  VR<TE, VEC> r;
  if constexpr (VEC == 2) {
    if constexpr (sizeof(TE) == 8) {
      const double2 t = *reinterpret_cast<const double2*>(p);
      r.v[0] = t.x;
      r.v[1] = t.y;
    } else {
      const float2 t = *reinterpret_cast<const float2*>(p);
      r.v[0] = t.x;
      r.v[1] = t.y;
    }
  } else {
    r.v[0] = *p;
  }
  return r;
}

// rows [t0, t1) of one field in double-buffered batches of 8, f(t, row)
template <int VEC, typename TE, typename F>
__device__ __forceinline__ void march(const TE* __restrict__ p, int64_t st, int64_t t0, int64_t t1, F&& f) {
  constexpr int U = 8;
  int64_t t = t0;
  const int64_t nfull = t1 > t0 ? (t1 - t0) / U : 0;
  if (nfull > 0) {
    VR<TE, VEC> buf[U];
#pragma unroll
    for (int u = 0; u < U; ++u) buf[u] = ldv<VEC>(p + (t + u) * st);
    for (int64_t b = 0; b < nfull; ++b) {
      VR<TE, VEC> nxt[U];
      const bool more = b + 1 < nfull;
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = ldv<VEC>(p + (t + U + u) * st);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) f(t + u, buf[u]);
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) buf[u] = nxt[u];
      }
      t += U;
    }
  }
  for (; t < t1; ++t) f(t, ldv<VEC>(p + t * st));
}

// the same over two fields read in step, f(t, row_a, row_b)
template <int VEC, typename TA, typename TB, typename F>
__device__ __forceinline__ void march2(const TA* __restrict__ pa, int64_t sa, const TB* __restrict__ pb, int64_t sb, int64_t t0,
                                       int64_t t1, F&& f) {
  constexpr int U = 8;
  int64_t t = t0;
  const int64_t nfull = t1 > t0 ? (t1 - t0) / U : 0;
  if (nfull > 0) {
    VR<TA, VEC> ba[U];
    VR<TB, VEC> bb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ba[u] = ldv<VEC>(pa + (t + u) * sa);
      bb[u] = ldv<VEC>(pb + (t + u) * sb);
    }
    for (int64_t b = 0; b < nfull; ++b) {
      VR<TA, VEC> na[U];
      VR<TB, VEC> nb[U];
      const bool more = b + 1 < nfull;
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          na[u] = ldv<VEC>(pa + (t + U + u) * sa);
          nb[u] = ldv<VEC>(pb + (t + U + u) * sb);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) f(t + u, ba[u], bb[u]);
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          ba[u] = na[u];
          bb[u] = nb[u];
        }
      }
      t += U;
    }
  }
  for (; t < t1; ++t) f(t, ldv<VEC>(pa + t * sa), ldv<VEC>(pb + t * sb));
}

inline int check_field(const char* fn, xh_ctx* ctx, const void* x, int64_t T, int64_t C, int64_t st, int64_t sc) {
  XH_REQUIRE(ctx && x, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(sc == 1 && st >= C, XH_ERR_LAYOUT, "%s: streaming kernels need a time-major view (sc == 1, st >= C); got st=%lld sc=%lld",
             fn, (long long)st, (long long)sc);
  return XH_OK;
}

// validates the segment table (host), then copies it to the context's scratch: nothing touches the device before the checks
inline int upload_segs(xh_ctx* ctx, size_t* cur, const int64_t* seg_off, int P, int64_t T, const char* fn, const int64_t** d_seg) {
  XH_REQUIRE(seg_off && P >= 1, XH_ERR_ARG, "%s: seg_off NULL or P < 1", fn);
  for (int p = 0; p < P; ++p)
    XH_REQUIRE(seg_off[p] <= seg_off[p + 1] && seg_off[p] >= 0 && seg_off[p + 1] <= T, XH_ERR_ARG,
               "%s: seg_off must be non-decreasing within [0, T]", fn);
  void* d = nullptr;
  const int rc = xh_scratch_upload(ctx, cur, seg_off, sizeof(int64_t) * (size_t)(P + 1), &d);
  if (rc) return rc;
  *d_seg = (const int64_t*)d;
  return XH_OK;
}

// two cells per lane when the view allows 2-element vector loads of `esz`-byte elements
inline int pick_vec(const void* p, int64_t C, int64_t st, size_t esz = 8) {
  return ((reinterpret_cast<uintptr_t>(p) & (2 * esz - 1)) == 0 && (C % 2) == 0 && (st % 2) == 0) ? 2 : 1;
}

}  // namespace
