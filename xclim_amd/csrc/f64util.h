// f64util.h — device helpers shared by the float64 FIELD units (f64.hip, f64run.hip, f64red.hip): the 2-element vector loads,
// the double-buffered row marches and the sort keys of a double.  Their host side (argument checks, uploads, cells per lane)
// is hostargs.h.
#pragma once

#include "common.h"
#include "hostargs.h"

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

// order-preserving double <-> uint64 key (ascending; NaN maps to the largest key, so it sorts last like numpy)
__device__ __forceinline__ uint64_t d2key(double d) {
  const uint64_t u = (uint64_t)__double_as_longlong(d);
  if (d != d) return ~0ull;
  return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double key2d(uint64_t k) {
  if (k == ~0ull) return xh_nan64();
  const uint64_t u = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
  return __longlong_as_double((long long)u);
}

}  // namespace
