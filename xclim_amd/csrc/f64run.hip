// f64run.hip — float64 FIELD twins of the compare, run-length, spell and day-of-year percentile entry points.
//
// The reference computes in the dtype of its data: compare() of a float64 DataArray is a float64 compare
// (indices/generic.py:301-326, 360), the rolling window statistics of spell_mask are float64 sums / means / extremes
// (generic.py:506-535), and _nan_quantile takes its `diff` in the data dtype (core/utils.py:486; percentile_doy keeps
// rrr.dtype, core/calendar.py:395-494).  Rounding such a field to float32 first flips every day that lies within one
// float32 ulp of its threshold, and every run built on it; these kernels read the float64 field as it is.
//
// The marches (compare, run statistics, spells) follow f64.hip: 16-byte double2 loads, two cells per lane, rows in
// double-buffered batches of 8.  The run state machines are those of runlen.hip / window.hip (runacc.h accumulator);
// only the element type and the compare differ.  percentile_doy gathers the window samples of a (doy, cell) block into
// LDS as order-preserving 64-bit keys and sorts them with integer compares (the key and the Hyndman-Fan arithmetic of
// xh_nan_quantile_f64, so both give bit-identical results for the same sample set).
#include <stdlib.h>

#include "common.h"
#include "f64util.h"
#include "runacc.h"

namespace {

template <int VEC>
using VD = VR<double, VEC>;

// ---- compare ------------------------------------------------------------------------------------------------------
// a op (b or thr) in float64; TA / TB are the element types of a and b (a float32 side is widened exactly, as numpy
// promotes float32 against float64).  out_kind 0: uint8 mask, 1: float32 1/0 with NaN where a is NaN, 3: float32 1/0.
template <typename TA, typename TB, bool HASB>
__global__ void __launch_bounds__(XH_BLOCK)
k_compare_map_f64(const TA* __restrict__ a, int64_t T, int64_t C, int64_t st, int op, double thr, const TB* __restrict__ b,
                  int64_t st_b, int out_kind, void* __restrict__ out_v, int64_t st_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * 2;
  if (c >= C) return;
  const int n = c + 1 < C ? 2 : 1;
  const int64_t chunk = cdiv64(T, (int64_t)gridDim.y);
  const int64_t ta = (int64_t)blockIdx.y * chunk;
  const int64_t tb = ta + chunk > T ? T : ta + chunk;
#pragma unroll 4
  for (int64_t t = ta; t < tb; ++t) {
    double av[2], bv[2];
    av[0] = (double)a[t * st + c];
    av[1] = n == 2 ? (double)a[t * st + c + 1] : 0.0;
    if (HASB) {
      bv[0] = (double)b[t * st_b + c];
      bv[1] = n == 2 ? (double)b[t * st_b + c + 1] : 0.0;
    } else {
      bv[0] = bv[1] = thr;
    }
    for (int i = 0; i < n; ++i) {
      const bool cond = xh_cmp_f64(av[i], op, bv[i]);
      if (out_kind == 0) reinterpret_cast<uint8_t*>(out_v)[t * st_out + c + i] = cond ? 1 : 0;
      else {
        float r = cond ? 1.f : 0.f;
        if (out_kind == 1 && av[i] != av[i]) r = xh_nan32();
        reinterpret_cast<float*>(out_v)[t * st_out + c + i] = r;
      }
    }
  }
}

// ---- run statistics of a float64 condition (runlen.hip k_run_stats with double rows) -------------------------------
struct RunSt {
  int run;
  bool vis, prevnan;
  int startp;
};

template <int VEC, bool CUT, int SG>
__global__ void __launch_bounds__(XH_BLOCK)
k_run_stats_f64(const double* __restrict__ x, int64_t C, int64_t st, int fused_op, double thr, int window, int stat,
                int index_first, const int64_t* __restrict__ seg_off, int P, float* __restrict__ out,
                int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const bool fused = fused_op >= 0;
  if (CUT) {
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
      const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
      RunAcc acc[VEC];
      RunSt s[VEC];
      int nvalid[VEC], plainsum[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        acc_reset(acc[i]);
        s[i].run = 0; s[i].vis = true; s[i].prevnan = false; s[i].startp = 0;
        nvalid[i] = 0; plainsum[i] = 0;
      }
      march<VEC>(x + c, st, t0, t1, [&](int64_t, const VD<VEC>& xv) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const double v = xv.v[i];
          const bool isn = v != v;
          const bool on = fused ? xh_cmp_f64(v, fused_op, thr) : (v > 0.0);
          const bool masknan = (!fused) && isn;
          nvalid[i] += isn ? 0 : 1;
          plainsum[i] += on ? 1 : 0;
          const bool visible = index_first >= 2 ? true : (index_first ? s[i].vis : !masknan);
          const bool ended = !on && s[i].run > 0;
          const int len = (ended && visible && s[i].run >= window) ? s[i].run : 0;
          acc_add_if<SG>(acc[i], len);
          s[i].vis = (on && s[i].run == 0) ? !s[i].prevnan : s[i].vis;
          s[i].run = on ? s[i].run + 1 : 0;
          s[i].prevnan = masknan;
        }
      });
      const int64_t o = (int64_t)p * C + c;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (s[i].run > 0) {
          const bool visible = index_first == 1 ? s[i].vis : true;  // beyond the segment end: shift fill_value 0
          if (visible && s[i].run >= window) acc_add(acc[i], s[i].run);
        }
        float r = acc_result(acc[i], stat, plainsum[i]);
        if (index_first == 3 && acc[i].cnt == 0 && nvalid[i] < (int)(t1 - t0) && stat != XH_RUN_COUNT && stat != XH_RUN_SUM)
          r = xh_nan32();  // statistics_run_1d: nan-reducer of no run (rl:1408-1437)
        out[o + i] = r;
        if (valid_out) valid_out[o + i] = nvalid[i];
      }
    }
  } else {
    // resample AFTER run length: a run is attributed to the period of its indexed element (runlen.hip, same flushes)
    RunAcc acc[VEC];
    RunSt s[VEC];
    int accp[VEC], nvalid[VEC], plainsum[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      acc_reset(acc[i]);
      s[i].run = 0; s[i].vis = true; s[i].prevnan = false; s[i].startp = 0;
      accp[i] = 0; nvalid[i] = 0; plainsum[i] = 0;
    }
    int pt = 0, pprev = 0;
    int64_t next_edge = seg_off[1];
    march<VEC>(x + c, st, seg_off[0], seg_off[P], [&](int64_t t, const VD<VEC>& xv) {
      while (t >= next_edge) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          if (valid_out) valid_out[(int64_t)pt * C + c + i] = nvalid[i];
          if (stat == XH_RUN_PLAINSUM) out[(int64_t)pt * C + c + i] = (float)plainsum[i];
          nvalid[i] = 0; plainsum[i] = 0;
        }
        pt++;
        next_edge = seg_off[pt + 1];
        if (stat != XH_RUN_PLAINSUM) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            if (s[i].run == 0) {
              while (accp[i] < pt) {
                out[(int64_t)accp[i] * C + c + i] = acc_result(acc[i], stat, 0);
                acc_reset(acc[i]);
                accp[i]++;
              }
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const double v = xv.v[i];
        const bool isn = v != v;
        const bool on = fused ? xh_cmp_f64(v, fused_op, thr) : (v > 0.0);
        const bool masknan = (!fused) && isn;
        nvalid[i] += isn ? 0 : 1;
        plainsum[i] += on ? 1 : 0;
        const bool visible = index_first >= 2 ? true : (index_first ? s[i].vis : !masknan);
        const bool qual = !on && visible && s[i].run >= window && stat != XH_RUN_PLAINSUM;
        const int pa = index_first ? s[i].startp : pprev;
        if (qual && accp[i] < pa) {
          do {
            out[(int64_t)accp[i] * C + c + i] = acc_result(acc[i], stat, 0);
            acc_reset(acc[i]);
            accp[i]++;
          } while (accp[i] < pa);
        }
        acc_add_if<SG>(acc[i], qual ? s[i].run : 0);
        const bool starts = on && s[i].run == 0;
        s[i].vis = starts ? !s[i].prevnan : s[i].vis;
        s[i].startp = starts ? pt : s[i].startp;
        s[i].run = on ? s[i].run + 1 : 0;
        s[i].prevnan = masknan;
      }
      pprev = pt;
    });
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if (s[i].run > 0 && stat != XH_RUN_PLAINSUM) {
        const bool visible = index_first == 1 ? s[i].vis : true;
        if (visible && s[i].run >= window) {
          const int pa = index_first ? s[i].startp : pt;
          while (accp[i] < pa) {
            out[(int64_t)accp[i] * C + c + i] = acc_result(acc[i], stat, 0);
            acc_reset(acc[i]);
            accp[i]++;
          }
          acc_add_if<SG>(acc[i], s[i].run);
        }
      }
      if (stat != XH_RUN_PLAINSUM) {
        while (accp[i] < P) {
          out[(int64_t)accp[i] * C + c + i] = acc_result(acc[i], stat, 0);
          acc_reset(acc[i]);
          accp[i]++;
        }
      }
      for (int p = pt; p < P; ++p) {
        if (valid_out) valid_out[(int64_t)p * C + c + i] = (p == pt) ? nvalid[i] : 0;
        if (stat == XH_RUN_PLAINSUM) out[(int64_t)p * C + c + i] = (p == pt) ? (float)plainsum[i] : 0.0f;
      }
    }
  }
}

// ---- spells: the window statistic in float64 (oracle/generic.py::rolling: rows t-w+1 .. t added in that order) -------
constexpr int WMAX = 8;

// window condition of the `w` newest ring slots (slot WMAX-1 = newest).  RED: XH_RED_SUM | MEAN | MIN | MAX.  A NaN in
// the window makes the statistic NaN and the condition False (as the float32 spell kernels).
template <int RED>
__device__ __forceinline__ bool ring_cond(const double (&r)[WMAX], int w, int op, double thr) {
  double s = 0.0, e = 0.0;
  bool nan = false, first = true;
#pragma unroll
  for (int k = 0; k < WMAX; ++k) {
    if (k >= WMAX - w) {
      const double v = r[k];
      nan |= v != v;
      if (RED == XH_RED_MIN) e = (first || v < e) ? v : e;
      else if (RED == XH_RED_MAX) e = (first || v > e) ? v : e;
      else s = first ? v : s + v;
      first = false;
    }
  }
  double stat;
  if (RED == XH_RED_MIN || RED == XH_RED_MAX) stat = e;
  else if (RED == XH_RED_MEAN) stat = s / (double)w;
  else stat = s;
  return !nan && xh_cmp_f64(stat, op, thr);
}

// the same over rows read from memory (windows longer than the ring)
template <int RED>
__device__ __forceinline__ bool mem_cond(const double* __restrict__ p, int64_t st, int64_t tp, int w, int op, double thr) {
  double s = 0.0, e = 0.0;
  bool nan = false;
  for (int k = 0; k < w; ++k) {
    const double v = p[(tp - w + 1 + k) * st];
    nan |= v != v;
    if (RED == XH_RED_MIN) e = (k == 0 || v < e) ? v : e;
    else if (RED == XH_RED_MAX) e = (k == 0 || v > e) ? v : e;
    else s = k == 0 ? v : s + v;
  }
  double stat;
  if (RED == XH_RED_MIN || RED == XH_RED_MAX) stat = e;
  else if (RED == XH_RED_MEAN) stat = s / (double)w;
  else stat = s;
  return !nan && xh_cmp_f64(stat, op, thr);
}

template <int VEC>
__device__ __forceinline__ void ring_push(double (&r)[VEC][WMAX], const VD<VEC>& xv) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
#pragma unroll
    for (int k = 0; k < WMAX - 1; ++k) r[i][k] = r[i][k + 1];
    r[i][WMAX - 1] = xv.v[i];
  }
}

// spell_mask (gen:519-535): out[t] = 1 iff one of the windows ending at t .. t+w-1 (complete, inside [0, T)) satisfies
// the condition.  The time axis is cut into chunks over blockIdx.y; a chunk re-reads its (w - 1)-row halo on each side.
template <int VEC, int RED, bool RING>
__global__ void __launch_bounds__(XH_BLOCK)
k_spell_mask_f64(const double* __restrict__ x, int64_t T, int64_t C, int64_t st, int w, int op, double thr,
                 float* __restrict__ out, int64_t out_st) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  const int64_t chunk = cdiv64(T, (int64_t)gridDim.y);
  const int64_t ta = (int64_t)blockIdx.y * chunk;
  const int64_t tb = ta + chunk > T ? T : ta + chunk;
  if (ta >= tb) return;
  double ring[VEC][WMAX];
#pragma unroll
  for (int i = 0; i < VEC; ++i)
#pragma unroll
    for (int k = 0; k < WMAX; ++k) ring[i][k] = xh_nan64();
  int since[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) since[i] = 1 << 20;
  auto emit = [&](int64_t tp, bool have_row) {
    const int64_t t = tp - (w - 1);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      bool cond = false;
      if (have_row && tp >= w - 1) cond = RING ? ring_cond<RED>(ring[i], w, op, thr) : mem_cond<RED>(x + c + i, st, tp, w, op, thr);
      since[i] = cond ? 0 : since[i] + 1;
      if (t >= ta) out[t * out_st + c + i] = since[i] < w ? 1.f : 0.f;
    }
  };
  // windows ending at tp in [ta, tb + w - 1) decide the outputs ta .. tb - 1; the ring needs rows from ta - (w - 1)
  const int64_t r0 = RING ? (ta - (w - 1) < 0 ? 0 : ta - (w - 1)) : ta;
  const int64_t r1 = tb + w - 1 > T ? T : tb + w - 1;
  march<VEC>(x + c, st, r0, r1, [&](int64_t tp, const VD<VEC>& xv) {
    if (RING) ring_push<VEC>(ring, xv);
    if (tp >= ta) emit(tp, true);
  });
  for (int64_t tp = r1; tp < tb + w - 1; ++tp) emit(tp, false);
}

// spell_length_statistics, window <= 8, runs cut at the period edges (window.hip k_spell_runs): the spell mask of step
// t = tp - (w - 1) feeds the run accumulator of its period directly; every period re-reads a (w - 1)-row halo.
template <int VEC, int RED, int SG>
__global__ void __launch_bounds__(XH_BLOCK)
k_spell_runs_f64(const double* __restrict__ x, int64_t T, int64_t C, int64_t st, int w, int op, double thr, int stat,
                 const int64_t* __restrict__ seg_off, int P, float* __restrict__ out, int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t ta = seg_off[p], tb = seg_off[p + 1];
    double ring[VEC][WMAX];
    RunAcc acc[VEC];
    int since[VEC], run[VEC], nvalid[VEC], days[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
#pragma unroll
      for (int k = 0; k < WMAX; ++k) ring[i][k] = xh_nan64();
      acc_reset(acc[i]);
      since[i] = 1 << 20; run[i] = 0; nvalid[i] = 0; days[i] = 0;
    }
    auto emit = [&](int64_t tp, bool have_row) {
      const int64_t t = tp - (w - 1);
      const bool inside = t >= ta && t < tb;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const bool cond = have_row && tp >= w - 1 && ring_cond<RED>(ring[i], w, op, thr);
        since[i] = cond ? 0 : since[i] + 1;
        const bool on = inside && since[i] < w;
        const int len = (inside && !on) ? run[i] : 0;  // a spell ended at t - 1
        acc_add_if<SG>(acc[i], len);
        run[i] = on ? run[i] + 1 : (inside ? 0 : run[i]);
        days[i] += on ? 1 : 0;
      }
    };
    if (ta < tb) {
      const int64_t r0 = ta - (w - 1) < 0 ? 0 : ta - (w - 1);
      const int64_t r1 = tb + w - 1 > T ? T : tb + w - 1;
      march<VEC>(x + c, st, r0, r1, [&](int64_t tp, const VD<VEC>& xv) {
        ring_push<VEC>(ring, xv);
        if (tp >= ta && tp < tb) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) nvalid[i] += xv.v[i] == xv.v[i] ? 1 : 0;
        }
        emit(tp, true);
      });
      for (int64_t tp = r1; tp < tb + w - 1; ++tp) emit(tp, false);
    }
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      acc_add_if<SG>(acc[i], run[i]);  // spell cut by the period end
      out[o + i] = acc_result(acc[i], stat, days[i]);
      if (valid_out) valid_out[o + i] = nvalid[i];
    }
  }
}

// ---- warm / cold spell duration: x[t] op table[tidx[t]], both float64 (runlen.hip k_run_stats_doy) -------------------
template <int VEC>
__global__ void __launch_bounds__(XH_BLOCK)
k_run_stats_doy_f64(const double* __restrict__ x, int64_t C, int64_t st, int op, const double* __restrict__ table,
                    const int32_t* __restrict__ tidx, int window, int stat, const int64_t* __restrict__ seg_off, int P,
                    float* __restrict__ out, int32_t* __restrict__ valid_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int64_t t0 = seg_off[p], t1 = seg_off[p + 1];
    RunAcc acc[VEC];
    int run[VEC], nvalid[VEC], plainsum[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { acc_reset(acc[i]); run[i] = 0; nvalid[i] = 0; plainsum[i] = 0; }
    auto step = [&](const VD<VEC>& xv, const VD<VEC>& tv) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const bool on = xh_cmp_f64(xv.v[i], op, tv.v[i]);
        nvalid[i] += xv.v[i] == xv.v[i] ? 1 : 0;
        plainsum[i] += on ? 1 : 0;
        const int len = (!on && run[i] >= window) ? run[i] : 0;
        acc_add_if<0>(acc[i], len);
        run[i] = on ? run[i] + 1 : 0;
      }
    };
    // rows and their table rows in batches of 8, every load of a batch issued before the first use (runlen.hip)
    int64_t t = t0;
    for (; t + 8 <= t1; t += 8) {
      int r[8];
      VD<VEC> xv[8], tv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = tidx[t + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) xv[u] = ldv<VEC>(x + (t + u) * st + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) tv[u] = ldv<VEC>(table + (int64_t)r[u] * C + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) step(xv[u], tv[u]);
    }
    for (; t < t1; ++t) step(ldv<VEC>(x + t * st + c), ldv<VEC>(table + (int64_t)tidx[t] * C + c));
    const int64_t o = (int64_t)p * C + c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if (run[i] >= window && run[i] > 0) acc_add(acc[i], run[i]);  // run cut by the period end
      out[o + i] = acc_result(acc[i], stat, plainsum[i]);
      if (valid_out) valid_out[o + i] = nvalid[i];
    }
  }
}

// ---- percentile_doy on float64 samples ----------------------------------------------------------------------------
// order-preserving 64-bit keys (f64util.h: d2key / key2d): NaN -> the largest key, sorted last and not counted
constexpr int PD_THREADS = 256;
constexpr int PD_LDS = 64 * 1024;  // bytes of keys per workgroup: L columns of NP keys

// One workgroup per (doy, L consecutive cells): the N = nyears * window samples of every cell are gathered as keys into
// column-interleaved LDS (key[i * L + col]: a row of L cells is one coalesced load), padded to NP = 2^k with NaN keys,
// bitonic-sorted per column by all threads together, then each requested percentile reads the two order statistics its
// Hyndman-Fan index needs.  Consecutive doys share (w - 1) / w of their samples; they are gathered again here (the
// re-reads hit L2), the sort is the cost.
__global__ void __launch_bounds__(PD_THREADS)
k_percentile_doy_f64(const double* __restrict__ x, int64_t T, int64_t C, int64_t st, const int32_t* __restrict__ tbase,
                     int nyears, int ndoy, int window, int N, int NP, int L, const double* __restrict__ qs, int nq,
                     double alpha, double beta, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* key = reinterpret_cast<uint64_t*>(smem);
  __shared__ int nvs[64];
  const int d = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * L;
  const int tid = threadIdx.x;
  const int half = window / 2;
  if (tid < L) nvs[tid] = 0;
  __syncthreads();
  // gather: entry e = i * L + col, sample i = y * window + k
  for (int e = tid; e < NP * L; e += PD_THREADS) {
    const int i = e / L, col = e - i * L;
    const int64_t c = c0 + col;
    uint64_t kk = ~0ull;
    if (i < N && c < C) {
      const int y = i / window, k = i - y * window;
      const int32_t tb = tbase[(int64_t)y * ndoy + d];
      const int64_t t = (int64_t)tb - half + k;
      if (tb >= 0 && t >= 0 && t < T) kk = d2key(x[t * st + c]);
    }
    key[e] = kk;
    if (kk != ~0ull) atomicAdd(&nvs[col], 1);
  }
  __syncthreads();
  // bitonic sort of every column (ascending): compare-exchange pairs (i, i ^ j) for i < (i ^ j)
  const int npairs = (NP / 2) * L;
  for (int k = 2; k <= NP; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < npairs; q += PD_THREADS) {
        const int pi = q / L, col = q - pi * L;
        // pi-th index with bit j clear
        const int i = ((pi & ~(j - 1)) << 1) | (pi & (j - 1));
        const int l = i | j;
        const bool up = (i & k) == 0;
        const uint64_t a = key[i * L + col], b = key[l * L + col];
        if ((a > b) == up) {
          key[i * L + col] = b;
          key[l * L + col] = a;
        }
      }
      __syncthreads();
    }
  }
  // Hyndman-Fan (utl:395, 486-488, 552-554) exactly as k_nan_quantile_f64
  for (int e = tid; e < nq * L; e += PD_THREADS) {
    const int jq = e / L, col = e - jq * L;
    const int64_t c = c0 + col;
    if (c >= C) continue;
    const int nv = nvs[col];
    const double q = qs[jq];
    double r;
    if (N == 1) r = key2d(key[col]);
    else if (nv < 2) r = nv == 1 ? key2d(key[col]) : xh_nan64();
    else {
      const double nn = (double)nv;
      const double vi = nn * q + (alpha + q * (1.0 - alpha - beta)) - 1.0;
      if (vi >= nn - 1.0) r = key2d(key[(nv - 1) * L + col]);
      else if (vi < 0.0) r = key2d(key[col]);
      else {
        const double prev = floor(vi);
        const int ip = (int)prev;
        const double gamma = vi - prev;
        const double left = key2d(key[ip * L + col]), right = key2d(key[(ip + 1) * L + col]);
        const double diff = right - left;
        r = left + diff * gamma;
        if (gamma >= 0.5) r = right - diff * (1.0 - gamma);
        if (r != r) r = key2d(key[(nv - 1) * L + col]);
      }
    }
    out[((int64_t)jq * ndoy + d) * C + c] = r;
  }
}

inline int stat_group(int stat) {  // runacc.h: 1 max, 2 sum / count / mean / plain sum, 0 all
  return stat == XH_RUN_MAX ? 1 : (stat == XH_RUN_SUM || stat == XH_RUN_COUNT || stat == XH_RUN_MEAN || stat == XH_RUN_PLAINSUM) ? 2 : 0;
}

}  // namespace

extern "C" {

int xh_compare_map_f64(xh_ctx* ctx, const void* a, int64_t T, int64_t C, int64_t st, int op, double thr, const void* b,
                       int64_t st_b, int dtypes, int out_kind, void* out, int64_t st_out) {
  XH_REQUIRE(ctx && a && out, XH_ERR_ARG, "xh_compare_map_f64: NULL argument");
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "xh_compare_map_f64: negative shape");
  XH_REQUIRE(st >= C && st_out >= C && (!b || st_b >= C), XH_ERR_LAYOUT, "xh_compare_map_f64: needs time-major views");
  XH_REQUIRE(op >= XH_OP_GT && op <= XH_OP_NE, XH_ERR_OP, "Operation `%d` not recognized.", op);
  XH_REQUIRE(dtypes >= 0 && dtypes <= 2, XH_ERR_ARG,
             "xh_compare_map_f64: dtypes must be 0 (a, b float64), 1 (a float32, b float64) or 2 (a float64, b float32)");
  XH_REQUIRE(dtypes == 0 || b, XH_ERR_ARG, "xh_compare_map_f64: a float32 side needs the float64 field b (else use xh_compare_map)");
  if (out_kind == 2 || out_kind == 4) {
    xh_set_error("xh_compare_map_f64: out_kind %d (float32 values of a) is not served for float64 fields", out_kind);
    return XH_ERR_NOTIMPL;
  }
  XH_REQUIRE(out_kind == 0 || out_kind == 1 || out_kind == 3, XH_ERR_ARG, "xh_compare_map_f64: out_kind must be 0, 1 or 3");
  if (T == 0 || C == 0) return XH_OK;
  const int64_t cblocks = cdiv64(cdiv64(C, 2), XH_BLOCK);
  int64_t gy = cdiv64((int64_t)ctx->num_cu * 16, cblocks);
  if (gy < 1) gy = 1;
  if (gy > T) gy = T;
  if (gy > 1024) gy = 1024;
  const dim3 grid((unsigned)cblocks, (unsigned)gy);
  if (!b)
    hipLaunchKernelGGL((k_compare_map_f64<double, double, false>), grid, dim3(XH_BLOCK), 0, ctx->stream, (const double*)a, T, C, st, op,
                       thr, (const double*)nullptr, st_b, out_kind, out, st_out);
  else if (dtypes == 0)
    hipLaunchKernelGGL((k_compare_map_f64<double, double, true>), grid, dim3(XH_BLOCK), 0, ctx->stream, (const double*)a, T, C, st, op,
                       thr, (const double*)b, st_b, out_kind, out, st_out);
  else if (dtypes == 1)
    hipLaunchKernelGGL((k_compare_map_f64<float, double, true>), grid, dim3(XH_BLOCK), 0, ctx->stream, (const float*)a, T, C, st, op,
                       thr, (const double*)b, st_b, out_kind, out, st_out);
  else
    hipLaunchKernelGGL((k_compare_map_f64<double, float, true>), grid, dim3(XH_BLOCK), 0, ctx->stream, (const double*)a, T, C, st, op,
                       thr, (const float*)b, st_b, out_kind, out, st_out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_run_stats_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int fused_op, double thr,
                     int window, int stat, int index_first, const int64_t* seg_off, int P, int cut_at_segments, float* out,
                     int32_t* valid_out) {
  int rc = xh_check_field("xh_run_stats_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(fused_op <= XH_OP_NE, XH_ERR_OP, "Operation `%d` not recognized.", fused_op);
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "xh_run_stats_f64: window must be >= 1");
  XH_REQUIRE(stat >= XH_RUN_MAX && stat <= XH_RUN_PLAINSUM, XH_ERR_OP, "xh_run_stats_f64: stat %d not recognized", stat);
  XH_REQUIRE(index_first >= 0 && index_first <= 3, XH_ERR_ARG, "xh_run_stats_f64: index mode %d not recognized", index_first);
  XH_REQUIRE(out, XH_ERR_ARG, "xh_run_stats_f64: out is NULL");
  if (stat == XH_RUN_FIRST || stat == XH_RUN_LAST) {
    xh_set_error("xh_run_stats_f64: first_run / last_run are not served for float64 fields");
    return XH_ERR_NOTIMPL;
  }
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_run_stats_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (!cut_at_segments)
    XH_REQUIRE(seg_off[0] == 0 && seg_off[P] == T, XH_ERR_ARG, "xh_run_stats_f64: resample-after mode needs segments covering [0, T)");
  if (C == 0) return XH_OK;
  // resample-after: one serial march over all periods per cell (gridDim.y = 1), one cell per lane — the grid is sized
  // with the VEC that is launched
  const int vec = cut_at_segments ? xh_pick_vec64(x, C, st) : 1;
  const int sg = stat_group(stat);
  const unsigned py = xh_period_blocks(P);
  const dim3 grid((unsigned)cdiv64(cdiv64(C, vec), XH_BLOCK), cut_at_segments ? py : 1u);
  xh_pick<2, 1>(vec, [&](auto V) {
    xh_pick<1, 2, 0>(sg, [&](auto G) {
      if (cut_at_segments)
        hipLaunchKernelGGL((k_run_stats_f64<decltype(V)::value, true, decltype(G)::value>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C,
                           st, fused_op, thr, window, stat, index_first, d_seg, P, out, valid_out);
      else if constexpr (decltype(V)::value == 1)  // resample-after: one cell per lane
        hipLaunchKernelGGL((k_run_stats_f64<1, false, decltype(G)::value>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C, st, fused_op,
                           thr, window, stat, index_first, d_seg, P, out, valid_out);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_spell_mask_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int window, int win_reducer,
                      int op, double thr, const double* weights, float* out, int64_t out_st) {
  int rc = xh_check_field("xh_spell_mask_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(out, XH_ERR_ARG, "xh_spell_mask_f64: out NULL");
  rc = xh_check_rows("xh_spell_mask_f64", out_st, C, "out_st");
  if (rc) return rc;
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "xh_spell_mask_f64: window must be >= 1");
  XH_REQUIRE(op >= XH_OP_GT && op <= XH_OP_NE, XH_ERR_OP, "Operation `%d` not recognized.", op);
  if (weights || win_reducer == 4) {
    xh_set_error("xh_spell_mask_f64: weighted windows are not served for float64 fields");
    return XH_ERR_NOTIMPL;
  }
  XH_REQUIRE(win_reducer >= 0 && win_reducer <= 3, XH_ERR_OP, "xh_spell_mask_f64: win_reducer %d not recognized", win_reducer);
  if (T == 0 || C == 0) return XH_OK;
  const bool ring = window <= WMAX;
  const int vec = ring ? xh_pick_vec64(x, C, st) : 1;  // windows longer than the ring: one cell per lane (the grid follows)
  const int64_t cblocks = cdiv64(cdiv64(C, vec), XH_BLOCK);
  int64_t gy = cdiv64((int64_t)ctx->num_cu * 8, cblocks);
  if (gy < 1) gy = 1;
  if (gy > cdiv64(T, 64)) gy = cdiv64(T, 64);  // chunks of >= 64 rows: the halo stays a small share
  if (gy > 1024) gy = 1024;
  const dim3 grid((unsigned)cblocks, (unsigned)gy);
  // win_reducer 0 sum, 1 mean, 2 min, 3 max: the values of XH_RED_SUM .. XH_RED_MAX
  xh_pick<XH_RED_SUM, XH_RED_MEAN, XH_RED_MIN, XH_RED_MAX>(win_reducer, [&](auto R) {
    xh_pick<10, 21, 11>(ring ? vec * 10 + 1 : 10, [&](auto VR) {  // (cells per lane, register ring): the instances that exist
      hipLaunchKernelGGL((k_spell_mask_f64<decltype(VR)::value / 10, decltype(R)::value, decltype(VR)::value % 10 != 0>), grid,
                         dim3(XH_BLOCK), 0, ctx->stream, x, T, C, st, window, op, thr, out, out_st);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_spell_run_stats_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int window, int win_reducer,
                           int op, double thr, const double* weights, int stat, const int64_t* seg_off, int P, float* out,
                           int32_t* valid_out) {
  int rc = xh_check_field("xh_spell_run_stats_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(out, XH_ERR_ARG, "xh_spell_run_stats_f64: out is NULL");
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "xh_spell_run_stats_f64: window must be >= 1");
  XH_REQUIRE(op >= XH_OP_GT && op <= XH_OP_NE, XH_ERR_OP, "Operation `%d` not recognized.", op);
  XH_REQUIRE(stat >= XH_RUN_MAX && stat <= XH_RUN_STD, XH_ERR_OP, "xh_spell_run_stats_f64: statistic %d not supported", stat);
  if (weights || win_reducer == 4) {
    xh_set_error("xh_spell_run_stats_f64: weighted windows are not served for float64 fields");
    return XH_ERR_NOTIMPL;
  }
  XH_REQUIRE(win_reducer >= 0 && win_reducer <= 3, XH_ERR_OP, "xh_spell_run_stats_f64: win_reducer %d not recognized", win_reducer);
  if (window > WMAX) {
    xh_set_error("xh_spell_run_stats_f64: window %d > %d (use xh_spell_mask_f64 + xh_run_stats)", window, WMAX);
    return XH_ERR_NOTIMPL;
  }
  size_t cur = 0;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_spell_run_stats_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (C == 0) return XH_OK;
  const unsigned py = xh_period_blocks(P);
  // two cells per lane (~155 VGPRs, 3 waves per SIMD) only when that still leaves >= 8 workgroups per CU; else one cell per
  // lane (~87 VGPRs, 5 waves per SIMD).  A period cannot be cut into time chunks, so the cells carry the parallelism.
  const int vec = (xh_pick_vec64(x, C, st) == 2 && cdiv64(cdiv64(C, 2), XH_BLOCK) * (int64_t)py >= 8 * (int64_t)ctx->num_cu) ? 2 : 1;
  const int sg = stat_group(stat);
  const dim3 grid((unsigned)cdiv64(cdiv64(C, vec), XH_BLOCK), py);
  xh_pick<XH_RED_SUM, XH_RED_MEAN, XH_RED_MIN, XH_RED_MAX>(win_reducer, [&](auto R) {  // (as in xh_spell_mask_f64)
    xh_pick<2, 1>(vec, [&](auto V) {
      xh_pick<1, 2, 0>(sg, [&](auto G) {
        hipLaunchKernelGGL((k_spell_runs_f64<decltype(V)::value, decltype(R)::value, decltype(G)::value>), grid, dim3(XH_BLOCK), 0,
                           ctx->stream, x, T, C, st, window, op, thr, stat, d_seg, P, out, valid_out);
      });
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_run_stats_doy_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, int op, const double* table,
                         int D, const int32_t* tidx, int window, int stat, const int64_t* seg_off, int P, float* out,
                         int32_t* valid_out) {
  int rc = xh_check_field("xh_run_stats_doy_f64", ctx, x, T, C, st, sc);
  if (rc) return rc;
  XH_REQUIRE(table && out && tidx, XH_ERR_ARG, "xh_run_stats_doy_f64: NULL argument");
  XH_REQUIRE(D >= 1, XH_ERR_ARG, "xh_run_stats_doy_f64: bad shape");
  XH_REQUIRE(op >= XH_OP_GT && op <= XH_OP_NE, XH_ERR_OP, "xh_run_stats_doy_f64: operator %d not recognized", op);
  XH_REQUIRE(window >= 1, XH_ERR_ARG, "xh_run_stats_doy_f64: window must be >= 1");
  XH_REQUIRE((stat >= XH_RUN_MAX && stat <= XH_RUN_STD) || stat == XH_RUN_PLAINSUM, XH_ERR_OP,
             "xh_run_stats_doy_f64: statistic %d not supported (run-length reducers only)", stat);
  rc = xh_check_tidx("xh_run_stats_doy_f64", tidx, T, D);
  if (rc) return rc;
  size_t cur = 0;
  const int32_t* d_tidx = nullptr;
  const int64_t* d_seg = nullptr;
  rc = xh_upload_segments("xh_run_stats_doy_f64", ctx, &cur, seg_off, P, T, &d_seg);
  if (rc) return rc;
  if (T > 0) {
    rc = xh_upload(ctx, &cur, tidx, (size_t)T, &d_tidx);
    if (rc) return rc;
  }
  if (C == 0) return XH_OK;
  const int vec = (xh_pick_vec64(x, C, st) == 2 && (reinterpret_cast<uintptr_t>(table) & 15) == 0) ? 2 : 1;
  const dim3 grid = xh_period_grid(C, vec, P);
  if (vec == 2)
    hipLaunchKernelGGL((k_run_stats_doy_f64<2>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C, st, op, table, d_tidx, window, stat,
                       d_seg, P, out, valid_out);
  else
    hipLaunchKernelGGL((k_run_stats_doy_f64<1>), grid, dim3(XH_BLOCK), 0, ctx->stream, x, C, st, op, table, d_tidx, window, stat,
                       d_seg, P, out, valid_out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_percentile_doy_f64(xh_ctx* ctx, const double* x, int64_t T, int64_t C, int64_t st, int64_t sc, const int32_t* tbase,
                          int nyears, int ndoy, int window, const double* per, int nper, double alpha, double beta,
                          double* out) {
  XH_REQUIRE(ctx && x && tbase && per && out, XH_ERR_ARG, "xh_percentile_doy_f64: NULL argument");
  XH_REQUIRE(T >= 1 && C >= 0 && nyears >= 1 && ndoy >= 1 && window >= 1 && nper >= 1, XH_ERR_ARG,
             "xh_percentile_doy_f64: bad shape");
  XH_REQUIRE(sc == 1 && st >= C, XH_ERR_LAYOUT, "xh_percentile_doy_f64: needs a time-major view (sc == 1, st >= C)");
  XH_REQUIRE(nper <= 64, XH_ERR_LIMIT, "xh_percentile_doy_f64: at most 64 percentiles per call");
  XH_REQUIRE(ndoy <= 65535, XH_ERR_LIMIT, "xh_percentile_doy_f64: at most 65535 days of the year");
  const int64_t N = (int64_t)nyears * window;
  XH_REQUIRE(N <= 4096, XH_ERR_LIMIT, "xh_percentile_doy_f64: nyears x window = %lld samples exceed 4096", (long long)N);
  for (int j = 0; j < nper; ++j)
    XH_REQUIRE(per[j] >= 0.0 && per[j] <= 100.0, XH_ERR_ARG, "xh_percentile_doy_f64: percentile %g outside [0, 100]", per[j]);
  for (int64_t i = 0; i < (int64_t)nyears * ndoy; ++i)
    XH_REQUIRE(tbase[i] >= -1 && tbase[i] < T, XH_ERR_ARG, "xh_percentile_doy_f64: tbase entry out of range");
  if (C == 0) return XH_OK;
  double qh[64];
  for (int j = 0; j < nper; ++j) qh[j] = per[j] / 100.0;  // utl:366
  size_t cur = 0;
  void *d_q = nullptr, *d_tb = nullptr;
  int rc = xh_scratch_upload(ctx, &cur, qh, sizeof(double) * nper, &d_q);
  if (rc) return rc;
  rc = xh_scratch_upload(ctx, &cur, tbase, sizeof(int32_t) * (size_t)nyears * ndoy, &d_tb);
  if (rc) return rc;
  int NP = 2;
  while (NP < N) NP <<= 1;
  int L = PD_LDS / (NP * 8);
  if (L > 64) L = 64;
  if (L < 1) L = 1;  // NP <= 4096: 32 KiB per column
  const dim3 grid((unsigned)cdiv64(C, L), (unsigned)ndoy);
  hipLaunchKernelGGL(k_percentile_doy_f64, grid, dim3(PD_THREADS), (size_t)NP * L * 8, ctx->stream, x, T, C, st,
                     (const int32_t*)d_tb, nyears, ndoy, window, (int)N, NP, L, (const double*)d_q, nper, alpha, beta, out);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

}  // extern "C"
