// doystats.hip — climatological_mean_doy (core/calendar.py:907-931) from per-day-set partial sums.
//
// The sample set of doy d is the union of the W day-sets {(year y, doy d + k)} (same decomposition as the multi-year
// percentile kernels, pdoy.h).  One lane per cell marches over a chunk of doys: every day-set is gathered ONCE (rows
// resolved with one vector load + readlane, unconditional loads) and reduced, in two passes over its registers, to
// (count, mean, M2 = sum of squares about ITS OWN mean), kept in a ring of W partials.  Every doy combines the W partials
// of its window afresh with the pairwise-variance formula, in fp64:
//     N = sum n_i,   mean = sum n_i mean_i / N,   M2 = sum (M2_i + n_i (mean_i - mean)^2),   var = M2 / N.
// There is no shift by a pivot sample and no running window sum: a partial reaches exactly the W doys whose window holds
// its day-set, so one huge sample (an unmasked fill value) changes those doys and no other, and the variance is a sum of
// non-negative terms whatever the magnitude of the field (relative error of a few 2^-53 of M2).
// The generic kernel (reduce2.hip) re-reads every row W times and twice for its two-pass std; it remains the exact path
// for irregular doys (calendar gaps).
#include <stdlib.h>

#include "hostargs.h"
#include "pdoy.h"

namespace {

template <int W, int NYP>
__global__ void __launch_bounds__(64)
k_doy_stats_sets(const float* __restrict__ x, int64_t T, int64_t C, int64_t st, const int32_t* __restrict__ tbase, int nyears,
                 int ndoy, int chunk, const uint8_t* __restrict__ regular, float* __restrict__ mean_out,
                 float* __restrict__ std_out) {
  const int lane = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool active = c < C;
  const int64_t cc = active ? c : C - 1;
  constexpr int half = W / 2;
  int d0 = blockIdx.y * chunk, d1 = d0 + chunk;
  if (d1 > ndoy) d1 = ndoy;
  double mu[W], m2[W];
  int n[W];
#pragma unroll
  for (int w = 0; w < W; ++w) { mu[w] = 0.0; m2[w] = 0.0; n[w] = 0; }
  float raw[NYP];
  const double inv_ny = 1.0 / (double)nyears;
  auto rows_of = [&](int dn) { return pdoy_row(lane, nyears, ndoy, dn, 0, tbase, nullptr, T, T); };
  // the day-set in raw[] -> (count, mean, M2 about that mean); an empty day-set is (0, 0, 0).  1 / n is a wave-uniform
  // constant when every lane's day-set is complete (the usual case; the same quotient either way)
  auto reduce_into = [&](double& amu, double& am2, int& an) {
    double b1 = 0.0;
    int bn = 0;
#pragma unroll
    for (int y = 0; y < NYP; ++y) {
      const float v = raw[y];
      const bool ok = v == v;
      b1 += ok ? (double)v : 0.0;
      bn += ok ? 1 : 0;
    }
    const bool allfull = __all(bn == nyears ? 1 : 0) != 0;
    const double m = b1 * (allfull ? inv_ny : 1.0 / (double)(bn > 0 ? bn : 1));
    double b2 = 0.0;
#pragma unroll
    for (int y = 0; y < NYP; ++y) {
      const float v = raw[y];
      const double dv = (v == v) ? (double)v - m : 0.0;
      b2 += dv * dv;
    }
    amu = m; am2 = b2; an = bn;
  };
  // ring[w] = day-set of doy (d - half + w); prologue fills slots 1 .. W-1 for d = d0 - 1
#pragma unroll
  for (int w = 1; w < W; ++w) {
    pdoy_gather<NYP>(raw, rows_of(d0 - 1 - half + w), x, st, cc);
    reduce_into(mu[w], m2[w], n[w]);
  }
  pdoy_gather<NYP>(raw, rows_of(d0 + half), x, st, cc);
  int rows_next = rows_of(d0 + half + 1);
  // The ring does not shift: the day loop is unrolled by W and the partial of the day-set that enters at step u of a group
  // lands in the static slot (u + W - 1) % W — the slot of the day-set that leaves (20 64-bit moves per doy before).
  // 1 / N is a wave-uniform constant when every lane's window is complete (the usual case), the standard deviation comes
  // from the hardware fp32 square root.
#pragma unroll
  for (int w = 0; w < W - 1; ++w) { mu[w] = mu[w + 1]; m2[w] = m2[w + 1]; n[w] = n[w + 1]; }  // prologue slots 1..W-1 -> 0..W-2
  mu[W - 1] = 0.0; m2[W - 1] = 0.0; n[W - 1] = 0;
  const int nfull = W * nyears;
  const double inv_full = 1.0 / (double)nfull;
  for (int db = d0; db < d1; db += W) {
#pragma unroll
    for (int u = 0; u < W; ++u) {
      const int d = db + u;
      if (d < d1) {
        const int SLOT = (u + W - 1) % W;  // (compile-time after unrolling)
        reduce_into(mu[SLOT], m2[SLOT], n[SLOT]);
        if (d + 1 < d1) {
          pdoy_gather<NYP>(raw, rows_next, x, st, cc);
          rows_next = rows_of(d + 2 + half);
        }
        if (regular[d]) {
          int N = 0;
          double S = 0.0;
#pragma unroll
          for (int w = 0; w < W; ++w) { N += n[w]; S += (double)n[w] * mu[w]; }
          const bool allfull = __all(N == nfull ? 1 : 0) != 0;
          float m = xh_nan32(), sd = xh_nan32();
          if (allfull || N > 0) {
            const double invN = allfull ? inv_full : 1.0 / (double)(N > 0 ? N : 1);
            const double mean = S * invN;
            double M2 = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
              const double dm = mu[w] - mean;
              M2 += m2[w] + (double)n[w] * (dm * dm);
            }
            m = (float)mean;
            sd = __builtin_amdgcn_sqrtf((float)(M2 * invN));
          }
          if (active) {
            mean_out[(int64_t)d * C + c] = m;
            std_out[(int64_t)d * C + c] = sd;
          }
        }
      }
    }
  }
}

// ONE contiguous year (row of doy index i = t0 + i): the day-sets are single rows, the climatology is a centred,
// NaN-skipping rolling mean / std over consecutive rows.  Four cells per lane, rows in double-buffered batches of 8
// (xh_march_rows), the window in a register ring with static slots; mean and population std (two passes over the W
// values in fp64) per doy.  The per-day-set kernel above moves 256 bytes per wave and row.
template <int W, int VEC>
__global__ void __launch_bounds__(XH_BLOCK)
k_doy_stats_year(const float* __restrict__ x, int64_t T, int64_t C, int64_t st, int64_t t0, int ndoy, int chunk,
                 const uint8_t* __restrict__ regular, float* __restrict__ mean_out, float* __restrict__ std_out) {
  const int64_t c = ((int64_t)blockIdx.x * XH_BLOCK + threadIdx.x) * VEC;
  if (c >= C) return;
  constexpr int half = W / 2;
  const int d0 = blockIdx.y * chunk;
  int d1 = d0 + chunk;
  if (d1 > ndoy) d1 = ndoy;
  if (d0 >= d1) return;
  float ring[VEC][W];
#pragma unroll
  for (int i = 0; i < VEC; ++i)
#pragma unroll
    for (int k = 0; k < W; ++k) ring[i][k] = xh_nan32();
  // rows t0 + d0 - half .. t0 + d1 - 1 + half; rows outside the series are absent days (NaN)
  const int64_t ta = t0 + d0 - half, tb = t0 + d1 - 1 + half + 1;
  const int64_t ra = ta < 0 ? 0 : ta, rb = tb > T ? T : tb;
  auto emit = [&](int64_t tnew) {  // tnew: the row that just entered = the newest of the window of doy d
    const int64_t d = tnew - half - t0;
    if (d < d0 || d >= d1 || !regular[d]) return;
    float m[VEC], sd[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      double sum = 0.0;
      int n = 0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float v = ring[i][k];
        const bool ok = v == v;
        sum += ok ? (double)v : 0.0;
        n += ok ? 1 : 0;
      }
      const double inv = 1.0 / (double)(n > 0 ? n : 1);
      const double mean = sum * inv;
      double s2 = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float v = ring[i][k];
        const double dv = (v == v) ? (double)v - mean : 0.0;
        s2 += dv * dv;
      }
      m[i] = n > 0 ? (float)mean : xh_nan32();
      sd[i] = n > 0 ? __builtin_amdgcn_sqrtf((float)(s2 * inv)) : xh_nan32();
    }
    float* mo = mean_out + d * C + c;
    float* so = std_out + d * C + c;
    if (VEC == 4) {
      *reinterpret_cast<float4*>(mo) = make_float4(m[0], m[1 % VEC], m[2 % VEC], m[3 % VEC]);
      *reinterpret_cast<float4*>(so) = make_float4(sd[0], sd[1 % VEC], sd[2 % VEC], sd[3 % VEC]);
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) { mo[i] = m[i]; so[i] = sd[i]; }
    }
  };
  auto push = [&](const VecF<VEC>& xv) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
#pragma unroll
      for (int k = 0; k < W - 1; ++k) ring[i][k] = ring[i][k + 1];
      ring[i][W - 1] = xv.v[i];
    }
  };
  VecF<VEC> nanv;
#pragma unroll
  for (int i = 0; i < VEC; ++i) nanv.v[i] = xh_nan32();
  for (int64_t t = ta; t < ra; ++t) { push(nanv); emit(t); }  // absent rows before the series
  xh_march_rows<VEC, 8>(x + c, st, ra, rb, [&](int64_t t, const VecF<VEC>& xv) {
    push(xv);
    emit(t);
  });
  for (int64_t t = (rb > ra ? rb : ra); t < tb; ++t) { push(nanv); emit(t); }  // absent rows after it
}

}  // namespace

int xh_launch_doy_stats_sets(xh_ctx* ctx, const float* x, int64_t T, int64_t C, int64_t st, const int32_t* d_tb, int nyears,
                             int ndoy, int window, const uint8_t* d_reg, float* mean_out, float* std_out, int64_t year_t0) {
  if (!(window == 3 || window == 5 || window == 7) || nyears > 64) return XH_ERR_NOTIMPL;
  if (nyears == 1 && year_t0 >= 0) {  // one contiguous year: rolling form
    const int vec = (xh_pick_vec(x, C, st) == 4 && xh_pick_vec(mean_out, C, C) == 4 && xh_pick_vec(std_out, C, C) == 4) ? 4 : 1;
    const int64_t cblocks = cdiv64(cdiv64(C, vec), XH_BLOCK);
    int64_t gy = cdiv64((int64_t)ctx->num_cu * 12, cblocks);
    if (gy < 1) gy = 1;
    if (gy > cdiv64(ndoy, 32)) gy = cdiv64(ndoy, 32);
    if (gy < 1) gy = 1;
    const int ychunk = (int)cdiv64(ndoy, gy);
    const dim3 ygrid((unsigned)cblocks, (unsigned)cdiv64(ndoy, ychunk));
    xh_pick<3, 5, 7>(window, [&](auto W) {
      xh_pick<4, 1>(vec, [&](auto V) {
        hipLaunchKernelGGL((k_doy_stats_year<decltype(W)::value, decltype(V)::value>), ygrid, dim3(XH_BLOCK), 0, ctx->stream, x, T, C,
                           st, year_t0, ndoy, ychunk, d_reg, mean_out, std_out);
      });
    });
    XH_LAUNCH_CHECK();
    return XH_OK;
  }
  int chunk = 24;
  if (const char* e = xh_diag_env("XH_DOYSTATS_CHUNK")) chunk = atoi(e) > 0 ? atoi(e) : chunk;  // diagnostics
  const dim3 grid((unsigned)cdiv64(C, 64), (unsigned)((ndoy + chunk - 1) / chunk));
  // samples per day-set the kernel is compiled for (1: no padded second slot to gather and mask)
  const int ny = nyears == 1 ? 1 : nyears <= 2 ? 2 : nyears <= 8 ? 8 : nyears <= 32 ? 32 : 64;
  xh_pick<3, 5, 7>(window, [&](auto W) {
    xh_pick<1, 2, 8, 32, 64>(ny, [&](auto NY) {
      hipLaunchKernelGGL((k_doy_stats_sets<decltype(W)::value, decltype(NY)::value>), grid, dim3(64), 0, ctx->stream, x, T, C, st, d_tb,
                         nyears, ndoy, chunk, d_reg, mean_out, std_out);
    });
  });
  XH_LAUNCH_CHECK();
  return XH_OK;
}
