// grid.hip — what reduces ACROSS the grid to one value per row: the spatial sums of sea_ice_area / sea_ice_extent
// (indices/_threshold.py:3057-3131) and the box mean, the filter and the maximum of jetstream_metric_woollings
// (indices/_synoptic.py:23-116).  C ABI, the exact definition of every result and every ORDER OF SUMMATION:
// include/units/xclim_hip_grid.h.
//
// k_masked_dot: the reference writes siconc.where(siconc >= t, 0), a masked copy of the field, and reads it back in an einsum,
// once per index.  Here a workgroup of 256 lanes owns XH_GRID_CHUNK cells and XH_GRID_ROWS rows: a lane loads its eight weights
// once, then reads per row two (float32) or four (float64) non-temporal 16-byte groups, all the groups of GD_BATCH rows issued
// before the first is used, and adds its eight terms per output.  The lane sums of all rows of the tile are folded through the
// wave with shuffles and through the workgroup in LDS: one float64 partial per (row, chunk, output) in the context's work
// buffer.  k_dot_finish (one wave per (row, output)) stages the partials of a row in LDS, 512 at a time, and adds them in chunk
// order.  No atomics; the order is the header's, whatever T, the tiling or the scheduling.
//
// k_box_mean_x (one wave per (t, latitude), lanes along the longitudes) and k_box_mean_y (one lane per (t, latitude), lanes
// along the latitudes, for the layout whose latitudes have stride 1) read u in place through three index lists.
// k_filter_argmax: one wave per row, lanes along the latitudes; the W products of a lane are added in row order; the maximum
// and its first index go through the wave with shuffles.
//
// All arithmetic is float64 on the widened fields (-ffp-contract=off).
#include "../../include/units/xclim_hip_grid.h"
#include "hostargs.h"

namespace {

constexpr int GD_BLOCK = 256;
constexpr int GD_WAVE = 64;
constexpr int GD_WAVES = GD_BLOCK / GD_WAVE;
constexpr int GD_HALF = XH_GRID_CHUNK / 2;   // a lane owns 4 consecutive cells in each half of the chunk
constexpr int GD_BATCH = 4;                  // rows whose loads are issued before the first is used
constexpr int GD_NOUT = 2;
constexpr int GF_STAGE = 512;                // partials of a row staged in LDS at a time
static_assert(GD_HALF == 4 * GD_BLOCK, "a lane owns four cells of each half of the chunk");
static_assert(XH_GRID_ROWS % GD_BATCH == 0, "the rows of a tile are read in whole batches");

#if defined(__clang__)
typedef float gd_f4 __attribute__((ext_vector_type(4)));
typedef double gd_d2 __attribute__((ext_vector_type(2)));
#endif

// lane m takes its value + the value of lane m + distance, distances 32 .. 1: lane 0 holds the wave's sum
__device__ __forceinline__ double gd_wave_sum(double v) {
#pragma unroll
  for (int d = GD_WAVE / 2; d >= 1; d >>= 1) v = v + __shfl_down(v, d);
  return v;
}

// ---- xh_grid_masked_dot ----------------------------------------------------------------------------------------------
struct GdArgs {
  const void* x;
  const double* w;
  double* part;   // [out][row][chunk]
  int64_t T, C, ld, nchunk, ntile;
  double thr;
};

// the four cells from c of a row (p: the row's first element); `whole`: all four inside C
template <typename TE, bool WIDE>
__device__ __forceinline__ void gd_load4(const TE* __restrict__ p, int64_t c, int64_t C, bool whole, TE (&v)[4]) {
  if (WIDE && whole) {
#if defined(__clang__)
    if constexpr (sizeof(TE) == 4) {
      const gd_f4 t = __builtin_nontemporal_load(reinterpret_cast<const gd_f4*>(p + c));
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      const gd_d2 t0 = __builtin_nontemporal_load(reinterpret_cast<const gd_d2*>(p + c));
      const gd_d2 t1 = __builtin_nontemporal_load(reinterpret_cast<const gd_d2*>(p + c + 2));
      v[0] = t0.x, v[1] = t0.y, v[2] = t1.x, v[3] = t1.y;
    }
#else
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = p[c + i];
#endif
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = c + i < C ? p[c + i] : (TE)0;
  }
}

template <typename TE, bool WIDE, int OUTS>
__global__ void __launch_bounds__(GD_BLOCK) k_masked_dot(GdArgs a) {
  __shared__ double red[GD_WAVES][XH_GRID_ROWS][GD_NOUT];
  const int lane = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int64_t c0 = chunk * XH_GRID_CHUNK + 4 * lane;
  int64_t cs[2];
  bool whole[2];
  double w[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    cs[h] = c0 + (int64_t)h * GD_HALF;
    whole[h] = cs[h] + 4 <= a.C;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[h][i] = cs[h] + i < a.C ? a.w[cs[h] + i] : 0.0;   // a cell beyond C: 0 * 0 = +0.0
  }
  const double thr = a.thr;
  for (int64_t tile = blockIdx.y; tile < a.ntile; tile += gridDim.y) {
    const int64_t r0 = tile * XH_GRID_ROWS;
    double acc[XH_GRID_ROWS][GD_NOUT];
#pragma unroll
    for (int rb = 0; rb < XH_GRID_ROWS; rb += GD_BATCH) {
      TE v[GD_BATCH][2][4];
#pragma unroll
      for (int r = 0; r < GD_BATCH; ++r) {
        const int64_t t = r0 + rb + r;
        if (t < a.T) {
          const TE* __restrict__ p = static_cast<const TE*>(a.x) + t * a.ld;
#pragma unroll
          for (int h = 0; h < 2; ++h) gd_load4<TE, WIDE>(p, cs[h], a.C, whole[h], v[r][h]);
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[r][h][i] = (TE)0;
        }
      }
#pragma unroll
      for (int r = 0; r < GD_BATCH; ++r) {
        double sd = 0.0, sm = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double xv = (double)v[r][h][i];
            const bool in = xv >= thr;
            if (OUTS & XH_GRID_DOT) sd = sd + (in ? xv : 0.0) * w[h][i];
            if (OUTS & XH_GRID_MSUM) sm = sm + (in ? 1.0 : 0.0) * w[h][i];
          }
        acc[rb + r][0] = sd, acc[rb + r][1] = sm;
      }
    }
#pragma unroll
    for (int r = 0; r < XH_GRID_ROWS; ++r)
#pragma unroll
      for (int o = 0; o < GD_NOUT; ++o) {
        if (OUTS & (1 << o)) {
          const double s = gd_wave_sum(acc[r][o]);
          if ((lane & (GD_WAVE - 1)) == 0) red[lane / GD_WAVE][r][o] = s;
        }
      }
    __syncthreads();
    if (lane < XH_GRID_ROWS * GD_NOUT) {
      const int r = lane / GD_NOUT, o = lane % GD_NOUT;
      if ((OUTS & (1 << o)) && r0 + r < a.T) {
        double s = red[0][r][o];
#pragma unroll
        for (int wv = 1; wv < GD_WAVES; ++wv) s = s + red[wv][r][o];
        a.part[((int64_t)o * a.T + r0 + r) * a.nchunk + chunk] = s;
      }
    }
    __syncthreads();   // red is written again by the next tile
  }
}

struct GfArgs {
  const double* part;   // [out][row][chunk]
  double* out[GD_NOUT];
  int64_t T, nchunk;
};

// one wave per (row, output): the partials of the row in chunk order
__global__ void __launch_bounds__(GD_WAVE) k_dot_finish(GfArgs a) {
  __shared__ double buf[GF_STAGE];
  const int o = blockIdx.y;
  double* __restrict__ out = a.out[o];
  if (!out) return;   // (uniform over the workgroup)
  for (int64_t t = blockIdx.x; t < a.T; t += gridDim.x) {
    const double* __restrict__ p = a.part + ((int64_t)o * a.T + t) * a.nchunk;
    double s = 0.0;
    for (int64_t base = 0; base < a.nchunk; base += GF_STAGE) {
      const int n = (int)(a.nchunk - base < GF_STAGE ? a.nchunk - base : GF_STAGE);
      for (int k = threadIdx.x; k < n; k += GD_WAVE) buf[k] = p[base + k];
      __syncthreads();
      int k = 0;
      if (base == 0) s = buf[0], k = 1;   // from the first partial
      for (; k < n; ++k) s = s + buf[k];   // (every lane adds the same staged values: broadcast reads)
      __syncthreads();
    }
    if (threadIdx.x == 0) out[t] = s;
  }
}

// ---- xh_grid_box_mean ------------------------------------------------------------------------------------------------
struct BmArgs {
  const void* u;
  const int32_t *iz, *iy, *ix;
  double* zm;
  int64_t T, ld, Z, Y, X, sz, sy, sx, ld_zm;
  int nz, ny, nx;
};

// lanes along the longitudes: one wave per (t, j)
template <typename TE>
__global__ void __launch_bounds__(GD_BLOCK) k_box_mean_x(BmArgs a) {
  const int lane = threadIdx.x & (GD_WAVE - 1);
  const int j = blockIdx.x * GD_WAVES + threadIdx.x / GD_WAVE;
  if (j >= a.ny) return;   // (uniform over the wave; the kernel has no workgroup barrier)
  const int64_t y = a.iy[j];
  const bool yin = y >= 0 && y < a.Y;
  for (int64_t t = blockIdx.y; t < a.T; t += gridDim.y) {
    double s = 0.0, n = 0.0;
    if (yin) {
      for (int za = 0; za < a.nz; ++za) {
        const int64_t z = a.iz[za];
        if (z < 0 || z >= a.Z) continue;
        const int64_t o = t * a.ld + z * a.sz + y * a.sy;
        for (int b = lane; b < a.nx; b += GD_WAVE) {
          const int64_t x = a.ix[b];
          if (x < 0 || x >= a.X) continue;
          const double v = xh_ldw<TE>(a.u, o + x * a.sx);
          if (v == v) s = s + v, n = n + 1.0;
        }
      }
    }
    s = gd_wave_sum(s), n = gd_wave_sum(n);
    if (lane == 0) a.zm[t * a.ld_zm + j] = n > 0.0 ? s / n : xh_nan64();
  }
}

// lanes along the latitudes: one lane per (t, j)
template <typename TE>
__global__ void __launch_bounds__(GD_WAVE) k_box_mean_y(BmArgs a) {
  const int j = blockIdx.x * GD_WAVE + threadIdx.x;
  if (j >= a.ny) return;
  const int64_t y = a.iy[j];
  const bool yin = y >= 0 && y < a.Y;
  for (int64_t t = blockIdx.y; t < a.T; t += gridDim.y) {
    double s = 0.0, n = 0.0;
    if (yin) {
      for (int za = 0; za < a.nz; ++za) {
        const int64_t z = a.iz[za];
        if (z < 0 || z >= a.Z) continue;
        const int64_t o = t * a.ld + z * a.sz + y * a.sy;
        for (int b = 0; b < a.nx; ++b) {
          const int64_t x = a.ix[b];
          if (x < 0 || x >= a.X) continue;
          const double v = xh_ldw<TE>(a.u, o + x * a.sx);
          if (v == v) s = s + v, n = n + 1.0;
        }
      }
    }
    a.zm[t * a.ld_zm + j] = n > 0.0 ? s / n : xh_nan64();
  }
}

// ---- xh_grid_filter_argmax -------------------------------------------------------------------------------------------
struct FaArgs {
  const double *zm, *wts;
  double *f, *smax;
  int32_t* jmax;
  int64_t T, ld_zm, ld_f;
  int ny, W;
};

// one wave per row, lanes along the latitudes
__global__ void __launch_bounds__(GD_WAVE) k_filter_argmax(FaArgs a) {
  const int lane = threadIdx.x;
  const int half = a.W / 2;
  for (int64_t t = blockIdx.x; t < a.T; t += gridDim.x) {
    const int64_t t0 = t - half;
    const bool inside = t0 >= 0 && t0 + a.W <= a.T;
    double best = xh_nan64();
    int bj = -1;
    for (int j = lane; j < a.ny; j += GD_WAVE) {
      double s = xh_nan64();
      if (inside) {
        const double* __restrict__ p = a.zm + t0 * a.ld_zm + j;
        s = p[0] * a.wts[0];
        for (int k = 1; k < a.W; ++k) s = s + p[(int64_t)k * a.ld_zm] * a.wts[k];
      }
      if (a.f) a.f[t * a.ld_f + j] = s;
      if (s == s && (bj < 0 || s > best)) best = s, bj = j;   // a lane meets its j in increasing order: the first of equals stays
    }
    if (a.smax || a.jmax) {
#pragma unroll
      for (int d = GD_WAVE / 2; d >= 1; d >>= 1) {
        const double ob = __shfl_down(best, d);
        const int oj = __shfl_down(bj, d);
        if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj < bj))) best = ob, bj = oj;
      }
      if (lane == 0) {
        if (a.smax) a.smax[t] = best;
        if (a.jmax) a.jmax[t] = bj;
      }
    }
  }
}

template <typename TE, bool WIDE>
void launch_masked_dot(int outs, dim3 g, hipStream_t stream, const GdArgs& a) {
  xh_pick<1, 2, 3>(outs, [&](auto O) {
    hipLaunchKernelGGL((k_masked_dot<TE, WIDE, decltype(O)::value>), g, dim3(GD_BLOCK), 0, stream, a);
  });
}

unsigned grid_rows(int64_t n) { return (unsigned)(n < 1 ? 1 : (n > 65535 ? 65535 : n)); }

}  // namespace

int xh_grid_masked_dot(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const double* w, double thr,
                       double* dot, double* msum) {
  const char* fn = "xh_grid_masked_dot";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(T >= 0 && C >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  const int rc0 = xh_check_rows(fn, ld, C, "ld");
  if (rc0) return rc0;
  XH_REQUIRE(T * ld + C < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  XH_REQUIRE((x && w) || C == 0 || T == 0, XH_ERR_ARG, "%s: NULL argument", fn);
  const int outs = (dot ? XH_GRID_DOT : 0) | (msum ? XH_GRID_MSUM : 0);
  XH_REQUIRE(outs, XH_ERR_ARG, "%s: no output requested", fn);
  if (T == 0) return XH_OK;

  const int64_t nchunk = cdiv64(C, XH_GRID_CHUNK), ntile = cdiv64(T, XH_GRID_ROWS);
  XH_REQUIRE(nchunk <= 0x7FFFFFFF, XH_ERR_LIMIT, "%s: too many cells", fn);
  void* work = nullptr;
  if (nchunk > 0) {
    const int rc = xh_big_scratch(ctx, sizeof(double) * (size_t)GD_NOUT * (size_t)T * (size_t)nchunk, &work);
    if (rc) return rc;
    GdArgs a{};
    a.x = x, a.w = w, a.part = static_cast<double*>(work);
    a.T = T, a.C = C, a.ld = ld, a.nchunk = nchunk, a.ntile = ntile, a.thr = thr;
    const size_t esz = f64 ? 8 : 4;
    const bool wide = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (ld * (int64_t)esz) % 16 == 0;
    const dim3 g((unsigned)nchunk, grid_rows(ntile));
    if (f64) {
      if (wide) launch_masked_dot<double, true>(outs, g, ctx->stream, a);
      else launch_masked_dot<double, false>(outs, g, ctx->stream, a);
    } else {
      if (wide) launch_masked_dot<float, true>(outs, g, ctx->stream, a);
      else launch_masked_dot<float, false>(outs, g, ctx->stream, a);
    }
    XH_LAUNCH_CHECK();
  }
  GfArgs fa{};
  fa.part = static_cast<const double*>(work);
  fa.out[0] = dot, fa.out[1] = msum;
  fa.T = T, fa.nchunk = nchunk;
  hipLaunchKernelGGL(k_dot_finish, dim3((unsigned)(T > 0x7FFFFFFF ? 0x7FFFFFFF : T), GD_NOUT), dim3(GD_WAVE), 0, ctx->stream, fa);
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_grid_box_mean(xh_ctx* ctx, int64_t T, int64_t ld, int64_t Z, int64_t Y, int64_t X, int64_t sz, int64_t sy, int64_t sx, int f64,
                     const void* u, int64_t nz, const int32_t* iz, int64_t ny, const int32_t* iy, int64_t nx, const int32_t* ix,
                     double* zm, int64_t ld_zm) {
  const char* fn = "xh_grid_box_mean";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(T >= 0 && Z >= 0 && Y >= 0 && X >= 0 && nz >= 0 && ny >= 0 && nx >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(nz <= 0x7FFFFFFF && ny <= 0x7FFFFFFF && nx <= 0x7FFFFFFF, XH_ERR_LIMIT, "%s: index list too long", fn);
  XH_REQUIRE(sz >= 1 && sy >= 1 && sx >= 1 && ld >= 0, XH_ERR_LAYOUT, "%s: strides must be at least 1", fn);
  XH_REQUIRE(Z < ((int64_t)1 << 31) && Y < ((int64_t)1 << 31) && X < ((int64_t)1 << 31) && sz < ((int64_t)1 << 40) &&
                 sy < ((int64_t)1 << 40) && sx < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  if (Z > 0 && Y > 0 && X > 0)
    XH_REQUIRE((Z - 1) * sz + (Y - 1) * sy + (X - 1) * sx < ld, XH_ERR_LAYOUT, "%s: a row (Z, Y, X) does not fit the row pitch ld", fn);
  const int rc0 = xh_check_rows(fn, ld_zm, ny, "ld_zm");
  if (rc0) return rc0;
  XH_REQUIRE(T * ld < ((int64_t)1 << 40) && T * ld_zm + ny < ((int64_t)1 << 40), XH_ERR_LIMIT, "%s: field too large", fn);
  if (T == 0 || ny == 0) return XH_OK;
  XH_REQUIRE(zm && iy && (nz == 0 || iz) && (nx == 0 || ix), XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(u || nz == 0 || nx == 0 || Z == 0 || Y == 0 || X == 0, XH_ERR_ARG, "%s: NULL argument", fn);

  BmArgs a{};
  a.u = u, a.iz = iz, a.iy = iy, a.ix = ix, a.zm = zm;
  a.T = T, a.ld = ld, a.Z = Z, a.Y = Y, a.X = X, a.sz = sz, a.sy = sy, a.sx = sx, a.ld_zm = ld_zm;
  a.nz = (int)nz, a.ny = (int)ny, a.nx = (int)nx;
  if (sy == 1 && sx != 1) {
    const dim3 g((unsigned)cdiv64(ny, GD_WAVE), grid_rows(T));
    xh_by_width(f64, [&](auto wd) { hipLaunchKernelGGL(k_box_mean_y<XH_WIDTH(wd)>, g, dim3(GD_WAVE), 0, ctx->stream, a); });
  } else {
    const dim3 g((unsigned)cdiv64(ny, GD_WAVES), grid_rows(T));
    xh_by_width(f64, [&](auto wd) { hipLaunchKernelGGL(k_box_mean_x<XH_WIDTH(wd)>, g, dim3(GD_BLOCK), 0, ctx->stream, a); });
  }
  XH_LAUNCH_CHECK();
  return XH_OK;
}

int xh_grid_filter_argmax(xh_ctx* ctx, int64_t T, int64_t ny, const double* zm, int64_t ld_zm, int W, const double* wts, double* f,
                          int64_t ld_f, double* smax, int32_t* jmax) {
  const char* fn = "xh_grid_filter_argmax";
  XH_REQUIRE(ctx, XH_ERR_ARG, "%s: NULL context", fn);
  XH_REQUIRE(T >= 0 && ny >= 0, XH_ERR_ARG, "%s: negative shape", fn);
  XH_REQUIRE(ny <= 0x7FFFFFFF, XH_ERR_LIMIT, "%s: row too long", fn);
  XH_REQUIRE(W >= 1, XH_ERR_ARG, "%s: the filter must have at least 1 weight, got %d", fn, W);
  XH_REQUIRE(W <= XH_GRID_MAX_WINDOW, XH_ERR_LIMIT, "%s: filters of up to %d weights are served, got %d", fn, XH_GRID_MAX_WINDOW, W);
  XH_REQUIRE(wts, XH_ERR_ARG, "%s: NULL argument", fn);
  XH_REQUIRE(f || smax || jmax, XH_ERR_ARG, "%s: no output requested", fn);
  int rc = xh_check_rows(fn, ld_zm, ny, "ld_zm");
  if (!rc && f) rc = xh_check_rows(fn, ld_f, ny, "ld_f");
  if (rc) return rc;
  XH_REQUIRE(T * ld_zm + ny < ((int64_t)1 << 40) && (!f || T * ld_f + ny < ((int64_t)1 << 40)), XH_ERR_LIMIT, "%s: field too large", fn);
  XH_REQUIRE(zm || ny == 0 || T == 0, XH_ERR_ARG, "%s: NULL argument", fn);
  if (T == 0) return XH_OK;

  FaArgs a{};
  size_t cur = 0;
  rc = xh_upload(ctx, &cur, wts, (size_t)W, &a.wts);
  if (rc) return rc;
  a.zm = zm, a.f = f, a.smax = smax, a.jmax = jmax;
  a.T = T, a.ld_zm = ld_zm, a.ld_f = ld_f, a.ny = (int)ny, a.W = W;
  hipLaunchKernelGGL(k_filter_argmax, dim3((unsigned)(T > 0x7FFFFFFF ? 0x7FFFFFFF : T)), dim3(GD_WAVE), 0, ctx->stream, a);
  XH_LAUNCH_CHECK();
  return XH_OK;
}
