// mix_ubench.hip — store and load SHAPES for the tx90p chain at its exact size (365 x 1440 x 720):
//   mix  : read 4 B fp32, write 8 B fp64 per cell (k_pdoy_slide: 1.52 GB read + 3.03 GB written)
//   rd   : read 4 B fp32 + 8 B fp64 per cell (k_threshold_count against the per-doy fp64 table: 4.54 GB read)
// Cell-to-lane maps of a wave's 256-cell segment:
//   split (L = 0): lane l owns cells 4l .. 4l+3 — one float4 load, two double2 accesses at a 32-byte lane stride
//                  (each wave instruction touches every other 16-byte piece of a 2 KiB span)
//   pair  (L = 1): lane l owns cells {2l, 2l+1} and {128+2l, 129+2l} — two float2 loads (512 B contiguous each) and two
//                  double2 accesses of 1 KiB contiguous each
// Store flavours: 0 plain, 1 nt, 2 sc1.  Forms: streaming (grid-stride over segments) and time march (a lane walks the
// rows of a doy chunk, R rows in flight, gy chunks on blockIdx.y as k_pdoy_slide).
// Build: hipcc --offload-arch=gfx950 -O3 mix_ubench.hip -o mix_ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef double d2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

template <int ST>
__device__ __forceinline__ void st16(double* p, double a, double b) {
  d2v v = {a, b};
  if (ST == 0) {
    *reinterpret_cast<d2v*>(p) = v;
  } else if (ST == 1) {
    __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(p));
  } else {
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  }
}

// the 4 cells of a lane at row base `p` (cells of the wave segment `seg`)
template <int L>
__device__ __forceinline__ void cells(int64_t seg, int lane, int64_t (&c)[2]) {
  if (L == 0) { c[0] = seg + 4 * lane; c[1] = c[0] + 2; }
  else { c[0] = seg + 2 * lane; c[1] = c[0] + 128; }
}
template <int L>
__device__ __forceinline__ f4v ld4(const float* __restrict__ x, const int64_t (&c)[2]) {
  if (L == 0) return *reinterpret_cast<const f4v*>(x + c[0]);
  const f2v a = *reinterpret_cast<const f2v*>(x + c[0]);
  const f2v b = *reinterpret_cast<const f2v*>(x + c[1]);
  return f4v{a.x, a.y, b.x, b.y};
}
template <int L, int ST>
__device__ __forceinline__ void st4(double* __restrict__ o, const int64_t (&c)[2], f4v v) {
  st16<ST>(o + c[0], (double)v.x, (double)v.y);
  st16<ST>(o + c[1], (double)v.z, (double)v.w);
}

// streaming: one 256-cell wave segment per grid-stride step
template <int L, int ST>
__global__ void __launch_bounds__(256) k_mix_stream(const float* __restrict__ x, double* __restrict__ o, int64_t nseg) {
  const int lane = threadIdx.x & 63;
  for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += (int64_t)gridDim.x * 4) {
    int64_t c[2];
    cells<L>(s * 256, lane, c);
    st4<L, ST>(o, c, ld4<L>(x, c));
  }
}

// time march: rows [d0, d1) of the chunk, R rows loaded ahead of use
template <int L, int ST, int R>
__global__ void __launch_bounds__(256) k_mix_march(const float* __restrict__ x, double* __restrict__ o, int64_t T, int64_t C,
                                                   int chunk) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256;
  if (seg >= C) return;
  int64_t c[2];
  cells<L>(seg, lane, c);
  int64_t d0 = (int64_t)blockIdx.y * chunk, d1 = d0 + chunk;
  if (d1 > T) d1 = T;
  f4v ring[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t t = d0 + r < T ? d0 + r : T - 1;
    ring[r] = ld4<L>(x + t * C, c);
  }
  for (int64_t d = d0; d < d1; d += R) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (d + r < d1) {
        const f4v v = ring[r];
        const int64_t t = d + r + R < T ? d + r + R : T - 1;  // clamped
        ring[r] = ld4<L>(x + t * C, c);
        int64_t oc[2] = {c[0] + (d + r) * C, c[1] + (d + r) * C};
        st4<L, ST>(o, oc, v);
      }
    }
  }
}

// read-only mix: fp32 row + fp64 table row, compare and count (k_threshold_count stand-in), R rows per batch
template <int L, int R>
__global__ void __launch_bounds__(256) k_rd_march(const float* __restrict__ x, const double* __restrict__ tab, int64_t T,
                                                  int64_t C, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t seg = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256;
  if (seg >= C) return;
  int64_t c[2];
  cells<L>(seg, lane, c);
  int n[4] = {0, 0, 0, 0};
  int64_t t = 0;
  for (; t + R <= T; t += R) {
    f4v v[R];
    d2v a[R], b[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = ld4<L>(x + (t + r) * C, c);
      a[r] = *reinterpret_cast<const d2v*>(tab + (t + r) * C + c[0]);
      b[r] = *reinterpret_cast<const d2v*>(tab + (t + r) * C + c[1]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      n[0] += (double)v[r].x > a[r].x; n[1] += (double)v[r].y > a[r].y;
      n[2] += (double)v[r].z > b[r].x; n[3] += (double)v[r].w > b[r].y;
    }
  }
  for (; t < T; ++t) {
    const f4v v = ld4<L>(x + t * C, c);
    const d2v a = *reinterpret_cast<const d2v*>(tab + t * C + c[0]);
    const d2v b = *reinterpret_cast<const d2v*>(tab + t * C + c[1]);
    n[0] += (double)v.x > a.x; n[1] += (double)v.y > a.y; n[2] += (double)v.z > b.x; n[3] += (double)v.w > b.y;
  }
  cnt[c[0]] = n[0]; cnt[c[0] + 1] = n[1]; cnt[c[1]] = n[2]; cnt[c[1] + 1] = n[3];
}

template <typename F>
float timeit(F f, int reps) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  for (int i = 0; i < 3; ++i) f();
  hipDeviceSynchronize();
  hipEventRecord(a);
  for (int i = 0; i < reps; ++i) f();
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms;
  hipEventElapsedTime(&ms, a, b);
  return ms / reps;
}

static const char* LN[2] = {"split", "pair "};
static const char* SN[3] = {"plain", "nt   ", "sc1  "};

int main() {
  const int64_t T = 365, C = 1440 * 720;  // C % 256 == 0: every wave segment is whole
  const size_t E = (size_t)T * C;
  float* x; double* o; int* cnt;
  CK(hipMalloc(&x, E * 4)); CK(hipMalloc(&o, E * 8)); CK(hipMalloc(&cnt, C * 4));
  CK(hipMemset(x, 0, E * 4)); CK(hipMemset(o, 0, E * 8));
  const double mixB = E * 12.0, rdB = E * 12.0;
  const int reps = 20;
  const int64_t nseg = (int64_t)E / 256;
  printf("# T=%lld C=%lld  mix = %.3f GB read + %.3f GB written, rd = %.3f GB read\n", (long long)T, (long long)C, E * 4e-9,
         E * 8e-9, E * 12e-9);
#define STREAM(LL, SS)                                                                                         \
  {                                                                                                            \
    for (int blocks : {2048, 8192, 32768}) {                                                                   \
      float ms = timeit([&] { hipLaunchKernelGGL((k_mix_stream<LL, SS>), dim3(blocks), dim3(256), 0, 0, x, o, nseg); }, reps); \
      printf("mix stream %s %s blocks=%6d  %.4f ms  %.0f GB/s\n", LN[LL], SN[SS], blocks, ms, mixB / ms / 1e6);  \
    }                                                                                                          \
  }
  STREAM(0, 0) STREAM(1, 0) STREAM(1, 1) STREAM(1, 2)
#undef STREAM
  const unsigned bx = (unsigned)((C / 256 + 3) / 4);  // one wave per 256-cell segment, 4 waves per block
#define MARCH(LL, SS, RR)                                                                                          \
  {                                                                                                                \
    for (int chunk : {32, 92, 365}) {                                                                              \
      dim3 g(bx, (unsigned)((T + chunk - 1) / chunk));                                                             \
      float ms = timeit([&] { hipLaunchKernelGGL((k_mix_march<LL, SS, RR>), g, dim3(256), 0, 0, x, o, T, C, chunk); }, reps); \
      printf("mix march  %s %s R=%d chunk=%3d gy=%2u  %.4f ms  %.0f GB/s\n", LN[LL], SN[SS], RR, chunk, g.y, ms, mixB / ms / 1e6); \
    }                                                                                                              \
  }
  MARCH(0, 0, 1) MARCH(0, 0, 2) MARCH(0, 0, 4)
  MARCH(1, 0, 1) MARCH(1, 0, 2) MARCH(1, 0, 4)
  MARCH(1, 1, 1) MARCH(1, 1, 2) MARCH(1, 1, 4)
  MARCH(1, 2, 1) MARCH(1, 2, 2) MARCH(1, 2, 4)
#undef MARCH
#define RD(LL, RR)                                                                                             \
  {                                                                                                            \
    float ms = timeit([&] { hipLaunchKernelGGL((k_rd_march<LL, RR>), dim3(bx), dim3(256), 0, 0, x, o, T, C, cnt); }, reps); \
    printf("rd  march  %s R=%d  %.4f ms  %.0f GB/s\n", LN[LL], RR, ms, rdB / ms / 1e6);                          \
  }
  RD(0, 4) RD(0, 8) RD(1, 4) RD(1, 8)
#undef RD
  CK(hipDeviceSynchronize());
  return 0;
}
