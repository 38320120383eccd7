// A HOST stand-in for <hip/hip_runtime.h> — TEST INFRASTRUCTURE ONLY (tests/test_hostsim_cpu.py): the translation units of
// xclim_amd/csrc that use neither LDS nor wave intrinsics (detrend, window, runlen, reduce, reduce2, spell, elemwise) are compiled
// unchanged with g++ against this header, and hipLaunchKernelGGL runs a kernel THREAD BY THREAD on the CPU.  That pins the
// kernels' arithmetic and the entry points' dispatch logic against the oracle without a GPU.  Nothing here is ever linked into
// libxclimhip.so; the product path has no CPU fallback.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
#define __constant__ static const
#define __noinline__ __attribute__((noinline))

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct SimIdx { unsigned x, y, z; };
extern thread_local SimIdx blockIdx, threadIdx, gridDim, blockDim;

typedef void* hipStream_t;
typedef void* hipEvent_t;
typedef int hipError_t;
enum { hipSuccess = 0 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
static inline const char* hipGetErrorString(hipError_t) { return "host simulation"; }
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
static inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
static inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
static inline hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return hipSuccess; }
static inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
static inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
template <typename F> static inline hipError_t hipFuncSetAttribute(F, int, int) { return hipSuccess; }
enum { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };

// HIP's unqualified device min / max (an overload set there; kernels call them on matching types): the templates serve the
// integer types, the float and double overloads are fminf / fmaxf / fmin / fmax as in HIP (a NaN operand gives the other one)
template <typename T> static inline T min(T a, T b) { return b < a ? b : a; }
template <typename T> static inline T max(T a, T b) { return a < b ? b : a; }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }

// normcdfinv (the inverse of the standard normal distribution function), written from the host's erfc: the Abramowitz-Stegun
// 26.2.23 start (4.5e-4) refined by Halley steps on Phi(x) - p, each of which cubes the error; solved in the lower tail, where
// erfc keeps its relative precision, and mirrored (1 - p is exact for p >= 0.5)
static inline double normcdfinv(double p) {
  if (!(p >= 0.0 && p <= 1.0)) return NAN;
  if (p == 0.0) return -INFINITY;
  if (p == 1.0) return INFINITY;
  const bool upper = p > 0.5;
  const double q = upper ? 1.0 - p : p;
  const double t = sqrt(-2.0 * log(q));
  double x = -(t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308))));
  for (int it = 0; it < 8; ++it) {
    const double pdf = 0.3989422804014326779 * exp(-0.5 * x * x);
    if (!(pdf > 0.0)) break;
    const double dx = (0.5 * erfc(-x * 0.70710678118654752440) - q) / pdf;
    const double step = dx / (1.0 + 0.5 * x * dx);
    x -= step;
    if (fabs(step) <= 1e-16 * fabs(x)) break;
  }
  return upper ? -x : x;
}

// (a macro, like the real one: kernels with default arguments are launched with fewer than they declare)
#ifdef SIM_FIBERS
#include "../simt.h"
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) sim_launch_fibers([=]() { kern(__VA_ARGS__); }, (grid), (block), (size_t)(lds))
#else
// thread by thread: atomics are plain read-modify-writes; `extern __shared__` memory (rewritten by simdevice.py to a pointer,
// for kernels whose lanes keep private columns in it) is a heap block of EXACTLY the launch's size, so that a sanitizer sees a
// lane that steps past the workgroup's allocation
template <typename T> static inline T atomicOr(T* p, T v) { const T old = *p; *p = old | v; return old; }
extern thread_local unsigned char* g_sim_dyn_lds;
static inline unsigned char* sim_dynamic_lds() { return g_sim_dyn_lds; }
template <typename F>
static inline void sim_launch_loop(F body, dim3 grid, dim3 block, size_t lds) {
  gridDim = {grid.x, grid.y, grid.z};
  blockDim = {block.x, block.y, block.z};
  unsigned char* const outer = g_sim_dyn_lds;
  g_sim_dyn_lds = lds ? (unsigned char*)malloc(lds) : nullptr;
  for (unsigned bz = 0; bz < grid.z; ++bz)
    for (unsigned by = 0; by < grid.y; ++by)
      for (unsigned bx = 0; bx < grid.x; ++bx) {
        blockIdx = {bx, by, bz};
        for (unsigned tz = 0; tz < block.z; ++tz)
          for (unsigned ty = 0; ty < block.y; ++ty)
            for (unsigned tx = 0; tx < block.x; ++tx) {
              threadIdx = {tx, ty, tz};
              body();
            }
      }
  free(g_sim_dyn_lds);
  g_sim_dyn_lds = outer;
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) sim_launch_loop([=]() { kern(__VA_ARGS__); }, (grid), (block), (size_t)(lds))
#endif

struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
static inline uint2 make_uint2(unsigned a, unsigned b) { return uint2{a, b}; }
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct double2 { double x, y; };
struct uchar4 { unsigned char x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
static inline float2 make_float2(float a, float b) { return float2{a, b}; }
static inline double2 make_double2(double a, double b) { return double2{a, b}; }
static inline uchar4 make_uchar4(unsigned char a, unsigned char b, unsigned char c, unsigned char d) { return uchar4{a, b, c, d}; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
static inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
static inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
#define __builtin_readcyclecounter() 0ull

// pdoy.h speaks to the wave (readlane, buffer loads): every unit that includes it is built on fibers (simt.h: real exchanges, the
// buffer loads are plain loads); thread by thread these stand-ins only let a header parse and abort if anything reaches them.
typedef struct { const void* p; } __amdgpu_buffer_rsrc_t;
#ifndef SIM_FIBERS
static inline int __builtin_amdgcn_readfirstlane(int) { abort(); }
static inline int __builtin_amdgcn_readlane(int, int) { abort(); }
static inline __amdgpu_buffer_rsrc_t __builtin_amdgcn_make_buffer_rsrc(void*, short, int, int) { abort(); }
static inline unsigned __builtin_amdgcn_raw_buffer_load_b32(__amdgpu_buffer_rsrc_t, int, int, int) { abort(); }
#else
static inline __amdgpu_buffer_rsrc_t __builtin_amdgcn_make_buffer_rsrc(void* p, short, int, int) { return __amdgpu_buffer_rsrc_t{p}; }
static inline unsigned __builtin_amdgcn_raw_buffer_load_b32(__amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  unsigned v;
  memcpy(&v, (const char*)r.p + (unsigned)voff + (unsigned)soff, 4);
  return v;
}
static inline void __builtin_amdgcn_raw_buffer_store_b32(unsigned v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  memcpy((char*)const_cast<void*>(r.p) + (unsigned)voff + (unsigned)soff, &v, 4);
}
#endif

// plane.hip: the work list is filled by wave-aggregated appends (ballot + one atomic per wave + shuffle).  One thread at a time IS a
// wave whose only active lane is that thread: the stand-ins below (selected per unit by -D in tests/hostsim/simdevice.py) make the
// same code append one entry per call; lane-private LDS columns become static arrays.
static inline unsigned sim_atomic_add(unsigned* p, unsigned v) { const unsigned old = *p; *p = old + v; return old; }
