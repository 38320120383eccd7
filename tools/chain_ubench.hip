// chain_ubench.hip — can the tx90p chain hand its (365, C) fp64 table over on the die?  Stand-ins at the exact size
// (365 x 1440 x 720) in the shapes of tools/mix_ubench.hip:
//   prod : read 4 B fp32, write 8 B fp64 per cell (k_pdoy_slide: pair map, time march over doy chunks on blockIdx.y)
//   cons : read 4 B fp32 + 8 B fp64 per cell, compare and count (k_tcount_year: split map, 4 rows per batch)
// on a cell axis cut into N chunks (bounds multiples of 1024 cells), in three schedules:
//   (a) whole producer, whole consumer, one stream — the chain as it is today
//   (b) producer chunk k, consumer chunk k, ... interleaved on one stream
//   (c) producer chunks on stream 1 with an event each, consumer chunk k on stream 2 behind event k, stream 1 joined
//       to stream 2 at the end of the step (the next step's producer overwrites the table)
// Swept: N, the producer's doy chunk, the consumer's row split S (partial counts added with integer atomics into a
// zeroed output when S > 1), plain against non-temporal consumer loads, plain against non-temporal producer stores.
// (a) is repeated through the run: its spread is what a gain of (b) or (c) has to clear.
// Every schedule is checked once per configuration against the known count (a stale table gives another count).
// Build: hipcc --offload-arch=gfx950 -O3 chain_ubench.hip -o chain_ubench        Run: ./chain_ubench [quick]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef double d2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

static const int MAXN = 128;

// the table the producer writes: below the sample on even rows, above it on odd rows -> count = ceil(T / 2) per cell
__device__ __forceinline__ double thr_of(float v, int64_t t) { return (double)v + ((t & 1) ? 0.5 : -0.5); }

__global__ void __launch_bounds__(256) k_fill(float* __restrict__ x, int64_t T, int64_t C) {
  const int64_t n = T * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    x[i] = (float)(1 + (i / C * 7 + i % C) % 13);
}

template <int ST>
__device__ __forceinline__ void st16(double* p, double a, double b) {
  d2v v = {a, b};
  if (ST == 0) *reinterpret_cast<d2v*>(p) = v;
  else __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(p));
}

// producer: cells [c0, c1) (multiples of 256), rows [d0, d1) of the doy chunk blockIdx.y, R = 2 rows loaded ahead;
// pair map: lane l owns cells {2l, 2l+1} and {128+2l, 129+2l} of its wave's 256-cell segment
template <int ST>
__global__ void __launch_bounds__(256) k_prod(const float* __restrict__ x, double* __restrict__ o, int64_t T, int64_t C,
                                              int64_t c0, int64_t c1, int chunk) {
  constexpr int R = 2;
  const int lane = threadIdx.x & 63;
  const int64_t seg = c0 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256;
  if (seg + 256 > c1) return;
  const int64_t ca = seg + 2 * lane, cb = ca + 128;
  int64_t d0 = (int64_t)blockIdx.y * chunk, d1 = d0 + chunk;
  if (d1 > T) d1 = T;
  f2v ra[R], rb[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t t = d0 + r < T ? d0 + r : T - 1;
    ra[r] = *reinterpret_cast<const f2v*>(x + t * C + ca);
    rb[r] = *reinterpret_cast<const f2v*>(x + t * C + cb);
  }
  for (int64_t d = d0; d < d1; d += R) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (d + r < d1) {
        const f2v a = ra[r], b = rb[r];
        const int64_t t = d + r + R < T ? d + r + R : T - 1;  // clamped
        ra[r] = *reinterpret_cast<const f2v*>(x + t * C + ca);
        rb[r] = *reinterpret_cast<const f2v*>(x + t * C + cb);
        st16<ST>(o + (d + r) * C + ca, thr_of(a.x, d + r), thr_of(a.y, d + r));
        st16<ST>(o + (d + r) * C + cb, thr_of(b.x, d + r), thr_of(b.y, d + r));
      }
    }
  }
}

template <int NT>
__device__ __forceinline__ f4v ldf(const float* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
  return *reinterpret_cast<const f4v*>(p);
}
template <int NT>
__device__ __forceinline__ d2v ldd(const double* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
  return *reinterpret_cast<const d2v*>(p);
}

// consumer: cells [c0, c1), rows [t0, t1) of the row slice blockIdx.y (rows_per rows each), R = 4 rows per batch;
// split map: lane l owns cells 4l .. 4l+3.  ATOMIC: partial counts are added into a zeroed cnt.
template <int NT, bool ATOMIC>
__global__ void __launch_bounds__(256) k_cons(const float* __restrict__ x, const double* __restrict__ tab, int64_t T, int64_t C,
                                              int64_t c0, int64_t c1, int rows_per, int* __restrict__ cnt) {
  constexpr int R = 4;
  const int lane = threadIdx.x & 63;
  const int64_t seg = c0 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 256;
  if (seg + 256 > c1) return;
  const int64_t c = seg + 4 * lane;
  int64_t t = (int64_t)blockIdx.y * rows_per, t1 = t + rows_per;
  if (t1 > T) t1 = T;
  int n[4] = {0, 0, 0, 0};
  for (; t + R <= t1; t += R) {
    f4v v[R];
    d2v a[R], b[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = ldf<NT>(x + (t + r) * C + c);
      a[r] = ldd<NT>(tab + (t + r) * C + c);
      b[r] = ldd<NT>(tab + (t + r) * C + c + 2);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      n[0] += (double)v[r].x > a[r].x; n[1] += (double)v[r].y > a[r].y;
      n[2] += (double)v[r].z > b[r].x; n[3] += (double)v[r].w > b[r].y;
    }
  }
  for (; t < t1; ++t) {
    const f4v v = ldf<NT>(x + t * C + c);
    const d2v a = ldd<NT>(tab + t * C + c), b = ldd<NT>(tab + t * C + c + 2);
    n[0] += (double)v.x > a.x; n[1] += (double)v.y > a.y; n[2] += (double)v.z > b.x; n[3] += (double)v.w > b.y;
  }
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(cnt + c + k, n[k]);
  } else {
    cnt[c] = n[0]; cnt[c + 1] = n[1]; cnt[c + 2] = n[2]; cnt[c + 3] = n[3];
  }
}

// the chunk planner: [0, C) cut into at most n chunks whose bounds are multiples of `align` cells (the last one ends
// at C); returns the number of chunks, bounds in b[0 .. count]
static int plan_chunks(int64_t C, int n, int64_t align, int64_t* b) {
  if (n < 1) n = 1;
  int64_t per = ((C + n - 1) / n + align - 1) / align * align;
  int k = 0;
  b[0] = 0;
  while (b[k] < C) { b[k + 1] = b[k] + per < C ? b[k] + per : C; ++k; }
  return k;
}

struct Cfg {
  int sched;  // 0 = (a), 1 = (b), 2 = (c)
  int N, dchunk, S, nt, st;
};

struct Bench {
  int64_t T, C;
  float* x; double* o; int* cnt;
  hipStream_t s1, s2;
  hipEvent_t ev[MAXN], join;

  void prod(const Cfg& g, int64_t c0, int64_t c1) {
    dim3 grid((unsigned)((c1 - c0 + 1023) / 1024), (unsigned)((T + g.dchunk - 1) / g.dchunk));
    if (g.st) hipLaunchKernelGGL((k_prod<1>), grid, dim3(256), 0, s1, x, o, T, C, c0, c1, g.dchunk);
    else hipLaunchKernelGGL((k_prod<0>), grid, dim3(256), 0, s1, x, o, T, C, c0, c1, g.dchunk);
  }
  void cons(const Cfg& g, hipStream_t s, int64_t c0, int64_t c1) {
    const int rows_per = (int)((T + g.S - 1) / g.S);
    dim3 grid((unsigned)((c1 - c0 + 1023) / 1024), (unsigned)((T + rows_per - 1) / rows_per));
#define CONS(NTV, ATV) hipLaunchKernelGGL((k_cons<NTV, ATV>), grid, dim3(256), 0, s, x, o, T, C, c0, c1, rows_per, cnt)
    if (g.S > 1) { if (g.nt) CONS(1, true); else CONS(0, true); }
    else { if (g.nt) CONS(1, false); else CONS(0, false); }
#undef CONS
  }
  // one step of the chain; everything is enqueued, nothing waits on the host
  void step(const Cfg& g) {
    int64_t b[MAXN + 1];
    const int n = g.sched == 0 ? plan_chunks(C, 1, 1024, b) : plan_chunks(C, g.N, 1024, b);
    hipStream_t sc = g.sched == 2 ? s2 : s1;
    if (g.S > 1) CK(hipMemsetAsync(cnt, 0, (size_t)C * 4, sc));
    for (int k = 0; k < n; ++k) {
      prod(g, b[k], b[k + 1]);
      if (g.sched == 2) {
        CK(hipEventRecord(ev[k], s1));
        CK(hipStreamWaitEvent(s2, ev[k], 0));
      }
      cons(g, sc, b[k], b[k + 1]);
    }
    if (g.sched == 2) {
      CK(hipEventRecord(join, s2));
      CK(hipStreamWaitEvent(s1, join, 0));
    }
  }
  bool check(const Cfg& g, std::vector<int>& h) {
    CK(hipMemsetAsync(o, 0, (size_t)T * C * 8, s1));  // a consumer that ran ahead of its producer counts T, not ceil(T / 2)
    CK(hipMemsetAsync(cnt, 0xff, (size_t)C * 4, s1));
    CK(hipDeviceSynchronize());
    step(g);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), cnt, (size_t)C * 4, hipMemcpyDeviceToHost));
    const int want = (int)((T + 1) / 2);
    for (int64_t i = 0; i < C; ++i)
      if (h[i] != want) { printf("!! wrong count at cell %lld: %d, expected %d\n", (long long)i, h[i], want); return false; }
    return true;
  }
  // ms per step by device events on stream 1, host microseconds spent enqueuing a step
  void time(const Cfg& g, int reps, float* ms, float* host_us) {
    hipEvent_t a, e;
    CK(hipEventCreate(&a)); CK(hipEventCreate(&e));
    for (int i = 0; i < 3; ++i) step(g);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(a, s1));
    const auto h0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; ++i) step(g);
    const auto h1 = std::chrono::steady_clock::now();
    CK(hipEventRecord(e, s1));
    CK(hipEventSynchronize(e));
    CK(hipDeviceSynchronize());
    CK(hipEventElapsedTime(ms, a, e));
    *ms /= reps;
    *host_us = std::chrono::duration<float, std::micro>(h1 - h0).count() / reps;
    CK(hipEventDestroy(a)); CK(hipEventDestroy(e));
  }
};

static const char* SCHED[3] = {"a whole   ", "b 1-stream", "c 2-stream"};

int main(int argc, char** argv) {
  const bool quick = argc > 1 && !strcmp(argv[1], "quick");
  Bench B;
  B.T = 365; B.C = 1440 * 720;  // C % 256 == 0: every wave segment is whole
  const size_t E = (size_t)B.T * B.C;
  CK(hipMalloc(&B.x, E * 4)); CK(hipMalloc(&B.o, E * 8)); CK(hipMalloc(&B.cnt, B.C * 4));
  CK(hipStreamCreateWithFlags(&B.s1, hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&B.s2, hipStreamNonBlocking));
  for (int k = 0; k < MAXN; ++k) CK(hipEventCreateWithFlags(&B.ev[k], hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&B.join, hipEventDisableTiming));
  hipLaunchKernelGGL(k_fill, dim3(8192), dim3(256), 0, B.s1, B.x, B.T, B.C);
  CK(hipDeviceSynchronize());
  std::vector<int> h(B.C);
  const int reps = quick ? 5 : 20;
  printf("# T=%lld C=%lld  prod = %.3f GB read + %.3f GB written, cons = %.3f GB read; %d steps per figure\n", (long long)B.T,
         (long long)B.C, E * 4e-9, E * 8e-9, E * 12e-9, reps);
  printf("# schedule | N chunks (cells per chunk, MB of table + field per chunk) | producer doy chunk | consumer row split S |"
         " consumer loads | producer stores | ms per step | host us per step\n");
  std::vector<float> base;
  auto run = [&](const Cfg& g) {
    if (!B.check(g, h)) exit(2);
    float ms, us;
    B.time(g, reps, &ms, &us);
    int64_t b[MAXN + 1];
    const int n = g.sched == 0 ? 1 : plan_chunks(B.C, g.N, 1024, b);
    const int64_t per = g.sched == 0 ? B.C : b[1];
    printf("%s N=%3d (%7lld, %6.1f MB) dchunk=%3d S=%2d ld=%s st=%s  %.4f ms  host %6.1f us\n", SCHED[g.sched], n,
           (long long)per, per * 12.0 * B.T * 1e-6, g.dchunk, g.S, g.nt ? "nt   " : "plain", g.st ? "nt   " : "plain", ms, us);
    fflush(stdout);
    return ms;
  };
  const Cfg today = {0, 1, 32, 1, 1, 0};  // the chain as committed: doy chunk 32, one row slice, nt loads, plain stores
  auto baseline = [&] { base.push_back(run(today)); };
  baseline(); baseline(); baseline();
  // (a) variants: what the flavours cost without any chunking
  for (int nt = 0; nt < 2; ++nt)
    for (int st = 0; st < 2; ++st)
      if (!(nt == 1 && st == 0)) run(Cfg{0, 1, 32, 1, nt, st});
  const int Ns_full[] = {8, 16, 24, 32, 48, 64, 96}, Ns_quick[] = {4, 32};
  const int* Ns = quick ? Ns_quick : Ns_full;
  const int nN = quick ? 2 : 7;
  for (int sched = 1; sched <= 2; ++sched) {
    for (int i = 0; i < nN; ++i) {
      for (int dchunk : {32, 8}) {
        for (int S : {1, 4, 8}) {
          for (int nt = 0; nt < 2; ++nt) {
            for (int st = 0; st < 2; ++st) {
              if (quick && (st || dchunk == 8)) continue;
              run(Cfg{sched, Ns[i], dchunk, S, nt, st});
            }
          }
        }
      }
      baseline();
    }
  }
  float lo = base[0], hi = base[0];
  for (float v : base) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
  printf("# (a) as committed over %zu measurements: min %.4f ms, max %.4f ms, spread %.4f ms\n", base.size(), lo, hi, hi - lo);
  CK(hipDeviceSynchronize());
  return 0;
}
