// pyminmax.h — Python's min / max on doubles, as numba compiles them: `max(a, b)` keeps a unless b > a, `min(a, b)` keeps
// a unless b < a.  A NaN first argument survives and a NaN second argument is dropped (fmin / fmax drop both), which the
// fire kernels (fire.hip, ffdi.hip) reproduce.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ double pymax(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double pymin(double a, double b) { return b < a ? b : a; }
