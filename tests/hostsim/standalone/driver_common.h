// driver_common.h — what the stand-alone sanitizer programs of the single units (bioclim_driver.cpp, agro_driver.cpp,
// hydro_driver.cpp, rain_driver.cpp) share: the case counter, the two ways to end (exit status 3: an entry point refused; 4: a
// property that needs no reference does not hold) and heap blocks of EXACTLY the size asked for, so that an access one element
// outside lands in a redzone.  TEST INFRASTRUCTURE ONLY.  A driver defines kProgram (its name in the messages) and includes this.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "xclim_hip.h"

extern const char* const kProgram;

static int g_cases = 0;

[[maybe_unused]] static void fail(const char* what) {
  fprintf(stderr, "%s: %s\n", kProgram, what);
  exit(4);
}

[[maybe_unused]] static void ok(int rc, const char* fn) {
  if (rc != XH_OK) {
    fprintf(stderr, "%s: %s returned %d: %s\n", kProgram, fn, rc, xh_last_error());
    exit(3);
  }
}

template <typename V>
V* exact(const std::vector<V>& v) {   // a heap block of exactly the table (one element for an empty one)
  V* p = (V*)malloc(sizeof(V) * (v.empty() ? 1 : v.size()));
  if (!v.empty()) memcpy(p, v.data(), sizeof(V) * v.size());
  return p;
}

template <typename V>
V* block(int64_t n, int fill = 0x7B) {
  V* p = (V*)malloc(sizeof(V) * (size_t)(n > 0 ? n : 1));
  memset(p, fill, sizeof(V) * (size_t)(n > 0 ? n : 1));
  return p;
}

// uniform pseudo-random values in [base, base + amp) with about one NaN in 97
template <typename TE>
TE* field(int64_t T, int64_t C, unsigned seed, double base, double amp) {
  TE* p = (TE*)malloc(sizeof(TE) * (size_t)(T * C > 0 ? T * C : 1));   // EXACTLY the field
  unsigned s = seed;
  for (int64_t i = 0; i < T * C; ++i) {
    s = s * 1664525u + 1013904223u;
    const double u = (double)(s >> 8) / (double)(1u << 24);
    p[i] = (s >> 8) % 97 == 0 ? (TE)NAN : (TE)(base + amp * u);
  }
  return p;
}
