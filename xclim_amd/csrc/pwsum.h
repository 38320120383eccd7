// pwsum.h — numpy's pairwise sum beyond one block: the sibling of fitcore.h's PwSum (n <= 128) for 128 < n <= 512.
// np.add.reduce splits a longer array in two, the first part n / 2 rounded down to a multiple of 8, and recurses until a part
// has at most 128 values; each such leaf is one PwSum.  Up to 512 values the recursion is at most three levels deep (n = 500:
// 248 + 252, 252 = 120 + 132, 132 = 64 + 68).  The values arrive in order (position p): the leaf that starts at p is found by
// walking down from the root, and a closed leaf is added to the waiting sum of its level, left + right, like a binary counter,
// so at most one partial sum waits per level.  Everything is a scalar: an array indexed at run time would live in scratch.
#ifndef XCLIM_AMD_PWSUM_H
#define XCLIM_AMD_PWSUM_H
#include "fitcore.h"

namespace {

constexpr int PW_LONG_MAX_N = 512;

struct PwSumLong {
  PwSum cur;
  double w1, w2, w3, total;  // the left sibling's sum waiting at levels 1 .. 3, and the root's
  bool h1, h2, h3;
  int n, start, end, level;  // the open leaf: [start, end) at `level`
  __device__ void open(int p) {
    int lo = 0, len = n, d = 0;
    while (len > 128) {
      int h = len / 2;
      h -= h % 8;
      if (p < lo + h) {
        len = h;
      } else {
        lo += h;
        len -= h;
      }
      ++d;
    }
    start = lo;
    end = lo + len;
    level = d;
    cur.init(len);
  }
  __device__ void init(int n_) {
    n = n_;
    w1 = w2 = w3 = total = 0.0;
    h1 = h2 = h3 = false;
    open(0);
  }
  __device__ void close() {
    double s = cur.sum();
    int d = level;
    if (d == 3) {
      if (!h3) {
        w3 = s, h3 = true;
        return;
      }
      s = w3 + s, h3 = false, d = 2;
    }
    if (d == 2) {
      if (!h2) {
        w2 = s, h2 = true;
        return;
      }
      s = w2 + s, h2 = false, d = 1;
    }
    if (d == 1) {
      if (!h1) {
        w1 = s, h1 = true;
        return;
      }
      s = w1 + s, h1 = false;
    }
    total = s;
  }
  __device__ void add(int p, double v) {
    if (p >= end) {  // leaves are never empty: one step
      close();
      open(p);
    }
    cur.add(p - start, v);
  }
  __device__ double sum() {  // once, after the last value
    close();
    return total;
  }
};

}  // namespace
#endif  // XCLIM_AMD_PWSUM_H
