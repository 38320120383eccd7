/* xclim_hip_analog.h — the C ABI of the spatial-analogue unit (xclim_amd/csrc/analog.hip), exported by libxclimhip.so next to
 * the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py EXT_SIGNATURES.  (Headers under include/ext/ belong to units added while the ABI tests
 * over include/ *.h are frozen; they are checked by tests/test_abi_ext_cpu.py.)
 *
 * The unit computes the eight dissimilarity metrics of xclim.analog (analog.py:181-628) between ONE target sample x (n, d) and
 * the candidate sample of every cell: row c of d fields (m, C).  One lane per candidate cell; all arithmetic is float64 in the
 * reference's order of operations where that order is defined (the library is built with -ffp-contract=off). */
#ifndef XCLIM_HIP_ANALOG_H
#define XCLIM_HIP_ANALOG_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the metrics, in the order of the reference's registry */
#define XH_ANALOG_SEUCLIDEAN 0
#define XH_ANALOG_NEAREST_NEIGHBOR 1
#define XH_ANALOG_ZECH_ASLAN 2
#define XH_ANALOG_SZEKELY_RIZZO 3
#define XH_ANALOG_FRIEDMAN_RAFSKY 4
#define XH_ANALOG_KOLMOGOROV_SMIRNOV 5
#define XH_ANALOG_KLDIV 6
#define XH_ANALOG_MAHALANOBIS 7
#define XH_ANALOG_NMETHODS 8

/* Indices per sample.  A lane keeps one point (d float64) and the per-index means and deviations of its cell in registers,
 * indexed by unrolled loops of this length; 10 is also where the reference's kldiv stops.  More answer XH_ERR_LIMIT. */
#define XH_ANALOG_MAX_D 10

/* kolmogorov_smirnov counts the points of both samples per orthant code: 2^d int32 counters per lane (the x count in the low
 * 16 bits, the y count in the high 16).  d = 6: 64 counters, 256 bytes per lane.  A larger d answers XH_ERR_LIMIT. */
#define XH_ANALOG_KS_MAX_D 6

/* Points per sample, for n and for m alike (so n + m up to 1024; a year of daily samples, 366 + 366, fits).  The target table
 * lies in LDS: (n d + 3 d + npar) float64 = at most (512 * 10 + 30 + 100) * 8 = 41 840 bytes of the 64 KiB a workgroup gets
 * without asking for more.  friedman_rafsky keeps 2 (n + m) float64 per lane in the work buffer: 16 KiB per lane at the limit,
 * 1 GiB for the 65 536 lanes a launch is capped at then (see the work buffer below).  The KS counters hold 16 bits per sample.
 * A larger n or m answers XH_ERR_LIMIT. */
#define XH_ANALOG_MAX_SAMPLE 512

/* kldiv: the largest k and the longest list of k.  A lane keeps its max(k) smallest squared distances in the work buffer and
 * one sum per k in registers.  Beyond: XH_ERR_LIMIT. */
#define XH_ANALOG_MAX_K 32
#define XH_ANALOG_MAX_NK 16

/* xh_analog: out[q * ld_out + c] = metric(x, y_c) for every cell c < C (q = 0; q < nk for kldiv).
 *
 *   method   one of XH_ANALOG_* (XH_ERR_ARG otherwise).
 *   n, m     points of the target and of every candidate sample; 1 <= n, m <= XH_ANALOG_MAX_SAMPLE (XH_ERR_ARG below,
 *            XH_ERR_LIMIT above).
 *   d        indices; 1 <= d <= XH_ANALOG_MAX_D, <= XH_ANALOG_KS_MAX_D for kolmogorov_smirnov (XH_ERR_LIMIT above).
 *   x        HOST float64 (n, d), C order: the target.  Its column means, variances and deviations (ddof = 1, in row order,
 *            as numpy computes them), its NaN test and kldiv's distances r are computed on the host by this call.
 *   C, ld    cells, and the row pitch ld >= C of the fields.  f64: the fields are float64 (else float32; widened on load).
 *   y        HOST array of d DEVICE pointers: field k is (m, C) with pitch ld, row i of field k holding index k of point i
 *            of every cell.
 *   par      HOST float64 (npar), the method's parameters:
 *              zech_aslan     npar = 1: dmin;
 *              szekely_rizzo  npar = 1: standardize (0 or not 0);
 *              mahalanobis    npar = d * d: VI, C order;
 *              the others     npar = 0 (par may be NULL).
 *   k, nk    kldiv only (else nk = 0, k may be NULL): HOST int32 (nk), 1 <= k[q] <= XH_ANALOG_MAX_K, 1 <= nk <= XH_ANALOG_MAX_NK
 *            (XH_ERR_ARG below, XH_ERR_LIMIT above).
 *   out      DEVICE float64 (1, C), or (nk, C) for kldiv, with row pitch ld_out >= C.  Every element (q, c < C) is written by
 *            every call that returns XH_OK with C > 0; nothing beyond column C of a row is touched.
 *
 * The metrics (y: the cell's sample; means and ddof = 1 deviations of y over its rows in row order; N = n + m):
 *   seuclidean          sqrt(sum_k (mean x_k - mean y_k)^2 / var x_k).
 *   mahalanobis         delta = mean x - mean y; sqrt(sum_j (sum_i delta_i VI[i][j]) delta_j).
 *   zech_aslan          v_k = std x_k * std y_k; dist(p, q) = sqrt(sum_k (p_k - q_k)^2 / v_k); L(S) = the sum over the pairs
 *                       S of log(max(dist, dmin)); (-L(xx)) / (n (n - 1)) + (-L(yy)) / (m (m - 1)) - (-L(xy)) / (n m), xx and
 *                       yy over the pairs i < j.
 *   szekely_rizzo       the same dist (standardize), or sqrt(sum_k (p_k - q_k)^2); D(S) = the sum of dist over the pairs S;
 *                       w = n m / (n + m); w * (D(xy) / (n m) + D(xy) / (n m) - D(xx) * 2 / n^2 - D(yy) * 2 / m^2).
 *   nearest_neighbor    s_k = sqrt(std x_k * std y_k); every coordinate divided by s_k; the share of the N pooled points whose
 *                       nearest other point (squared Euclidean distance, first of equals) is of their own sample.  NaN for a
 *                       cell with a non-finite distance (s_k zero or not finite), where the reference raises for the whole call.
 *   friedman_rafsky     the minimum spanning tree of the pooled points by Prim's algorithm on squared Euclidean distances,
 *                       started at point 0 of x, first of equals; 1 - (1 + edges between the samples) / N.  NaN if no finite
 *                       edge leaves the tree.
 *   kolmogorov_smirnov  for every pivot p of x, then of y: the code of a point q has bit k set where p_k <= q_k; cx, cy = the
 *                       points of x and of y per code; the largest |cx / n - cy / m| over codes and pivots.
 *   kldiv               r_i = the distance from x_i to its k-th nearest other point of x (the (k + 1)-th smallest of the n
 *                       distances from x_i, its own 0 included; +inf when there is none), s_i = the k-th smallest distance
 *                       from x_i to the points of y (+inf when m < k); (-(sum_i log(r_i / s_i))) * d / n + log(m / (n - 1.0)).
 *                       NaN for n < 5 or m < 5.
 * A NaN anywhere in x makes every cell NaN; a NaN anywhere in a cell's sample makes that cell NaN.  A zero or non-finite
 * divisor is not special-cased anywhere else: the IEEE result is the result.
 *
 * The work buffer.  A lane's candidate sample is read from the fields every time (neighbouring lanes read neighbouring
 * addresses); its per-lane arrays — Prim's keys and sides (2 N float64), the KS counters (2^d int32), kldiv's max(k) smallest
 * squared distances — live slot-major ([slot][lane]) in the context's scratch, never in registers.  The launch is capped at the
 * lanes whose arrays fit 1 GiB (at least one workgroup of 256) and at 8 workgroups per CU; lanes stride over the cells
 * (XH_ANALOG_MAX_BLOCKS, read with XH_DIAGNOSTICS=1 only, caps the workgroups further: the tests stride with a few hundred
 * cells).  There is ONE path: no switch between an LDS and a scratch form.
 *
 * Every check answers before anything is launched and leaves out untouched; C == 0 launches nothing and returns XH_OK. */
int xh_analog(xh_ctx* ctx, int method, int64_t n, int64_t m, int d, const double* x /* host */, int64_t C, int64_t ld, int f64,
              const void* const* y /* host array of device pointers */, const double* par /* host */, int64_t npar,
              const int32_t* k /* host */, int64_t nk, double* out, int64_t ld_out);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_ANALOG_H */
