/* xclim_hip_grid.h — the C ABI of the grid-reduction unit (xclim_amd/csrc/grid.hip): what reduces ACROSS the grid to one value
 * per row instead of along time — the spatial sums of sea_ice_area and sea_ice_extent (indices/_threshold.py:3057-3131) and the
 * box mean, the filter and the maximum of jetstream_metric_woollings (indices/_synoptic.py:23-116).  Exported by libxclimhip.so
 * next to the entry points of xclim_hip.h, which this header includes for the context, the return codes and the conventions.
 * ctypes prototypes: xclim_amd/_capi.py UNIT_SIGNATURES.
 *
 * Common to the three entry points.  Fields are time-major with row pitch ld (DEVICE), float32 (f64 = 0) or float64; values are
 * widened to float64 on load (exact) and all arithmetic is float64 (the library is built with -ffp-contract=off).  Tables marked
 * HOST are read (and checked) on the host before anything is launched; every other pointer is DEVICE memory.  Every check answers
 * before anything is launched and leaves the outputs untouched; a call without a row launches nothing and returns XH_OK.  Every
 * element of a requested output is stored; an output that is NULL costs no load, store or arithmetic.  No sum uses a
 * floating-point atomic: every order of summation below is fixed, so a result depends neither on T, nor on the tiling of the
 * rows, nor on which workgroup ran first. */
#ifndef XCLIM_HIP_GRID_H
#define XCLIM_HIP_GRID_H

#include "../xclim_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tile of xh_grid_masked_dot: a workgroup of 256 lanes owns XH_GRID_CHUNK consecutive cells (chunk k: the cells
 * [k * XH_GRID_CHUNK, (k + 1) * XH_GRID_CHUNK)) and XH_GRID_ROWS consecutive rows, and keeps the chunk's weights in registers
 * (eight per lane) across those rows. */
#define XH_GRID_CHUNK 2048
#define XH_GRID_ROWS 8
/* The two sums of xh_grid_masked_dot, as the bits of the output set a launch is compiled for. */
#define XH_GRID_DOT 1  /* sum of (x >= thr ? x : 0) * w */
#define XH_GRID_MSUM 2 /* sum of (x >= thr ? 1 : 0) * w */
/* The longest filter of xh_grid_filter_argmax; a longer one answers XH_ERR_LIMIT. */
#define XH_GRID_MAX_WINDOW 128

/* xh_grid_masked_dot: from ONE read of x (T, C) and the weights w (C, float64), any subset of
 *   dot[t]  = sum over c of (x[t,c] >= thr ? x[t,c] : 0) * w[c]      (the sea-ice area before the division by its factor)
 *   msum[t] = sum over c of (x[t,c] >= thr ? 1 : 0) * w[c]           (the sea-ice extent)
 *   both (T) float64.  The compare is float64 on the widened sample; a NaN sample or a NaN thr compares false.  The product is
 *   taken for EVERY cell, masked or not: a NaN sample adds 0 * w[c], so a NaN or infinite weight makes every row NaN, as
 *   xarray.dot (einsum, no skipna) does.  The set of outputs is uniform over the launch and chosen at compile time.
 *   ORDER OF SUMMATION.  Lane l (0 .. 255) of the workgroup of chunk k adds, starting from +0.0, the terms of the cells
 *   k * 2048 + h * 1024 + 4 * l + i in the order h = 0, 1 (outer), i = 0 .. 3 (inner); a cell at or beyond C adds +0.0.  The 64
 *   lane sums of a wave are folded in six steps, with distances 32, 16, 8, 4, 2, 1: in each step lane m takes (its value) + (the
 *   value of lane m + distance); lane 0 holds the wave's sum.  The four wave sums are added in wave order, ((w0 + w1) + w2) + w3:
 *   the partial of (row, chunk), kept in the context's work buffer.  A second kernel adds the partials of a row in chunk order,
 *   from the first; a row without a cell (C = 0) is +0.0.
 *   Lanes read 16 bytes of a field row (4 float32 or 2 float64 cells) with non-temporal loads where x is 16-byte aligned and
 *   ld * (element size) is a multiple of 16; a last partial group of cells, and every cell of a view that is not aligned so, is
 *   read cell by cell.  The terms and their order are the same on both paths. */
int xh_grid_masked_dot(xh_ctx* ctx, int64_t T, int64_t C, int64_t ld, int f64, const void* x, const double* w, double thr,
                       double* dot, double* msum);

/* xh_grid_box_mean: the mean over selected levels and longitudes, for selected latitudes.
 *   u (T, Z, Y, X): sample (t, z, y, x) is element t * ld + z * sz + y * sy + x * sx; strides at least 1 and a row inside its
 *   pitch: (Z-1) * sz + (Y-1) * sy + (X-1) * sx < ld (XH_ERR_LAYOUT otherwise), so that (Z, Y, X) and (Z, X, Y) are read in place.
 *   iz[nz], iy[ny], ix[nx] (DEVICE int32): the selected levels, latitudes and longitudes, in any order, contiguous or not.  An
 *   index outside its axis selects nothing: its samples count as NaN, and nothing outside the field is read.
 *   zm[t, j] (T, ny) float64 with row pitch ld_zm >= ny = (sum of the samples (t, iz[a], iy[j], ix[b]) that are not NaN) /
 *   (their number); NaN without one (xarray's mean over two dimensions pools them, skipna for floats).
 *   ORDER OF SUMMATION.  With sy == 1 and sx != 1 (lanes along the latitudes, one lane per (t, j)): from +0.0, a = 0 .. nz - 1
 *   (outer), b = 0 .. nx - 1 (inner).  Otherwise (lanes along the longitudes, one wave per (t, j)): lane l adds from +0.0 the
 *   samples b = l, l + 64, l + 128 ... (inner) of a = 0 .. nz - 1 (outer); the 64 lane sums and the 64 lane counts are folded in
 *   six steps with distances 32, 16, 8, 4, 2, 1, lane m taking (its value) + (the value of lane m + distance). */
int xh_grid_box_mean(xh_ctx* ctx, int64_t T, int64_t ld, int64_t Z, int64_t Y, int64_t X, int64_t sz, int64_t sy, int64_t sx, int f64,
                     const void* u, int64_t nz, const int32_t* iz, int64_t ny, const int32_t* iy, int64_t nx, const int32_t* ix,
                     double* zm, int64_t ld_zm);

/* xh_grid_filter_argmax: a centred filter along time and the first maximum along the row.
 *   zm (T, ny) float64 with row pitch ld_zm >= ny.  wts (HOST float64, W), 1 <= W <= XH_GRID_MAX_WINDOW (XH_ERR_LIMIT beyond).
 *   f[t, j] = zm[t - W/2, j] * wts[0] + zm[t - W/2 + 1, j] * wts[1] + ... added in row order from its first term (W/2 rounds
 *   down); NaN where a row of the window is outside [0, T) or holds a NaN: what rolling(time=W, center=True).construct().dot(wts)
 *   gives.  f (T, ny) with row pitch ld_f >= ny.
 *   smax[t] (T, float64) = the largest f[t, j] that is not NaN; jmax[t] (T, int32) = the first j, in field order, that holds it;
 *   NaN and -1 when every f[t, j] is NaN (or ny = 0).
 *   f, smax and jmax are each optional; one at least must be requested. */
int xh_grid_filter_argmax(xh_ctx* ctx, int64_t T, int64_t ny, const double* zm, int64_t ld_zm, int W, const double* wts /* host */,
                          double* f, int64_t ld_f, double* smax, int32_t* jmax);

#ifdef __cplusplus
}
#endif
#endif /* XCLIM_HIP_GRID_H */
