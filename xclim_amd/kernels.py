"""Typed Python wrappers over the C ABI (one function per entry point of include/xclim_hip.h).

Inputs are :class:`~xclim_amd._capi.DeviceArray` views of shape (T, C) (time-major, C contiguous) unless stated;
numpy inputs are uploaded.  Outputs stay on the device (call ``.get()``), so chained ops (percentile_doy ->
threshold_count) never cross PCIe.  No CPU fallback exists here by design.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi
from ._capi import OPS, REDUCERS, RUN_STATS, Device, DeviceArray, np_ptr

_vp = C.c_void_p


def as_device(dev: Device, a, dtype=np.float32) -> DeviceArray:
    if isinstance(a, DeviceArray):
        if a.dtype != np.dtype(dtype):
            raise TypeError(f"device array dtype {a.dtype} != {np.dtype(dtype)}")
        return a
    return dev.to_device(np.asarray(a), dtype=dtype)


def _tc(x: DeviceArray, dtype=np.float32):
    """Shape of a 2-D device field; the kernels read raw pointers, so the element type is checked here."""
    if len(x.shape) != 2:
        raise ValueError(f"expected a 2-D (time, cells) array, got shape {x.shape}")
    if dtype is not None and np.dtype(x.dtype) != np.dtype(dtype):
        raise TypeError(f"expected a {np.dtype(dtype).name} device array, got {np.dtype(x.dtype).name}")
    return int(x.shape[0]), int(x.shape[1])


def _field(x: DeviceArray):
    """(T, C, is_float64) of a float32 or float64 field: a float64 field picks the entry point's ``_f64`` twin."""
    f64 = np.dtype(x.dtype) == np.float64
    T, C_ = _tc(x, np.float64 if f64 else np.float32)
    return T, C_, f64


def _f32_only(x, what: str) -> None:
    """A float64 field on a form without a float64 kernel: Float64FieldError (never rounded)."""
    if isinstance(x, DeviceArray) and np.dtype(x.dtype) == np.float64:
        capi.refuse_float64(what)


def _seg(seg_off):
    s = np.ascontiguousarray(seg_off, dtype=np.int64)
    return s, len(s) - 1


def _same_fields(who: str, fields: dict):
    """(T, C, is_float64) of a dict of device fields: all float32 or all float64, and of one (T, C) shape."""
    kinds = {np.dtype(v.dtype) for v in fields.values()}
    if len(kinds) != 1 or not kinds <= {np.dtype(np.float32), np.dtype(np.float64)}:
        raise TypeError(f"{who}: {', '.join(fields) or 'the fields'} must be all float32 or all float64")
    shapes = {_tc(v, None) for v in fields.values()}
    if len(shapes) != 1:
        raise ValueError(f"{who}: every field must have the same (T, C) shape")
    return (*shapes.pop(), int(kinds.pop() == np.float64))


def _offsets(who: str, seg, rows: int, what: str = "period"):
    """Host offsets as int64: 1-D, non-decreasing, within [0, rows]."""
    s = np.ascontiguousarray(seg, dtype=np.int64)
    if s.ndim != 1 or len(s) < 1 or s[0] < 0 or s[-1] > rows or np.any(np.diff(s) < 0):
        raise ValueError(f"{who}: {what} offsets must be non-decreasing within [0, {rows}]")
    return s


def _periods(who: str, seg, rows: int, what: str = "period"):
    """(offsets, P) of a period table: _offsets, and no more periods than the second grid axis holds."""
    s = _offsets(who, seg, rows, what)
    if len(s) - 1 > 65535:
        raise ValueError(f"{who}: at most 65535 periods, got {len(s) - 1}")
    return s, len(s) - 1


def _row_selection(who: str, sel, rows: int):
    """A row selection as uint8 (None stays None): a bool or uint8 array with one entry per row."""
    if sel is None:
        return None
    m = np.ascontiguousarray(sel)
    if m.shape != (rows,) or m.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise ValueError(f"{who}: the selection must be a bool or uint8 array of length {rows}")
    return m.astype(np.uint8)


def _subset(who: str, outputs, allowed):
    """The requested outputs in the order of ``allowed``; none is a ValueError."""
    outputs = [o for o in allowed if o in set(outputs)]
    if not outputs:
        raise ValueError(f"{who}: outputs must be a non-empty subset of {', '.join(allowed)}")
    return outputs


def _ptr(arrays: dict, name: str):
    """The device pointer of a dict entry, NULL for a name it does not hold."""
    a = arrays.get(name)
    return _vp(a.ptr) if a is not None else _vp(0)


def op_code(op: str) -> int:
    if op == "gteq":
        op = "ge"
    if op == "lteq":
        op = "le"
    if op not in OPS:
        raise ValueError(f"Operation `{op}` not recognized.")
    return OPS[op]


def fill_synthetic(dev: Device, T, C_, kind, seed, base, amp, p_wet=0.3, nan_per_million=0, cell0=0) -> DeviceArray:
    out = dev.empty((T, C_), np.float32)
    dbase = as_device(dev, np.asarray(base, dtype=np.float32))
    dev.call("xh_fill_synthetic", _vp(out.ptr), T, C_, C_, int(kind), int(seed), int(cell0), _vp(dbase.ptr), float(amp),
             float(p_wet), int(nan_per_million))
    dev.sync()
    return out


def transpose(dev: Device, x: DeviceArray) -> DeviceArray:
    r, c = _tc(x)
    out = dev.empty((c, r), np.float32)
    dev.call("xh_transpose_f32", _vp(x.ptr), r, c, c, _vp(out.ptr), r)
    return out


def threshold_count(dev: Device, x: DeviceArray, op: str, seg_off, *, scalar=None, scalar_f64=False, doy_table=None,
                    tidx=None, full=None, want_valid=True, out=None):
    """xh_threshold_count.  Exactly one of scalar / (doy_table, tidx) / full.  Returns (count, valid) (P, C) int32."""
    f64 = x.dtype == np.float64  # float64 field: float64 compare against any threshold (numpy promotion), xh_*_f64
    T, C_ = _tc(x, np.float64 if f64 else np.float32)
    seg, P = _seg(seg_off)
    if out is not None:
        count, valid = out
    else:
        count = dev.empty((P, C_), np.int32)
        valid = dev.empty((P, C_), np.int32) if want_valid else None
    table_ptr, tstride, tidx_ptr, kind, thr = _vp(0), 0, _vp(0), capi.THR_SCALAR_F32, 0.0
    keep = []
    if scalar is not None:
        kind = capi.THR_SCALAR_F64 if scalar_f64 else capi.THR_SCALAR_F32
        thr = float(scalar)
    elif doy_table is not None:
        kind = capi.THR_DOY_F64 if doy_table.dtype == np.float64 else capi.THR_DOY_F32
        table_ptr, tstride = _vp(doy_table.ptr), int(doy_table.shape[-1])
        if isinstance(tidx, DeviceArray):
            dt = tidx
        else:
            dt = dev.to_device(np.ascontiguousarray(tidx, dtype=np.int32))
            keep.append(dt)
        tidx_ptr = _vp(dt.ptr)
    elif full is not None:
        kind = capi.THR_FULL_F64 if full.dtype == np.float64 else capi.THR_FULL_F32
        table_ptr, tstride = _vp(full.ptr), int(full.shape[-1])
    else:
        raise ValueError("a threshold is required")
    if f64:
        if kind in (capi.THR_DOY_F32, capi.THR_FULL_F32):
            raise TypeError("a float64 field needs float64 threshold tables (a float32 table widens exactly: upload it as float64)")
        kind = capi.THR_SCALAR_F64 if kind == capi.THR_SCALAR_F32 else kind
    if kind == capi.THR_DOY_F64 and not f64:
        # the table's row count is known here: the multi-year tile kernel (tcount.hip) needs it to size its LDS slice
        dev.call("xh_threshold_count_doy", _vp(x.ptr), T, C_, C_, 1, op_code(op), table_ptr, tstride,
                 int(np.prod(doy_table.shape[:-1])), tidx_ptr, np_ptr(seg), P, _vp(count.ptr), _vp(valid.ptr if valid else 0))
    else:
        dev.call("xh_threshold_count_f64" if f64 else "xh_threshold_count", _vp(x.ptr), T, C_, C_, 1, op_code(op), kind, thr,
                 table_ptr, tstride, tidx_ptr, np_ptr(seg), P, _vp(count.ptr), _vp(valid.ptr if valid else 0))
    if keep:
        dev.sync()
    return count, valid


def domain_count(dev: Device, x: DeviceArray, op1, thr1, op2, thr2, combine, seg_off, want_valid=True):
    T, C_, f64 = _field(x)  # a float64 field compares in float64 (xh_domain_count_f64)
    seg, P = _seg(seg_off)
    count = dev.empty((P, C_), np.int32)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    dev.call("xh_domain_count_f64" if f64 else "xh_domain_count", _vp(x.ptr), T, C_, C_, 1, op_code(op1), float(thr1), op_code(op2), float(thr2),
             {"and": 1, "or": 2}[combine], np_ptr(seg), P, _vp(count.ptr), _vp(valid.ptr if valid else 0))
    return count, valid


def resample_reduce(dev: Device, x: DeviceArray, reducer: str, seg_off, skipna=True, want_valid=True):
    f64 = x.dtype == np.float64  # float64 field -> float64 statistics (xh_resample_reduce_f64)
    T, C_ = _tc(x, np.float64 if f64 else np.float32)
    seg, P = _seg(seg_off)
    if reducer not in REDUCERS:
        raise ValueError(f"Reducer `{reducer}` not recognized.")
    odt = np.int32 if reducer in ("count", "argmin", "argmax") else (np.float64 if f64 else np.float32)
    out = dev.empty((P, C_), odt)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    dev.call("xh_resample_reduce_f64" if f64 else "xh_resample_reduce", _vp(x.ptr), T, C_, C_, 1, REDUCERS[reducer], int(bool(skipna)), np_ptr(seg), P,
             _vp(out.ptr), _vp(valid.ptr if valid else 0))
    return out, valid


def apply_missing_mask(dev: Device, value: DeviceArray, valid: DeviceArray, expected, out=None) -> DeviceArray:
    P, C_ = _tc(value, None)
    exp = np.ascontiguousarray(expected, dtype=np.int32)
    assert exp.shape == (P,)
    out = out if out is not None else dev.empty((P, C_), np.float64)
    kinds = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}  # float64: the results of the _f64 twins
    if np.dtype(value.dtype) not in kinds:
        raise TypeError(f"apply_missing_mask: values must be int32, float32 or float64, got {np.dtype(value.dtype).name}")
    kind = kinds[np.dtype(value.dtype)]
    dev.call("xh_apply_missing_mask", _vp(value.ptr), kind, _vp(valid.ptr), np_ptr(exp), P, C_, _vp(out.ptr))
    return out


def rolling_reduce(dev: Device, x: DeviceArray, window: int, reducer: str, center=True) -> DeviceArray:
    """xh_rolling_reduce; a float64 field gives a float64 result (xh_rolling_reduce_f64, the window added in float64)."""
    T, C_, f64 = _field(x)
    out = dev.empty((T, C_), np.float64 if f64 else np.float32)
    dev.call("xh_rolling_reduce_f64" if f64 else "xh_rolling_reduce", _vp(x.ptr), T, C_, C_, 1, int(window), int(bool(center)), REDUCERS[reducer],
             _vp(out.ptr), C_)
    return out


def rolling_dot(dev: Device, x: DeviceArray, weights) -> DeviceArray:
    """xh_rolling_dot: trailing weighted window sum (float64 sum, float32 result, NaN until the window is full)."""
    T, C_ = _tc(x)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_rolling_dot", _vp(x.ptr), T, C_, C_, 1, len(w), np_ptr(w), _vp(out.ptr), C_)
    return out


def cumsum_reset(dev: Device, x: DeviceArray, index="last") -> DeviceArray:
    T, C_ = _tc(x)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_cumsum_reset", _vp(x.ptr), T, C_, C_, 1, int(index == "first"), _vp(out.ptr), C_)
    return out


def rle(dev: Device, x: DeviceArray, index="first") -> DeviceArray:
    T, C_ = _tc(x)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_rle", _vp(x.ptr), T, C_, C_, 1, int(index == "first"), _vp(out.ptr), C_)
    return out


def run_stats(dev: Device, x: DeviceArray, stat: str, window: int, seg_off, *, cut=True, index="first", fused_op=None,
              thresh=0.0, want_valid=True, out=None, one_dim=False):
    """xh_run_stats.  ``one_dim``: the NaN semantics of the reference's 1-D ufunc path (index "first" only); True = the
    windowed_run_count / windowed_run_events form, "stat" = the statistics_run_1d form (NaN for a series with NaN steps and
    no qualifying run)."""
    T, C_, f64 = _field(x)
    seg, P = _seg(seg_off)
    if out is not None:
        out, valid = out
    else:
        out = dev.empty((P, C_), np.float32)
        valid = dev.empty((P, C_), np.int32) if want_valid else None
    fop = -1 if fused_op is None else op_code(fused_op)
    if f64 and stat in ("first", "last"):
        capi.refuse_float64(f"run_stats({stat})")
    dev.call("xh_run_stats_f64" if f64 else "xh_run_stats", _vp(x.ptr), T, C_, C_, 1, fop, float(thresh), int(window), RUN_STATS[stat],
             ((3 if one_dim == "stat" else 2) if one_dim else 1) if index == "first" else 0, np_ptr(seg), P, int(bool(cut)), _vp(out.ptr),
             _vp(valid.ptr if valid else 0))
    return out, valid


def _pair(a: DeviceArray, b: DeviceArray):
    """(T, C, dtypes) of two fields of one shape: dtypes None for two float32 fields (the float32 kernel), else the `dtypes`
    argument of the ``_f64`` twins (0: both float64, 1: the first float32, 2: the second float32)."""
    assert b.shape == a.shape
    T, C_ = _tc(a, None)
    da, db = np.dtype(a.dtype), np.dtype(b.dtype)
    for d in (da, db):
        if d not in (np.float32, np.float64):
            raise TypeError(f"expected a float32 or float64 device array, got {d.name}")
    if da == np.float32 and db == np.float32:
        return T, C_, None
    return T, C_, 1 if da == np.float32 else (2 if db == np.float32 else 0)


def bivariate_count(dev: Device, x1: DeviceArray, x2: DeviceArray, op1, thr1, op2, thr2, combine, seg_off, want_valid=True):
    """A float64 field on either side: xh_bivariate_count_f64 (a float32 side compares against its threshold rounded to
    float32, as numpy does with a python float)."""
    T, C_, dtypes = _pair(x1, x2)
    seg, P = _seg(seg_off)
    count = dev.empty((P, C_), np.int32)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    comb = {"all": 1, "and": 1, "any": 2, "or": 2}[combine]
    if dtypes is None:
        dev.call("xh_bivariate_count", _vp(x1.ptr), _vp(x2.ptr), T, C_, C_, C_, op_code(op1), float(thr1), op_code(op2), float(thr2),
                 comb, np_ptr(seg), P, _vp(count.ptr), _vp(valid.ptr if valid else 0))
    else:
        dev.call("xh_bivariate_count_f64", _vp(x1.ptr), _vp(x2.ptr), T, C_, C_, C_, dtypes, op_code(op1), float(thr1), op_code(op2),
                 float(thr2), comb, np_ptr(seg), P, _vp(count.ptr), _vp(valid.ptr if valid else 0))
    return count, valid


def range_reduce(dev: Device, low: DeviceArray, high: DeviceArray, mode: str, reducer: str, seg_off, want_valid=True):
    """mode: "range" (reducer of high - low) | "interday" (mean |diff|) | "extreme" (max(high) - min(low)).  A float64 field
    on either side: xh_range_reduce_f64 (float64 result, a float32 side widened)."""
    T, C_, dtypes = _pair(low, high)
    seg, P = _seg(seg_off)
    out = dev.empty((P, C_), np.float32 if dtypes is None else np.float64)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    m = {"range": 0, "interday": 1, "extreme": 2}[mode]
    if dtypes is None:
        dev.call("xh_range_reduce", _vp(low.ptr), _vp(high.ptr), T, C_, C_, C_, m, REDUCERS.get(reducer, 0), np_ptr(seg), P,
                 _vp(out.ptr), _vp(valid.ptr if valid else 0))
    else:
        dev.call("xh_range_reduce_f64", _vp(low.ptr), _vp(high.ptr), T, C_, C_, C_, dtypes, m, REDUCERS.get(reducer, 0), np_ptr(seg),
                 P, _vp(out.ptr), _vp(valid.ptr if valid else 0))
    return out, valid


def compare_map(dev: Device, a: DeviceArray, op, thr, kind: str = "mask") -> DeviceArray:
    """kind: "mask" (uint8) | "maskf" (float 1/0) | "events" (float 1/0/NaN) | "where" (a where cond else NaN) | "excess"
    ((a - thr).clip(0), NaN kept; op unused); thr: scalar or DeviceArray."""
    ok = {"mask": 0, "events": 1, "where": 2, "maskf": 3, "excess": 4}[kind]
    if a.dtype == np.float64 or (isinstance(thr, DeviceArray) and thr.dtype == np.float64):
        return _compare_map_f64(dev, a, op, thr, ok)
    T, C_ = _tc(a)
    out = dev.empty(a.shape, np.uint8 if ok == 0 else np.float32)
    if isinstance(thr, DeviceArray):
        assert thr.shape == a.shape and thr.dtype == np.float32
        dev.call("xh_compare_map", _vp(a.ptr), T, C_, C_, op_code(op), 0.0, 0, _vp(thr.ptr), C_, ok, _vp(out.ptr), C_)
    else:
        dev.call("xh_compare_map", _vp(a.ptr), T, C_, C_, op_code(op), float(thr), int(isinstance(thr, np.float64)), _vp(0), 0, ok,
                 _vp(out.ptr), C_)
    return out


def _compare_map_f64(dev: Device, a: DeviceArray, op, thr, ok: int) -> DeviceArray:
    """xh_compare_map_f64: the compare in float64 (numpy promotion: a float32 side is widened).  Masks only."""
    if ok in (2, 4):
        capi.refuse_float64("compare_map(where / excess)")
    T, C_ = _tc(a, None)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError(f"expected a float32 or float64 device array, got {np.dtype(a.dtype).name}")
    out = dev.empty(a.shape, np.uint8 if ok == 0 else np.float32)
    if isinstance(thr, DeviceArray):
        assert thr.shape == a.shape and thr.dtype in (np.float32, np.float64)
        dtypes = 1 if a.dtype == np.float32 else (2 if thr.dtype == np.float32 else 0)
        dev.call("xh_compare_map_f64", _vp(a.ptr), T, C_, C_, op_code(op), 0.0, _vp(thr.ptr), C_, dtypes, ok, _vp(out.ptr), C_)
    else:
        dev.call("xh_compare_map_f64", _vp(a.ptr), T, C_, C_, op_code(op), float(thr), _vp(0), 0, 0, ok, _vp(out.ptr), C_)
    return out


def select_rows(dev: Device, x: DeviceArray, idx, out: DeviceArray | None = None, out_row: int = 0, out_stride_rows: int = 1) -> DeviceArray:
    """out row i = x row idx[i], NaN where idx[i] < 0 (xh_select_rows).  With ``out`` (rows, C): row i goes to row
    ``out_row + i * out_stride_rows`` of it (a strided scatter into an existing sample matrix)."""
    T, C_ = _tc(x)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if out is None:
        out = dev.empty((len(idx), C_), np.float32)
        dev.call("xh_select_rows", _vp(x.ptr), T, C_, C_, 1, np_ptr(idx), len(idx), _vp(out.ptr), C_)
        return out
    rows, Co = _tc(out)
    if Co != C_ or out_row < 0 or (len(idx) and out_row + (len(idx) - 1) * out_stride_rows >= rows) or out_stride_rows < 1:
        raise ValueError("select_rows: the strided destination does not fit `out`")
    dev.call("xh_select_rows", _vp(x.ptr), T, C_, C_, 1, np_ptr(idx), len(idx), _vp(out.ptr + out_row * C_ * 4), out_stride_rows * C_)
    return out


def mask_to_f32(dev: Device, mask: DeviceArray) -> DeviceArray:
    """uint8 / bool device mask -> float32 1 / 0 mask of the same shape (xh_mask_u8_to_f32)."""
    if np.dtype(mask.dtype).itemsize != 1:
        raise TypeError(f"expected a 1-byte mask, got {np.dtype(mask.dtype).name}")
    out = dev.empty(mask.shape, np.float32)
    dev.call("xh_mask_u8_to_f32", _vp(mask.ptr), int(mask.size), _vp(out.ptr))
    return out


def thresholded_reduce(dev: Device, x: DeviceArray, op, thr, mode: int, reducer: str, seg_off, want_valid=True):
    T, C_, f64 = _field(x)  # a float64 field: differences, sums and compares in float64, float64 result
    seg, P = _seg(seg_off)
    out = dev.empty((P, C_), np.float64 if f64 else np.float32)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    dev.call("xh_thresholded_reduce_f64" if f64 else "xh_thresholded_reduce", _vp(x.ptr), T, C_, C_, 1, op_code(op), float(thr), int(mode), REDUCERS.get(reducer, 0),
             np_ptr(seg), P, _vp(out.ptr), _vp(valid.ptr if valid else 0))
    return out, valid


def mask_rows(dev: Device, x: DeviceArray, seg_off, lo, hi, invert=False) -> DeviceArray:
    T, C_ = _tc(x)
    seg, P = _seg(seg_off)
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    hi = np.ascontiguousarray(hi, dtype=np.int32)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_mask_rows", _vp(x.ptr), T, C_, C_, 1, np_ptr(seg), P, np_ptr(lo), np_ptr(hi), int(bool(invert)), _vp(out.ptr), C_)
    return out


def doy_mean_std(dev: Device, x: DeviceArray, tbase, window: int):
    T, C_ = _tc(x)
    tb = np.ascontiguousarray(tbase, dtype=np.int32)
    nyears, ndoy = tb.shape
    m, s = dev.empty((ndoy, C_), np.float32), dev.empty((ndoy, C_), np.float32)
    dev.call("xh_doy_mean_std", _vp(x.ptr), T, C_, C_, 1, np_ptr(tb), nyears, ndoy, int(window), _vp(m.ptr), _vp(s.ptr))
    return m, s


WIN_REDUCERS = {"sum": 0, "mean": 1, "min": 2, "max": 3, "wmean": 4}


def spell_mask(dev: Device, x: DeviceArray, window: int, win_reducer: str, op: str, thresh: float, weights=None) -> DeviceArray:
    T, C_, f64 = _field(x)
    out = dev.empty((T, C_), np.float32)
    if f64:  # xh_spell_mask_f64: window statistic and compare in float64; weighted windows are not served
        if weights is not None:
            capi.refuse_float64("spell_mask(weights=...)")
        dev.call("xh_spell_mask_f64", _vp(x.ptr), T, C_, C_, 1, int(window), WIN_REDUCERS[win_reducer or "min"], op_code(op),
                 float(thresh), _vp(0), _vp(out.ptr), C_)
        return out
    w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
    red = WIN_REDUCERS["wmean" if w is not None else (win_reducer or "min")]
    dev.call("xh_spell_mask", _vp(x.ptr), T, C_, C_, 1, int(window), red, op_code(op), float(thresh),
             np_ptr(w) if w is not None else _vp(0), _vp(out.ptr), C_)
    return out


def spell_run_stats(dev: Device, x: DeviceArray, window: int, win_reducer: str, op: str, thresh: float, stat: str, seg_off,
                    weights=None, want_valid=True):
    """xh_spell_run_stats: run statistics of the spell mask, the mask itself is never written (runs cut at the periods).
    Returns None when the shape is not covered (window > 8): the caller then takes spell_mask + run_stats."""
    from ._capi import XH_ERR_NOTIMPL, XclimHipError

    T, C_, f64 = _field(x)
    seg, P = _seg(seg_off)
    if f64 and weights is not None:
        capi.refuse_float64("spell_run_stats(weights=...)")
    out = dev.empty((P, C_), np.float32)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
    red = WIN_REDUCERS["wmean" if w is not None else (win_reducer or "min")]
    try:
        dev.call("xh_spell_run_stats_f64" if f64 else "xh_spell_run_stats", _vp(x.ptr), T, C_, C_, 1, int(window), red, op_code(op),
                 float(thresh), np_ptr(w) if w is not None else _vp(0), RUN_STATS[stat], np_ptr(seg), P, _vp(out.ptr),
                 _vp(valid.ptr if valid else 0))
    except XclimHipError as e:
        if e.code == XH_ERR_NOTIMPL:
            return None
        raise
    return out, valid


def spell_mask_multi(dev: Device, xs, window: int, win_reducer: str, op: str, threshs, var_reducer="all", weights=None) -> DeviceArray:
    """spell_mask on a list of (T, C) device arrays with one threshold each (xh_spell_mask_multi)."""
    T, C_ = _tc(xs[0])
    assert all(x.shape == xs[0].shape for x in xs) and len(threshs) == len(xs)
    out = dev.empty((T, C_), np.float32)
    w = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
    red = WIN_REDUCERS["wmean" if w is not None else (win_reducer or "min")]
    ptrs = np.array([x.ptr for x in xs], dtype=np.uint64)
    thr = np.ascontiguousarray(threshs, dtype=np.float64)
    dev.call("xh_spell_mask_multi", np_ptr(ptrs), len(xs), np_ptr(thr), {"all": 1, "any": 2}[var_reducer], T, C_, C_, 1,
             int(window), red, op_code(op), np_ptr(w) if w is not None else _vp(0), _vp(out.ptr), C_)
    return out


def runs_with_holes(dev: Device, start: DeviceArray, window_start: int, stop: DeviceArray | None, window_stop: int) -> DeviceArray:
    T, C_ = _tc(start)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_runs_with_holes", _vp(start.ptr), _vp(stop.ptr if stop is not None else 0), T, C_, C_, 1, int(window_start),
             int(window_stop), _vp(out.ptr), C_)
    return out


def run_events(dev: Device, runs: DeviceArray, seg_off, maxev: int, eff: DeviceArray | None = None,
               data: DeviceArray | None = None, want=("start", "end", "len")):
    """Event compaction (xh_run_events): dict of (P, maxev, C) float32 arrays, NaN past the last run."""
    T, C_ = _tc(runs)
    seg, P = _seg(seg_off)
    out = {k: dev.empty((P, int(maxev), C_), np.float32) for k in want}
    if "start" not in out:
        out["start"] = dev.empty((P, int(maxev), C_), np.float32)
    ptr = lambda k: _vp(out[k].ptr if k in out else 0)
    dev.call("xh_run_events", _vp(runs.ptr), _vp(eff.ptr if eff is not None else 0), _vp(data.ptr if data is not None else 0), T, C_,
             C_, 1, np_ptr(seg), P, int(maxev), ptr("start"), ptr("end"), ptr("len"), ptr("eff"), ptr("sum"))
    return out


def suspicious_run(dev: Device, x: DeviceArray, window: int, op=None, thresh=None) -> DeviceArray:
    T, C_ = _tc(x)
    out = dev.empty((T, C_), np.uint8)
    dev.call("xh_suspicious_run", _vp(x.ptr), T, C_, C_, 1, int(window), -1 if thresh is None else op_code(op),
             0.0 if thresh is None else float(thresh), _vp(out.ptr), C_)
    return out


def keep_longest_run(dev: Device, x: DeviceArray, seg_off) -> DeviceArray:
    T, C_ = _tc(x)
    seg, P = _seg(seg_off)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_keep_longest_run", _vp(x.ptr), T, C_, C_, 1, np_ptr(seg), P, _vp(out.ptr), C_)
    return out


def season(dev: Device, x: DeviceArray, window: int, seg_off, mid_idx=None):
    T, C_ = _tc(x)
    seg, P = _seg(seg_off)
    s, e, ln = (dev.empty((P, C_), np.float32) for _ in range(3))
    mid = np.ascontiguousarray(mid_idx, dtype=np.int32) if mid_idx is not None else None
    dev.call("xh_season", _vp(x.ptr), T, C_, C_, 1, int(window), np_ptr(seg), np_ptr(mid) if mid is not None else _vp(0), P,
             _vp(s.ptr), _vp(e.ptr), _vp(ln.ptr))
    return s, e, ln


def max_run_sum(dev: Device, x: DeviceArray, window: int, seg_off, cut=True) -> DeviceArray:
    """xh_max_run_sum; cut=False: the reference's resample-after semantics (runs cross the period edges)."""
    T, C_ = _tc(x)
    seg, P = _seg(seg_off)
    out = dev.empty((P, C_), np.float32)
    dev.call("xh_max_run_sum", _vp(x.ptr), T, C_, C_, 1, int(window), np_ptr(seg), P, int(bool(cut)), _vp(out.ptr))
    return out


def nan_quantile(dev: Device, x: DeviceArray, q, alpha=1.0, beta=1.0, sample_axis=0) -> DeviceArray:
    """x: (N, C) if sample_axis == 0 else (C, N).  Returns (nq, C) float64."""
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    f64 = x.dtype == np.float64  # float64 samples: `diff` in float64 (utl:486), xh_nan_quantile_f64
    if sample_axis == 0:
        N, C_ = _tc(x, np.float64 if f64 else np.float32)
        sn, sc = C_, 1
    else:
        C_, N = _tc(x, np.float64 if f64 else np.float32)
        sn, sc = 1, N
    out = dev.empty((len(q), C_), np.float64)
    dev.call("xh_nan_quantile_f64" if f64 else "xh_nan_quantile", _vp(x.ptr), N, C_, sn, sc, np_ptr(q), len(q), float(alpha), float(beta), _vp(out.ptr))
    return out


def weighted_quantile(dev: Device, x: DeviceArray, weights, q) -> DeviceArray:
    """xh_weighted_quantile: x (N, C) member-major -> (nq, C) float64."""
    N, C_ = _tc(x)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    if w.shape != (N,):
        raise ValueError(f"weights must have one value per member ({N}), got shape {w.shape}")
    out = dev.empty((len(q), C_), np.float64)
    dev.call("xh_weighted_quantile", _vp(x.ptr), N, C_, C_, 1, np_ptr(w), np_ptr(q), len(q), _vp(out.ptr))
    return out


def percentile_doy(dev: Device, x: DeviceArray, tbase, window: int, per, alpha=1.0 / 3, beta=1.0 / 3,
                   out=None, vmap=None) -> DeviceArray:
    """Returns (nper, ndoy, C) float64 — percentile_doy before the 366-day adjustment.

    `vmap` (int32[Tv], optional): virtual-day -> physical-row table; `tbase` then indexes virtual days.  A float64 field
    takes xh_percentile_doy_f64 (no virtual axis: bootstrap is not served for float64)."""
    T, C_, f64 = _field(x)
    if f64 and vmap is not None:
        capi.refuse_float64("percentile_doy(bootstrap)")
    if f64 and np.shape(tbase)[0] * int(window) > 4096:  # xh_percentile_doy_f64 gathers <= 4096 samples per (doy, cell)
        capi.refuse_float64(f"percentile_doy({np.shape(tbase)[0]} years x window {window} > 4096 samples)")
    tb = np.ascontiguousarray(tbase, dtype=np.int32)
    nyears, ndoy = tb.shape
    per = np.ascontiguousarray(np.atleast_1d(per), dtype=np.float64)
    out = out if out is not None else dev.empty((len(per), ndoy, C_), np.float64)
    if vmap is None:
        dev.call("xh_percentile_doy_f64" if f64 else "xh_percentile_doy", _vp(x.ptr), T, C_, C_, 1, np_ptr(tb), nyears, ndoy, int(window), np_ptr(per), len(per),
                 float(alpha), float(beta), _vp(out.ptr))
    else:
        vm = np.ascontiguousarray(vmap, dtype=np.int32)
        dev.call("xh_percentile_doy_mapped", _vp(x.ptr), T, C_, C_, 1, np_ptr(tb), nyears, ndoy, int(window), np_ptr(per),
                 len(per), float(alpha), float(beta), np_ptr(vm), len(vm), _vp(out.ptr))
    return out


def percentile_doy_count(dev: Device, x: DeviceArray, tbase, window: int, per: float, op: str, doy_period, P: int,
                         alpha=1.0 / 3, beta=1.0 / 3, want_valid=True, out=None):
    """Fused percentile_doy + threshold_count (xh_percentile_doy_count): (count, valid) int32 (P, C), or None when the
    shape is not covered by the fused kernel (the caller then runs the two-step chain)."""
    from ._capi import XH_ERR_NOTIMPL, XclimHipError

    T, C_ = _tc(x)
    tb = np.ascontiguousarray(tbase, dtype=np.int32)
    nyears, ndoy = tb.shape
    dp = np.ascontiguousarray(doy_period, dtype=np.int32).reshape(-1)
    assert dp.shape == (nyears * ndoy,)  # period of every (year, doy) day, < 0 where the day is absent
    if out is not None:
        cnt, val = out
    else:
        cnt = dev.empty((int(P), C_), np.int32)
        val = dev.empty((int(P), C_), np.int32) if want_valid else None
    try:
        dev.call("xh_percentile_doy_count", _vp(x.ptr), T, C_, C_, 1, np_ptr(tb), nyears, ndoy, int(window), float(per),
                 float(alpha), float(beta), op_code(op), np_ptr(dp), int(P), _vp(cnt.ptr), _vp(val.ptr if val else 0))
    except XclimHipError as e:
        if e.code == XH_ERR_NOTIMPL:
            return None
        raise
    return cnt, val


def doy_interp(dev: Device, table: DeviceArray, i0, i1, dxn, dxs, xsrc=None) -> DeviceArray:
    """table (D_in, C) float64 -> (D_out, C) float64 (xh_doy_interp).  `xsrc`: dayofyear coordinate of the source rows for
    the interpolate_na step (None: uniform)."""
    D_in, C_ = _tc(table, np.float64)
    xs = None if xsrc is None else np.ascontiguousarray(xsrc, dtype=np.float64)
    assert xs is None or len(xs) == D_in
    i0 = np.ascontiguousarray(i0, dtype=np.int32)
    i1 = np.ascontiguousarray(i1, dtype=np.int32)
    dxn = np.ascontiguousarray(dxn, dtype=np.float64)
    dxs = np.ascontiguousarray(dxs, dtype=np.float64)
    out = dev.empty((len(i0), C_), np.float64)
    dev.call("xh_doy_interp", _vp(table.ptr), D_in, C_, np_ptr(i0), np_ptr(i1), np_ptr(dxn), np_ptr(dxs), len(i0),
             _vp(out.ptr), np_ptr(xs) if xs is not None else _vp(0))
    return out


def doy_broadcast(dev: Device, table: DeviceArray, tidx) -> DeviceArray:
    """(D, C) float64 per-doy table -> (T, C) float64 field, row tidx[t] at step t (resample_doy)."""
    D, C_ = table.shape
    tidx = np.ascontiguousarray(tidx, dtype=np.int32)
    out = dev.empty((len(tidx), C_), np.float64)
    dev.call("xh_doy_broadcast", _vp(table.ptr), D, C_, np_ptr(tidx), len(tidx), _vp(out.ptr))
    return out


def within_bnds_doy(dev: Device, x: DeviceArray, low: DeviceArray, high: DeviceArray, tidx) -> DeviceArray:
    T, C_ = _tc(x)
    D = low.shape[0]
    tidx = np.ascontiguousarray(tidx, dtype=np.int32)
    assert len(tidx) == T and low.shape == high.shape == (D, C_)
    out = dev.empty((T, C_), np.uint8)
    dev.call("xh_within_bnds_doy", _vp(x.ptr), T, C_, C_, 1, _vp(low.ptr), _vp(high.ptr), D, np_ptr(tidx), _vp(out.ptr))
    return out


def compare_doy(dev: Device, x: DeviceArray, op: str, table: DeviceArray, tidx) -> DeviceArray:
    """float32 1/0 mask of x[t] op table[tidx[t]] (fp64 compare, (D, C) float64 per-doy table)."""
    _f32_only(x, "compare against a per-cell or per-doy threshold (resample after run length)")
    T, C_ = _tc(x)
    D = table.shape[0]
    tidx = np.ascontiguousarray(tidx, dtype=np.int32)
    assert len(tidx) == T and table.shape == (D, C_)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_compare_doy", _vp(x.ptr), T, C_, C_, 1, op_code(op), _vp(table.ptr), D, np_ptr(tidx), _vp(out.ptr), C_)
    return out


def run_stats_doy(dev: Device, x: DeviceArray, op: str, table: DeviceArray, tidx, stat: str, window: int, seg_off, want_valid=True):
    """xh_run_stats_doy: run statistics (cut at the period edges) of x[t] op table[tidx[t]]; table (D, C) float64."""
    T, C_, f64 = _field(x)
    D = table.shape[0]
    tidx = np.ascontiguousarray(tidx, dtype=np.int32)
    assert len(tidx) == T and table.shape == (D, C_) and table.dtype == np.float64
    seg, P = _seg(seg_off)
    out = dev.empty((P, C_), np.float32)
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    dev.call("xh_run_stats_doy_f64" if f64 else "xh_run_stats_doy", _vp(x.ptr), T, C_, C_, 1, op_code(op), _vp(table.ptr), D, np_ptr(tidx), int(window), RUN_STATS[stat],
             np_ptr(seg), P, _vp(out.ptr), _vp(valid.ptr if valid else 0))
    return out, valid


def precip_over_doy(dev: Device, x: DeviceArray, op: str, thr: float, table: DeviceArray, tidx, seg_off, want=("count",),
                    want_valid=True):
    """xh_precip_over_doy: (count | frac | both, valid) against max(table[tidx[t]], thr); table (D, C) float64."""
    T, C_ = _tc(x)
    D = table.shape[0]
    tidx = np.ascontiguousarray(tidx, dtype=np.int32)
    assert len(tidx) == T and table.shape == (D, C_) and table.dtype == np.float64
    seg, P = _seg(seg_off)
    cnt = dev.empty((P, C_), np.int32) if "count" in want else None
    frac = dev.empty((P, C_), np.float32) if "frac" in want else None
    valid = dev.empty((P, C_), np.int32) if want_valid else None
    dev.call("xh_precip_over_doy", _vp(x.ptr), T, C_, C_, 1, op_code(op), float(thr), _vp(table.ptr), D, np_ptr(tidx), np_ptr(seg),
             P, _vp(frac.ptr if frac else 0), _vp(cnt.ptr if cnt else 0), _vp(valid.ptr if valid else 0))
    return cnt, frac, valid


def quantile_series(dev: Device, x: DeviceArray, q, time_axis=0, out=None) -> DeviceArray:
    """Per-cell quantiles of the whole series: x (T, C) [time_axis 0] or (C, T) [time_axis 1] -> (nq, C) float32."""
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    if time_axis == 0:
        T, C_ = _tc(x)
        st, sc = C_, 1
    else:
        C_, T = _tc(x)
        st, sc = 1, T
    if out is None:
        out = dev.empty((len(q), C_), np.float32)
    dev.call("xh_quantile_series", _vp(x.ptr), T, C_, st, sc, np_ptr(q), len(q), _vp(out.ptr))
    return out


def eqm_train(dev: Device, ref: DeviceArray, hist: DeviceArray, q, kind="+", time_axis=0, out=None):
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    if time_axis == 0:
        T, C_ = _tc(ref)
        st, sc = C_, 1
    else:
        C_, T = _tc(ref)
        st, sc = 1, T
    if out is not None:
        af, hq = out
    else:
        af = dev.empty((len(q), C_), np.float32)
        hq = dev.empty((len(q), C_), np.float32)
    dev.call("xh_eqm_train", _vp(ref.ptr), _vp(hist.ptr), T, C_, st, sc, np_ptr(q), len(q), {"+": 0, "*": 1}[kind],
             _vp(af.ptr), _vp(hq.ptr))
    return af, hq


def eqm_train_window(dev: Device, ref: DeviceArray, hist: DeviceArray, rows0, enter, leave, q, kind="+", out=None, normalised=False):
    """xh_eqm_train_window: EQM training over a sliding row sample (day-of-year groups with a window).  rows0 (n0,): the time
    steps of the first group's sample; enter / leave (G - 1, per): the steps that enter / leave from one group to the next (-1 =
    none).  Returns (af, hist_q) as (G, nq, C) device arrays, or None when the kernel does not take the shape (the caller
    gathers every group's sample and calls :func:`eqm_train`).  ``normalised=True`` (xh_dqm_train_window, the training of a
    detrended quantile mapping): the quantiles of the samples divided by / shifted by their own means; returns (af, hist_q,
    scaling, mu_hist), the last two (G, C) float64 (``out`` then holds four arrays)."""
    from ._capi import XH_ERR_NOTIMPL, XclimHipError

    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    T, C_ = _tc(ref)
    rows0 = np.ascontiguousarray(rows0, dtype=np.int32)
    enter = np.ascontiguousarray(enter, dtype=np.int32).reshape(-1, enter.shape[-1] if np.ndim(enter) == 2 else 1)
    leave = np.ascontiguousarray(leave, dtype=np.int32).reshape(enter.shape)
    G, per = enter.shape[0] + 1, enter.shape[1]
    if out is not None:
        af, hq = out[:2]
    else:
        af = dev.empty((G, len(q), C_), np.float32)
        hq = dev.empty((G, len(q), C_), np.float32)
    res, extra, name = (af, hq), (), "xh_eqm_train_window"
    if normalised:
        # xh_dqm_train_window: the samples normalised by their own means (dqm_train); + scaling, mu_hist (G, C) float64
        sc, muh = out[2:4] if out is not None else (dev.empty((G, C_), np.float64), dev.empty((G, C_), np.float64))
        res, extra, name = (af, hq, sc, muh), (_vp(sc.ptr), _vp(muh.ptr)), "xh_dqm_train_window"
    try:
        dev.call(name, _vp(ref.ptr), _vp(hist.ptr), T, C_, C_, np_ptr(rows0), len(rows0), np_ptr(enter), np_ptr(leave),
                 G, per, np_ptr(q), len(q), {"+": 0, "*": 1}[kind], _vp(af.ptr), _vp(hq.ptr), *extra)
    except XclimHipError as e:
        if e.code == XH_ERR_NOTIMPL:
            return None
        raise
    return res


def eqm_train_groups(dev: Device, ref: DeviceArray, hist: DeviceArray, rows, offs, q, kind="+", normalised=False):
    """xh_eqm_train_groups / xh_dqm_train_groups: the training of ALL (small) groups in one launch per field — rows: the row
    numbers group after group, offs (G + 1).  Returns (af, hist_q) (G, nq, C) — with ``normalised`` (dqm_train: the samples
    normalised by their group's mean) also (scaling, mu_hist) (G, C) float64 — or None when a group has more than 64 rows
    (gather each group and call :func:`eqm_train`)."""
    from ._capi import XH_ERR_NOTIMPL, XclimHipError

    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    T, C_ = _tc(ref)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    G = len(offs) - 1
    if int(np.diff(offs).max(initial=0)) > 64:
        return None
    af = dev.empty((G, len(q), C_), np.float32)
    hq = dev.empty((G, len(q), C_), np.float32)
    res, extra, name = (af, hq), (), "xh_eqm_train_groups"
    if normalised:
        sc, muh = dev.empty((G, C_), np.float64), dev.empty((G, C_), np.float64)
        res, extra, name = (af, hq, sc, muh), (_vp(sc.ptr), _vp(muh.ptr)), "xh_dqm_train_groups"
    try:
        dev.call(name, _vp(ref.ptr), _vp(hist.ptr), T, C_, C_, np_ptr(rows), np_ptr(offs), G, np_ptr(q), len(q), {"+": 0, "*": 1}[kind],
                 _vp(af.ptr), _vp(hq.ptr), *extra)
    except XclimHipError as e:
        if e.code == XH_ERR_NOTIMPL:
            return None
        raise
    return res


def eqm_adjust(dev: Device, sim: DeviceArray, af: DeviceArray, hist_q: DeviceArray, kind="+", interp="nearest",
               extrapolation="constant", out: DeviceArray | None = None) -> DeviceArray:
    T, C_ = _tc(sim)
    nq = int(af.shape[0])
    scen = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_eqm_adjust", _vp(sim.ptr), T, C_, C_, 1, _vp(af.ptr), _vp(hist_q.ptr), nq, {"+": 0, "*": 1, "factor": 2}[kind],
             {"nearest": 0, "linear": 1, "cubic": 2}[interp], {"constant": 0, "nan": 1}[extrapolation], _vp(scen.ptr), C_)
    return scen


def mask_doy_cells(dev: Device, x: DeviceArray, doy, start: DeviceArray, end: DeviceArray) -> DeviceArray:
    """xh_mask_doy_cells: x where doy[t] is inside the cell's [start, end] (wrapping when start > end), NaN elsewhere."""
    T, C_ = _tc(x)
    d = np.ascontiguousarray(doy, dtype=np.int32)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_mask_doy_cells", _vp(x.ptr), T, C_, C_, 1, np_ptr(d), _vp(start.ptr), _vp(end.ptr), _vp(out.ptr), C_)
    return out


def mask_days_cells(dev: Device, x: DeviceArray, seg_off, lo: DeviceArray, hi: DeviceArray) -> DeviceArray:
    """xh_mask_days_cells: x where lo[p, c] <= t - seg_off[p] <= hi[p, c] (p = the period of step t), NaN elsewhere."""
    T, C_ = _tc(x)
    seg, P = _seg(seg_off)
    assert lo.shape == (P, C_) and hi.shape == (P, C_)
    out = dev.empty((T, C_), np.float32)
    dev.call("xh_mask_days_cells", _vp(x.ptr), T, C_, C_, 1, np_ptr(seg), P, _vp(lo.ptr), _vp(hi.ptr), _vp(out.ptr), C_)
    return out


def poly_trend(dev: Device, x: DeviceArray, degree: int = 1, u: DeviceArray | None = None):
    """xh_poly_trend: (p0, p1) float64 (C,) device arrays of the per-cell trend p0 + p1 (t - (T - 1) / 2); p1 None for degree 0.
    ``u`` (device float64, T): the rows' own coordinate instead of the centred row number (xh_poly_trend_u)."""
    T, C_ = _tc(x)
    p0 = dev.empty((C_,), np.float64)
    p1 = dev.empty((C_,), np.float64) if degree >= 1 else None
    if u is None:
        dev.call("xh_poly_trend", _vp(x.ptr), T, C_, C_, 1, int(degree), _vp(p0.ptr), _vp(p1.ptr if p1 else 0), _vp(0))
    else:
        dev.call("xh_poly_trend_u", _vp(x.ptr), T, C_, C_, 1, int(degree), _vp(u.ptr), _vp(p0.ptr), _vp(p1.ptr if p1 else 0), _vp(0))
    return p0, p1


def window_nanmean(dev: Device, x: DeviceArray, window: int, out: DeviceArray | None = None) -> DeviceArray:
    """xh_window_nanmean: the centred ``window``-step mean over the valid samples (the ends of the series see fewer rows)."""
    T, C_ = _tc(x)
    out = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_window_nanmean", _vp(x.ptr), T, C_, C_, 1, int(window), _vp(out.ptr), C_)
    return out


def trend_apply(dev: Device, x: DeviceArray, p0: DeviceArray, p1, op: str, out: DeviceArray | None = None,
                u: DeviceArray | None = None) -> DeviceArray:
    """xh_trend_apply: x OP (p0[c] + p1[c] (t - (T - 1) / 2)), op in "+", "-", "*", "/"; p1 None: per-cell constant.
    ``u``: the rows' own coordinate (xh_trend_apply_u)."""
    T, C_ = _tc(x)
    out = out if out is not None else dev.empty((T, C_), np.float32)
    mode = {"+": 0, "-": 1, "*": 2, "/": 3}[op]
    if u is None:
        dev.call("xh_trend_apply", _vp(x.ptr), T, C_, C_, 1, _vp(p0.ptr), _vp(p1.ptr if p1 is not None else 0), mode, _vp(out.ptr), C_)
    else:
        dev.call("xh_trend_apply_u", _vp(x.ptr), T, C_, C_, 1, _vp(u.ptr), _vp(p0.ptr), _vp(p1.ptr if p1 is not None else 0), mode,
                 _vp(out.ptr), C_)
    return out


def qdm_adjust_groups(dev: Device, sim: DeviceArray, rows, offs, af_all: DeviceArray, q, kind="+", interp="nearest",
                      extrapolation="constant", out: DeviceArray | None = None):
    """xh_qdm_adjust_groups: QDM adjust of every (small) group of rows in one launch — rows: the row numbers group after group,
    offs (G + 1), af_all (G, nq, C).  Returns scen (T, C) (rows in no group keep what ``out`` held), or None when the kernel does
    not take the shape (a group of more than 64 rows, more than 32 nodes): gather each group and call :func:`qdm_adjust`."""
    from ._capi import XH_ERR_NOTIMPL, XclimHipError

    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    if interp not in ("nearest", "linear"):
        return None
    T, C_ = _tc(sim)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    if int(np.diff(offs).max(initial=0)) > 64 or len(q) > 32:
        return None
    scen = out if out is not None else dev.empty((T, C_), np.float32)
    try:
        dev.call("xh_qdm_adjust_groups", _vp(sim.ptr), T, C_, C_, np_ptr(rows), np_ptr(offs), len(offs) - 1, _vp(af_all.ptr), np_ptr(q), len(q),
                 {"+": 0, "*": 1, "factor": 2}[kind], {"nearest": 0, "linear": 1}[interp], {"constant": 0, "nan": 1}[extrapolation],
                 _vp(scen.ptr), C_)
    except XclimHipError as e:
        if e.code == XH_ERR_NOTIMPL:
            return None
        raise
    return scen


def poly_trend_groups(dev: Device, x: DeviceArray, rows, offs, u: DeviceArray, degree: int = 1):
    """xh_poly_trend_groups: the per-cell trend of every GROUP of rows in one launch.  rows: the row numbers group after group,
    offs (G + 1): where each group's rows start, u (device float64, T): the coordinate of every row.  (p0, p1): (G, C) float64
    device arrays (p1 None for degree 0)."""
    T, C_ = _tc(x)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    G = len(offs) - 1
    p0 = dev.empty((G, C_), np.float64)
    p1 = dev.empty((G, C_), np.float64) if degree >= 1 else None
    dev.call("xh_poly_trend_groups", _vp(x.ptr), T, C_, C_, np_ptr(rows), np_ptr(offs), G, _vp(u.ptr), int(degree), _vp(p0.ptr),
             _vp(p1.ptr if p1 is not None else 0))
    return p0, p1


def trend_apply_groups(dev: Device, x: DeviceArray, rows, offs, p0: DeviceArray, p1, op: str, u: DeviceArray | None = None,
                       out: DeviceArray | None = None) -> DeviceArray:
    """xh_trend_apply_groups: x OP (p0[g, c] + p1[g, c] u[t]) for the rows t of every group g (p0, p1: (G, C) float64 device arrays;
    p1 None: a per-group constant).  Rows in no group keep what ``out`` held (a fresh ``out`` is NaN-free only if every row is
    listed)."""
    T, C_ = _tc(x)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    out = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_trend_apply_groups", _vp(x.ptr), T, C_, C_, np_ptr(rows), np_ptr(offs), len(offs) - 1, _vp(u.ptr if u is not None else 0),
             _vp(p0.ptr), _vp(p1.ptr if p1 is not None else 0), {"+": 0, "-": 1, "*": 2, "/": 3}[op], _vp(out.ptr), C_)
    return out


def qdm_adjust(dev: Device, sim: DeviceArray, af: DeviceArray, q, kind="+", interp="nearest", extrapolation="constant",
               time_axis=0, out: DeviceArray | None = None) -> DeviceArray:
    """xh_qdm_adjust: sim (T, C) [time_axis 0] or (C, T) [time_axis 1], af (nq, C), q the nq quantile nodes; scen in the
    layout of sim."""
    q = np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    if interp not in ("nearest", "linear"):
        raise NotImplementedError(f"qdm_adjust: interp={interp!r} (nearest and linear are built)")
    if time_axis == 0:
        T, C_ = _tc(sim)
        st, sc = C_, 1
    else:
        C_, T = _tc(sim)
        st, sc = 1, T
    if int(af.shape[0]) != len(q):
        raise ValueError("qdm_adjust: af must hold one row per quantile node")
    if np.any(np.diff(q) <= 0):
        raise ValueError("qdm_adjust: the quantile nodes must be strictly increasing")
    scen = out if out is not None else dev.empty(tuple(sim.shape), np.float32)
    dev.call("xh_qdm_adjust", _vp(sim.ptr), T, C_, st, sc, _vp(af.ptr), np_ptr(q), len(q), {"+": 0, "*": 1, "factor": 2}[kind],
             {"nearest": 0, "linear": 1}[interp], {"constant": 0, "nan": 1}[extrapolation], _vp(scen.ptr))
    return scen


def quantile_cells(dev: Device, x: DeviceArray, q_cell, time_axis=0) -> DeviceArray:
    """xh_quantile_cells (xsdba.nbutils.vecquantiles): one quantile per cell at its own probability `q_cell` (C float64,
    host or device); x (T, C) [time_axis 0] or (C, T)."""
    if time_axis == 0:
        T, C_ = _tc(x)
        st, sc = C_, 1
    else:
        C_, T = _tc(x)
        st, sc = 1, T
    qd = q_cell if isinstance(q_cell, DeviceArray) else dev.to_device(np.ascontiguousarray(q_cell, dtype=np.float64))
    out = dev.empty((C_,), np.float32)
    dev.call("xh_quantile_cells", _vp(x.ptr), T, C_, st, sc, _vp(qd.ptr), _vp(out.ptr))
    return out


def adapt_freq(dev: Device, sim: DeviceArray, p0_ref, p0_sim, dp0, pth, thresh: float, seed: int = 0, tindex=None, cell0: int = 0,
               out: DeviceArray | None = None) -> DeviceArray:
    """xh_adapt_freq: the value-replacement step of xsdba.processing.adapt_freq on sim (T, C); per-cell P0_ref / P0_sim /
    dP0 (float64) and pth (float32), host or device arrays of C."""
    T, C_ = _tc(sim)

    def up(a, dt):
        return a if isinstance(a, DeviceArray) else dev.to_device(np.ascontiguousarray(a, dtype=dt))

    pr, ps, dp, pt = up(p0_ref, np.float64), up(p0_sim, np.float64), up(dp0, np.float64), up(pth, np.float32)
    ti = None if tindex is None else dev.to_device(np.ascontiguousarray(tindex, dtype=np.int64))
    scen = out if out is not None else dev.empty(tuple(sim.shape), np.float32)
    dev.call("xh_adapt_freq", _vp(sim.ptr), T, C_, C_, 1, _vp(pr.ptr), _vp(ps.ptr), _vp(dp.ptr), _vp(pt.ptr), float(thresh),
             int(seed) & 0xFFFFFFFFFFFFFFFF, _vp(ti.ptr) if ti is not None else None, int(cell0), _vp(scen.ptr))
    return scen


def eqm_adjust_g2d(dev: Device, sim: DeviceArray, af_all: DeviceArray, hq_all: DeviceArray, gcoord: int, kind="+",
                   extrapolation="constant", out: DeviceArray | None = None) -> DeviceArray:
    """xh_eqm_adjust_g2d: the rows of ONE group (coordinate `gcoord` in 1 .. G) adjusted with xsdba's 2-D "nearest" over the
    nodes of all groups; af_all / hq_all (G, nq, C)."""
    n, C_ = _tc(sim)
    G, nq = int(af_all.shape[0]), int(af_all.shape[1])
    scen = out if out is not None else dev.empty((n, C_), np.float32)
    dev.call("xh_eqm_adjust_g2d", _vp(sim.ptr), n, C_, C_, _vp(af_all.ptr), _vp(hq_all.ptr), G, nq, int(gcoord),
             {"+": 0, "*": 1, "factor": 2}[kind], {"constant": 0, "nan": 1}[extrapolation], _vp(scen.ptr), C_)
    return scen


def plane_linear(dev: Device, xnew: DeviceArray, gnew, yq_all: DeviceArray, *, xq_all: DeviceArray | None = None, xq_common=None,
                 base: DeviceArray | None = None, kind="+", out: DeviceArray | None = None) -> DeviceArray:
    """xh_plane_linear: xsdba's 2-D ``interp_on_quantiles(method="linear")`` (Delaunay interpolation over the nodes of all
    groups, constant extrapolation).  xnew (T, C) abscissa of every step, gnew (T) float64 group coordinate (host or
    device), yq_all (G, nq, C) factors, node abscissae ``xq_all`` (G, nq, C) or ``xq_common`` (nq, host: QDM's quantiles);
    ``base`` (T, C): the values the factor is applied to (default xnew); kind "+" | "*" | "factor"."""
    T, C_ = _tc(xnew)
    G, nq = int(yq_all.shape[0]), int(yq_all.shape[1])
    if (xq_all is None) == (xq_common is None):
        raise ValueError("plane_linear: give xq_all or xq_common")
    gd = gnew if isinstance(gnew, DeviceArray) else dev.to_device(np.ascontiguousarray(gnew, dtype=np.float64))
    if int(gd.shape[0]) != T:
        raise ValueError("plane_linear: one group coordinate per time step")
    qc = None if xq_common is None else np.ascontiguousarray(xq_common, dtype=np.float64)
    if qc is not None and len(qc) != nq:
        raise ValueError("plane_linear: xq_common must hold one abscissa per node")
    scen = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_plane_linear", _vp(xnew.ptr), _vp(base.ptr) if base is not None else None, T, C_, C_, _vp(gd.ptr),
             _vp(xq_all.ptr) if xq_all is not None else None, np_ptr(qc) if qc is not None else None, _vp(yq_all.ptr), G, nq,
             {"+": 0, "*": 1, "factor": 2}[kind], _vp(scen.ptr), C_)
    return scen


def plane_nearest(dev: Device, xnew: DeviceArray, gnew, yq_all: DeviceArray, xq_all: DeviceArray, kind="+", extrapolation="constant",
                  out: DeviceArray | None = None) -> DeviceArray:
    """xh_plane_nearest: xsdba's 2-D ``interp_on_quantiles(method="nearest")`` for a month / day-of-year grouping over the
    whole series in one call; gnew (T): the INTEGER group coordinate 1 .. G of every step; yq_all / xq_all (G, nq <= 32, C)."""
    T, C_ = _tc(xnew)
    G, nq = int(yq_all.shape[0]), int(yq_all.shape[1])
    gd = gnew if isinstance(gnew, DeviceArray) else dev.to_device(np.ascontiguousarray(gnew, dtype=np.float64))
    if int(gd.shape[0]) != T:
        raise ValueError("plane_nearest: one group coordinate per time step")
    scen = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_plane_nearest", _vp(xnew.ptr), None, T, C_, C_, _vp(gd.ptr), _vp(xq_all.ptr), None, _vp(yq_all.ptr), G, nq,
             {"+": 0, "*": 1, "factor": 2}[kind], {"constant": 0, "nan": 1}[extrapolation], _vp(scen.ptr), C_)
    return scen


def apply_factor(dev: Device, base: DeviceArray, fac: DeviceArray, kind="+", out: DeviceArray | None = None) -> DeviceArray:
    """xh_apply_factor: base (+|*) fac, two (T, C) float32 fields."""
    T, C_ = _tc(base)
    out = out if out is not None else dev.empty((T, C_), np.float32)
    dev.call("xh_apply_factor", _vp(base.ptr), _vp(fac.ptr), T, C_, C_, C_, {"+": 0, "*": 1}[kind], _vp(out.ptr), C_)
    return out


FIRE_INDEXES = ("DC", "DMC", "FFMC", "ISI", "BUI", "FWI", "DSR")
FIRE_SEASONS = {None: 0, "mask": 1, "WF93": 2, "LA08": 3, "GFWED": 4}
FIRE_DRY = {None: 0, "CFS": 1, "GFWED": 2, "GFWED+SNOW": 3}
FIRE_PARAMS = ("temp_start_thresh", "temp_end_thresh", "snow_thresh", "prec_thresh", "carry_over_fraction",
               "wetting_efficiency_fraction", "dc_start", "dmc_start", "ffmc_start", "dc_dry_factor", "dmc_dry_factor")


def fire_weather(dev: Device, fields: dict, month, lat: DeviceArray | None, starts: dict, indexes, params: dict, *,
                 season_method=None, season_mask: DeviceArray | None = None, overwintering=False, dry_start=None,
                 initial_start_up=True, want_mask=False, want_winter_pr=False):
    """xh_fire_weather.  ``fields``: name -> (T, C) float32 DeviceArray for tas / pr / hurs / sfcWind / snd (the ones the
    request reads); ``month`` host int (T); ``lat`` float64 (C); ``starts``: dc0 / dmc0 / ffmc0 / winter_pr float32 (C)
    DeviceArrays or None; ``indexes``: the (closed) subset of FIRE_INDEXES.  Returns ``{name: DeviceArray}`` with the
    indexes, "season_mask" (uint8) and "winter_pr" when asked for.  Raises NotImplementedError for the forms the kernel does
    not serve (GFWED+SNOW dry starts, GFWED windows over 7 days) and ValueError for an invalid latitude."""
    ref = next(iter(fields.values()))
    T, C_ = _tc(ref)
    for v in fields.values():
        if _tc(v) != (T, C_):
            raise ValueError("fire_weather: every field must have the same (T, C) shape")
    m = np.ascontiguousarray(month, dtype=np.int32)
    if m.shape != (T,):
        raise ValueError(f"fire_weather: month must have {T} entries, got {m.shape}")
    outs = {}
    ptrs = (_vp * 7)()
    for k, name in enumerate(FIRE_INDEXES):
        if name in indexes:
            outs[name] = dev.empty((T, C_), np.float32)
            ptrs[k] = outs[name].ptr
    mask_out = dev.empty((T, C_), np.uint8) if want_mask else None
    wpr_out = dev.empty((C_,), np.float32) if want_winter_pr else None
    p = np.array([float(params[k]) for k in FIRE_PARAMS], dtype=np.float64)

    def ptr(a, dtype, shape):
        if a is None:
            return _vp(0)
        if a.dtype != np.dtype(dtype) or tuple(a.shape) != shape:
            raise TypeError(f"fire_weather: expected {np.dtype(dtype).name} {shape}, got {np.dtype(a.dtype).name} {a.shape}")
        return _vp(a.ptr)

    f = {k: ptr(fields.get(k), np.float32, (T, C_)) for k in ("tas", "pr", "hurs", "sfcWind", "snd")}
    try:
        dev.call("xh_fire_weather", T, C_, C_, f["tas"], f["pr"], f["hurs"], f["sfcWind"], f["snd"], np_ptr(m),
                 ptr(lat, np.float64, (C_,)), ptr(starts.get("dc0"), np.float32, (C_,)), ptr(starts.get("dmc0"), np.float32, (C_,)),
                 ptr(starts.get("ffmc0"), np.float32, (C_,)), ptr(starts.get("winter_pr"), np.float32, (C_,)),
                 ptr(season_mask, np.uint8, (T, C_)), C_, FIRE_SEASONS[season_method], int(params["temp_condition_days"]),
                 int(params["snow_condition_days"]), int(bool(overwintering)), FIRE_DRY[dry_start], int(bool(initial_start_up)),
                 np_ptr(p), ptrs, C_, _vp(mask_out.ptr if mask_out is not None else 0), _vp(wpr_out.ptr if wpr_out is not None else 0))
    except capi.XclimHipError as err:
        if err.code == capi.XH_ERR_NOTIMPL:
            raise NotImplementedError(f"fire_weather: dry_start={dry_start!r} / {season_method} windows of "
                                      f"{params['temp_condition_days']}, {params['snow_condition_days']} days are not served") from None
        if err.msg == "Invalid lat specified.":
            raise ValueError("Invalid lat specified.") from None
        raise
    if mask_out is not None:
        outs["season_mask"] = mask_out
    if wpr_out is not None:
        outs["winter_pr"] = wpr_out
    return outs


def overwintering_dc(dev: Device, last_dc: DeviceArray, winter_pr: DeviceArray, carry_over_fraction, wetting_efficiency_fraction,
                     min_dc) -> DeviceArray:
    """xh_overwintering_dc: element-wise over two float32 device arrays of one shape."""
    if last_dc.shape != winter_pr.shape or last_dc.dtype != np.float32 or winter_pr.dtype != np.float32:
        raise TypeError("overwintering_dc: last_dc and winter_pr must be float32 arrays of one shape")
    out = dev.empty(last_dc.shape, np.float32)
    dev.call("xh_overwintering_dc", _vp(last_dc.ptr), _vp(winter_pr.ptr), last_dc.size, float(carry_over_fraction),
             float(wetting_efficiency_fraction), float(min_dc), _vp(out.ptr))
    return out


PET_DAILY = {"BR65": 0, "HG85": 1, "MB05": 2, "FAO_PM98": 3}
PET_MONTHLY = {"TW48": 4, "DA02": 5}
_PET_FIELDS = ("tasmin", "tasmax", "tas", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind", "pr")


def pet_solar_table(dev: Device, day_angle, lat_deg, solar_constant: float = 1361.0, *, ra: bool = True, dl: bool = False):
    """xh_solar_table.  ``day_angle`` (R) [rad] and ``lat_deg`` (L) host float64 arrays.  Returns ``(ra, dl)``: (R, L)
    float64 DeviceArrays of Ra [J m-2 d-1] and the day length [h], None for the one not requested."""
    da = np.ascontiguousarray(day_angle, dtype=np.float64)
    la = np.ascontiguousarray(lat_deg, dtype=np.float64)
    if da.ndim != 1 or la.ndim != 1:
        raise ValueError("pet_solar_table: day_angle and lat_deg must be 1-D")
    if not (ra or dl):
        raise ValueError("pet_solar_table: no output requested")
    R, L = len(da), len(la)
    o_ra = dev.empty((R, L), np.float64) if ra else None
    o_dl = dev.empty((R, L), np.float64) if dl else None
    d_da, d_la = dev.to_device(da), dev.to_device(la)
    dev.call("xh_solar_table", R, L, _vp(d_da.ptr), _vp(d_la.ptr), float(solar_constant),
             _vp(o_ra.ptr) if ra else _vp(0), _vp(o_dl.ptr) if dl else _vp(0))
    return o_ra, o_dl


def pet_month_table(dev: Device, daily: DeviceArray, seg, kind: int) -> DeviceArray:
    """xh_pet_month_table: (M, L) float64 from the (D, L) daily table; ``seg`` (M + 1) host offsets of the months' days.
    kind 0: mean of day length / 12 over the non-NaN days (TW48); 1: 0.408 x the sum of Ra in MJ (DA02)."""
    D, L = _tc(daily, np.float64)
    s = _offsets("pet_month_table", seg, D, "month")
    if kind not in (0, 1):
        raise ValueError(f"pet_month_table: kind must be 0 or 1, got {kind!r}")
    M = len(s) - 1
    out = dev.empty((M, L), np.float64)
    d_s = dev.to_device(s)  # held until the launch is enqueued: a freed buffer goes back to the pool
    dev.call("xh_pet_month_table", D, L, _vp(daily.ptr), M, _vp(d_s.ptr), int(kind), _vp(out.ptr))
    return out


def _pet_fields(fields: dict, need):
    got = {n: fields[n] for n in _PET_FIELDS if fields.get(n) is not None}
    for n in need:
        if n not in got:
            raise TypeError(f"pet: {n} is needed")
    return (got, *_same_fields("pet", got))


def _pet_lat_idx(dev, lat_idx, C_, L):
    li = np.ascontiguousarray(lat_idx, dtype=np.int32)
    if li.shape != (C_,) or (C_ and (li.min() < 0 or li.max() >= L)):
        raise ValueError(f"pet: lat_idx must be ({C_},) indices into {L} table columns")
    return dev.to_device(li)


def _pet_outs(dev, outputs, rows, C_, got):
    outputs = _subset("pet", outputs, ("pet", "wb"))
    if "wb" in outputs and "pr" not in got:
        raise TypeError("pet: the water budget needs pr")
    return {o: dev.empty((rows, C_), np.float64) for o in outputs}


def pet_daily(dev: Device, method: str, fields: dict, ra: DeviceArray | None = None, lat_idx=None, *,
              peta: float = 0.00516409319477, petb: float = 0.0874972822289, outputs=("pet",)) -> dict:
    """xh_pet_daily.  ``fields``: name -> (T, C) DeviceArray, all float32 or all float64 (tasmin, tasmax, tas, hurs, rsds,
    rsus, rlds, rlus, sfcWind, pr); ``ra`` (T, L) float64 from :func:`pet_solar_table` and ``lat_idx`` (C) host int
    indices into its columns (not used by FAO_PM98).  Returns ``{"pet" | "wb": (T, C) float64 DeviceArray}``
    [kg m-2 s-1]."""
    code = PET_DAILY[method]
    need = {0: ("tasmin", "tasmax"), 1: ("tasmin", "tasmax"), 2: () if fields.get("tas") is not None else ("tasmin", "tasmax"),
            3: ("tasmin", "tasmax", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind")}[code]
    got, T, C_, f64 = _pet_fields(fields, need)
    if code == 2 and "tas" not in got and not {"tasmin", "tasmax"} <= set(got):
        raise TypeError("pet: MB05 needs tas or tasmin and tasmax")
    outs = _pet_outs(dev, outputs, T, C_, got)
    L, d_li = 0, None
    if code != 3:
        T2, L = _tc(ra, np.float64)
        if T2 != T:
            raise ValueError(f"pet_daily: the Ra table has {T2} rows for {T} field rows")
        d_li = _pet_lat_idx(dev, lat_idx, C_, L)
    dev.call("xh_pet_daily", T, C_, C_, code, f64, *(_ptr(got, n) for n in _PET_FIELDS), _vp(ra.ptr) if code != 3 else _vp(0), L,
             _vp(d_li.ptr) if d_li is not None else _vp(0), float(peta), float(petb), _ptr(outs, "pet"), _ptr(outs, "wb"), C_)
    return outs


def pet_monthly(dev: Device, method: str, fields: dict, seg, first_month: int, month_table: DeviceArray, month_seconds,
                lat_idx, *, outputs=("pet",)) -> dict:
    """xh_pet_monthly.  ``fields`` as :func:`pet_daily` (tasmin, tasmax, tas, pr); ``seg`` (M + 1) host offsets of the
    months' rows, ``first_month`` 0..11 the month of year of the first one, ``month_table`` (M, L) float64 from
    :func:`pet_month_table`, ``month_seconds`` (M) host.  Returns ``{"pet" | "wb": (M, C) float64 DeviceArray}``."""
    code = PET_MONTHLY[method]
    need = ("tasmin", "tasmax", "pr") if code == 5 else (() if fields.get("tas") is not None else ("tasmin", "tasmax"))
    got, T, C_, f64 = _pet_fields(fields, need)
    s = _offsets("pet_monthly", seg, T, "month")
    M = len(s) - 1
    M2, L = _tc(month_table, np.float64)
    sec = np.ascontiguousarray(month_seconds, dtype=np.float64)
    if M2 != M or sec.shape != (M,):
        raise ValueError(f"pet_monthly: the month table and seconds must have {M} rows")
    if not 0 <= int(first_month) < 12:
        raise ValueError(f"pet_monthly: first_month must be 0..11, got {first_month!r}")
    outs = _pet_outs(dev, outputs, M, C_, got)
    d_li = _pet_lat_idx(dev, lat_idx, C_, L)
    d_s, d_sec = dev.to_device(s), dev.to_device(sec)
    dev.call("xh_pet_monthly", T, C_, C_, code, f64, *(_ptr(got, n) for n in ("tasmin", "tasmax", "tas", "pr")), M,
             int(first_month), _vp(d_s.ptr), _vp(month_table.ptr), _vp(d_sec.ptr), L, _vp(d_li.ptr), _ptr(outs, "pet"),
             _ptr(outs, "wb"), C_)
    return outs


MCARTHUR_LIMITS = {"xlim": 0, "discrete": 1}
MCARTHUR_N13 = np.array([n ** 1.3 for n in range(1, 21)], dtype=np.float64)  # python's pow, as numba and the reference


def mcarthur(dev: Device, fields: dict, pr_annual: DeviceArray | None = None, kbdi0: DeviceArray | None = None, *,
             outputs=("KBDI", "DF", "FFDI"), lim: int = 0) -> dict:
    """xh_mcarthur.  ``fields``: name -> (T, C) float32 or float64 DeviceArray for pr / tasmax / hurs / sfcWind / smd / df
    (the ones the requested ``outputs`` read; hurs and sfcWind of tasmax's dtype, smd and df of one dtype); ``pr_annual``
    and ``kbdi0`` float64 (C) (kbdi0 None = 0).  DF reads the KBDI of the same launch when both are requested (smd
    otherwise), FFDI the DF of the same launch (df otherwise).  Returns ``{name: (T, C) float64 DeviceArray}``."""
    outputs = _subset("mcarthur", outputs, ("KBDI", "DF", "FFDI"))
    if lim not in (0, 1):
        raise ValueError(f"mcarthur: lim must be 0 (xlim) or 1 (discrete), got {lim!r}")
    k, d, f = "KBDI" in outputs, "DF" in outputs, "FFDI" in outputs
    need = {"pr": k or d, "tasmax": k or f, "hurs": f, "sfcWind": f, "smd": d and not k, "df": f and not d}
    for name, used in need.items():
        if used and fields.get(name) is None:
            raise TypeError(f"mcarthur: {name} is needed for {outputs}")
    got = {n: fields[n] for n, used in need.items() if used}
    # a dtype per group: pr | tasmax, hurs, sfcWind | smd, df; one shape for all
    groups = [{n: got[n] for n in names if n in got} for names in (("pr",), ("tasmax", "hurs", "sfcWind"), ("smd", "df"))]
    tcf = [_same_fields("mcarthur", g) if g else None for g in groups]
    if len({g[:2] for g in tcf if g}) != 1:
        raise ValueError("mcarthur: every field must have the same (T, C) shape")
    T, C_ = next(g[:2] for g in tcf if g)
    pr64, tas64, smd64 = (g[2] if g else 0 for g in tcf)

    def cell(a, name):
        if a is None:
            return _vp(0)
        if np.dtype(a.dtype) != np.float64 or tuple(a.shape) != (C_,):
            raise TypeError(f"mcarthur: {name} must be float64 ({C_},), got {np.dtype(a.dtype).name} {a.shape}")
        return _vp(a.ptr)

    if k and pr_annual is None:
        raise TypeError("mcarthur: KBDI needs pr_annual")
    outs = {o: dev.empty((T, C_), np.float64) for o in outputs}
    dev.call("xh_mcarthur", T, C_, C_, pr64, tas64, smd64, *(_ptr(got, n) for n in need),  # (need: in the order of the arguments)
             cell(pr_annual, "pr_annual") if k else _vp(0), cell(kbdi0, "kbdi0") if k else _vp(0), int(lim),
             np_ptr(MCARTHUR_N13), *(_ptr(outs, o) for o in ("KBDI", "DF", "FFDI")), C_)
    return outs


CHILL_OUTPUTS = ("cp", "cu", "valid")


def _chill_common(dev, who, rows, seg, sel, outputs, allowed):
    outputs = _subset(who, outputs, allowed)
    s, _ = _periods(who, seg, rows)
    sel = _row_selection(who, sel, rows)
    return outputs, s, None if sel is None else dev.to_device(sel)


def chill_hourly(dev: Device, tas: DeviceArray, seg, row_sel=None, *, add_K: float = 0.0, sub_C: float = 273.15,
                 positive_only: bool = False, outputs=("cp",), rows_per_day: int = 24) -> dict:
    """xh_chill_hourly.  ``tas`` (H, C) float32 or float64 DeviceArray, day-major hourly rows; ``seg`` (P + 1) host ROW
    offsets of the periods; ``row_sel`` host bool / uint8 (H) or None.  ``outputs``: a subset of cp, cu, valid ((P, C);
    float64, float64, int32) and delta ((H, C) float64).  Returns ``{name: DeviceArray}``."""
    H, C_, f64 = _same_fields("chill_hourly", {"tas": tas})
    outputs, s, d_sel = _chill_common(dev, "chill_hourly", H, seg, row_sel, outputs, CHILL_OUTPUTS + ("delta",))
    P = len(s) - 1
    outs = {o: dev.empty((H, C_) if o == "delta" else (P, C_), np.int32 if o == "valid" else np.float64) for o in outputs}
    if "delta" in outs and (s[0] != 0 or s[-1] != H):
        raise ValueError("chill_hourly: delta needs periods that cover every row")
    d_s = dev.to_device(s)  # held until the launch is enqueued: a freed buffer goes back to the pool
    dev.call("xh_chill_hourly", H, C_, C_, f64, _vp(tas.ptr), int(rows_per_day), P, _vp(d_s.ptr),
             _vp(d_sel.ptr) if d_sel is not None else _vp(0), float(add_K), float(sub_C), int(bool(positive_only)),
             *(_ptr(outs, o) for o in CHILL_OUTPUTS + ("delta",)), C_)
    return outs


def chill_daily(dev: Device, tasmin: DeviceArray, tasmax: DeviceArray, dl: DeviceArray, lat_idx, seg, day_sel=None, *,
                add_K: float = 0.0, sub_C: float = 273.15, positive_only: bool = False, outputs=("cp",)) -> dict:
    """xh_chill_daily.  ``tasmin`` / ``tasmax`` (D, C) DeviceArrays, both float32 or both float64; ``dl`` (D, L) float64 from
    :func:`pet_solar_table` and ``lat_idx`` (C) host indices into its columns; ``seg`` (P + 1) host DAY offsets; ``day_sel``
    host bool / uint8 (D) or None.  ``outputs``: a subset of cp, cu, valid ((P, C)) and hourly ((24 D, C) float64, the
    hourly temperatures).  Returns ``{name: DeviceArray}``."""
    D, C_, f64 = _same_fields("chill_daily", {"tasmin": tasmin, "tasmax": tasmax})
    D2, L = _tc(dl, np.float64)
    if D2 != D:
        raise ValueError(f"chill_daily: the day-length table has {D2} rows for {D} days")
    outputs, s, d_sel = _chill_common(dev, "chill_daily", D, seg, day_sel, outputs, CHILL_OUTPUTS + ("hourly",))
    P = len(s) - 1
    if "hourly" in outputs and (s[0] != 0 or s[-1] != D):
        raise ValueError("chill_daily: hourly needs periods that cover every day")
    d_li = _pet_lat_idx(dev, lat_idx, C_, L)
    outs = {o: dev.empty((24 * D, C_) if o == "hourly" else (P, C_), np.int32 if o == "valid" else np.float64) for o in outputs}
    d_s = dev.to_device(s)
    dev.call("xh_chill_daily", D, C_, C_, f64, _vp(tasmin.ptr), _vp(tasmax.ptr), _vp(dl.ptr), L, _vp(d_li.ptr), P, _vp(d_s.ptr),
             _vp(d_sel.ptr) if d_sel is not None else _vp(0), float(add_K), float(sub_C), int(bool(positive_only)),
             *(_ptr(outs, o) for o in CHILL_OUTPUTS + ("hourly",)), C_)
    return outs


BIOCLIM_FIELDS = ("tas", "tasmin", "tasmax", "pr")
BIOCLIM_VARS = tuple(f"bio{k}" for k in range(1, 20))
BIOCLIM_WHICH = ("wettest", "driest", "warmest", "coldest")
BIOCLIM_COUNTS = tuple("n_" + f for f in BIOCLIM_FIELDS)


def bioclim(dev: Device, fields: dict, step_off, factor, seg_rows, seg_steps, W: int, *, binned: bool = True,
            kelvin_offset: float = 0.0, cv_scale: float = 1.0, thresh: float = 0.0, outputs=BIOCLIM_VARS) -> dict:
    """xh_bioclim.  ``fields``: name -> (T, C) DeviceArray for tas / tasmin / tasmax / pr (the ones the requested outputs
    read), all float32 or all float64.  Host tables: ``step_off`` (S + 1) first rows of the steps, ``factor`` (T) amount per
    unit of pr, ``seg_rows`` / ``seg_steps`` (P + 1) first row / first step of the periods.  ``outputs``: a subset of
    bio1 .. bio19 ((P, C) float64), wettest / driest / warmest / coldest (the step index of that quarter, int32, -1 without
    one) and n_tas / n_tasmin / n_tasmax / n_pr (rows with a value, int32).  Returns ``{name: DeviceArray}``; one launch."""
    allowed = BIOCLIM_VARS + BIOCLIM_WHICH + BIOCLIM_COUNTS
    unknown = set(outputs) - set(allowed)
    if unknown:
        raise ValueError(f"bioclim: unknown outputs {sorted(unknown)}")
    outputs = _subset("bioclim", outputs, allowed)
    got = {n: fields[n] for n in BIOCLIM_FIELDS if fields.get(n) is not None}
    T, C_, f64 = _same_fields("bioclim", got)
    so = np.ascontiguousarray(step_off, dtype=np.int64)
    fa = np.ascontiguousarray(factor, dtype=np.float64)
    sr = np.ascontiguousarray(seg_rows, dtype=np.int64)
    ss = np.ascontiguousarray(seg_steps, dtype=np.int64)
    if so.ndim != 1 or len(so) < 1 or fa.shape != (T,) or sr.ndim != 1 or sr.shape != ss.shape or len(sr) < 1:
        raise ValueError("bioclim: step_off (S + 1), factor (T), seg_rows and seg_steps (P + 1 each) expected")
    S, P = len(so) - 1, len(sr) - 1
    outs = {o: dev.empty((P, C_), np.float64 if o in BIOCLIM_VARS else np.int32) for o in outputs}

    def table(names):
        arr = (_vp * len(names))()
        for k, n in enumerate(names):
            if n in outs:
                arr[k] = outs[n].ptr
        return arr

    dev.call("xh_bioclim", T, C_, C_, f64, *(_ptr(got, n) for n in BIOCLIM_FIELDS), S,
             np_ptr(so), np_ptr(fa if T else np.zeros(1)), int(bool(binned)), P, np_ptr(sr), np_ptr(ss), int(W), float(kelvin_offset),
             float(cv_scale), float(thresh), table(BIOCLIM_VARS), table(BIOCLIM_WHICH), table(BIOCLIM_COUNTS), C_)
    return outs


SI_DISTS = {"gamma": 0, "fisk": 1}
SI_METHODS = {"APP": 0, "ML": 1}
SI_STAGING = {"auto": 0, "global": 1, "lds": 2}


def si_fit(dev: Device, x: DeviceArray, group, G: int, dist: str, method: str, floc=None, zero_inflated=False,
           staging="auto", want_nfev=False):
    """xh_si_fit: per-(group, cell) fits of a (T, C) float32 field, or float64 (xh_si_fit_f64, read without rounding);
    ``group`` host int (T), -1 = row not used.  Returns ``(params (G, 3, C) float64, nzeros, nnotnull (G, C) float64 or
    None, nfev (G, C) int32 or None)`` as DeviceArrays."""
    T, C_, f64 = _field(x)
    g = np.ascontiguousarray(group, dtype=np.int32)
    if g.shape != (T,):
        raise ValueError(f"si_fit: group must have {T} entries, got {g.shape}")
    params = dev.empty((G, 3, C_), np.float64)
    nz = dev.empty((G, C_), np.float64) if zero_inflated else None
    nn = dev.empty((G, C_), np.float64) if zero_inflated else None
    nfev = dev.empty((G, C_), np.int32) if want_nfev else None
    dev.call("xh_si_fit_f64" if f64 else "xh_si_fit", _vp(x.ptr), T, C_, C_, np_ptr(g), int(G), SI_DISTS[dist],
             SI_METHODS[method], int(floc is not None), float(floc if floc is not None else 0.0), int(bool(zero_inflated)),
             SI_STAGING[staging], _vp(params.ptr), _vp(nz.ptr if nz is not None else 0), _vp(nn.ptr if nn is not None else 0),
             _vp(nfev.ptr if nfev is not None else 0))
    return params, nz, nn, nfev


def si_apply(dev: Device, x: DeviceArray, group, params: DeviceArray, dist: str, nzeros: DeviceArray | None = None,
             nnotnull: DeviceArray | None = None, alpha=0.0, beta=1.0, interp=1.0) -> DeviceArray:
    """xh_si_apply: the standardized index (T, C) float64 of a float32 or float64 field (xh_si_apply_f64) from (G, 3, C)
    float64 parameters; with ``nzeros`` / ``nnotnull`` ((G, C) float64) the zero-inflated mixture."""
    T, C_, f64 = _field(x)
    G = int(params.shape[0])
    if tuple(params.shape) != (G, 3, C_) or np.dtype(params.dtype) != np.float64:
        raise TypeError(f"si_apply: params must be float64 (G, 3, {C_}), got {np.dtype(params.dtype).name} {params.shape}")
    for a in (nzeros, nnotnull):
        if a is not None and (tuple(a.shape) != (G, C_) or np.dtype(a.dtype) != np.float64):
            raise TypeError(f"si_apply: zero counts must be float64 ({G}, {C_})")
    g = np.ascontiguousarray(group, dtype=np.int32)
    if g.shape != (T,):
        raise ValueError(f"si_apply: group must have {T} entries, got {g.shape}")
    out = dev.empty((T, C_), np.float64)
    dev.call("xh_si_apply_f64" if f64 else "xh_si_apply", _vp(x.ptr), T, C_, C_, np_ptr(g), G, _vp(params.ptr),
             _vp(nzeros.ptr if nzeros is not None else 0), _vp(nnotnull.ptr if nnotnull is not None else 0), SI_DISTS[dist],
             float(alpha), float(beta), float(interp), _vp(out.ptr), C_)
    return out


# ---- the agroclimatic heat-sum unit (include/xclim_hip_agro.h, xclim_amd/csrc/agro.hip) ------------------------------
AGRO_DEGREE_OUTPUTS = ("hi", "bedd", "valid")
AGRO_MONTHLY_OUTPUTS = ("cni", "mtwm", "di", "valid")
EGDD_OUTPUTS = ("egdd", "start", "end", "valid")
EGDD_METHODS = {"bootsma": 0, "qian": 1}
AGRO_HEMISPHERES = {None: 0, "north": 1, "south": 2}


def _period_outs(dev, outputs, P, C_):
    return {o: dev.empty((P, C_), np.int32 if o == "valid" else np.float64) for o in outputs}


def _host_table(who, a, dtype, n, what):
    t = np.ascontiguousarray(a, dtype=dtype)
    if t.shape != (n,):
        raise ValueError(f"{who}: {what} must have {n} entries, got {t.shape}")
    return t


def _agro_f64(who, a, shape, what):
    if a is None:
        return None
    if not isinstance(a, DeviceArray) or np.dtype(a.dtype) != np.float64 or tuple(a.shape) != shape:
        raise TypeError(f"{who}: {what} must be a float64 {shape} device array")
    return a


def agro_degree_sum(dev: Device, fields: dict, seg, day_sel=None, *, k_cell: DeviceArray | None = None,
                    k_day: DeviceArray | None = None, k_period: DeviceArray | None = None, lat_idx=None, sub_C: float = 273.15,
                    thresh_hi: float = 10.0, thresh_bedd: float = 10.0, tr_adj: bool = True, low_dtr: float = 10.0,
                    high_dtr: float = 13.0, max_dd: float = 9.0, outputs=("hi", "bedd")) -> dict:
    """xh_agro_degree_sum.  ``fields``: name -> (T, C) DeviceArray, all float32 or all float64: tasmax always, tas for "hi",
    tasmin for "bedd".  ``seg`` (P + 1) host row offsets, ``day_sel`` host bool / uint8 (T) or None.  The day factor: at most
    one of ``k_cell`` (C) and ``k_day`` (T, L); ``k_period`` (P, L) scales the sum; ``lat_idx`` (C) host indices into the L
    columns.  ``outputs``: a subset of hi, bedd ((P, C) float64) and valid (int32).  Returns ``{name: DeviceArray}``."""
    who = "agro_degree_sum"
    outputs = _subset(who, outputs, AGRO_DEGREE_OUTPUTS)
    if not {"hi", "bedd"} & set(outputs):
        raise ValueError(f"{who}: valid comes with hi or bedd")
    need = ["tasmax"] + (["tas"] if "hi" in outputs else []) + (["tasmin"] if "bedd" in outputs else [])
    for n in need:
        if fields.get(n) is None:
            raise TypeError(f"{who}: {n} is needed for {outputs}")
    got = {n: fields[n] for n in need}
    T, C_, f64 = _same_fields(who, got)
    s, P = _periods(who, seg, T)
    sel = _row_selection(who, day_sel, T)
    if k_cell is not None and k_day is not None:
        raise ValueError(f"{who}: at most one day factor (k_cell or k_day)")
    L, d_li = 0, None
    if k_day is not None or k_period is not None:
        L = int((k_day if k_day is not None else k_period).shape[-1])
        d_li = _pet_lat_idx(dev, lat_idx, C_, L)
    k_cell = _agro_f64(who, k_cell, (C_,), "k_cell")
    k_day = _agro_f64(who, k_day, (T, L), "k_day")
    k_period = _agro_f64(who, k_period, (P, L), "k_period")
    outs = _period_outs(dev, outputs, P, C_)
    dev.call("xh_agro_degree_sum", T, C_, C_, f64, *(_ptr(got, n) for n in ("tas", "tasmin", "tasmax")), P, np_ptr(s),
             np_ptr(sel) if sel is not None else _vp(0), *(_vp(a.ptr) if a is not None else _vp(0) for a in (k_cell, k_day, k_period)),
             L, _vp(d_li.ptr) if d_li is not None else _vp(0), float(sub_C), float(thresh_hi), float(thresh_bedd),
             int(bool(tr_adj)), float(low_dtr), float(high_dtr), float(max_dd), *(_ptr(outs, o) for o in AGRO_DEGREE_OUTPUTS), C_)
    return outs


def agro_monthly(dev: Device, fields: dict, month_off, month_cal, month_days, seg_months, *, lat: DeviceArray | None = None,
                 hemisphere: str | None = None, sub_C: float = 273.15, per_day: float = 86400.0, wo: float = 200.0,
                 outputs=("cni", "mtwm", "di")) -> dict:
    """xh_agro_monthly.  ``fields``: name -> (T, C) DeviceArray, one dtype: tasmin for "cni", tas for "mtwm", pr and
    evspsblpot for "di".  Host tables: ``month_off`` (M + 1) first row of every month, ``month_cal`` / ``month_days`` (M),
    ``seg_months`` (P + 1) first month of every period.  ``lat`` (C) float64 DeviceArray, or ``hemisphere`` "north" / "south"
    for every cell.  ``outputs``: a subset of cni, mtwm, di ((P, C) float64) and valid (int32).  Returns ``{name:
    DeviceArray}``; one launch."""
    who = "agro_monthly"
    outputs = _subset(who, outputs, AGRO_MONTHLY_OUTPUTS)
    reads = {"cni": ("tasmin",), "mtwm": ("tas",), "di": ("pr", "evspsblpot")}
    need = [f for o in ("cni", "mtwm", "di") if o in outputs for f in reads[o]]
    if not need:
        raise ValueError(f"{who}: valid comes with cni, mtwm or di")
    for n in need:
        if fields.get(n) is None:
            raise TypeError(f"{who}: {n} is needed for {outputs}")
    got = {n: fields[n] for n in need}
    T, C_, f64 = _same_fields(who, got)
    mo = _offsets(who, month_off, T, "month")
    M = len(mo) - 1
    sm, P = _periods(who, seg_months, M)
    mc = _host_table(who, month_cal, np.int32, M, "month_cal")
    md = _host_table(who, month_days, np.int32, M, "month_days")
    if hemisphere not in AGRO_HEMISPHERES:
        raise ValueError(f"{who}: hemisphere must be None, 'north' or 'south', got {hemisphere!r}")
    if hemisphere is None and {"cni", "di"} & set(outputs):
        lat = _agro_f64(who, lat, (C_,), "lat")
        if lat is None:
            raise TypeError(f"{who}: lat is needed unless hemisphere is given")
    outs = _period_outs(dev, outputs, P, C_)
    one = np.ones(1, np.int32)
    dev.call("xh_agro_monthly", T, C_, C_, f64, *(_ptr(got, n) for n in ("tasmin", "tas", "pr", "evspsblpot")), M, np_ptr(mo),
             np_ptr(mc if M else one), np_ptr(md if M else one), P, np_ptr(sm), _vp(lat.ptr) if lat is not None else _vp(0),
             AGRO_HEMISPHERES[hemisphere], float(sub_C), float(per_day), float(wo), *(_ptr(outs, o) for o in AGRO_MONTHLY_OUTPUTS), C_)
    return outs


def egdd(dev: Device, tasmin: DeviceArray, tasmax: DeviceArray, seg, doy, start_from, end_from, day0, label_doy, label_days, *,
         method: str = "bootsma", sub_C: float = 273.15, thresh: float = 5.0, outputs=("egdd",)) -> dict:
    """xh_egdd.  ``tasmin`` / ``tasmax`` (T, C) DeviceArrays of one dtype.  Host tables: ``seg`` (P + 1) row offsets, ``doy``
    (T) day of year of every row, and per period ``start_from`` / ``end_from`` (row of the date the bound is looked for from,
    -1 = not in the period), ``day0`` (days from the label to the first row), ``label_doy``, ``label_days``.  ``outputs``: a
    subset of egdd, start, end ((P, C) float64) and valid (int32).  Returns ``{name: DeviceArray}``."""
    who = "egdd"
    outputs = _subset(who, outputs, EGDD_OUTPUTS)
    if outputs == ["valid"]:
        raise ValueError(f"{who}: valid comes with egdd, start or end")
    if method not in EGDD_METHODS:
        raise NotImplementedError(f"Method: {method}.")
    T, C_, f64 = _same_fields(who, {"tasmin": tasmin, "tasmax": tasmax})
    s, P = _periods(who, seg, T)
    d = _host_table(who, doy, np.int32, T, "doy")
    tabs = [_host_table(who, a, dt, P, n) for a, dt, n in ((start_from, np.int64, "start_from"), (end_from, np.int64, "end_from"),
                                                            (day0, np.int64, "day0"), (label_doy, np.int32, "label_doy"),
                                                            (label_days, np.int32, "label_days"))]
    outs = _period_outs(dev, outputs, P, C_)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)  # noqa: E731  (a pointer the entry point may check against NULL)
    dev.call("xh_egdd", T, C_, C_, f64, _vp(tasmin.ptr), _vp(tasmax.ptr), P, np_ptr(s), np_ptr(pad(d)), *(np_ptr(pad(t)) for t in tabs),
             EGDD_METHODS[method], float(sub_C), float(thresh), *(_ptr(outs, o) for o in EGDD_OUTPUTS), C_)
    return outs


def corn_heat_units(dev: Device, tasmin: DeviceArray, tasmax: DeviceArray, *, sub_C: float = 273.15, thresh_tasmin: float = 4.44,
                    thresh_tasmax: float = 10.0) -> DeviceArray:
    """xh_corn_heat_units: (T, C) float64 from two fields of one dtype; thresholds in degC."""
    T, C_, f64 = _same_fields("corn_heat_units", {"tasmin": tasmin, "tasmax": tasmax})
    out = dev.empty((T, C_), np.float64)
    dev.call("xh_corn_heat_units", T, C_, C_, f64, _vp(tasmin.ptr), _vp(tasmax.ptr), float(sub_C), float(thresh_tasmin),
             float(thresh_tasmax), _vp(out.ptr), C_)
    return out


def qian_wma(dev: Device, tas: DeviceArray) -> DeviceArray:
    """xh_qian_wma: the five-day binomial mean (T, C) float64 of a float32 or float64 field, NaN within 2 rows of the ends."""
    T, C_, f64 = _same_fields("qian_wma", {"tas": tas})
    out = dev.empty((T, C_), np.float64)
    dev.call("xh_qian_wma", T, C_, C_, f64, _vp(tas.ptr), _vp(out.ptr), C_)
    return out


# ---- the streamflow and snow-melt unit (include/xclim_hip_hydro.h, xclim_amd/csrc/hydro.hip) -------------------------
FLOW_OUTPUTS = ("bfi", "rbi", "mean", "sum", "valid")
SEN_OUTPUTS = ("slope", "p", "n")


def _hydro_window(who, window):
    if not isinstance(window, (int, np.integer)) or isinstance(window, bool) or window < 1:
        raise ValueError(f"{who}: window must be an integer of at least 1, got {window!r}")
    if window > capi.HYDRO_MAX_WINDOW:
        raise ValueError(f"{who}: windows of up to {capi.HYDRO_MAX_WINDOW} rows are served, got {window}")
    return int(window)


def flow_period_stats(dev: Device, q: DeviceArray, seg, outputs=("bfi", "rbi")) -> dict:
    """xh_flow_period_stats.  ``q`` (T, C) float32 or float64 DeviceArray, ``seg`` (P + 1) host row offsets.  ``outputs``: a
    subset of bfi, rbi, mean, sum ((P, C) float64) and valid (int32).  Returns ``{name: DeviceArray}``; one launch."""
    who = "flow_period_stats"
    outputs = _subset(who, outputs, FLOW_OUTPUTS)
    T, C_, f64 = _same_fields(who, {"q": q})
    s, P = _periods(who, seg, T)
    outs = _period_outs(dev, outputs, P, C_)
    dev.call("xh_flow_period_stats", T, C_, C_, f64, _vp(q.ptr), P, np_ptr(s), *(_ptr(outs, o) for o in FLOW_OUTPUTS), C_)
    return outs


def melt_period_max(dev: Device, snw: DeviceArray, seg, pr: DeviceArray | None = None, *, window: int = 3,
                    per_day: float = 86400.0) -> DeviceArray:
    """xh_melt_period_max: the period maximum of the ``window``-row sums of ``pr * per_day - diff(snw)`` (without ``pr``: of
    ``-diff(snw)``), (P, C) float64.  ``snw`` / ``pr`` (T, C) DeviceArrays of one dtype."""
    who = "melt_period_max"
    T, C_, f64 = _same_fields(who, {"snw": snw, "pr": pr} if pr is not None else {"snw": snw})
    s, P = _periods(who, seg, T)
    window = _hydro_window(who, window)
    out = dev.empty((P, C_), np.float64)
    dev.call("xh_melt_period_max", T, C_, C_, f64, _vp(snw.ptr), _vp(pr.ptr) if pr is not None else _vp(0), float(per_day), window, P,
             np_ptr(s), _vp(out.ptr), C_)
    return out


def antecedent_precip(dev: Device, pr: DeviceArray, weights, *, per_day: float = 86400.0) -> DeviceArray:
    """xh_antecedent_precip: the trailing weighted sum ``sum_k weights[k] * (pr[i - window + 1 + k] * per_day)`` with
    ``window = len(weights)``, (T, C) float64, NaN until the window is full."""
    who = "antecedent_precip"
    T, C_, f64 = _same_fields(who, {"pr": pr})
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError(f"{who}: weights must be one-dimensional")
    window = _hydro_window(who, len(w))
    out = dev.empty((T, C_), np.float64)
    dev.call("xh_antecedent_precip", T, C_, C_, f64, _vp(pr.ptr), float(per_day), window, np_ptr(w), _vp(out.ptr), C_)
    return out


def sen_slope(dev: Device, x: DeviceArray, period_of, outputs=("slope", "p")) -> dict:
    """xh_sen_slope.  ``x`` (P, C) float32 or float64 DeviceArray of period values; ``period_of`` host int (Y, K): the row of
    ``x`` of year y of season k, -1 for none.  ``outputs``: a subset of slope, p ((K, C) float64) and n (int32, the values
    used).  Returns ``{name: DeviceArray}``; one launch."""
    who = "sen_slope"
    outputs = _subset(who, outputs, SEN_OUTPUTS)
    if outputs == ["n"]:
        raise ValueError(f"{who}: n comes with slope or p")
    P, C_, f64 = _same_fields(who, {"x": x})
    po = np.ascontiguousarray(period_of, dtype=np.int64)
    if po.ndim != 2:
        raise ValueError(f"{who}: period_of must be a (years, seasons) table")
    Y, K_ = po.shape
    if Y > capi.SEN_MAX_YEARS:
        raise ValueError(f"{who}: series of up to {capi.SEN_MAX_YEARS} years are served, got {Y}")
    if po.size and (po.min() < -1 or po.max() >= P):
        raise ValueError(f"{who}: period_of must hold rows of x (0 .. {P - 1}) or -1")
    outs = {o: dev.empty((K_, C_), np.int32 if o == "n" else np.float64) for o in outputs}
    dev.call("xh_sen_slope", P, C_, C_, f64, _vp(x.ptr), Y, K_, np_ptr(po if po.size else np.full(1, -1, np.int64)),
             *(_ptr(outs, o) for o in SEN_OUTPUTS), C_)
    return outs


# ---- the rain-season and hardiness-zone unit (include/xclim_hip_rain.h, xclim_amd/csrc/rainseason.hip) ---------------
RAIN_OUTPUTS = ("start", "end", "length")
RAIN_METHODS = ("per_day", "total")


def _rain_window(who, name, window, least=1):
    if not isinstance(window, (int, np.integer)) or isinstance(window, bool) or window < least:
        raise ValueError(f"{who}: {name} must be an integer of at least {least}, got {window!r}")
    return int(window)


def rain_season(dev: Device, pr: DeviceArray, seg, flags, doy, *, per_day: float = 86400.0, thresh_wet_start: float = 25.0,
                window_wet_start: int = 3, window_not_dry_start: int = 30, thresh_dry_start: float = 1.0, window_dry_start: int = 7,
                method_dry_start: str = "per_day", thresh_dry_end: float = 0.0, window_dry_end: int = 20,
                method_dry_end: str = "per_day", outputs=RAIN_OUTPUTS) -> dict:
    """xh_rain_season.  ``pr`` (T, C) float32 or float64 DeviceArray, ``seg`` (P + 1) host row offsets, ``flags`` host uint8 (T)
    of the ``capi.RAIN_*`` bits, ``doy`` host int (T).  Thresholds in mm per day of ``pr * per_day``.  ``outputs``: a subset of
    start, end (day of year) and length (days), (P, C) float64 with NaN.  Returns ``{name: DeviceArray}``; one launch."""
    who = "rain_season"
    outputs = _subset(who, outputs, RAIN_OUTPUTS)
    T, C_, f64 = _same_fields(who, {"pr": pr})
    s, P = _periods(who, seg, T)
    for name, m in (("method_dry_start", method_dry_start), ("method_dry_end", method_dry_end)):
        if m not in RAIN_METHODS:
            raise ValueError(f"Unknown {name}: {m}.")
    ww = _rain_window(who, "window_wet_start", window_wet_start)
    wnd = _rain_window(who, "window_not_dry_start", window_not_dry_start, 0)
    wd = _rain_window(who, "window_dry_start", window_dry_start)
    we = _rain_window(who, "window_dry_end", window_dry_end)
    sums = [ww] + [w for w, m in ((wd, method_dry_start), (we, method_dry_end)) if m == "total"]
    if max(sums) > capi.RAIN_MAX_WINDOW:
        raise ValueError(f"{who}: sum windows of up to {capi.RAIN_MAX_WINDOW} rows are served, got {max(sums)}")
    fl = _host_table(who, flags, np.uint8, T, "flags")
    dy = _host_table(who, doy, np.int32, T, "doy")
    outs = {o: dev.empty((P, C_), np.float64) for o in outputs}
    dev.call("xh_rain_season", T, C_, C_, f64, _vp(pr.ptr), float(per_day), P, np_ptr(s), np_ptr(fl), np_ptr(dy), float(thresh_wet_start), ww,
             wnd, float(thresh_dry_start), wd, int(method_dry_start == "total"), float(thresh_dry_end), we, int(method_dry_end == "total"),
             *(_ptr(outs, o) for o in RAIN_OUTPUTS), C_)
    return outs


def rolling_zones(dev: Device, x: DeviceArray, window: int, edges) -> DeviceArray:
    """xh_rolling_zones: the zone (``np.digitize(mean, edges) - 1``, the last zone closed on the right, NaN outside the edges) of
    the mean of the last ``window`` rows of ``x`` (P, C) float32 or float64; (P, C) float64, NaN for the first ``window - 1``
    rows."""
    who = "rolling_zones"
    P, C_, f64 = _same_fields(who, {"x": x})
    window = _rain_window(who, "window", window)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    if e.ndim != 1 or len(e) < 2 or not np.all(np.diff(e) > 0):
        raise ValueError(f"{who}: at least two strictly increasing bin edges")
    if len(e) > capi.ZONES_MAX_EDGES:
        raise ValueError(f"{who}: at most {capi.ZONES_MAX_EDGES} bin edges, got {len(e)}")
    out = dev.empty((P, C_), np.float64)
    dev.call("xh_rolling_zones", P, C_, C_, f64, _vp(x.ptr), window, len(e), np_ptr(e), _vp(out.ptr), C_)
    return out


# ---- the data-quality-flag unit (include/xclim_hip_flags.h, xclim_amd/csrc/dataflags.hip) ----------------------------
FLAG_KINDS = {"cmp": capi.FLAG_CMP, "outside": capi.FLAG_OUTSIDE, "pair": capi.FLAG_PAIR, "repeat": capi.FLAG_REPEAT, "clim": capi.FLAG_CLIM}


def flag_check(kind: str, op=None, a: float = 0.0, b: float = 0.0, n: int = 0, other: int = 0) -> tuple:
    """One entry of the check list of :func:`data_flags`: ``("cmp", op, a)``, ``("outside", None, a, b)``, ``("pair", op,
    other=0 | 1)``, ``("repeat", op | None, a, n=...)`` or ``("clim",)`` as the tuple ``(kind, op, n, other, a, b)`` of
    ``xh_flag_check``."""
    if kind not in FLAG_KINDS:
        raise ValueError(f"data_flags: unknown check kind {kind!r}")
    code = -1 if op is None else op_code(op)
    if kind == "repeat" and (isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1):
        raise ValueError(f"data_flags: n must be an integer of at least 1, got {n!r}")
    return (FLAG_KINDS[kind], code, int(n), int(other), float(a), float(b))


def data_flags(dev: Device, x: DeviceArray, checks, seg, *, y0: DeviceArray | None = None, y1: DeviceArray | None = None, tidx=None,
               lo: DeviceArray | None = None, hi: DeviceArray | None = None, reduce_cells: bool = False) -> DeviceArray:
    """xh_data_flags.  ``x`` and the companions ``y0`` / ``y1`` (T, C) DeviceArrays of one dtype, ``checks`` a list of
    :func:`flag_check` tuples (at most ``capi.FLAGS_MAX_CHECKS``), ``seg`` (P + 1) host row offsets covering [0, T]; for a
    "clim" check ``tidx`` host int (T) and the bound tables ``lo`` / ``hi`` (D, C) in the fields' dtype.  Returns the uint8
    flags (K, P, C), or (K, P) with ``reduce_cells``; one launch."""
    who = "data_flags"
    fields = {"x": x, **({"y0": y0} if y0 is not None else {}), **({"y1": y1} if y1 is not None else {})}
    T, C_, f64 = _same_fields(who, fields)
    s = _offsets(who, seg, T)
    P = len(s) - 1
    if s[0] != 0 or s[-1] != T:
        raise ValueError(f"{who}: the periods must cover [0, {T}]")
    chk = np.array(list(checks), dtype=capi.FLAG_CHECK_DTYPE).reshape(-1)
    K_ = len(chk)
    if K_ > capi.FLAGS_MAX_CHECKS:
        raise ValueError(f"{who}: at most {capi.FLAGS_MAX_CHECKS} checks in one launch, got {K_}")
    clim = bool((chk["kind"] == capi.FLAG_CLIM).any())
    D = 0
    ti = None
    if clim:
        if lo is None or hi is None or tidx is None:
            raise ValueError(f"{who}: the climatology check needs tidx and both bound tables")
        for t_ in (lo, hi):
            if np.dtype(t_.dtype) != np.dtype(x.dtype) or len(t_.shape) != 2 or t_.shape[1] != C_ or t_.shape != lo.shape:
                raise TypeError(f"{who}: the bound tables must be (D, {C_}) device arrays of the field's dtype")
        D = int(lo.shape[0])
        ti = _host_table(who, tidx, np.int32, T, "tidx")
    out = dev.empty((K_, P) if reduce_cells else (K_, P, C_), np.uint8)
    p = lambda d: _vp(d.ptr) if d is not None else _vp(0)  # noqa: E731
    dev.call("xh_data_flags", T, C_, C_, f64, _vp(x.ptr), p(y0), C_, p(y1), C_, K_, np_ptr(chk) if K_ else _vp(0), P, np_ptr(s),
             np_ptr(ti) if ti is not None else _vp(0), D, p(lo if clim else None), p(hi if clim else None), C_, int(bool(reduce_cells)),
             _vp(out.ptr), C_)
    return out


def doy_bounds(dev: Device, x: DeviceArray, tbase, window: int, n: float):
    """xh_doy_bounds: ``(lo, hi)``, the (ndoy, C) tables ``mean -+ n * std`` of the day-of-year climatology over all years and the
    centred ``window``, in the dtype of ``x`` (T, C) float32 or float64.  ``tbase`` host int (nyears, ndoy) as for
    :func:`doy_mean_std`."""
    who = "doy_bounds"
    T, C_, f64 = _same_fields(who, {"x": x})
    tb = np.ascontiguousarray(tbase, dtype=np.int32)
    if tb.ndim != 2 or tb.shape[0] < 1:
        raise ValueError(f"{who}: tbase must be a (years, days of year) table")
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"{who}: window must be an integer of at least 1, got {window!r}")
    nyears, ndoy = tb.shape
    lo, hi = dev.empty((ndoy, C_), x.dtype), dev.empty((ndoy, C_), x.dtype)
    dev.call("xh_doy_bounds", T, C_, C_, f64, _vp(x.ptr), np_ptr(tb if tb.size else np.full(1, -1, np.int32)), nyears, ndoy, int(window),
             float(n), _vp(lo.ptr), _vp(hi.ptr), C_)
    return lo, hi


# ---- the snow / rain partition unit (include/xclim_hip_phase.h, xclim_amd/csrc/phase.hip) ----------------------------
PHASE_MAP_OUTPUTS = ("snow", "rain")
PHASE_LIMITS = ("snow_low", "snow_high", "snow_thresh", "hplt_pr", "hplt_tas", "rofg_pr", "rofg_frz")


def _phase_partition(who, part: dict, T, C_):
    """The arguments (method, par, tab, ntab, season, land) of a partition ``{"method", "par", "tab", "season", "land"}`` (built by
    :func:`xclim_amd.phase.partition`), with the host arrays that must outlive the call."""
    method = part["method"]
    if method not in capi.PHASE_METHODS:
        raise ValueError(f"{who}: unknown method {method!r}")
    par = _host_table(who, part["par"], np.float64, capi.PHASE_NPAR, "par")
    tab, ntab = part.get("tab"), 0
    if tab is not None:
        tab = np.ascontiguousarray(tab, dtype=np.float64).reshape(-1)
        ntab = len(tab) // 2 if method == "auer" else len(tab)
    season = part.get("season")
    if season is not None:
        season = _host_table(who, season, np.uint8, T, "season")
    land = part.get("land")
    if land is not None and (not isinstance(land, DeviceArray) or np.dtype(land.dtype) != np.uint8 or int(np.prod(land.shape)) != C_):
        raise TypeError(f"{who}: land must be a uint8 device array with one entry per cell")
    keep = (par, tab, season)
    args = (capi.PHASE_METHODS[method], np_ptr(par), np_ptr(tab) if tab is not None else _vp(0), ntab,
            np_ptr(season) if season is not None else _vp(0), _vp(land.ptr) if land is not None else _vp(0))
    return args, keep


def precip_phase_map(dev: Device, pr: DeviceArray, tas: DeviceArray, part: dict, outputs=PHASE_MAP_OUTPUTS) -> dict:
    """xh_precip_phase_map: the snow and / or rain part of every sample of ``pr`` by ``tas`` (T, C), both float32 or both float64,
    one launch.  Outputs have the dtype of the fields for the "binary" method and are float64 otherwise."""
    who = "precip_phase_map"
    outputs = _subset(who, outputs, PHASE_MAP_OUTPUTS)
    T, C_, f64 = _same_fields(who, {"pr": pr, "tas": tas})
    args, keep = _phase_partition(who, part, T, C_)
    dtype = pr.dtype if part["method"] == "binary" else np.float64
    outs = {o: dev.empty((T, C_), dtype) for o in outputs}
    dev.call("xh_precip_phase_map", T, C_, C_, f64, _vp(pr.ptr), _vp(tas.ptr), *args, *(_ptr(outs, o) for o in PHASE_MAP_OUTPUTS), C_)
    del keep
    return outs


def precip_phase_period(dev: Device, pr: DeviceArray, tas: DeviceArray, seg, part: dict, outputs, *, per_day: float = 86400.0,
                        doy=None, window: int = 7, **limits) -> dict:
    """xh_precip_phase_period: any subset of ``capi.PHASE_OUTPUTS`` per period from ONE launch and one read of ``pr`` and of the
    second field (``tas``, or the solid precipitation itself with the "given" method).  ``seg`` (P + 1) host row offsets, ``doy``
    host int (T), needed by first_snow / last_snow.  ``limits``: ``PHASE_LIMITS`` (snow limits in mm of ``snow * per_day``, the
    others in the fields' own units).  Returns ``{name: (P, C) float64 DeviceArray}``."""
    who = "precip_phase_period"
    outputs = _subset(who, outputs, capi.PHASE_OUTPUTS)
    T, C_, f64 = _same_fields(who, {"pr": pr, "tas": tas})
    s, P = _periods(who, seg, T)
    if set(limits) - set(PHASE_LIMITS):
        raise TypeError(f"{who}: unknown limits {sorted(set(limits) - set(PHASE_LIMITS))}")
    if part["method"] == "given" and {"hplt_days", "rofg_days"} & set(outputs):
        raise ValueError(f"{who}: hplt_days and rofg_days need a temperature")
    window = _rain_window(who, "window", window)
    defaults = {"snow_low": 0.0, "snow_high": np.inf, "snow_thresh": 1.0, "hplt_pr": 0.0, "hplt_tas": 0.0, "rofg_pr": 0.0, "rofg_frz": 0.0}
    lim = np.array([float(limits.get(k, defaults[k])) for k in PHASE_LIMITS], np.float64)
    dy = None
    if {"first_snow", "last_snow"} & set(outputs):
        if doy is None:
            raise ValueError(f"{who}: first_snow / last_snow need doy")
        dy = _host_table(who, doy, np.int32, T, "doy")
    args, keep = _phase_partition(who, part, T, C_)
    outs = {o: dev.empty((P, C_), np.float64) for o in outputs}
    ptrs = np.array([outs[o].ptr if o in outs else 0 for o in capi.PHASE_OUTPUTS], np.uint64)
    mask = sum(1 << k for k, o in enumerate(capi.PHASE_OUTPUTS) if o in outs)
    dev.call("xh_precip_phase_period", T, C_, C_, f64, _vp(pr.ptr), _vp(tas.ptr), float(per_day), P, np_ptr(s),
             np_ptr(dy) if dy is not None else _vp(0), *args, np_ptr(lim), window, mask, np_ptr(ptrs), C_)
    del keep
    return outs


# ---- the spatial-analogue unit (include/ext/xclim_hip_analog.h, xclim_amd/csrc/analog.hip) ---------------------------
def _ext_call(dev: Device, name: str, *args):
    """``dev.call`` of an entry point of ``capi.EXT_SIGNATURES`` or ``capi.UNIT_SIGNATURES`` with every argument converted to
    the ctypes type of its table here: the call is right on a library handle whose ``argtypes`` were never set."""
    table = capi.EXT_SIGNATURES if name in capi.EXT_SIGNATURES else capi.UNIT_SIGNATURES
    kinds = table[name][1:]
    if len(kinds) != len(args):
        raise TypeError(f"{name}: {len(kinds)} arguments, got {len(args)}")
    dev.call(name, *(a if isinstance(a, kind) else kind(a) for kind, a in zip(kinds, args)))


def analog(dev: Device, method: str, x, fields, *, par=None, k=None, C_: int | None = None, ld: int | None = None,
           out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_analog: the dissimilarity ``method`` (a key of ``capi.ANALOG_METHODS``) between the target sample ``x``, host float64
    (n, d), and the candidate sample of every cell: ``fields``, a sequence of d DeviceArrays (m, C), all float32 or all float64.
    ``par``: the method's host parameters (zech_aslan: [dmin]; szekely_rizzo: [standardize]; mahalanobis: VI (d, d)).  ``k``:
    kldiv's list.  Returns float64 (1, C), or (nk, C) for kldiv; one launch.  ``C_`` / ``ld`` / ``out`` / ``ld_out``: the cells
    and the row pitches of padded views, and an output buffer of the caller's (default: dense fields, a new (rows, C) array)."""
    who = "analog"
    if method not in capi.ANALOG_METHODS:
        raise ValueError(f"{who}: unknown method {method!r}")
    x = np.ascontiguousarray(x, dtype=np.float64)
    fields = list(fields)
    if x.ndim != 2 or len(fields) != x.shape[1] or not fields:
        raise ValueError(f"{who}: x must be (n, d) and fields hold d arrays")
    n, d = x.shape
    m, width, f64 = _same_fields(who, {f"field {i}": f for i, f in enumerate(fields)})
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    par = np.zeros(0) if par is None else np.ascontiguousarray(par, dtype=np.float64).reshape(-1)
    ks = np.zeros(0, np.int32) if k is None else np.ascontiguousarray(k, dtype=np.int32).reshape(-1)
    rows = len(ks) if method == "kldiv" else 1
    if out is None:
        ld_out = C_
        out = dev.empty((rows, C_), np.float64)
    ptrs = np.array([f.ptr for f in fields], np.uint64)
    _ext_call(dev, "xh_analog", capi.ANALOG_METHODS[method], n, m, d, np_ptr(x), C_, ld, f64, np_ptr(ptrs),
              np_ptr(par) if par.size else _vp(0), par.size, np_ptr(ks) if ks.size else _vp(0), ks.size, _vp(out.ptr),
              C_ if ld_out is None else int(ld_out))
    return out


# ---- the distribution-fit unit (include/units/xclim_hip_distfit.h, xclim_amd/csrc/distfit.hip) --------------------------
def dist_nparams(dist: str) -> int:
    return 2 if dist in ("norm", "gumbel_r") else 3


def dist_fit(dev: Device, x: DeviceArray, dist: str, method: str = "ML", floc=None, q=None, qfunc: str = "ppf", *,
             C_: int | None = None, ld: int | None = None, outs: dict | None = None, pitches: dict | None = None):
    """xh_dist_fit: the parameters of ``dist`` (a key of ``capi.DIST_CODES``) for every cell of a (T, C) float32 or float64
    field, one launch.  ``q`` (at most ``capi.DISTFIT_MAX_Q`` probabilities) adds the fused levels ``qfunc`` ("ppf" / "isf").
    Returns ``(params (nparams, C) float64, nfev (C) int32, status (C) uint8, levels (nq, C) float64 or None)`` as
    DeviceArrays.  ``C_`` / ``ld`` / ``outs`` / ``pitches``: the cells and the row pitch of a padded view, output buffers of the
    caller's (keys params, nfev, status, levels) and their row pitches (keys params, levels)."""
    who = "dist_fit"
    if dist not in capi.DIST_CODES:
        raise ValueError(f"{who}: unknown distribution {dist!r}")
    if method not in capi.DIST_METHODS:
        raise ValueError(f"{who}: unknown method {method!r}")
    T, width, f64 = _field(x)
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    qs = np.zeros(0) if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    outs = dict(outs or {})
    pitches = dict(pitches or {})
    params = outs.get("params") or dev.empty((dist_nparams(dist), C_), np.float64)
    nfev = outs.get("nfev") or dev.empty((C_,), np.int32)
    status = outs.get("status") or dev.empty((C_,), np.uint8)
    levels = (outs.get("levels") or dev.empty((len(qs), C_), np.float64)) if len(qs) else None
    _ext_call(dev, "xh_dist_fit", _vp(x.ptr), T, C_, ld, int(f64), capi.DIST_CODES[dist], capi.DIST_METHODS[method],
              int(floc is not None), float(floc if floc is not None else 0.0), np_ptr(qs) if len(qs) else _vp(0), len(qs),
              capi.DIST_FUNCS[qfunc], _vp(params.ptr), int(pitches.get("params", C_)), _vp(nfev.ptr), _vp(status.ptr),
              _vp(levels.ptr if levels is not None else 0), int(pitches.get("levels", C_)))
    return params, nfev, status, levels


def dist_eval(dev: Device, params: DeviceArray, dist: str, func: str, v, *, C_: int | None = None, ld: int | None = None,
              out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_dist_eval: ``func`` ("ppf" / "isf" / "cdf" / "pdf") of ``dist`` at the host values ``v`` for every cell of the
    (nparams, C) float64 parameters; returns (nv, C) float64.  ``C_`` / ``ld`` / ``out`` / ``ld_out``: padded views."""
    who = "dist_eval"
    if dist not in capi.DIST_CODES or func not in capi.DIST_FUNCS:
        raise ValueError(f"{who}: unknown distribution or function ({dist!r}, {func!r})")
    if np.dtype(params.dtype) != np.float64 or len(params.shape) != 2 or params.shape[0] != dist_nparams(dist):
        raise TypeError(f"{who}: params must be float64 ({dist_nparams(dist)}, C), got {np.dtype(params.dtype).name} {params.shape}")
    ld = int(params.shape[1]) if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    vs = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if out is None:
        ld_out = C_
        out = dev.empty((len(vs), C_), np.float64)
    _ext_call(dev, "xh_dist_eval", capi.DIST_CODES[dist], capi.DIST_FUNCS[func], _vp(params.ptr), C_, ld,
              np_ptr(vs) if len(vs) else _vp(0), len(vs), _vp(out.ptr), C_ if ld_out is None else int(ld_out))
    return out


# ---- the thermal-comfort unit (include/units/xclim_hip_thermal.h, xclim_amd/csrc/thermal.hip) -----------------------------
def esat(dev: Device, tas: DeviceArray, method: str = "sonntag90", case: str = "water", ice_thresh: float = 0.0,
         water_thresh: float = 273.15, interp_power: float = 1.0, *, C_: int | None = None, ld: int | None = None,
         out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_esat: the saturation vapour pressure [Pa] of a (R, C) float32 or float64 field [K], in the field's dtype.  ``method``: a
    key of ``capi.ESAT_METHODS``; ``case``: a key of ``capi.ESAT_CASES``.  ``C_`` / ``ld`` / ``out`` / ``ld_out``: padded views."""
    who = "esat"
    if method not in capi.ESAT_METHODS or case not in capi.ESAT_CASES:
        raise ValueError(f"{who}: unknown method or case ({method!r}, {case!r})")
    R, width, f64 = _field(tas)
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    if out is None:
        ld_out = C_
        out = dev.empty((R, C_), tas.dtype)
    _ext_call(dev, "xh_esat", _vp(tas.ptr), R, C_, ld, int(f64), capi.ESAT_METHODS[method], capi.ESAT_CASES[case], float(ice_thresh),
              float(water_thresh), float(interp_power), _vp(out.ptr), C_ if ld_out is None else int(ld_out))
    return out


THERMAL_FIELDS = ("tas", "hurs", "sfcWind", "mrt", "rsds", "rsus", "rlds", "rlus")
THERMAL_OUTPUTS = ("utci", "mrt", "csza")


def thermal_comfort(dev: Device, fields: dict, rows=None, lat=None, lon=None, *, mode: str = "daily", stat: str = "sunlit",
                    mask_invalid: bool = True, wind_cap_min: bool = False, outputs=("utci",), shape=None, C_: int | None = None,
                    ld: int | None = None, outs: dict | None = None, ld_out: int | None = None) -> dict:
    """xh_thermal_comfort: one launch over the (R, C) device fields of ``fields`` (keys of ``THERMAL_FIELDS``, all float32 or all
    float64; ``mrt`` given: the radiation fields are not read).  ``rows``: the float64 (``capi.THERMAL_NROW``, R) per-row solar
    table; ``lat`` / ``lon``: float64 (C), the wrapped latitude and the longitude in rad (host arrays, uploaded per call, or device arrays).  ``outputs``: of ``THERMAL_OUTPUTS``;
    returns ``{name: DeviceArray (R, C)}``, utci in the fields' dtype, mrt and csza float64.  ``shape``: (R, C, float64?) when no
    field is passed (csza alone).  ``C_`` / ``ld`` / ``outs`` / ``ld_out``: padded views and output buffers of the caller's."""
    who = "thermal_comfort"
    fields = {k: v for k, v in fields.items() if v is not None}
    if set(fields) - set(THERMAL_FIELDS) or set(outputs) - set(THERMAL_OUTPUTS) or not outputs:
        raise ValueError(f"{who}: fields of {THERMAL_FIELDS}, outputs of {THERMAL_OUTPUTS}")
    if mode not in capi.THERMAL_MODES or stat not in capi.THERMAL_STATS:
        raise ValueError(f"{who}: unknown mode or stat ({mode!r}, {stat!r})")
    R, width, f64 = _same_fields(who, fields) if fields else shape
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    keep = []

    def table(a, shape_, what):
        if a is None:
            return _vp(0)
        if isinstance(a, DeviceArray):   # a table the caller keeps on the device
            if np.dtype(a.dtype) != np.float64 or tuple(a.shape) != shape_:
                raise TypeError(f"{who}: {what} must be a float64 {shape_} device array")
            return _vp(a.ptr)
        t = np.ascontiguousarray(a, dtype=np.float64)
        if t.shape != shape_:
            raise ValueError(f"{who}: {what} must have the shape {shape_}, got {t.shape}")
        keep.append(dev.to_device(t))
        return _vp(keep[-1].ptr)

    d_rows = table(rows, (capi.THERMAL_NROW, R), "rows")
    d_lat, d_lon = table(lat, (C_,), "lat"), table(lon, (C_,), "lon")
    outs = dict(outs or {})
    res = {}
    for o in outputs:
        res[o] = outs[o] if o in outs else dev.empty((R, C_), (np.float64 if f64 else np.float32) if o == "utci" else np.float64)
    flags = (capi.THERMAL_FLAGS["mask_invalid"] if mask_invalid else 0) | (capi.THERMAL_FLAGS["wind_cap_min"] if wind_cap_min else 0)

    def p(d, k):
        return _vp(d[k].ptr if k in d else 0)

    _ext_call(dev, "xh_thermal_comfort", R, C_, ld, int(f64), p(fields, "tas"), p(fields, "hurs"), p(fields, "sfcWind"), p(fields, "mrt"),
              p(fields, "rsds"), p(fields, "rsus"), p(fields, "rlds"), p(fields, "rlus"), d_rows, d_lat, d_lon, capi.THERMAL_MODES[mode],
              capi.THERMAL_STATS[stat], flags, p(res, "utci"), p(res, "mrt"), p(res, "csza"), C_ if ld_out is None else int(ld_out))
    del keep   # (released to the pool: the stream's order protects the tables of the launch)
    return res


# ---- the humidity, heat-stress and wind unit (include/units/xclim_hip_humidity.h, xclim_amd/csrc/humidity.hip) -------------
AM_FIELDS = ("tas", "tdps", "hurs", "huss", "ps")


def air_moisture(dev: Device, fields: dict, outputs, *, celsius: bool = False, method: str = "sonntag90", case: str = "water",
                 ice_thresh: float = 0.0, water_thresh: float = 273.15, interp_power: float = 1.0, rh_method: str = "esat",
                 invalid_rh: str = "clip", invalid_q: str = "none", dew_method: str = "buck81", dew_variant: str = "water",
                 C_: int | None = None, ld: int | None = None, outs: dict | None = None, ld_out: int | None = None) -> dict:
    """xh_air_moisture: one launch over the (R, C) device fields of ``fields`` (keys of ``AM_FIELDS``, all float32 or all float64)
    for the ``outputs`` (keys of ``capi.AM_OUTPUTS``); returns ``{name: DeviceArray (R, C)}`` in the fields' dtype.  ``celsius``:
    tas and tdps are in degC.  ``C_`` / ``ld`` / ``outs`` / ``ld_out``: padded views and output buffers of the caller's."""
    who = "air_moisture"
    fields = {k: v for k, v in fields.items() if v is not None}
    outputs = tuple(outputs)
    if set(fields) - set(AM_FIELDS) or set(outputs) - set(capi.AM_OUTPUTS) or not fields:
        raise ValueError(f"{who}: fields of {AM_FIELDS}, outputs of {tuple(capi.AM_OUTPUTS)}")
    if method not in capi.ESAT_METHODS or case not in capi.ESAT_CASES:
        raise ValueError(f"{who}: unknown method or case ({method!r}, {case!r})")
    if dew_variant not in ("water", "ice"):
        raise ValueError(f"{who}: dew_variant must be 'water' or 'ice', got {dew_variant!r}")
    R, width, f64 = _same_fields(who, fields)
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    outs = dict(outs or {})
    res = {o: outs[o] if o in outs else dev.empty((R, C_), np.float64 if f64 else np.float32) for o in outputs}
    ptrs = np.zeros(capi.AM_NOUT, np.uint64)
    for o, v in res.items():
        ptrs[capi.AM_OUTPUTS[o]] = v.ptr

    def p(k):
        return _vp(fields[k].ptr if k in fields else 0)

    _ext_call(dev, "xh_air_moisture", R, C_, ld, int(f64), p("tas"), p("tdps"), p("hurs"), p("huss"), p("ps"), int(bool(celsius)),
              capi.ESAT_METHODS[method], capi.ESAT_CASES[case], float(ice_thresh), float(water_thresh), float(interp_power),
              capi.RH_METHODS[rh_method], capi.INVALID_RULES[invalid_rh], capi.INVALID_RULES[invalid_q], capi.DEW_METHODS[dew_method],
              int(dew_variant == "ice"), np_ptr(ptrs), C_ if ld_out is None else int(ld_out))
    return res


def wind_map(dev: Device, op: str, a: DeviceArray, b: DeviceArray | None = None, par=None, *, flags=(), outputs=(0,),
             C_: int | None = None, ld: int | None = None, outs: dict | None = None, ld_out: int | None = None) -> dict:
    """xh_wind_map: the operation ``op`` (a key of ``capi.WIND_OPS``) on the (R, C) device fields ``a`` and ``b`` of one dtype;
    ``par``: its host parameters, ``flags``: names of ``capi.WIND_FLAGS``, ``outputs``: of 0 and 1.  Returns ``{0 / 1: DeviceArray
    (R, C)}`` in the fields' dtype.  ``C_`` / ``ld`` / ``outs`` / ``ld_out``: padded views and output buffers of the caller's."""
    who = "wind_map"
    if op not in capi.WIND_OPS or set(outputs) - {0, 1} or not outputs:
        raise ValueError(f"{who}: op of {tuple(capi.WIND_OPS)}, outputs of 0 and 1")
    R, width, f64 = _same_fields(who, {"a": a} if b is None else {"a": a, "b": b})
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    outs = dict(outs or {})
    res = {o: outs[o] if o in outs else dev.empty((R, C_), np.float64 if f64 else np.float32) for o in outputs}
    pv = np.zeros(capi.WIND_NPAR)
    if par is not None:
        pv[:len(par)] = par
    _ext_call(dev, "xh_wind_map", capi.WIND_OPS[op], R, C_, ld, int(f64), _vp(a.ptr), _vp(b.ptr if b is not None else 0), np_ptr(pv),
              sum(capi.WIND_FLAGS[f] for f in flags), _vp(res[0].ptr if 0 in res else 0), _vp(res[1].ptr if 1 in res else 0),
              C_ if ld_out is None else int(ld_out))
    return res


# ---- the change-robustness unit (include/units/xclim_hip_robust.h, xclim_amd/csrc/robust.hip) -----------------------------
CT_OUTPUTS =("delta", "mean_ref", "n_fut", "n_ref", "stat", "df", "pvals", "status")
_CT_DTYPES = {"delta": np.float64, "mean_ref": np.float64, "n_fut": np.int32, "n_ref": np.int32, "stat": np.float64, "df": np.float64,
              "pvals": np.float64, "status": np.uint8}


def change_test(dev: Device, fut: DeviceArray, ref: DeviceArray, test: str = "moments", sf=None, *, C_: int | None = None,
                ld_fut: int | None = None, ld_ref: int | None = None, outs: dict | None = None, ld_out: int | None = None) -> dict:
    """xh_change_test: ``fut`` (R, T1, C) and ``ref`` (R, T2, C) or (T2, C), both float32 or both float64 device arrays; ``test``
    a key of ``capi.CT_TESTS``; ``sf``: the host table of the exact Mann-Whitney route (``ensembles.mwu_exact_sf``), needed where
    a length is at most 8.  Returns ``{name: DeviceArray (R, C)}`` for ``CT_OUTPUTS`` (the first four for "moments").  ``C_`` /
    ``ld_*`` / ``outs`` / ``ld_out``: the cells and row pitches of padded views and output buffers of the caller's."""
    who = "change_test"
    if test not in capi.CT_TESTS:
        raise ValueError(f"{who}: unknown test {test!r}")
    if len(fut.shape) != 3 or len(ref.shape) not in (2, 3) or np.dtype(fut.dtype) != np.dtype(ref.dtype):
        raise TypeError(f"{who}: fut (R, T1, C) and ref (R, T2, C) or (T2, C) of one dtype, got {fut.shape} {fut.dtype}, {ref.shape} {ref.dtype}")
    if np.dtype(fut.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{who}: float32 or float64 fields, got {np.dtype(fut.dtype).name}")
    R, T1, width = (int(v) for v in fut.shape)
    T2 = int(ref.shape[-2])
    if (ld_ref is None and int(ref.shape[-1]) != width) or (len(ref.shape) == 3 and int(ref.shape[0]) != R):
        raise ValueError(f"{who}: ref {ref.shape} does not match fut {fut.shape}")
    ld_fut = width if ld_fut is None else int(ld_fut)
    ld_ref = int(ref.shape[-1]) if ld_ref is None else int(ld_ref)
    C_ = width if C_ is None else int(C_)
    names = CT_OUTPUTS[:4] if test == "moments" else CT_OUTPUTS
    outs = dict(outs or {})
    res = {k: outs[k] if k in outs else dev.empty((R, C_), _CT_DTYPES[k]) for k in names}
    table = None if sf is None else np.ascontiguousarray(sf, dtype=np.float64).reshape(-1)

    def p(k):
        return _vp(res[k].ptr if k in res else 0)

    _ext_call(dev, "xh_change_test", _vp(fut.ptr), _vp(ref.ptr), R, T1, T2, C_, ld_fut, T1 * ld_fut, ld_ref,
              T2 * ld_ref if len(ref.shape) == 3 else 0, int(np.dtype(fut.dtype) == np.float64), capi.CT_TESTS[test],
              np_ptr(table) if table is not None else _vp(0), 0 if table is None else table.size, *(p(k) for k in CT_OUTPUTS),
              C_ if ld_out is None else int(ld_out))
    return res


def robust_fractions(dev: Device, delta: DeviceArray, weights, *, changed: DeviceArray | None = None, valid: DeviceArray | None = None,
                     mean_ref: DeviceArray | None = None, strict_sign: bool = True, abs_thresh=None, rel_thresh=None,
                     C_: int | None = None, ld: int | None = None, out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_robust_fractions: the seven fractions (``capi.RF_ROWS``) of the float64 (R, C) ``delta``; ``changed`` / ``valid`` uint8
    (R, C) or None, ``weights`` host (R).  ``abs_thresh`` / ``rel_thresh`` (with ``mean_ref``) decide ``changed`` in the kernel.
    Returns float64 (7, C).  ``C_`` / ``ld`` / ``out`` / ``ld_out``: padded views."""
    who = "robust_fractions"
    if np.dtype(delta.dtype) != np.float64 or len(delta.shape) != 2:
        raise TypeError(f"{who}: delta must be float64 (R, C), got {np.dtype(delta.dtype).name} {delta.shape}")
    for name, m in (("changed", changed), ("valid", valid)):
        if m is not None and (np.dtype(m.dtype) != np.uint8 or tuple(m.shape) != tuple(delta.shape)):
            raise TypeError(f"{who}: {name} must be uint8 {tuple(delta.shape)}")
    if mean_ref is not None and (np.dtype(mean_ref.dtype) != np.float64 or tuple(mean_ref.shape) != tuple(delta.shape)):
        raise TypeError(f"{who}: mean_ref must be float64 {tuple(delta.shape)}")
    R, width = (int(v) for v in delta.shape)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size != R:
        raise ValueError(f"{who}: {R} weights needed, got {w.size}")
    if abs_thresh is not None and rel_thresh is not None:
        raise ValueError(f"{who}: abs_thresh and rel_thresh are both given")
    kind = "abs" if abs_thresh is not None else "rel" if rel_thresh is not None else "none"
    thresh = float(abs_thresh if kind == "abs" else rel_thresh if kind == "rel" else 0.0)
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    if out is None:
        ld_out = C_
        out = dev.empty((capi.RF_NFRAC, C_), np.float64)
    _ext_call(dev, "xh_robust_fractions", _vp(delta.ptr), _vp(changed.ptr if changed is not None else 0),
              _vp(valid.ptr if valid is not None else 0), _vp(mean_ref.ptr if mean_ref is not None else 0), R, C_, ld, np_ptr(w),
              int(bool(strict_sign)), capi.RF_THRESH[kind], thresh, _vp(out.ptr), C_ if ld_out is None else int(ld_out))
    return out


def robust_coefficient(dev: Device, fut: DeviceArray, ref: DeviceArray, *, C_: int | None = None, ld_fut: int | None = None,
                       ld_ref: int | None = None, outs: dict | None = None, parts: bool = False):
    """xh_robust_coefficient: ``fut`` (R, T1, C) and ``ref`` (T2, C), both float32 or both float64; returns the float64 (C)
    coefficient, with ``parts`` the tuple (R, A1, A2).  ``C_`` / ``ld_*`` / ``outs`` (keys out, a1, a2): padded views."""
    who = "robust_coefficient"
    if len(fut.shape) != 3 or len(ref.shape) != 2 or np.dtype(fut.dtype) != np.dtype(ref.dtype):
        raise TypeError(f"{who}: fut (R, T1, C) and ref (T2, C) of one dtype, got {fut.shape} {fut.dtype}, {ref.shape} {ref.dtype}")
    if np.dtype(fut.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{who}: float32 or float64 fields, got {np.dtype(fut.dtype).name}")
    R, T1, width = (int(v) for v in fut.shape)
    T2 = int(ref.shape[0])
    if ld_ref is None and int(ref.shape[1]) != width:
        raise ValueError(f"{who}: ref {ref.shape} does not match fut {fut.shape}")
    ld_fut = width if ld_fut is None else int(ld_fut)
    ld_ref = width if ld_ref is None else int(ld_ref)
    C_ = width if C_ is None else int(C_)
    outs = dict(outs or {})
    names = ("out", "a1", "a2") if parts else ("out",)
    res = {k: outs[k] if k in outs else dev.empty((C_,), np.float64) for k in names}
    _ext_call(dev, "xh_robust_coefficient", _vp(fut.ptr), _vp(ref.ptr), R, T1, T2, C_, ld_fut, T1 * ld_fut, ld_ref,
              int(np.dtype(fut.dtype) == np.float64), _vp(res["out"].ptr), _vp(res["a1"].ptr if parts else 0),
              _vp(res["a2"].ptr if parts else 0))
    return (res["out"], res["a1"], res["a2"]) if parts else res["out"]


def ar6_gamma(dev: Device, y: DeviceArray, x, deg: int, factor: float, seg=None, *, C_: int | None = None, ld: int | None = None,
              out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_ar6_gamma: ``y`` (R, T, C) annual values, float32 or float64; ``x`` host (T) days; ``deg`` 1 or 2; ``seg`` the host offsets
    of the blocks or None.  Returns float64 (R, C): ``factor`` * std of the detrended values (or of their block means).  ``C_`` /
    ``ld`` / ``out`` / ``ld_out``: padded views."""
    who = "ar6_gamma"
    if len(y.shape) != 3 or np.dtype(y.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{who}: y must be float32 or float64 (R, T, C), got {np.dtype(y.dtype).name} {y.shape}")
    R, T, width = (int(v) for v in y.shape)
    xs = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if xs.size != T:
        raise ValueError(f"{who}: {T} abscissa values needed, got {xs.size}")
    sg = None if seg is None else np.ascontiguousarray(seg, dtype=np.int64).reshape(-1)
    ld = width if ld is None else int(ld)
    C_ = ld if C_ is None else int(C_)
    if out is None:
        ld_out = C_
        out = dev.empty((R, C_), np.float64)
    _ext_call(dev, "xh_ar6_gamma", _vp(y.ptr), R, T, C_, ld, T * ld, int(np.dtype(y.dtype) == np.float64), np_ptr(xs), int(deg),
              np_ptr(sg) if sg is not None else _vp(0), 0 if sg is None else sg.size - 1, float(factor), _vp(out.ptr),
              C_ if ld_out is None else int(ld_out))
    return out


# ---- the uncertainty-partitioning unit (include/units/xclim_hip_partition.h, xclim_amd/csrc/partition.hip) ----------------
PT_SMOOTH_OUTPUTS = ("sm", "roll", "n_valid", "status", "flag")


def _float_field(who: str, a: DeviceArray, ndim: int, what: str):
    if len(a.shape) != ndim or np.dtype(a.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{who}: {what} must be a float32 or float64 array of {ndim} dimensions, got {np.dtype(a.dtype).name} {a.shape}")


def partition_smooth(dev: Device, y: DeviceArray | None, q=None, *, sm_in: DeviceArray | None = None, window: int = 11, stat: str = "var",
                     baseline=None, kind: str = "+", outputs=PT_SMOOTH_OUTPUTS, C_: int | None = None, ld: int | None = None,
                     stride_n: int | None = None, outs: dict | None = None, ld_out: int | None = None, stride_n_out: int | None = None,
                     ld_nc: int | None = None) -> dict:
    """xh_partition_smooth: ``y`` (T, N, C) float32 or float64; ``q`` the host basis (T, deg + 1), or ``sm_in`` (T, N, C) of y's
    dtype instead of a fit; ``window`` / ``stat`` (10, "mean") or (11, "var"); ``baseline`` a row range (b0, b1) with ``kind`` "+"
    or "*".  Returns ``{name: DeviceArray}`` for the requested ``outputs``: sm and roll float64 (T, N, C), n_valid int32 and
    status uint8 (N, C), flag uint8 (1).  ``C_`` / ``ld`` / ``stride_n`` / ``outs`` / ``ld_out`` / ``stride_n_out`` / ``ld_nc``:
    the cells, pitches and output buffers of padded views."""
    who = "partition_smooth"
    lead = y if y is not None else sm_in
    if lead is None:
        raise ValueError(f"{who}: neither y nor sm_in")
    for name, a in (("y", y), ("sm_in", sm_in)):
        if a is not None:
            _float_field(who, a, 3, name)
            if tuple(a.shape) != tuple(lead.shape) or np.dtype(a.dtype) != np.dtype(lead.dtype):
                raise TypeError(f"{who}: y and sm_in must have one shape and dtype")
    if stat not in capi.PT_ROLL:
        raise ValueError(f"{who}: unknown statistic {stat!r}")
    if kind not in ("+", "*"):
        raise ValueError(kind)
    T, N, width = (int(v) for v in lead.shape)
    C_ = width if C_ is None else int(C_)
    stride_n = width if stride_n is None else int(stride_n)
    ld = N * stride_n if ld is None else int(ld)
    stride_n_out = C_ if stride_n_out is None else int(stride_n_out)
    ld_out = N * stride_n_out if ld_out is None else int(ld_out)
    ld_nc = C_ if ld_nc is None else int(ld_nc)
    deg = 0
    basis = None
    if sm_in is None:
        basis = np.ascontiguousarray(q, dtype=np.float64)
        if basis.ndim != 2 or basis.shape[0] != T:
            raise ValueError(f"{who}: the basis must be (T, deg + 1), got {basis.shape}")
        deg = basis.shape[1] - 1
    outputs = _subset(who, outputs, PT_SMOOTH_OUTPUTS)
    shapes = {"sm": ((T, N, C_), np.float64), "roll": ((T, N, C_), np.float64), "n_valid": ((N, C_), np.int32),
              "status": ((N, C_), np.uint8), "flag": ((1,), np.uint8)}
    outs = dict(outs or {})
    res = {k: outs[k] if k in outs else dev.empty(*shapes[k]) for k in outputs}
    b0, b1 = (0, 0) if baseline is None else (int(baseline[0]), int(baseline[1]))
    base = "none" if baseline is None else ("sub" if kind == "+" else "div")
    _ext_call(dev, "xh_partition_smooth", _vp(y.ptr if y is not None else 0), _vp(sm_in.ptr if sm_in is not None else 0), T, N, C_, ld,
              stride_n, int(np.dtype(lead.dtype) == np.float64), np_ptr(basis) if basis is not None else _vp(0), deg, int(window),
              capi.PT_ROLL[stat], capi.PT_BASE[base], b0, b1, _ptr(res, "sm"), _ptr(res, "roll"), ld_out, stride_n_out,
              _ptr(res, "n_valid"), _ptr(res, "status"), ld_nc, _ptr(res, "flag"))
    return res


def partition_components(dev: Device, sm: DeviceArray, roll: DeviceArray, dims, comps, *, weights=None, w_axis: int = 0,
                         variab: str = "mean_all", t0: int = 0, g_order=(0, 1, 2, 3), with_g: bool = True, C_: int | None = None,
                         ld: int | None = None, stride_n: int | None = None, out: DeviceArray | None = None, g: DeviceArray | None = None,
                         ld_out: int | None = None):
    """xh_partition_components: ``sm`` and ``roll`` float64 (T, N, C) with N the product of ``dims`` (up to 4 member axes);
    ``comps`` a sequence of (axis, rule, weight) with the names of ``capi.PT_RULES`` / ``capi.PT_WEIGHTS``; ``weights`` the host
    vector over ``w_axis``; ``variab`` a key of ``capi.PT_VARIAB`` with ``t0``.  Returns (out (K + 2, T, C), g (T, C) or None):
    plane 0 the variability, then the components, then the total."""
    who = "partition_components"
    for name, a in (("sm", sm), ("roll", roll)):
        if len(a.shape) != 3 or np.dtype(a.dtype) != np.float64 or tuple(a.shape) != tuple(sm.shape):
            raise TypeError(f"{who}: {name} must be float64 (T, N, C) like sm")
    T, N, width = (int(v) for v in sm.shape)
    d = [int(v) for v in dims]
    if len(d) > capi.PT_MAX_AXES:
        raise ValueError(f"{who}: at most {capi.PT_MAX_AXES} member axes, got {len(d)}")
    d4 = np.array(d + [1] * (capi.PT_MAX_AXES - len(d)), np.int64)
    if int(np.prod(d4)) != N:
        raise ValueError(f"{who}: the member axes {d} do not multiply to {N}")
    table = np.array([[int(ax), capi.PT_RULES[rule], capi.PT_WEIGHTS[wt]] for ax, rule, wt in comps], np.int32).reshape(-1, 3)
    K_ = table.shape[0]
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and (not 0 <= int(w_axis) < capi.PT_MAX_AXES or w.size != d4[int(w_axis)]):
        raise ValueError(f"{who}: the weights do not fit axis {w_axis}")
    order = np.array(list(g_order) + [k for k in range(capi.PT_MAX_AXES) if k not in g_order], np.int32)
    C_ = width if C_ is None else int(C_)
    stride_n = width if stride_n is None else int(stride_n)
    ld = N * stride_n if ld is None else int(ld)
    ld_out = C_ if ld_out is None else int(ld_out)
    if out is None:
        out = dev.empty((K_ + 2, T, C_), np.float64)
    if g is None and with_g:
        g = dev.empty((T, C_), np.float64)
    _ext_call(dev, "xh_partition_components", _vp(sm.ptr), _vp(roll.ptr), T, np_ptr(d4), C_, ld, stride_n, np_ptr(table) if K_ else _vp(0),
              K_, np_ptr(w) if w is not None else _vp(0), int(w_axis), capi.PT_VARIAB[variab], int(t0), np_ptr(order), _vp(out.ptr), ld_out,
              _vp(g.ptr if g is not None else 0))
    return out, g


def ensemble_stats(dev: Device, x: DeviceArray, weights=None, min_members: int = 1, *, E_: int | None = None, ld: int | None = None,
                   out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_ensemble_stats: ``x`` (R, E) float32 or float64; ``weights`` host (R) or None.  Returns float64 (4, E): the rows of
    ``capi.ES_ROWS``.  ``E_`` / ``ld`` / ``out`` / ``ld_out``: padded views."""
    who = "ensemble_stats"
    _float_field(who, x, 2, "x")
    R, width = (int(v) for v in x.shape)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and w.size != R:
        raise ValueError(f"{who}: {R} weights needed, got {w.size}")
    ld = width if ld is None else int(ld)
    E_ = ld if E_ is None else int(E_)
    if out is None:
        ld_out = E_
        out = dev.empty((capi.ES_NSTAT, E_), np.float64)
    _ext_call(dev, "xh_ensemble_stats", _vp(x.ptr), R, E_, ld, int(np.dtype(x.dtype) == np.float64), np_ptr(w) if w is not None else _vp(0),
              int(min_members), _vp(out.ptr), E_ if ld_out is None else int(ld_out))
    return out


# ---- the compound-extreme unit (include/units/xclim_hip_compound.h, xclim_amd/csrc/compound.hip) -------------------------
CD_TABLES = ("tas_lo", "tas_hi", "pr_lo", "pr_hi")
CD_NEEDS = {"cold_dry": ("tas_lo", "pr_lo"), "warm_dry": ("tas_hi", "pr_lo"), "warm_wet": ("tas_hi", "pr_hi"), "cold_wet": ("tas_lo", "pr_hi")}


def _padded(width, C_, ld):
    """(cells, row pitch) of a field of ``width`` columns: dense by default, a padded view with ``C_`` / ``ld``."""
    ld = width if ld is None else int(ld)
    return (ld if C_ is None else int(C_)), ld


def _period_out(dev, P, C_, out, ld_out):
    if out is None:
        return dev.empty((P, C_), np.float64), C_
    return out, C_ if ld_out is None else int(ld_out)


def compound_doy_days(dev: Device, tas: DeviceArray, pr: DeviceArray, tables: dict, tidx, seg, outputs, *, C_: int | None = None,
                      ld: int | None = None, ld_tab: int | None = None, outs: dict | None = None, ld_out: int | None = None) -> dict:
    """xh_compound_doy_days: ``tas`` and ``pr`` (T, C) DeviceArrays, both float32 or both float64; ``tables``: the float64
    (ndoy, C) DeviceArrays of ``CD_TABLES`` that the ``outputs`` (keys of ``capi.CD_OUTPUTS``) need (``CD_NEEDS``), all of one
    shape; ``tidx`` host int (T), the table row of every field row; ``seg`` host (P + 1).  Returns ``{name: DeviceArray (P, C)
    float64}``; one launch.  ``C_`` / ``ld`` / ``ld_tab`` / ``outs`` / ``ld_out``: padded views and output buffers of the caller's."""
    who = "compound_doy_days"
    outputs = _subset(who, outputs, tuple(capi.CD_OUTPUTS))
    T, width, f64 = _same_fields(who, {"tas": tas, "pr": pr})
    C_, ld = _padded(width, C_, ld)
    tables = {k: v for k, v in tables.items() if v is not None}
    needed = {t for o in outputs for t in CD_NEEDS[o]}
    if set(tables) - set(CD_TABLES) or needed - set(tables):
        raise ValueError(f"{who}: the outputs {outputs} need the tables {sorted(needed)}, got {sorted(tables)}")
    shapes = {tuple(int(s) for s in tables[t].shape) for t in needed}
    if len(shapes) != 1 or len(next(iter(shapes))) != 2 or any(np.dtype(tables[t].dtype) != np.float64 for t in needed):
        raise TypeError(f"{who}: the tables must be float64 (ndoy, C) device arrays of one shape")
    ndoy, twidth = shapes.pop()
    ld_tab = twidth if ld_tab is None else int(ld_tab)
    s, P = _periods(who, seg, T)
    ti = _host_table(who, tidx, np.int32, T, "tidx")
    outs = dict(outs or {})
    res = {o: outs[o] if o in outs else dev.empty((P, C_), np.float64) for o in outputs}
    _ext_call(dev, "xh_compound_doy_days", T, C_, ld, f64, _vp(tas.ptr), _vp(pr.ptr), ndoy, ld_tab,
              *(_vp(tables[t].ptr if t in needed else 0) for t in CD_TABLES), np_ptr(ti), P, np_ptr(s),
              *(_ptr(res, o) for o in capi.CD_OUTPUTS), C_ if ld_out is None else int(ld_out))
    return res


def degree_exceedance_date(dev: Device, tas: DeviceArray, seg, start, never, doy, *, thresh: float, sum_thresh: float, below: bool = False,
                           C_: int | None = None, ld: int | None = None, out: DeviceArray | None = None,
                           ld_out: int | None = None) -> DeviceArray:
    """xh_degree_exceedance_date: ``tas`` (T, C) float32 or float64; ``seg`` host (P + 1); ``start`` host int (P), the row the sum
    starts on or -1 for a NaN period; ``never`` host float64 (P), NaN for None; ``doy`` host int (T).  ``thresh`` in the units of
    the field.  Returns float64 (P, C)."""
    who = "degree_exceedance_date"
    T, width, f64 = _same_fields(who, {"tas": tas})
    C_, ld = _padded(width, C_, ld)
    s, P = _periods(who, seg, T)
    st = _host_table(who, start, np.int64, P, "start")
    nv = _host_table(who, never, np.float64, P, "never")
    dy = _host_table(who, doy, np.int32, T, "doy")
    out, ld_out = _period_out(dev, P, C_, out, ld_out)
    _ext_call(dev, "xh_degree_exceedance_date", T, C_, ld, f64, _vp(tas.ptr), float(thresh), int(bool(below)), float(sum_thresh), P,
              np_ptr(s), np_ptr(st), np_ptr(nv), np_ptr(dy), _vp(out.ptr), ld_out)
    return out


def blowing_snow_days(dev: Device, snd: DeviceArray, sfcWind: DeviceArray, seg, flags=None, *, snd_thresh: float, wind_thresh: float,
                      window: int = 3, C_: int | None = None, ld: int | None = None, out: DeviceArray | None = None,
                      ld_out: int | None = None) -> DeviceArray:
    """xh_blowing_snow_days: ``snd`` and ``sfcWind`` (T, C), both float32 or both float64; ``seg`` host (P + 1); ``flags``: host
    bool / uint8 (T), the rows the indexer selects, or None for all.  Thresholds in the units of the fields.  Returns float64
    (P, C)."""
    who = "blowing_snow_days"
    T, width, f64 = _same_fields(who, {"snd": snd, "sfcWind": sfcWind})
    C_, ld = _padded(width, C_, ld)
    s, P = _periods(who, seg, T)
    window = _rain_window(who, "window", window)
    if window > capi.BS_MAX_WINDOW:
        raise ValueError(f"{who}: windows of up to {capi.BS_MAX_WINDOW} rows are served, got {window}")
    fl = _row_selection(who, flags, T)
    out, ld_out = _period_out(dev, P, C_, out, ld_out)
    _ext_call(dev, "xh_blowing_snow_days", T, C_, ld, f64, _vp(snd.ptr), _vp(sfcWind.ptr), float(snd_thresh), float(wind_thresh), window, P,
              np_ptr(s), np_ptr(fl) if fl is not None else _vp(0), _vp(out.ptr), ld_out)
    return out


def pair_period_sum(dev: Device, a: DeviceArray, b: DeviceArray, seg, scale: float = 1.0, *, C_: int | None = None, ld: int | None = None,
                    out: DeviceArray | None = None, ld_out: int | None = None) -> DeviceArray:
    """xh_pair_period_sum: the NaN-skipping period sums of ``(a + b) * scale``, ``a`` and ``b`` (T, C) of one dtype; float64 (P, C)."""
    who = "pair_period_sum"
    T, width, f64 = _same_fields(who, {"a": a, "b": b})
    C_, ld = _padded(width, C_, ld)
    s, P = _periods(who, seg, T)
    out, ld_out = _period_out(dev, P, C_, out, ld_out)
    _ext_call(dev, "xh_pair_period_sum", T, C_, ld, f64, _vp(a.ptr), _vp(b.ptr), float(scale), P, np_ptr(s), _vp(out.ptr), ld_out)
    return out


# ---- the grid-reduction unit (include/units/xclim_hip_grid.h, xclim_amd/csrc/grid.hip) -----------------------------------
def grid_masked_dot(dev: Device, x: DeviceArray, w: DeviceArray, thr: float, outputs=("dot", "msum"), *, C_: int | None = None,
                    ld: int | None = None, outs: dict | None = None) -> dict:
    """xh_grid_masked_dot: ``x`` (T, C) float32 or float64, ``w`` (C) float64 device weights, ``thr`` in the units of the field.
    ``outputs``: keys of ``capi.GRID_OUTPUTS`` — "dot", the sums of ``(x >= thr ? x : 0) * w``, and "msum", those of
    ``(x >= thr ? 1 : 0) * w``.  Returns ``{name: DeviceArray (T) float64}``; one launch reads the field once for both.
    ``C_`` / ``ld`` / ``outs``: a padded view and output buffers of the caller's."""
    who = "grid_masked_dot"
    outputs = _subset(who, outputs, tuple(capi.GRID_OUTPUTS))
    T, width, f64 = _same_fields(who, {"x": x})
    C_, ld = _padded(width, C_, ld)
    if not isinstance(w, DeviceArray) or np.dtype(w.dtype) != np.float64 or int(np.prod(w.shape, dtype=np.int64)) < C_:
        raise TypeError(f"{who}: the weights must be a float64 device array of {C_} cells")
    outs = dict(outs or {})
    res = {o: outs[o] if o in outs else dev.empty((T,), np.float64) for o in outputs}
    _ext_call(dev, "xh_grid_masked_dot", T, C_, ld, f64, _vp(x.ptr), _vp(w.ptr), float(thr), *(_ptr(res, o) for o in capi.GRID_OUTPUTS))
    return res


def grid_box_mean(dev: Device, u: DeviceArray, T: int, ld: int, extents, strides, iz, iy, ix, *, out: DeviceArray | None = None,
                  ld_out: int | None = None) -> DeviceArray:
    """xh_grid_box_mean: ``u`` a float32 or float64 device array of at least ``T * ld`` elements whose sample (t, z, y, x) is
    element ``t * ld + z * sz + y * sy + x * sx``; ``extents`` (Z, Y, X), ``strides`` (sz, sy, sx); ``iz`` / ``iy`` / ``ix``: the
    selected indices along each axis (host integers, or int32 device arrays).  Returns the float64 (T, ny) means over the selected
    levels and longitudes of the samples that are not NaN."""
    who = "grid_box_mean"
    if np.dtype(u.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{who}: u must be float32 or float64")
    (Z, Y, X), (sz, sy, sx) = (int(v) for v in extents), (int(v) for v in strides)
    T, ld = int(T), int(ld)
    if int(np.prod(u.shape, dtype=np.int64)) < T * ld:
        raise ValueError(f"{who}: u holds fewer than T * ld = {T * ld} elements")
    lists = []
    for name, idx, n in (("iz", iz, Z), ("iy", iy, Y), ("ix", ix, X)):
        if not isinstance(idx, DeviceArray):
            h = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
            if h.size and (h.min() < 0 or h.max() >= n):
                raise ValueError(f"{who}: {name} outside [0, {n})")
            idx = dev.to_device(h.astype(np.int32)) if h.size else dev.empty((1,), np.int32)
            idx = (idx, int(h.size))
        else:
            if np.dtype(idx.dtype) != np.int32:
                raise TypeError(f"{who}: {name} must be int32")
            idx = (idx, int(np.prod(idx.shape, dtype=np.int64)))
        lists.append(idx)
    (dz, nz), (dy, ny), (dx, nx) = lists
    if out is None:
        out, ld_out = dev.empty((T, ny), np.float64), ny
    _ext_call(dev, "xh_grid_box_mean", T, ld, Z, Y, X, sz, sy, sx, int(np.dtype(u.dtype) == np.float64), _vp(u.ptr), nz, _vp(dz.ptr),
              ny, _vp(dy.ptr), nx, _vp(dx.ptr), _vp(out.ptr), ny if ld_out is None else int(ld_out))
    return out


def grid_filter_argmax(dev: Device, zm: DeviceArray, wts, outputs=("smax", "jmax"), *, ny: int | None = None, ld: int | None = None,
                       outs: dict | None = None, ld_f: int | None = None) -> dict:
    """xh_grid_filter_argmax: ``zm`` (T, ny) float64; ``wts`` host float64 (W), 1 <= W <= ``capi.GRID_MAX_WINDOW``.  ``outputs``: a
    subset of "f" (the centred filter, float64 (T, ny), NaN where the window leaves the rows or holds a NaN), "smax" (float64 (T),
    the row maximum of the values that are not NaN) and "jmax" (int32 (T), its first index, -1 for a row of NaN)."""
    who = "grid_filter_argmax"
    outputs = _subset(who, outputs, ("f", "smax", "jmax"))
    T, width = _tc(zm, np.float64)
    ny, ld = _padded(width, ny, ld)
    w = np.ascontiguousarray(wts, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError(f"{who}: the filter must have at least 1 weight")
    if w.size > capi.GRID_MAX_WINDOW:
        raise ValueError(f"{who}: filters of up to {capi.GRID_MAX_WINDOW} weights are served, got {w.size}")
    outs = dict(outs or {})
    shapes = {"f": ((T, ny), np.float64), "smax": ((T,), np.float64), "jmax": ((T,), np.int32)}
    res = {o: outs[o] if o in outs else dev.empty(*shapes[o]) for o in outputs}
    _ext_call(dev, "xh_grid_filter_argmax", T, ny, _vp(zm.ptr), ld, int(w.size), np_ptr(w), _ptr(res, "f"), ny if ld_f is None else int(ld_f),
              _ptr(res, "smax"), _ptr(res, "jmax"))
    return res
