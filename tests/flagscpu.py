"""The data-quality flags of xclim.core.dataflags restated in numpy (TEST INFRASTRUCTURE ONLY): the masks of the five check kinds of
include/xclim_hip_flags.h on ``oracle.run_length.suspicious_run``, ``oracle.calendar.climatological_mean_doy`` and plain numpy
comparisons, their aggregation over periods and cells, and ``data_flags`` on the plans of ``xclim_amd.dataflags.describe`` (names,
thresholds and descriptions are host bookkeeping of the mirror; every mask is computed here).

A sample compared with a threshold is widened to float64 first (the ASSUMPTION of the header); samples compared with samples or
with the bound tables are compared in the field's dtype."""
import operator
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import calendar as ocal  # noqa: E402
from oracle import run_length as orl  # noqa: E402

OPS = {">": operator.gt, "<": operator.lt, ">=": operator.ge, "<=": operator.le, "==": operator.eq, "!=": operator.ne}


def doy_bounds(x, time, window, n):
    """(lo, hi, doys): ``m -+ n * s`` of ``climatological_mean_doy`` in the dtype of ``x``; ``time`` has ``.doy``."""
    x = np.asarray(x)
    m, s, doys = ocal.climatological_mean_doy(x, time, window)
    n = x.dtype.type(n)
    with np.errstate(invalid="ignore"):
        return m - n * s, m + n * s, doys


def clim_mask(x, time, window, n, tables=None):
    """``~within_bnds_doy``: True where the sample is not strictly inside its day's bounds (NaN and a zero deviation included)."""
    x = np.asarray(x)
    lo, hi, doys = tables if tables is not None else doy_bounds(x, time, window, n)
    idx = np.searchsorted(doys, time.doy)
    with np.errstate(invalid="ignore"):
        return ~((lo[idx] < x) & (x < hi[idx]))


def mask(x, spec, companions=None, time=None, tables=None):
    """The ``(T, *cells)`` bool mask of one check: ("cmp", op, a) | ("outside", a, b) | ("pair", op, name or array) | ("repeat", op or
    None, a, n) | ("clim", n, window)."""
    x = np.asarray(x)
    wide = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if spec[0] == "cmp":
            return OPS[spec[1]](wide, float(spec[2]))
        if spec[0] == "outside":
            return (wide < float(spec[1])) | (wide > float(spec[2]))
        if spec[0] == "pair":
            y = companions[spec[2]] if isinstance(spec[2], str) else spec[2]
            return OPS[spec[1]](x, np.asarray(y))
        if spec[0] == "repeat":
            runs = orl.suspicious_run(x, window=spec[3])
            return runs if spec[1] is None else runs & OPS[spec[1]](wide, float(spec[2]))
        if spec[0] == "clim":
            return clim_mask(x, time, spec[2], spec[1], tables)
    raise ValueError(spec[0])


def aggregate(m, seg, reduce_cells):
    """``any`` over the rows of every period (False for an empty one), and over the cells as well with ``reduce_cells``."""
    m = np.asarray(m, bool)
    seg = np.asarray(seg)
    out = np.zeros((len(seg) - 1,) + m.shape[1:], bool)
    for p, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        out[p] = m[a:b].any(axis=0)
    return out.reshape(len(out), -1).any(axis=1) if reduce_cells else out


def flags(x, specs, seg, reduce_cells, companions=None, time=None, tables=None):
    """What ``xh_data_flags`` returns: uint8 (K, P, C), or (K, P) with ``reduce_cells``; ``x`` (T, C)."""
    out = [aggregate(mask(x, s, companions, time, tables), seg, reduce_cells) for s in specs]
    P = len(seg) - 1
    return np.array(out, np.uint8).reshape((len(specs), P) if reduce_cells else (len(specs), P, np.shape(x)[1]))


def data_flags(da, ds=None, flags=None, dims="all", freq=None, *, name, time=None, units=None, variables=None):
    """``data_flags`` of the reference on numpy arrays: flag name -> bool array or None."""
    from xclim_amd import dataflags as D

    ds = {} if ds is None else ds
    plans = D.describe(name, flags, ds, units, variables)
    T = np.shape(da)[0]
    if freq is not None:
        seg = np.asarray(time.segments(freq)[0])
    out = {}
    for label, plan in plans.items():
        if plan is None:
            out[label] = None
            continue
        m = mask(da, plan[0], ds, time)
        if freq is not None:
            m = aggregate(m, seg, False)
        elif dims in ("all", "time"):
            m = m.any(axis=0)
        if dims in ("all", "cells"):
            m = m.reshape(m.shape[:0 if (freq is None and dims == "all") else 1] + (-1,)).any(axis=-1)
        out[label] = m
    return out
