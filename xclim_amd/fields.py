"""The host front end of a unit that takes several named ``(T, *cells)`` fields (ffdi, converters, chill, anuclim, agro,
hydrology, rainseason and the adapter callees of fire): dtypes, shapes, uploads, per-cell inputs, the empty result, the
download, and the transposition of the time-last arrays ``xr.apply_ufunc`` hands over.  The period units (chill, anuclim,
agro, hydrology, rainseason) also take their period front end from here: the ``freq`` check, the period offsets, the
``keep`` / ``mask_missing`` guard, the MissingAny mask of downloaded results, and the unit tables their adapters share.

float32 and float64 fields are taken as given and every other dtype is widened to float64 (exact), so nothing here depends on
``XCLIM_AMD_FLOAT64``; the single-field float32 indices keep ``calendar._flatten``, which carries that policy.  This module
imports numpy and ``_capi`` only (``daily_axis`` reaches for ``converters`` when it is called): every mirror and ``xr_adapter``
can import it.
"""

from __future__ import annotations

import numpy as np

from ._capi import DeviceArray, get_device

__all__ = ["NotServed", "Forward", "SERVED", "native", "native_set", "shape_of", "rows_on_device", "per_cell", "empty_result",
           "host_result", "time_first", "time_last", "FLUX_UNITS", "FLUX_SPELLINGS", "T_SPELLINGS", "KELVIN_OFFSET", "per_day", "daily_axis",
           "check_freq", "period_segments", "no_keep_with_mask", "mask_incomplete"]

SERVED = (np.float32, np.float64)


# the precipitation-rate units of the daily units (agro, hydrology): the factor that makes a rate a daily amount in mm (kg m-2),
# and the spellings of the ``units`` attribute their adapters take for them
FLUX_UNITS = ("kg m-2 s-1", "mm/s", "mm/d")
_FLUX_PER_DAY = {"kg m-2 s-1": 86400.0, "mm/s": 86400.0, "mm/d": 1.0}
FLUX_SPELLINGS = {"kg m-2 s-1": "kg m-2 s-1", "kg/m2/s": "kg m-2 s-1", "mm/s": "mm/s", "mm s-1": "mm/s", "mm/d": "mm/d", "mm/day": "mm/d",
                  "mm d-1": "mm/d", "mm day-1": "mm/d", "mm / d": "mm/d"}
KELVIN_OFFSET = 273.15  # pint's degC <-> K offset
# the spellings of a temperature's ``units`` attribute the adapters take for the kernels' "K" / "degC"
T_SPELLINGS = {"K": "K", "kelvin": "K", "degK": "K", "degC": "degC", "°C": "degC", "celsius": "degC", "degree_Celsius": "degC", "C": "degC"}


class NotServed(NotImplementedError):
    """A form the device path does not take (an unserved time axis, calendar, distribution ...); the xarray adapters forward
    it to the reference."""


class Forward(Exception):
    """A form an ``apply_ufunc`` callee does not take: the adapter hands the call to the reference's own function."""


def per_day(flux_units):
    """Seconds (or days) per day of a precipitation rate in ``flux_units``: rate * per_day = the daily amount in mm."""
    if flux_units not in FLUX_UNITS:
        raise ValueError(f"flux_units must be one of {list(FLUX_UNITS)}, got {flux_units!r}")
    return _FLUX_PER_DAY[flux_units]


def daily_axis(time, T, who):
    """``time`` is the daily, gap-free TimeAxis of the ``T`` rows (``T`` None: any length); :class:`NotServed` for an axis that is
    not, in the name of ``who``."""
    from .converters import _check_time
    from .timeaxis import TimeAxis

    if not isinstance(time, TimeAxis):
        raise TypeError("time must be the daily TimeAxis of the rows")
    if T is not None and T != len(time):
        raise ValueError(f"time has {len(time)} rows, the fields {T}")
    try:
        _check_time(time)
    except NotServed as e:
        raise NotServed(str(e).replace("potential evapotranspiration", who)) from None


def check_freq(freq):
    """The reference's own complaint about a ``freq`` that is not a string."""
    if not isinstance(freq, str):
        raise TypeError("Freq must be a string.")


def period_segments(time, freq):
    """The int64 row offsets (P + 1) of the periods of ``time.segments(freq)``; :class:`NotServed` for a ``freq`` the axis does not
    parse."""
    try:
        return np.asarray(time.segments(freq)[0], np.int64)
    except NotImplementedError as e:
        raise NotServed(str(e)) from None


def no_keep_with_mask(keep, mask_missing):
    """The mask is applied on the host, to downloaded results: ``keep`` cannot have it."""
    if keep and mask_missing:
        raise ValueError("keep=True returns the device arrays as computed: pass mask_missing=False")


def mask_incomplete(res: dict, valid, expected) -> dict:
    """The MissingAny rule on downloaded results: float64 copies of ``{name: (P, *cells)}`` with NaN where ``valid`` (P, *cells), the
    rows with a value, differs from ``expected`` (P), the rows of a complete period.  An integer count becomes float64."""
    bad = valid != np.asarray(expected).reshape((valid.shape[0],) + (1,) * (valid.ndim - 1))
    out = {}
    for n, v in res.items():
        out[n] = v.astype(np.float64)
        out[n][bad] = np.nan
    return out


def native(a, name):
    """A field as float32 / float64 (other dtypes widened to float64); device arrays must already be one of the two."""
    if isinstance(a, DeviceArray):
        if np.dtype(a.dtype) not in SERVED:
            raise TypeError(f"{name}: device arrays must be float32 or float64, got {np.dtype(a.dtype).name}")
        return a
    a = np.asarray(a)
    return a if a.dtype in SERVED else a.astype(np.float64)


def native_set(fields: dict) -> dict:
    """The fields that are not None, as :func:`native`, sharing one dtype: a mixed set is widened to float64 (device arrays
    must share it already)."""
    out = {n: native(a, n) for n, a in fields.items() if a is not None}
    if len({np.dtype(a.dtype) for a in out.values()}) > 1:
        if any(isinstance(a, DeviceArray) for a in out.values()):
            raise TypeError(f"{', '.join(out)}: device arrays must share one dtype")
        out = {n: a.astype(np.float64) for n, a in out.items()}
    return out


def shape_of(fields: dict):
    """(T, cell_shape, C) of the fields; every field must have the shape of the first."""
    shapes = {n: tuple(a.shape) for n, a in fields.items()}
    first = next(iter(shapes.values()))
    if len(first) < 1:
        raise ValueError("fields must have a time axis (axis 0)")
    for n, s in shapes.items():
        if s != first:
            raise ValueError(f"{n}: shape {s} differs from {first}")
    return first[0], first[1:], int(np.prod(first[1:], dtype=np.int64))


def rows_on_device(dev, a, rows, C_):
    """The field as a ``(rows, C)`` device array: a view of a device array, an upload of anything else."""
    if isinstance(a, DeviceArray):
        return a.reshape(rows, C_)
    return dev.to_device(np.ascontiguousarray(a).reshape(rows, C_))


def per_cell(a, cell_shape, name):
    """A per-cell input broadcast to the cell shape, as a float64 (C) array (None stays None)."""
    if a is None:
        return None
    try:
        b = np.broadcast_to(np.asarray(a, dtype=np.float64), cell_shape)
    except ValueError:
        raise ValueError(f"{name}: shape {np.shape(a)} does not broadcast to the cell shape {tuple(cell_shape)}") from None
    return np.ascontiguousarray(b).reshape(-1)


def empty_result(dtypes: dict, rows, cell_shape, keep=False, device=None) -> dict:
    """What a unit returns without a launch when there are no rows or no cells: ``{name: (rows, *cells)}`` numpy arrays of
    ``dtypes[name]``, or ``(rows, C)`` device arrays with ``keep``."""
    if keep:
        dev, C_ = device or get_device(), int(np.prod(cell_shape, dtype=np.int64))
        return {n: dev.empty((rows, C_), dt) for n, dt in dtypes.items()}
    return {n: np.empty((rows,) + tuple(cell_shape), dt) for n, dt in dtypes.items()}


def host_result(outs: dict, rows, cell_shape) -> dict:
    """``{name: (rows, C) device array}`` downloaded, in order, as ``{name: (rows, *cells)}``."""
    return {n: v.get().reshape((rows,) + tuple(cell_shape)) for n, v in outs.items()}


def time_first(a, loop=None):
    """A time-last array ``(..., n)`` as a C-contiguous time-first ``(n, C)`` one; ``loop`` broadcasts its leading axes to
    that loop shape first."""
    a = np.asarray(a)
    if loop is not None:
        a = np.broadcast_to(a, tuple(loop) + a.shape[-1:])
    return np.ascontiguousarray(np.moveaxis(a, -1, 0)).reshape(a.shape[-1], int(np.prod(a.shape[:-1], dtype=np.int64)))


def time_last(a, loop):
    """A time-first ``(n, C)`` numpy array as the time-last ``(*loop, n)`` view."""
    return np.moveaxis(a.reshape(a.shape[:1] + tuple(loop)), 0, -1)
