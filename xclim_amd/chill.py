"""Host mirror of the winter-chill indices (reference: src/xclim/indices/_agro.py:1436-1592 ``chill_portions`` /
``chill_units``, src/xclim/indices/helpers.py:977-1123 ``make_hourly_temperature``).

``chill_portions`` (the Dynamic Model) and ``chill_units`` (the Utah model) run in ``xh_chill_hourly``: one lane per
(cell, period) marches down the hours of its period.  The workflow the reference recommends,
``chill_portions(make_hourly_temperature(tasmin, tasmax))``, runs as ONE launch of ``xh_chill_daily``: the 24 hourly
temperatures of a day are built in registers from ``tasmin``, ``tasmax`` and a day-length table and fed to the same hour
step, so the hourly field (24 times the daily one, in float64) never exists.  See xclim_amd/csrc/chill.hip.

Inputs are numpy arrays (or ``(rows, C)`` device arrays) with TIME ON AXIS 0.  ``time`` is always the DAILY
:class:`~xclim_amd.timeaxis.TimeAxis` of the days: an hourly field has exactly ``24 * len(time)`` rows, day-major from hour
0 (sub-daily time axes are not served in general; the hourly field rides on the daily axis).  float32 and float64 fields are
read natively and computed in float64; other dtypes are widened to float64 first.  Results are float64 ``(P, *cells)`` on
the periods of ``time.segments(freq)``, or ``(P, C)`` device arrays with ``keep=True`` (which needs ``mask_missing=False``:
the mask is applied on the host).

``mask_missing=True`` applies the MissingAny rule on hours, as the reference's indicators do: a period is NaN unless its
count of selected, non-NaN hours equals ``24 * time.expected_count(freq, **indexer)``.  The default is False, the
reference's index functions.  ASSUMPTION: a period without a single selected hour (``month=[12, 1, 2]`` with ``freq="MS"``
in July) is NaN for chill portions; what xarray's resample gives for a period that ``select_time(drop=True)`` emptied could
not be executed where this was written.  Chill units of a period without data are 0, as the reference's sum is.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import get_device
from .converters import NotServed, _check_time, _lat_table, day_angle
from .fields import KELVIN_OFFSET
from .timeaxis import TimeAxis

__all__ = ["make_hourly_temperature", "chill_portions", "chill_units", "chill_portions_from_daily", "chill_units_from_daily",
           "chill_from_daily", "ChillIndices", "NotServed", "HOURS"]

HOURS = 24
ChillIndices = namedtuple("ChillIndices", ["chill_portions", "chill_units"])

_UNITS = {"K": (0.0, KELVIN_OFFSET), "degC": (KELVIN_OFFSET, 0.0)}
_INDEXERS = ("season", "month", "doy_bounds", "date_bounds", "include_bounds")


def _offsets(units):
    """(add_K, sub_C): what takes the field to K and to degC; one of the two is 0."""
    try:
        return _UNITS[units]
    except KeyError:
        raise ValueError(f"units must be one of {sorted(_UNITS)}, got {units!r}") from None


def day_selection(time: TimeAxis, **indexer):
    """The per-day mask of ``select_time(**indexer)`` (None without an indexer)."""
    unknown = set(indexer) - set(_INDEXERS)
    if unknown:
        raise TypeError(f"unknown indexer {sorted(unknown)}; one of season, month, doy_bounds, date_bounds")
    from .calendar import select_time_mask

    return select_time_mask(time, **indexer)


def row_selection(time: TimeAxis, **indexer):
    """The hourly ``row_sel`` of an indexer: the per-day mask repeated 24 times (None without an indexer)."""
    m = day_selection(time, **indexer)
    return None if m is None else np.repeat(np.asarray(m, bool), HOURS)


def hourly_segments(time: TimeAxis, freq: str):
    """Hourly row offsets of the periods: ``24 * time.segments(freq)``."""
    seg, _ = time.segments(freq)
    return HOURS * np.asarray(seg, np.int64)


def hourly_expected_count(time: TimeAxis, freq: str, **indexer):
    """Hours a complete period holds: ``24 * time.expected_count(freq, **indexer)``."""
    return HOURS * np.asarray(time.expected_count(freq, **indexer), np.int64)


def _check_hourly(rows, time):
    if not isinstance(time, TimeAxis):
        raise TypeError("time must be the daily TimeAxis of the days")
    if rows != HOURS * len(time):
        raise ValueError(f"the hourly field has {rows} rows; {HOURS} * {len(time)} days = {HOURS * len(time)} expected "
                         "(day-major from hour 0)")


def _selected_days(time, seg, sel):
    """Selected days of each period (``seg`` in day offsets)."""
    if sel is None:
        return np.diff(seg)
    return np.array([int(np.sum(sel[a:b])) for a, b in zip(seg[:-1], seg[1:])], np.int64)


def _reduce(run, names, time, freq, indexer, cell_shape, C_, P, nsel, keep, mask_missing, device):
    """Shared tail: ``run(outputs) -> {name: DeviceArray}`` with cp / cu / valid, then the period rules."""
    F.no_keep_with_mask(keep, mask_missing)
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device)
    outs = run(list(names) + ([] if keep else ["valid"]))
    if keep:
        return {n: outs[n] for n in names}
    res = F.host_result({n: outs[n] for n in ("valid",) + tuple(names)}, P, cell_shape)
    valid = res.pop("valid")
    if mask_missing:
        expected = hourly_expected_count(time, freq, **indexer).reshape((P,) + (1,) * len(cell_shape))
    for n, a in res.items():
        if n == "cp":
            a[nsel == 0] = np.nan  # a period without a selected hour (see the module text)
        if mask_missing:
            a[valid != expected] = np.nan
    return res


def _hourly(tas, time, freq, units, names, positive_only, indexer, device, keep, mask_missing):
    add_K, sub_C = _offsets(units)
    tas = F.native(tas, "tas")
    H, cell_shape, C_ = F.shape_of({"tas": tas})
    _check_hourly(H, time)
    seg = hourly_segments(time, freq)
    P = len(seg) - 1
    sel = row_selection(time, **indexer)
    nsel = _selected_days(time, seg // HOURS, day_selection(time, **indexer))

    def run(outputs):
        dev = device or get_device()
        return K.chill_hourly(dev, F.rows_on_device(dev, tas, H, C_), seg, sel, add_K=add_K, sub_C=sub_C,
                              positive_only=positive_only, outputs=outputs)

    return _reduce(run, names, time, freq, indexer, cell_shape, C_, P, nsel, keep, mask_missing, device)


def chill_portions(tas, time: TimeAxis, freq: str = "YS", *, units: str = "K", device=None, keep: bool = False,
                   mask_missing: bool = False, **indexer):
    """_agro.py:1482-1534: chill portions of the Dynamic Model per period, float64 ``(P, *cells)``.  ``tas`` is the hourly
    field ``(24 * len(time), *cells)`` in ``units`` ("K" or "degC"), ``time`` the daily axis of its days.  ``**indexer``
    (``season`` / ``month`` / ``doy_bounds`` / ``date_bounds``) is ``select_time(..., drop=True)``: unselected days are
    skipped and the state carries across the gap inside a period; the selected field is never materialised."""
    return _hourly(tas, time, freq, units, ("cp",), False, indexer, device, keep, mask_missing)["cp"]


def chill_units(tas, time: TimeAxis, positive_only: bool = False, freq: str = "YS", *, units: str = "degC", device=None,
                keep: bool = False, mask_missing: bool = False):
    """_agro.py:1537-1592: chill units of the Utah model per period, float64 ``(P, *cells)``; with ``positive_only`` only
    calendar days with a positive sum are added.  The reference takes no indexer here, and neither does this."""
    return _hourly(tas, time, freq, units, ("cu",), positive_only, {}, device, keep, mask_missing)["cu"]


def _daily_inputs(tasmin, tasmax, lat, time, infill_polar_days):
    if infill_polar_days:
        raise NotServed("make_hourly_temperature: infill_polar_days=True is not served")
    tn, tx = F.native_set({"tasmin": tasmin, "tasmax": tasmax}).values()  # (a mixed pair is float64, as its difference would be)
    D, cell_shape, C_ = F.shape_of({"tasmin": tn, "tasmax": tx})
    if not isinstance(time, TimeAxis):
        raise TypeError("time must be the daily TimeAxis of the days")
    if D != len(time):
        raise ValueError(f"time has {len(time)} rows, the fields {D}")
    try:
        _check_time(time)
    except NotServed as e:
        raise NotServed(str(e).replace("potential evapotranspiration", "make_hourly_temperature")) from None
    lat_u, li = _lat_table(lat, cell_shape)
    return tn, tx, cell_shape, C_, lat_u, li


def _daily(tasmin, tasmax, lat, time, freq, units, names, positive_only, indexer, device, keep, mask_missing,
           infill_polar_days=False):
    add_K, sub_C = _offsets(units)
    tn, tx, cell_shape, C_, lat_u, li = _daily_inputs(tasmin, tasmax, lat, time, infill_polar_days)
    D = len(time)
    seg = np.asarray(time.segments(freq)[0], np.int64)
    P = len(seg) - 1
    sel = day_selection(time, **indexer)
    nsel = _selected_days(time, seg, sel)

    def run(outputs):
        dev = device or get_device()
        _, dl = K.pet_solar_table(dev, day_angle(time), lat_u, ra=False, dl=True)
        return K.chill_daily(dev, F.rows_on_device(dev, tn, D, C_), F.rows_on_device(dev, tx, D, C_), dl, li, seg, sel,
                             add_K=add_K, sub_C=sub_C, positive_only=positive_only, outputs=outputs)

    return _reduce(run, names, time, freq, indexer, cell_shape, C_, P, nsel, keep, mask_missing, device)


def make_hourly_temperature(tasmin, tasmax, lat, time: TimeAxis, infill_polar_days: bool = False, *, device=None,
                            keep: bool = False):
    """helpers.py:1059-1123: Linvill's sine / log profile, float64 ``(24 * D, *cells)`` in the inputs' units.  ``time`` is the
    daily, gap-free axis, ``lat`` [degrees north] broadcasts to the cells.  Sunrise is at hour 0 of every day and sunset
    ``day_lengths`` hours later; the night runs to the next day's ``tasmin`` (the last day's to its own).  Polar days and
    nights have a NaN day length and give NaN hours; ``infill_polar_days=True`` raises :class:`NotServed`."""
    tn, tx, cell_shape, C_, lat_u, li = _daily_inputs(tasmin, tasmax, lat, time, infill_polar_days)
    D = len(time)
    if C_ == 0:
        return F.empty_result({"hourly": np.float64}, HOURS * D, cell_shape, keep, device)["hourly"]
    dev = device or get_device()
    _, dl = K.pet_solar_table(dev, day_angle(time), lat_u, ra=False, dl=True)
    out = K.chill_daily(dev, F.rows_on_device(dev, tn, D, C_), F.rows_on_device(dev, tx, D, C_), dl, li, [0, D],
                        outputs=("hourly",))
    return (out if keep else F.host_result(out, HOURS * D, cell_shape))["hourly"]


def chill_portions_from_daily(tasmin, tasmax, lat, time: TimeAxis, freq: str = "YS", *, units: str = "K", device=None,
                              keep: bool = False, mask_missing: bool = False, **indexer):
    """``chill_portions(make_hourly_temperature(tasmin, tasmax, lat, time), time, freq, units=units, **indexer)`` in one
    launch, bit for bit, without the hourly field."""
    return _daily(tasmin, tasmax, lat, time, freq, units, ("cp",), False, indexer, device, keep, mask_missing)["cp"]


def chill_units_from_daily(tasmin, tasmax, lat, time: TimeAxis, positive_only: bool = False, freq: str = "YS", *,
                           units: str = "degC", device=None, keep: bool = False, mask_missing: bool = False):
    """``chill_units(make_hourly_temperature(tasmin, tasmax, lat, time), time, positive_only, freq, units=units)`` in one
    launch, bit for bit."""
    return _daily(tasmin, tasmax, lat, time, freq, units, ("cu",), positive_only, {}, device, keep, mask_missing)["cu"]


def chill_from_daily(tasmin, tasmax, lat, time: TimeAxis, positive_only: bool = False, freq: str = "YS", *, units: str = "K",
                     device=None, keep: bool = False, mask_missing: bool = False, **indexer):
    """Both indices from one launch: ``ChillIndices(chill_portions, chill_units)``.  The indexer applies to BOTH (the
    reference's ``chill_units`` has none: pass no indexer for its result)."""
    out = _daily(tasmin, tasmax, lat, time, freq, units, ("cp", "cu"), positive_only, indexer, device, keep, mask_missing)
    return ChillIndices(out["cp"], out["cu"])


# ---- the adapter callee (patch.install): the reference's numpy function, time LAST ------------------------------------
_Forward = F.Forward


def chill_portion_one_season(tas_K, *, device=None):
    """Drop-in for ``_chill_portion_one_season(tas_K)`` (_agro.py:1442-1465) on the numpy array ``xr.apply_ufunc`` passes:
    time last, any loop shape, temperatures in K; returns ``delta`` in the input's shape and dtype (for float32 the
    float64 ``delta`` rounded once).  Raises ``_Forward`` for other dtypes, 0-d and empty arrays."""
    a = np.asarray(tas_K)
    if a.dtype not in F.SERVED or a.ndim < 1 or a.size == 0:
        raise _Forward("dtype or shape")
    dev = device or get_device()
    out = K.chill_hourly(dev, dev.to_device(F.time_first(a)), [0, a.shape[-1]], add_K=0.0, sub_C=KELVIN_OFFSET,
                         outputs=("delta",))["delta"]
    return F.time_last(out.get(), a.shape[:-1]).astype(a.dtype)


def make_adapters(orig):
    """The module attribute patch.install() puts into xclim.indices._agro; it forwards to the saved original for the forms
    the device path does not take."""

    def _chill_portion_one_season(tas_K):
        try:
            return chill_portion_one_season(tas_K)
        except _Forward:
            return orig(tas_K)

    _chill_portion_one_season.__wrapped__ = orig
    return {"_chill_portion_one_season": _chill_portion_one_season}
