"""Host mirror of the viticulture and agroclimatic heat-sum indices (reference: src/xclim/indices/_agro.py ``corn_heat_units``
:69-142, ``huglin_index`` :151-263, ``biologically_effective_degree_days`` :275-443, ``cool_night_index`` :447-528,
``dryness_index`` :532-724, ``latitude_temperature_index`` :728-787, ``qian_weighted_mean_average`` :1245-1284,
``effective_growing_degree_days`` :1292-1384) and of the three latitude coefficients behind them
(src/xclim/indices/helpers.py:528-806).  The kernels are in xclim_amd/csrc/agro.hip, their C ABI in
include/xclim_hip_agro.h.

The functions carry the reference's names, parameters and defaults (so ``huglin_index`` has the reference's default
``method="smoothed"``, which the reference itself refuses with NotImplementedError), plus ``time``, ``units``, ``device``,
``keep`` and ``mask_missing``.  Inputs are numpy arrays (or ``(T, C)`` device arrays) with TIME ON AXIS 0 on a daily, gap-free
:class:`~xclim_amd.timeaxis.TimeAxis`; thresholds are plain numbers in degC (the reference's defaults), ``wo`` in mm.
``units`` of the temperatures is "K" or "degC"; ``flux_units`` of ``pr`` / ``evspsblpot`` is one of anuclim's rate units
("kg m-2 s-1", "mm/s", "mm/d").  Results are float64 ``(P, *cells)`` on the periods of ``time.segments(freq)`` (``(T,
*cells)`` for the two element-wise functions), or device arrays with ``keep=True`` (which needs ``mask_missing=False``).

ASSUMPTION: float32 fields are widened to float64 before 273.15 is subtracted and everything after it is float64; the
reference subtracts in float32 and goes on in float32 for such fields, which this unit does not reproduce.

``mask_missing=True``: a period whose count of selected rows with every field present differs from
``time.expected_count(freq, ...)`` over the same selection is NaN.  The default is False, the reference's index functions.

:class:`NotServed` (the adapter forwards these to the reference): non-daily or gappy axes; ``dryness_index`` on an axis that
does not run from a 1 January to a 31 December; ``cool_night_index`` on an axis with a period that has neither a March nor a
September row; for the Jones coefficient, latitudes with a polar day or night in the season and periods without a season day
(the reference drops them, which changes the shape of the result).
"""

from __future__ import annotations

import warnings
from collections import namedtuple

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import get_device
from .calendar import select_time_mask
from .converters import day_angle
from .fields import KELVIN_OFFSET, NotServed, daily_axis as _axis, per_day as _per_day
from .timeaxis import TimeAxis, _is_leap, parse_freq

__all__ = ["corn_heat_units", "huglin_index", "biologically_effective_degree_days", "heat_sums", "cool_night_index",
           "dryness_index", "latitude_temperature_index", "qian_weighted_mean_average", "effective_growing_degree_days",
           "huglin_day_length_latitude_coefficient", "gladstones_day_length_latitude_coefficient",
           "jones_day_length_latitude_coefficient", "month_tables", "egdd_tables", "HeatSums", "NotServed"]

_SUB_C = {"K": KELVIN_OFFSET, "degC": 0.0}
HeatSums = namedtuple("HeatSums", ["huglin_index", "biologically_effective_degree_days"])


def _sub_c(units):
    try:
        return _SUB_C[units]
    except KeyError:
        raise ValueError(f"units must be one of {sorted(_SUB_C)}, got {units!r}") from None


def _lats(lat, cell_shape, who):
    """The distinct latitudes (L) and each cell's int32 index into them (C)."""
    if lat is None:
        raise ValueError(f"{who}: lat is required")
    u, inv = np.unique(F.per_cell(lat, cell_shape, "lat"), return_inverse=True)
    return u, inv.astype(np.int32).reshape(-1)


# ---- the latitude coefficients ---------------------------------------------------------------------------------------
def huglin_day_length_latitude_coefficient(lat, method: str, cap_value: float = np.nan) -> np.ndarray:
    """helpers.py:528-615: the stepwise ("huglin") or smoothed ("interpolated") coefficient of |lat|, in the shape of ``lat``.
    Beyond 50 degrees "interpolated" gives ``cap_value`` and "huglin" gives ``cap_value + 1`` — the reference's line 604 is
    ``k = xr.full_like(lat_abs, _cap_value + 1)`` — so 2.0 with the default cap of ``huglin_index``; kept as it is."""
    if not isinstance(cap_value, float):
        raise TypeError("Argument 'cap_value' must be a float (or numpy.nan).")
    la = np.abs(np.asarray(lat, dtype=np.float64))
    if method == "huglin":
        k = np.full(la.shape, cap_value + 1)
        for f, lo, hi in ((0, -np.inf, 40), (0.02, 40, 42), (0.03, 42, 44), (0.04, 44, 46), (0.05, 46, 48), (0.06, 48, 50)):
            k = np.where((lo < la) & (la <= hi), 1 + f, k)
        return k
    if method == "interpolated":
        return np.where(la <= 50, 1 + np.clip((la - 40) / 10, 0, None) * 0.06, cap_value)
    raise NotImplementedError("Method is not implemented. Only 'huglin' and 'interpolated' are permitted.")


def _day_length_table(time, lats, device):
    """(T, L) float64 hours for the latitudes ``lats`` ("spencer", no infill): one xh_solar_table call."""
    dev = device or get_device()
    _, dl = K.pet_solar_table(dev, day_angle(time), np.asarray(lats, np.float64), ra=False, dl=True)
    return dl.get()


def _gladstones_table(time, lat_u, device):
    """(T, L): dl(t, lat) / dl(t, +-40), from one table over the distinct latitudes plus the two neutral ones."""
    dl = _day_length_table(time, np.concatenate([lat_u, [40.0, -40.0]]), device)
    L = len(lat_u)
    with np.errstate(invalid="ignore"):
        return np.where(lat_u[None, :] >= 0.0, dl[:, :L] / dl[:, L:L + 1], dl[:, :L] / dl[:, L + 1:])


def gladstones_day_length_latitude_coefficient(time: TimeAxis, lat, *, device=None) -> np.ndarray:
    """helpers.py:618-685 with the "spencer" day length, ``neutral_latitude="40.0 deg"`` and no constraint: ``(T, *lat.shape)``,
    the day length of every row at ``lat`` over the one at 40 degrees of the same hemisphere; NaN in the polar day and night
    (such a day is skipped by the sums that use it)."""
    _axis(time, None, "gladstones_day_length_latitude_coefficient")
    shape = np.shape(lat)
    lat_u, li = _lats(lat, shape, "gladstones_day_length_latitude_coefficient")
    return _gladstones_table(time, lat_u, device)[:, li].reshape((len(time),) + tuple(shape))


def _jones_table(time, lat_u, start_date, end_date, freq, device):
    """(P, L) of the Jones coefficient on the periods of ``time.segments(freq)``."""
    if parse_freq(freq) not in (("Y", 1), ("Y", 7)):
        raise NotImplementedError(f"Freq {freq} not supported. Must be 'YS'/'YS-JAN', or 'YS-JUL' for method 'jones'. "
                                  "An annual frequency is required for the current implementation.")
    sel = select_time_mask(time, date_bounds=(start_date, end_date), include_bounds=(True, False))
    dl = _day_length_table(time, lat_u, device)
    if np.isnan(dl[sel]).any():
        raise NotServed("jones_day_length_latitude_coefficient: a latitude with a polar day or night in the season")
    seg = np.asarray(time.segments(freq)[0], np.int64)
    P = len(seg) - 1
    k = np.empty((P, len(lat_u)))
    for p in range(P):
        rows = np.arange(seg[p], seg[p + 1])
        rows = rows[sel[rows]]
        if rows.size == 0:
            raise NotServed("jones_day_length_latitude_coefficient: a period without a day of the season")
        k[p] = 2.8311e-4 * dl[rows].sum(axis=0) + 0.30834
    k[(k < 1.0).all(axis=1)] = np.nan      # all_below_1 over the latitudes given (helpers.py:786-787)
    if np.isnan(k).all():
        raise ValueError("All latitudes for every growing season have a day length latitude coefficient below 1.0. "
                         "This is likely due to the start and end dates of the growing season being too restrictive "
                         "or an incomplete time series.")
    return k


def jones_day_length_latitude_coefficient(time: TimeAxis, lat, method: str = "jones", floor: bool = False,
                                          start_date: str = "04-01", end_date: str = "11-01", freq: str = "YS", *,
                                          device=None) -> np.ndarray:
    """helpers.py:688-806: ``(P, *lat.shape)``, ``2.8311e-4 * S + 0.30834`` with S the sum of the day lengths over the season
    of each period ("gladstones": ``1.1135 k - 0.1352``; ``floor``: at least 1).  A period in which every latitude given is
    below 1 is NaN; ValueError when every period is.  NotImplementedError for a freq other than YS / YS-JAN / YS-JUL."""
    if method not in ("gladstones", "jones"):
        raise NotImplementedError("Method not implemented. Only 'gladstones' or 'jones' are supported.")
    _axis(time, None, "jones_day_length_latitude_coefficient")
    shape = np.shape(lat)
    lat_u, li = _lats(lat, shape, "jones_day_length_latitude_coefficient")
    k = _jones_table(time, lat_u, start_date, end_date, freq, device)
    if method == "gladstones":
        k = 1.1135 * k - 0.1352
    if floor:
        k = np.where(k >= 1.0, k, 1.0)
    return k[:, li].reshape((k.shape[0],) + tuple(shape))


# ---- huglin_index / biologically_effective_degree_days ----------------------------------------------------------------
def _finish(outs, names, valid_expected, P, cell_shape, keep):
    """Download, apply the MissingAny rule when asked (``valid_expected`` = the expected counts, else None)."""
    if keep:
        return {n: outs[n] for n in names}
    res = F.host_result({n: outs[n] for n in list(names) + (["valid"] if valid_expected is not None else [])}, P, cell_shape)
    if valid_expected is None:
        return res
    valid = res.pop("valid")
    return F.mask_incomplete(res, valid, valid_expected)


def _degree(names, fields, lat, time, factor, cap_value, tr_adj, thresh_hi, thresh_bedd, low_dtr, high_dtr, max_dd, start_date,
            end_date, freq, units, device, keep, mask_missing, who):
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    sub_C = _sub_c(units)
    got = F.native_set(fields)
    T, cell_shape, C_ = F.shape_of(got)
    _axis(time, T, who)
    seg = np.asarray(time.segments(freq)[0], np.int64)
    P = len(seg) - 1
    sel = select_time_mask(time, date_bounds=(start_date, end_date), include_bounds=(True, False))
    dev = device or get_device()
    kw = {}
    if factor in ("huglin", "interpolated"):
        if lat is None:
            raise ValueError(f"{who}: lat is required")
        k = huglin_day_length_latitude_coefficient(F.per_cell(lat, cell_shape, "lat"), factor, cap_value)
        kw = dict(k_cell=dev.to_device(np.ascontiguousarray(k)))
    elif factor == "gladstones":
        lat_u, li = _lats(lat, cell_shape, who)
        kw = dict(k_day=dev.to_device(_gladstones_table(time, lat_u, dev)), lat_idx=li)
    elif factor == "jones":
        lat_u, li = _lats(lat, cell_shape, who)
        kw = dict(k_period=dev.to_device(_jones_table(time, lat_u, start_date, end_date, freq, dev)), lat_idx=li)
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device)
    d = {n: F.rows_on_device(dev, a, T, C_) for n, a in got.items()}
    outs = K.agro_degree_sum(dev, d, seg, sel, sub_C=sub_C, thresh_hi=float(thresh_hi), thresh_bedd=float(thresh_bedd),
                             tr_adj=tr_adj, low_dtr=float(low_dtr), high_dtr=float(high_dtr), max_dd=float(max_dd),
                             outputs=list(names) + (["valid"] if mask_missing else []), **kw)
    expected = time.expected_count(freq, date_bounds=(start_date, end_date), include_bounds=(True, False)) if mask_missing else None
    return _finish(outs, names, expected, P, cell_shape, keep)


_HI_METHODS = "Method is not implemented. Only 'huglin', 'icclim', 'interpolated', and 'jones' are supported."
_BEDD_METHODS = "Method is not implemented. Only 'gladstones', 'huglin', 'icclim', 'interpolated', and 'jones' are supported."


def huglin_index(tas, tasmax, lat=None, thresh: float = 10.0, method: str = "smoothed", cap_value: float = 1.0,
                 start_date: str = "04-01", end_date: str = "10-01", freq: str = "YS", *, time: TimeAxis = None, units: str = "K",
                 device=None, keep: bool = False, mask_missing: bool = False):
    """_agro.py:151-263: the sum over the season of ``max((tas + tasmax) / 2 - thresh, 0) * k``, float64 ``(P, *cells)``.
    ``method``: "huglin" / "icclim" (deprecated, the same) / "interpolated" (k per cell from |lat|, ``cap_value`` beyond 50
    degrees) or "jones" (k per period and latitude).  ``lat`` [degrees north] broadcasts to the cells."""
    F.check_freq(freq)
    method = method.lower()
    if method == "icclim":
        warnings.warn("Method 'icclim' is deprecated. Use 'stepwise' instead.", DeprecationWarning, stacklevel=2)
        method = "huglin"
    if method not in ("huglin", "interpolated", "jones"):
        raise NotImplementedError(_HI_METHODS)
    return _degree(("hi",), dict(tas=tas, tasmax=tasmax), lat, time, method, cap_value, False, thresh, 0.0, 0.0, 0.0, np.inf,
                   start_date, end_date, freq, units, device, keep, mask_missing, "huglin_index")["hi"]


def biologically_effective_degree_days(tasmin, tasmax, lat=None, thresh_tasmin: float = 10.0, method: str = "gladstones",
                                       cap_value: float = 1.0, low_dtr: float = 10.0, high_dtr: float = 13.0,
                                       max_daily_degree_days: float = 9.0, start_date: str = "04-01", end_date: str = "11-01",
                                       freq: str = "YS", *, time: TimeAxis = None, units: str = "K", device=None,
                                       keep: bool = False, mask_missing: bool = False):
    """_agro.py:275-443: the sum over the season of ``min(max((tasmin + tasmax) / 2 - thresh_tasmin, 0) * k + tr_adj,
    max_daily_degree_days)``, float64 ``(P, *cells)`` [K days].  ``method``: "gladstones" (k per day and latitude), "huglin" /
    "interpolated" (k per cell), "jones" (k per period and latitude) or "icclim" (k = 1, no range adjustment; a ``lat`` given
    with it is not used, UserWarning)."""
    F.check_freq(freq)
    if method.lower() == "icclim":
        if lat is not None:
            warnings.warn("Lat coordinate is not used for method 'icclim' in 'biologically_effective_degree_days' calculation.",
                          UserWarning, stacklevel=2)
        factor, tr_adj = None, False
    elif method in ("gladstones", "huglin", "interpolated", "jones"):
        factor, tr_adj = method, True
    else:
        raise NotImplementedError(_BEDD_METHODS)
    return _degree(("bedd",), dict(tasmin=tasmin, tasmax=tasmax), lat, time, factor, cap_value, tr_adj, 0.0, thresh_tasmin, low_dtr,
                   high_dtr, max_daily_degree_days, start_date, end_date, freq, units, device, keep, mask_missing,
                   "biologically_effective_degree_days")["bedd"]


def heat_sums(tas, tasmin, tasmax, lat=None, *, method: str, thresh: float = 10.0, thresh_tasmin: float = 10.0,
              cap_value: float = 1.0, low_dtr: float = 10.0, high_dtr: float = 13.0, max_daily_degree_days: float = 9.0,
              start_date: str = "04-01", end_date: str = "11-01", freq: str = "YS", time: TimeAxis = None, units: str = "K",
              device=None, keep: bool = False, mask_missing: bool = False) -> HeatSums:
    """``HeatSums(huglin_index, biologically_effective_degree_days)`` of the same ``tasmax``, dates, freq and ``method`` from ONE
    launch (``tasmax`` is read once).  ``method`` is one both functions take with the same factor: "huglin", "interpolated"
    or "jones"."""
    if method not in ("huglin", "interpolated", "jones"):
        raise NotImplementedError("heat_sums: the methods both indices share are 'huglin', 'interpolated' and 'jones'")
    out = _degree(("hi", "bedd"), dict(tas=tas, tasmin=tasmin, tasmax=tasmax), lat, time, method, cap_value, True, thresh, thresh_tasmin,
                  low_dtr, high_dtr, max_daily_degree_days, start_date, end_date, freq, units, device, keep, mask_missing, "heat_sums")
    return HeatSums(out["hi"], out["bedd"])


# ---- cool_night_index / latitude_temperature_index / dryness_index ------------------------------------------------------
def month_tables(time: TimeAxis, freq: str = "YS"):
    """The host tables of ``xh_agro_monthly`` for a gap-free daily axis: ``(month_off (M + 1), month_cal (M), month_days (M),
    seg_months (P + 1))``."""
    if parse_freq(freq)[0] not in ("Y", "Q", "M"):
        raise NotServed(f"agro: periods of {freq!r} are not served")
    key = time.year * 12 + (time.month - 1)
    new = np.concatenate(([True], np.diff(key) != 0))
    month_off = np.append(np.flatnonzero(new), len(time)).astype(np.int64)
    first = time.subset(month_off[:-1])
    seg = np.asarray(time.segments(freq)[0], np.int64)
    seg_months = np.searchsorted(month_off[:-1], seg, side="left").astype(np.int64)
    return month_off, first.month.astype(np.int32), first.days_in_month().astype(np.int32), seg_months


def _hemisphere(lat, cell_shape, who, error):
    """(per-cell latitudes or None, "north" / "south" or None)"""
    if isinstance(lat, str):
        if lat.lower() not in ("north", "south"):
            raise error(f"Latitude value not implemented: {lat}.")
        return None, lat.lower()
    if lat is None:
        raise ValueError(f"{who}: lat is required (an array, 'north' or 'south')")
    return F.per_cell(lat, cell_shape, "lat"), None


def _monthly(names, fields, lat, time, freq, sub_C, per_day, wo, device, keep, mask_missing, who, error=ValueError, check=None):
    F.no_keep_with_mask(keep, mask_missing)
    got = F.native_set(fields)
    T, cell_shape, C_ = F.shape_of(got)
    _axis(time, T, who)
    month_off, month_cal, month_days, seg_months = month_tables(time, freq)
    if check is not None:
        check(month_cal, seg_months)
    P = len(seg_months) - 1
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device), cell_shape
    dev = device or get_device()
    lats, hemisphere = _hemisphere(lat, cell_shape, who, error)
    d = {n: F.rows_on_device(dev, a, T, C_) for n, a in got.items()}
    outs = K.agro_monthly(dev, d, month_off, month_cal, month_days, seg_months, lat=dev.to_device(lats) if lats is not None else None,
                          hemisphere=hemisphere, sub_C=sub_C, per_day=per_day, wo=float(wo),
                          outputs=list(names) + (["valid"] if mask_missing else []))
    return _finish(outs, names, time.expected_count(freq) if mask_missing else None, P, cell_shape, keep), cell_shape


def cool_night_index(tasmin, lat=None, freq: str = "YS", *, time: TimeAxis = None, units: str = "K", device=None,
                     keep: bool = False, mask_missing: bool = False):
    """_agro.py:447-528: the mean of ``tasmin`` [degC] over September (cells with lat > 0) or March (the others) of each year,
    float64 ``(P, *cells)``.  ``lat``: an array that broadcasts to the cells, or "north" / "south" for every cell."""
    F.check_freq(freq)
    if parse_freq(freq) != ("Y", 1):
        raise ValueError(f"Freq not allowed: {freq}. Must be `YS` or `YS-JAN`")
    if not isinstance(lat, str) and lat is None:
        raise ValueError("Latitude must be a DataArray or str ('north' or 'south').")

    def check(month_cal, seg_months):
        for a, b in zip(seg_months[:-1], seg_months[1:]):
            if not np.isin(month_cal[a:b], (3, 9)).any():
                raise NotServed("cool_night_index: a period with neither a March nor a September row")

    return _monthly(("cni",), dict(tasmin=tasmin), lat, time, freq, _sub_c(units), 1.0, 0.0, device, keep, mask_missing,
                    "cool_night_index", NotImplementedError, check)[0]["cni"]


def dryness_index(pr, evspsblpot, lat=None, wo: float = 200.0, freq: str = "YS", *, time: TimeAxis = None,
                  flux_units: str = "kg m-2 s-1", device=None, keep: bool = False, mask_missing: bool = False):
    """_agro.py:532-724: ``wo`` plus the sum over the year's months of ``P k' - E k - (E / N) (1 - k) min(P k' / 5, N)`` [mm],
    float64 ``(P, *cells)``; the year is January - December for cells with lat >= 0 and July of the year before - June for the
    others.  ``pr`` / ``evspsblpot`` are rates in ``flux_units``; ``lat``: an array, or "north" / "south" for every cell."""
    F.check_freq(freq)
    if parse_freq(freq) != ("Y", 1):
        raise ValueError(f"Freq not allowed: {freq}. Must be `YS` or `YS-JAN`")
    if not isinstance(lat, str) and lat is None:
        raise ValueError("Latitude must be a DataArray or str ('north' or 'south').")
    if isinstance(time, TimeAxis) and len(time) and not (time.month[0] == 1 and time.day[0] == 1 and time.month[-1] == 12
                                                          and time.day[-1] == (30 if time.calendar == "360_day" else 31)):
        raise NotServed("dryness_index: the axis must run from a 1 January to a 31 December")
    return _monthly(("di",), dict(pr=pr, evspsblpot=evspsblpot), lat, time, freq, 0.0, _per_day(flux_units), wo, device, keep,
                    mask_missing, "dryness_index")[0]["di"]


def latitude_temperature_index(tas, lat=None, lat_factor: float = 75, freq: str = "YS", *, time: TimeAxis = None, units: str = "K",
                               device=None, keep: bool = False, mask_missing: bool = False):
    """_agro.py:728-787: the mean temperature of the warmest month [degC] times ``lat_factor - |lat|`` (0 beyond
    ``lat_factor``), float64 ``(P, *cells)``.  The product is taken on the host, on the (P, C) result."""
    if lat is None:
        raise ValueError("latitude_temperature_index: lat is required")
    res, cell_shape = _monthly(("mtwm",), dict(tas=tas), "north", time, freq, _sub_c(units), 1.0, 0.0, device, False, mask_missing,
                               "latitude_temperature_index")
    la = np.abs(F.per_cell(lat, cell_shape, "lat")).reshape(cell_shape)
    lti = res["mtwm"] * np.where((la >= 0) & (la <= lat_factor), lat_factor - la, 0)
    if keep:
        return (device or get_device()).to_device(np.ascontiguousarray(lti.reshape(lti.shape[0], -1)))
    return lti


# ---- corn_heat_units / qian_weighted_mean_average / effective_growing_degree_days --------------------------------------
def _rows(out, T, cell_shape, keep):
    return out if keep else out.get().reshape((T,) + tuple(cell_shape))


def corn_heat_units(tasmin, tasmax, thresh_tasmin: float = 4.44, thresh_tasmax: float = 10.0, *, units: str = "K", device=None,
                    keep: bool = False):
    """_agro.py:69-142: daily corn heat units, float64 ``(T, *cells)``; a half whose comparison is false (a NaN input
    included) contributes 0, as ``xarray.where(mask, ..., 0)`` gives it."""
    sub_C = _sub_c(units)
    got = F.native_set(dict(tasmin=tasmin, tasmax=tasmax))
    T, cell_shape, C_ = F.shape_of(got)
    if T == 0 or C_ == 0:
        return F.empty_result({"chu": np.float64}, T, cell_shape, keep, device)["chu"]
    dev = device or get_device()
    out = K.corn_heat_units(dev, F.rows_on_device(dev, got["tasmin"], T, C_), F.rows_on_device(dev, got["tasmax"], T, C_), sub_C=sub_C,
                            thresh_tasmin=float(thresh_tasmin), thresh_tasmax=float(thresh_tasmax))
    return _rows(out, T, cell_shape, keep)


def qian_weighted_mean_average(tas, dim: str = "time", *, device=None, keep: bool = False):
    """_agro.py:1245-1284: the five-day binomial mean along axis 0 in the units of ``tas``, float64 ``(T, *cells)``, NaN within
    two rows of either end."""
    if dim != "time":
        raise NotServed("qian_weighted_mean_average: the time dimension (axis 0) only")
    a = F.native(tas, "tas")
    T, cell_shape, C_ = F.shape_of({"tas": a})
    if T == 0 or C_ == 0:
        return F.empty_result({"q": np.float64}, T, cell_shape, keep, device)["q"]
    dev = device or get_device()
    return _rows(K.qian_wma(dev, F.rows_on_device(dev, a, T, C_)), T, cell_shape, keep)


def egdd_tables(time: TimeAxis, freq: str = "YS", after_date: str = "07-01", start_date: str = "01-01"):
    """The host tables of ``xh_egdd``: ``(seg, doy, start_from, end_from, day0, label_doy, label_days)``.  ``start_from`` /
    ``end_from``: the row of ``start_date`` / ``after_date`` in each period (-1 when the period does not hold it); ``day0``: days
    from the period's label (its first day, present or not) to its first row."""
    seg, starts = time.segments(freq)
    if starts and len(starts[0]) != 2:
        raise NotServed(f"effective_growing_degree_days: periods of {freq!r} are not served")
    seg = np.asarray(seg, np.int64)
    P = len(seg) - 1
    start_from, end_from, day0 = (np.full(P, -1, np.int64) for _ in range(3))
    label_doy, label_days = np.ones(P, np.int32), np.full(P, 365, np.int32)
    ordinal = time.ordinal()

    def row_of(date, a, b):
        m, d = (int(v) for v in date.split("-"))
        hit = np.flatnonzero((time.month[a:b] == m) & (time.day[a:b] == d))
        return a + int(hit[0]) if hit.size else -1

    for p, (y, m) in enumerate(starts):
        a, b = int(seg[p]), int(seg[p + 1])
        label = TimeAxis(np.array([y]), np.array([m]), np.array([1]), time.calendar)
        label_doy[p] = label.doy[0]
        label_days[p] = 360 if time.calendar == "360_day" else 365 + int(bool(_is_leap(y, time.calendar)))
        day0[p] = int(ordinal[a] - label.ordinal()[0]) if b > a else 0
        if b > a:
            start_from[p], end_from[p] = row_of(start_date, a, b), row_of(after_date, a, b)
    return seg, time.doy.astype(np.int32), start_from, end_from, day0, label_doy, label_days


def effective_growing_degree_days(tasmax, tasmin, *, thresh: float = 5.0, method: str = "bootsma", after_date: str = "07-01",
                                  dim: str = "time", freq: str = "YS", time: TimeAxis = None, units: str = "K", device=None,
                                  keep: bool = False, mask_missing: bool = False, bounds: bool = False):
    """_agro.py:1292-1384: growing degree days above ``thresh`` between a start found from the temperature ("bootsma": ten
    days after the first day above ``thresh``; "qian": the first of five days whose Qian mean is above it) and the day before
    the first frost on or after ``after_date``, float64 ``(P, *cells)`` [K days]; NaN without both bounds.  ``bounds=True``
    returns ``(egdd, start, end)`` with the two days of year."""
    if method.lower() not in K.EGDD_METHODS:
        raise NotImplementedError(f"Method: {method}.")
    if dim != "time":
        raise NotServed("effective_growing_degree_days: the time dimension (axis 0) only")
    F.no_keep_with_mask(keep, mask_missing)
    sub_C = _sub_c(units)
    got = F.native_set(dict(tasmin=tasmin, tasmax=tasmax))
    T, cell_shape, C_ = F.shape_of(got)
    _axis(time, T, "effective_growing_degree_days")
    tabs = egdd_tables(time, freq, after_date)
    P = len(tabs[0]) - 1
    names = ("egdd", "start", "end") if bounds else ("egdd",)
    if P == 0 or C_ == 0:
        res = F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device)
    else:
        dev = device or get_device()
        outs = K.egdd(dev, F.rows_on_device(dev, got["tasmin"], T, C_), F.rows_on_device(dev, got["tasmax"], T, C_), *tabs,
                      method=method.lower(), sub_C=sub_C, thresh=float(thresh), outputs=list(names) + (["valid"] if mask_missing else []))
        res = _finish(outs, names, time.expected_count(freq) if mask_missing else None, P, cell_shape, keep)
    return tuple(res[n] for n in names) if bounds else res["egdd"]


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
ADAPTED = ("huglin_index", "biologically_effective_degree_days", "cool_night_index", "dryness_index", "latitude_temperature_index",
           "effective_growing_degree_days")


def make_adapters(env, originals: dict, gather_lat=None, device=None) -> dict:
    """Same-signature replacements of the six period functions of ``xclim.indices._agro`` on DataArrays with a time dimension.
    Thresholds (strings such as "10 degC", or numbers) go through ``env.convert_units_to``; the fields' ``units`` attribute
    picks the kernel's ``units`` / ``flux_units`` keyword; ``lat=None`` goes through ``gather_lat`` (the reference's
    ``_gather_lat``).  The result keeps the cell dimensions and coordinates of the first field, has the period starts of
    ``resample(time=freq)`` as its time coordinate — every period of the series, also for the two season sums, which are 0 in a
    period without a day of the season (the reference's ``select_time`` keeps the whole axis, ``drop=False``) — and the
    attributes the reference gives it.  Chunked or time-less fields, fields on different dimensions, units this module has no keyword for and everything
    :class:`NotServed` refuses go to the saved originals."""
    from .fields import FLUX_SPELLINGS, T_SPELLINGS
    from .xr_adapter import _cell_dims, forwarding_adapter, on_period_starts, served_fields, threshold_number, units_keyword

    DA = env.DataArray

    def _number(q, units):
        return threshold_number(env, q, units)

    def _lat_cells(lat, a, first):
        """lat (a DataArray over some cell dims, array-like, or None = gathered from ``first``) broadcast to the cell dims."""
        if lat is None:
            if gather_lat is None:
                raise NotServed("no lat")
            lat = gather_lat(first)
        dims = _cell_dims(a)
        if isinstance(lat, DA):
            if not set(lat.dims) <= set(dims):
                raise NotServed("lat: dimensions outside the field's cell dimensions")
            v = np.asarray(lat.transpose(*[d for d in dims if d in lat.dims]).values, np.float64)
            return v.reshape([a.shape[a.dims.index(d)] if d in lat.dims else 1 for d in dims])
        return np.asarray(lat, np.float64)

    def _serve(p, names, table):
        a, vals, time = served_fields(DA, p, names)
        units = {units_keyword(p[n], table, n) for n in names}
        if len(units) != 1:
            raise NotServed("fields in different units")
        return a, vals, time, units.pop()

    def _hi(p):
        a, v, time, units = _serve(p, ("tas", "tasmax"), T_SPELLINGS)
        lat = _lat_cells(p["lat"], a, p["tas"])
        out = huglin_index(v["tas"], v["tasmax"], lat, _number(p["thresh"], "degC"), p["method"], p["cap_value"], p["start_date"],
                           p["end_date"], p["freq"], time=time, units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": ""})

    def _bedd(p):
        a, v, time, units = _serve(p, ("tasmin", "tasmax"), T_SPELLINGS)
        icclim = str(p["method"]).lower() == "icclim"
        lat = p["lat"] if icclim and p["lat"] is None else _lat_cells(p["lat"], a, p["tasmin"])
        out = biologically_effective_degree_days(
            v["tasmin"], v["tasmax"], lat, _number(p["thresh_tasmin"], "degC"), p["method"], p["cap_value"], _number(p["low_dtr"], "degC"),
            _number(p["high_dtr"], "degC"), _number(p["max_daily_degree_days"], "degC"), p["start_date"], p["end_date"], p["freq"],
            time=time, units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": "K days"})

    def _cni(p):
        a, v, time, units = _serve(p, ("tasmin",), T_SPELLINGS)
        lat = p["lat"] if isinstance(p["lat"], str) else _lat_cells(p["lat"], a, p["tasmin"])
        out = cool_night_index(v["tasmin"], lat, p["freq"], time=time, units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], dict(p["tasmin"].attrs, units="degC"))

    def _di(p):
        a, v, time, units = _serve(p, ("pr", "evspsblpot"), FLUX_SPELLINGS)
        lat = p["lat"] if isinstance(p["lat"], str) else _lat_cells(p["lat"], a, p["pr"])
        out = dryness_index(v["pr"], v["evspsblpot"], lat, _number(p["wo"], "mm"), p["freq"], time=time, flux_units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": "mm"})

    def _lti(p):
        a, v, time, units = _serve(p, ("tas",), T_SPELLINGS)
        out = latitude_temperature_index(v["tas"], _lat_cells(p["lat"], a, p["tas"]), p["lat_factor"], p["freq"], time=time, units=units,
                                         device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": ""})

    def _egdd(p):
        a, v, time, units = _serve(p, ("tasmax", "tasmin"), T_SPELLINGS)
        out = effective_growing_degree_days(v["tasmax"], v["tasmin"], thresh=_number(p["thresh"], "degC"), method=p["method"],
                                            after_date=p["after_date"], dim=p["dim"], freq=p["freq"], time=time, units=units, device=device)
        # to_agg_units(egdd, tas [degC], op="integral") (_agro.py:1383)
        return env.to_agg_units(on_period_starts(DA, a, out, p["freq"], {}), DA(np.zeros(1), dims=("x",), attrs={"units": "degC"}), "integral")

    runners = {"huglin_index": _hi, "biologically_effective_degree_days": _bedd, "cool_night_index": _cni, "dryness_index": _di,
               "latitude_temperature_index": _lti, "effective_growing_degree_days": _egdd}
    return {name: forwarding_adapter(name, originals[name], runners[name]) for name in ADAPTED}
