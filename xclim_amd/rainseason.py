"""Host mirror of ``rain_season`` and ``hardiness_zones`` (reference: src/xclim/indices/_agro.py:796-980 and :1388-1433, with
``get_zones`` / ``_get_zone_bins`` of src/xclim/indices/generic.py:1611-1708).  The kernels are in xclim_amd/csrc/rainseason.hip,
their C ABI in include/xclim_hip_rain.h.  With these two, every function of ``_agro.py`` has a device form.

The two functions carry the reference's names, parameters and defaults (thresholds as plain numbers in mm), plus ``time``,
``flux_units`` / ``units``, ``device``, ``keep`` and, for ``rain_season``, ``mask_missing``.  Inputs are numpy arrays (or ``(T, C)``
device arrays) with TIME ON AXIS 0 on a daily, gap-free :class:`~xclim_amd.timeaxis.TimeAxis`.  Results are float64
``(P, *cells)`` on the periods of ``time.segments(freq)``, or device arrays with ``keep=True`` (which needs
``mask_missing=False``).

``rain_season`` is ONE launch of ``xh_rain_season``: the three date selections of the reference are made here, per period, with
``calendar.select_time_mask`` and travel as one flag byte per row (:func:`rain_flags`); nothing calendar-aware runs on the device.

ASSUMPTIONS (xarray is neither needed nor used here).  All arithmetic is float64 on the widened field: a float32
"kg m-2 s-1" field is multiplied by 86400 in float64 and compared with float64 thresholds, where the reference goes on in
float32; likewise the rolling mean of float32 period minima is a float64 mean.  Window sums are added in row order from their
first term (where xarray runs on bottleneck its running sum rounds differently).  The bin edges of the zones are
``(degF + 459.67) * 5 / 9`` in K, less 273.15 in degC, in float64.

:class:`NotServed` (the adapter forwards these to the reference): non-daily or gappy axes, sum windows beyond
``RAIN_MAX_WINDOW`` rows (``window_wet_start`` always, ``window_dry_start`` / ``window_dry_end`` with their "total" method), a
period with no row inside the start or the end bounds (xarray raises there), a period whose rows inside the start window are not
its last rows (periods longer than a year).
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import RAIN_END_BOUNDS, RAIN_MAX_WINDOW, RAIN_START_BOUNDS, RAIN_START_WINDOW, get_device
from .calendar import select_time_mask
from .fields import KELVIN_OFFSET, NotServed, daily_axis
from .fields import per_day as _per_day
from .timeaxis import TimeAxis

__all__ = ["rain_season", "hardiness_zones", "rain_flags", "zone_edges", "RainSeason", "NotServed", "RAIN_MAX_WINDOW", "ADAPTED",
           "make_adapters"]

RainSeason = namedtuple("RainSeason", ["rain_season_start", "rain_season_end", "rain_season_length"])
_METHODS = ("per_day", "total")


def _int(name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name} must be an integer of at least {least}, got {v!r}")
    return int(v)


def rain_flags(time: TimeAxis, seg, date_min_start="05-01", date_max_start="12-31", date_min_end="09-01", date_max_end="12-31"):
    """The flag byte of every row for ``xh_rain_season``: ``RAIN_START_WINDOW`` inside ``date_bounds = (date_min_start, the
    month-day of the LAST row of the row's period)`` (_agro.py:905-906), ``RAIN_START_BOUNDS`` inside ``(date_min_start,
    date_max_start)``, ``RAIN_END_BOUNDS`` inside ``(date_min_end, date_max_end)`` (:899).  A date selection looks at a row's month
    and day only, so the two bounds are one mask of the whole axis and the start window one mask per distinct last day.
    :class:`NotServed` for a period without a row inside the start or the end bounds, and for a period whose start-window rows
    are not its last rows."""
    seg = np.asarray(seg, np.int64)
    flags = np.zeros(len(time), np.uint8)
    flags[select_time_mask(time, date_bounds=(date_min_start, date_max_start))] |= RAIN_START_BOUNDS
    flags[select_time_mask(time, date_bounds=(date_min_end, date_max_end))] |= RAIN_END_BOUNDS
    windows = {}
    for k in range(len(seg) - 1):
        r0, r1 = int(seg[k]), int(seg[k + 1])
        if r1 <= r0:
            continue
        last = f"{int(time.month[r1 - 1]):02d}-{int(time.day[r1 - 1]):02d}"
        if last not in windows:
            windows[last] = select_time_mask(time, date_bounds=(date_min_start, last))
        inside = windows[last][r0:r1]
        flags[r0:r1][inside] |= RAIN_START_WINDOW
        if (np.diff(inside.astype(np.int8)) < 0).any():
            raise NotServed("rain_season: a period whose start window is not made of its last rows")
        for bit, what in ((RAIN_START_BOUNDS, "start"), (RAIN_END_BOUNDS, "end")):
            if not (flags[r0:r1] & bit).any():
                raise NotServed(f"rain_season: a period with no row inside the {what} bounds")
    return flags


def rain_season(pr, thresh_wet_start: float = 25.0, window_wet_start: int = 3, window_not_dry_start: int = 30,
                thresh_dry_start: float = 1.0, window_dry_start: int = 7, method_dry_start: str = "per_day",
                date_min_start: str = "05-01", date_max_start: str = "12-31", thresh_dry_end: float = 0.0, window_dry_end: int = 20,
                method_dry_end: str = "per_day", date_min_end: str = "09-01", date_max_end: str = "12-31", freq: str = "YS-JAN", *,
                time: TimeAxis = None, flux_units: str = "kg m-2 s-1", device=None, keep: bool = False,
                mask_missing: bool = False) -> RainSeason:
    """_agro.py:796-980: ``RainSeason(rain_season_start, rain_season_end, rain_season_length)``, the day of year of the start and
    of the end of the rain season of every period and its length in days, float64 ``(P, *cells)`` with NaN.  ``pr`` is a rate in
    ``flux_units``; the thresholds are daily amounts in mm.  One launch of ``xh_rain_season``."""
    who = "rain_season"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    if method_dry_start not in _METHODS:
        raise ValueError(f"Unknown method_dry_start: {method_dry_start}.")
    if method_dry_end not in _METHODS:
        raise ValueError(f"Unknown method_dry_end: {method_dry_end}.")
    per_day = _per_day(flux_units)
    ww = _int("window_wet_start", window_wet_start, 1)
    wnd = _int("window_not_dry_start", window_not_dry_start, 0)
    wd = _int("window_dry_start", window_dry_start, 1)
    we = _int("window_dry_end", window_dry_end, 1)
    for name, w, is_sum in (("window_wet_start", ww, True), ("window_dry_start", wd, method_dry_start == "total"),
                            ("window_dry_end", we, method_dry_end == "total")):
        if is_sum and w > RAIN_MAX_WINDOW:
            raise NotServed(f"{who}: sum windows of up to {RAIN_MAX_WINDOW} rows are served, got {name} = {w}")
    a = F.native(pr, "pr")
    T, cell_shape, C_ = F.shape_of({"pr": a})
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    flags = rain_flags(time, seg, date_min_start, date_max_start, date_min_end, date_max_end)
    names = RainSeason._fields
    if P == 0 or C_ == 0:
        return RainSeason(**F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device))
    dev = device or get_device()
    x = F.rows_on_device(dev, a, T, C_)
    outs = K.rain_season(dev, x, seg, flags, time.doy, per_day=per_day, thresh_wet_start=float(thresh_wet_start), window_wet_start=ww,
                         window_not_dry_start=wnd, thresh_dry_start=float(thresh_dry_start), window_dry_start=wd,
                         method_dry_start=method_dry_start, thresh_dry_end=float(thresh_dry_end), window_dry_end=we,
                         method_dry_end=method_dry_end)
    outs = dict(zip(names, (outs[o] for o in K.RAIN_OUTPUTS)))
    if keep:
        return RainSeason(**outs)
    res = F.host_result(outs, P, cell_shape)
    if mask_missing:   # MissingAny: a period whose rows with a value are not all the days of the period
        valid = K.resample_reduce(dev, x, "count", seg, want_valid=False)[0].get().reshape((P,) + tuple(cell_shape))
        res = F.mask_incomplete(res, valid, time.expected_count(freq))
    return RainSeason(**res)


def zone_edges(method: str = "usda", units: str = "K") -> np.ndarray:
    """The bin edges of ``_get_zone_bins`` (generic.py:1633-1639) for the two methods of ``hardiness_zones`` (:1420-1427), in the
    field's ``units`` ("K" or "degC"), float64: -60 .. 70 degF or -15 .. 20 degC in steps of 5."""
    if units not in ("K", "degC"):
        raise ValueError(f"units must be one of ['K', 'degC'], got {units!r}")
    if not isinstance(method, str) or method.lower() not in ("usda", "anbg"):
        raise NotImplementedError(f"Method must be one of `usda` or `anbg`. Got {method}.")
    if method.lower() == "usda":
        kelvin = (np.arange(-60.0, 70.0 + 5.0, 5.0) + 459.67) * 5.0 / 9.0
        return kelvin if units == "K" else kelvin - KELVIN_OFFSET
    celsius = np.arange(-15.0, 20.0 + 5.0, 5.0)
    return celsius + KELVIN_OFFSET if units == "K" else celsius


def hardiness_zones(tasmin, window: int = 30, method: str = "usda", freq: str = "YS", *, time: TimeAxis = None, units: str = "K",
                    device=None, keep: bool = False):
    """_agro.py:1388-1433: the hardiness zone of the mean over ``window`` periods of the period minimum of ``tasmin``, float64
    ``(P, *cells)``; NaN for the first ``window - 1`` periods, where a minimum of the window is NaN and outside the zones.  Zones
    count from 0 ("usda": half zones, 26 of them; "anbg": 7).  ``xh_resample_reduce`` (min) + ``xh_rolling_zones``."""
    who = "hardiness_zones"
    F.check_freq(freq)
    edges = zone_edges(method, units)
    window = _int("window", window, 1)
    a = F.native(tasmin, "tasmin")
    T, cell_shape, C_ = F.shape_of({"tasmin": a})
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return F.empty_result({"zones": np.float64}, P, cell_shape, keep, device)["zones"]
    dev = device or get_device()
    tn_min = K.resample_reduce(dev, F.rows_on_device(dev, a, T, C_), "min", seg, want_valid=False)[0]
    out = K.rolling_zones(dev, tn_min, window, edges)
    return out if keep else out.get().reshape((P,) + tuple(cell_shape))


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
ADAPTED = ("rain_season", "hardiness_zones")


def make_adapters(env, originals: dict, device=None) -> dict:
    """Same-signature replacements of ``rain_season`` and ``hardiness_zones`` of ``xclim.indices._agro`` on DataArrays with a time
    dimension.  Thresholds (strings such as "25.0 mm", or numbers) go through ``env.convert_units_to``; the field's ``units``
    attribute picks ``flux_units`` / ``units``.  The results keep the cell dimensions and coordinates of the field, have the period
    starts of ``resample(time=freq)`` as their time coordinate and the reference's attributes (:977-979, :1432).  Chunked or
    time-less fields, units this module has no keyword for and everything :class:`NotServed` refuses go to the saved originals;
    no other exception is caught."""
    from .fields import FLUX_SPELLINGS, T_SPELLINGS
    from .xr_adapter import forwarding_adapter, on_period_starts, served_fields, threshold_number, units_keyword

    DA = env.DataArray

    def _rain(p):
        a, v, time = served_fields(DA, p, ("pr",))
        flux = units_keyword(p["pr"], FLUX_SPELLINGS, "pr")
        mm = [threshold_number(env, p[n], "mm") for n in ("thresh_wet_start", "thresh_dry_start", "thresh_dry_end")]
        out = rain_season(v["pr"], mm[0], p["window_wet_start"], p["window_not_dry_start"], mm[1], p["window_dry_start"],
                          p["method_dry_start"], p["date_min_start"], p["date_max_start"], mm[2], p["window_dry_end"], p["method_dry_end"],
                          p["date_min_end"], p["date_max_end"], p["freq"], time=time, flux_units=flux, device=device)
        doy = {"units": "", "is_dayofyear": np.int32(1)}
        return (on_period_starts(DA, a, out.rain_season_start, p["freq"], dict(doy)),
                on_period_starts(DA, a, out.rain_season_end, p["freq"], dict(doy)),
                on_period_starts(DA, a, out.rain_season_length, p["freq"], {"units": "days"}))

    def _zones(p):
        a, v, time = served_fields(DA, p, ("tasmin",))
        units = units_keyword(p["tasmin"], T_SPELLINGS, "tasmin")
        out = hardiness_zones(v["tasmin"], p["window"], p["method"], p["freq"], time=time, units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": ""})

    runners = {"rain_season": _rain, "hardiness_zones": _zones}
    return {name: forwarding_adapter(name, originals[name], runners[name]) for name in ADAPTED}
