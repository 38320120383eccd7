"""Host mirror of the compound percentile-day counts ``cold_and_dry_days``, ``warm_and_dry_days``, ``warm_and_wet_days`` and
``cold_and_wet_days`` (reference: src/xclim/indices/_multivariate.py:162-423), ``degree_days_exceedance_date``
(src/xclim/indices/_threshold.py:3215-3310), ``blowing_snow`` (_multivariate.py:1833-1884) and ``water_cycle_intensity``
(:1888-1918).  The kernels are in xclim_amd/csrc/compound.hip, their C ABI in include/units/xclim_hip_compound.h.

The seven functions carry the reference's names, parameters and defaults (thresholds as plain numbers in the units of the data),
plus ``time``, ``device``, ``keep`` and ``mask_missing`` (and ``units`` / ``flux_units`` where a default or a factor depends on
them).  Inputs are numpy arrays (or ``(T, C)`` device arrays) with TIME ON AXIS 0 on a daily, gap-free
:class:`~xclim_amd.timeaxis.TimeAxis`.  Results are float64 ``(P, *cells)`` on the periods of ``time.segments(freq)``, or ``(P, C)``
device arrays with ``keep=True`` (which needs ``mask_missing=False``).  :func:`compound_days` is the fused form of the four counts:
any subset of them from ONE launch of ``xh_compound_doy_days``, which reads ``tas`` and ``pr`` once.

The percentile tables are :class:`~xclim_amd.calendar.DoyPercentile` objects (as ``percentile_doy`` returns them: the table stays on
the device) or arrays ``(ndoy, *cells)`` whose row ``k`` is day of year ``k + 1``.  A table whose day-of-year axis differs from the
field's calendar goes through ``calendar.adjust_doy_calendar``, as in ``calendar.resample_doy``; no ``(T, cells)`` threshold field
is made.

ASSUMPTIONS (xarray is neither needed nor used here).  All arithmetic is float64 on the widened fields.  The counts compare a
float32 sample with the float64 table in float64, as numpy does: widening is exact and the counts are the reference's bit for bit.
The running sum of ``degree_days_exceedance_date`` is float64, added in row order, of ``tas - thresh`` (or ``thresh - tas``) in the
units of the field; on a float32 field the reference converts to K and accumulates in float32.  The window sum of ``blowing_snow``
is added in row order from its first term (where xarray runs on bottleneck its running sum rounds differently).
``water_cycle_intensity`` adds ``(pr + evspsbl) * seconds per day`` in float64 in row order, where the reference stays in the
fields' dtype.

:class:`NotServed` (the adapter forwards these to the reference): non-daily or gappy axes, a ``freq`` the axis does not parse, a
table that does not cover every day of year of the field or tables on different day-of-year axes, windows beyond
``BS_MAX_WINDOW`` rows.
"""

from __future__ import annotations

import types

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import BS_MAX_WINDOW, CD_OUTPUTS, DeviceArray, get_device
from .calendar import DoyPercentile, adjust_doy_calendar, select_time_mask
from .fields import KELVIN_OFFSET, NotServed, daily_axis
from .fields import per_day as _per_day
from .run_length import index_of_date
from .timeaxis import TimeAxis

__all__ = ["cold_and_dry_days", "warm_and_dry_days", "warm_and_wet_days", "cold_and_wet_days", "compound_days",
           "degree_days_exceedance_date", "blowing_snow", "water_cycle_intensity", "compound_table_rows", "compound_tables",
           "exceedance_tables", "blowing_snow_periods", "COMPOUND_OUTPUTS", "NotServed", "BS_MAX_WINDOW", "multivariate", "threshold",
           "ADAPTED", "make_adapters"]

# the reference's names -> the outputs of xh_compound_doy_days, in the order of their bits
COMPOUND_OUTPUTS = dict(zip(("cold_and_dry_days", "warm_and_dry_days", "warm_and_wet_days", "cold_and_wet_days"), CD_OUTPUTS))
_TABLE_ARGS = {"tas_lo": "tas_per_low", "tas_hi": "tas_per_high", "pr_lo": "pr_per_low", "pr_hi": "pr_per_high"}
_BELOW = ("<", "lt", "<=", "le")
_ABOVE = (">", "gt", ">=", "ge")


def _valid_rows(dev, x, seg):
    return K.resample_reduce(dev, x, "count", seg, want_valid=False)[0].get()


def _missing_any(res: dict, dev, fields, seg, time, freq, cell_shape, rows=slice(None)) -> dict:
    """MissingAny on downloaded results: NaN where a field of the period has a row without a value."""
    expected = np.asarray(time.expected_count(freq))
    for x in fields:
        valid = _valid_rows(dev, x, seg)[rows].reshape((-1,) + tuple(cell_shape))
        res = F.mask_incomplete(res, valid, expected[rows])
    return res


# ---- the four compound percentile-day counts --------------------------------------------------------------------------------
def _doy_table(name, per, cell_shape, dev):
    """A percentile table as a one-percentile DoyPercentile on the cells of the fields."""
    if isinstance(per, DoyPercentile):
        if tuple(per.cell_shape) != tuple(cell_shape):
            raise ValueError(f"{name}: cells {tuple(per.cell_shape)} differ from the fields' {tuple(cell_shape)}")
        if len(per.percentiles) != 1:
            raise ValueError(f"{name}: select one percentile first (DoyPercentile.sel)")
        return per
    if isinstance(per, DeviceArray):
        if np.dtype(per.dtype) != np.float64 or len(per.shape) != 2 or int(per.shape[1]) != int(np.prod(cell_shape, dtype=np.int64)):
            raise TypeError(f"{name}: a device table must be float64 (ndoy, C)")
        data = per.reshape(1, int(per.shape[0]), int(per.shape[1]))
        return DoyPercentile(data, np.arange(1, int(per.shape[0]) + 1), [np.nan], cell_shape, {})
    a = np.asarray(per, dtype=np.float64)
    if a.ndim < 1 or tuple(a.shape[1:]) != tuple(cell_shape):
        raise ValueError(f"{name}: shape {a.shape} is not (ndoy, *cells) on the cells {tuple(cell_shape)}")
    return DoyPercentile(None, np.arange(1, a.shape[0] + 1), [np.nan], cell_shape, {}, host=a[None], device=dev)


def compound_table_rows(tables: dict, time: TimeAxis):
    """The table row of every field row (``resample_doy_index``) on the day-of-year axis the tables have after
    ``adjust_doy_calendar`` — known on the host: a table that ends on the last day of year of the calendar keeps its own axis, any
    other is re-gridded onto the days of year of ``time``.  ``tables``: {kernel table name: DoyPercentile}.  :class:`NotServed` for a
    table that does not hold every day of year of the axis and for tables on different day-of-year axes."""
    tidx, axis = None, None
    for k, per in tables.items():
        doys = np.asarray(per.dayofyear)
        if int(doys.max()) != time.max_doy():
            doys = np.arange(int(time.doy.min()), int(time.doy.max()) + 1)
        pos = np.clip(np.searchsorted(doys, time.doy), 0, len(doys) - 1)
        if not np.all(doys[pos] == time.doy):
            raise NotServed(f"{_TABLE_ARGS[k]}: the day-of-year table does not cover every day of the time axis")
        if axis is not None and not np.array_equal(doys, axis):
            raise NotServed("the percentile tables must share their day-of-year axis")
        tidx, axis = pos.astype(np.int32), doys
    return tidx


def compound_tables(tables: dict, time: TimeAxis, dev):
    """``{kernel table name: (ndoy, C) float64 DeviceArray}``: every table on the day-of-year axis of ``time``
    (``adjust_doy_calendar``, an interpolation on the device where the axes differ)."""
    out = {}
    for k, per in tables.items():
        adoy = adjust_doy_calendar(per, time, dev)
        out[k] = adoy.data.reshape(int(adoy.data.shape[1]), int(adoy.data.shape[2]))
    return out


def compound_days(tas, pr, tas_per_low=None, tas_per_high=None, pr_per_low=None, pr_per_high=None,
                  outputs=tuple(COMPOUND_OUTPUTS), freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False,
                  mask_missing: bool = False) -> dict:
    """Any subset of the four compound counts (``outputs``: names of ``COMPOUND_OUTPUTS``) from ONE launch of
    ``xh_compound_doy_days``: the days of every period with ``tas`` below ``tas_per_low`` / above ``tas_per_high`` AND ``pr`` below
    ``pr_per_low`` / above ``pr_per_high``, float64 ``{name: (P, *cells)}``.  A NaN on either side of a compare is False.  Only the
    tables the requested outputs need are looked at."""
    who = "compound_days"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    outputs = tuple(outputs)
    if not outputs or set(outputs) - set(COMPOUND_OUTPUTS):
        raise ValueError(f"{who}: outputs must be a non-empty subset of {', '.join(COMPOUND_OUTPUTS)}")
    outputs = tuple(o for o in COMPOUND_OUTPUTS if o in outputs)
    given = {"tas_lo": tas_per_low, "tas_hi": tas_per_high, "pr_lo": pr_per_low, "pr_hi": pr_per_high}
    needed = [t for t in K.CD_TABLES if any(t in K.CD_NEEDS[COMPOUND_OUTPUTS[o]] for o in outputs)]
    for t in needed:
        if given[t] is None:
            raise ValueError(f"{who}: {', '.join(outputs)} need {_TABLE_ARGS[t]}")
    f = F.native_set({"tas": tas, "pr": pr})
    T, cell_shape, C_ = F.shape_of(f)
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    pers = {t: _doy_table(_TABLE_ARGS[t], given[t], cell_shape, device) for t in needed}
    tidx = compound_table_rows(pers, time)
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(outputs, np.float64), P, cell_shape, keep, device)
    dev = device or get_device()
    tables = compound_tables(pers, time, dev)
    x = {n: F.rows_on_device(dev, a, T, C_) for n, a in f.items()}
    outs = K.compound_doy_days(dev, x["tas"], x["pr"], tables, tidx, seg, [COMPOUND_OUTPUTS[o] for o in outputs])
    outs = {o: outs[COMPOUND_OUTPUTS[o]] for o in outputs}
    if keep:
        return outs
    res = F.host_result(outs, P, cell_shape)
    if mask_missing:
        res = _missing_any(res, dev, x.values(), seg, time, freq, cell_shape)
    return res


def _one(name, tables):
    def fn(tas, pr, tas_per, pr_per, freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False,
           mask_missing: bool = False):
        return compound_days(tas, pr, **dict(zip(tables, (tas_per, pr_per))), outputs=(name,), freq=freq, time=time, device=device,
                             keep=keep, mask_missing=mask_missing)[name]

    fn.__name__ = fn.__qualname__ = name
    return fn


cold_and_dry_days = _one("cold_and_dry_days", ("tas_per_low", "pr_per_low"))
cold_and_dry_days.__doc__ = """_multivariate.py:162-219: the days of every period with ``tas < tas_per`` and ``pr < pr_per``."""
warm_and_dry_days = _one("warm_and_dry_days", ("tas_per_high", "pr_per_low"))
warm_and_dry_days.__doc__ = """_multivariate.py:228-285: the days of every period with ``tas > tas_per`` and ``pr < pr_per``."""
warm_and_wet_days = _one("warm_and_wet_days", ("tas_per_high", "pr_per_high"))
warm_and_wet_days.__doc__ = """_multivariate.py:294-351: the days of every period with ``tas > tas_per`` and ``pr > pr_per``."""
cold_and_wet_days = _one("cold_and_wet_days", ("tas_per_low", "pr_per_high"))
cold_and_wet_days.__doc__ = """_multivariate.py:360-417: the days of every period with ``tas < tas_per`` and ``pr > pr_per``."""


# ---- degree_days_exceedance_date ---------------------------------------------------------------------------------------------
def _doy_from_string(date: str, year: int, calendar: str) -> int:
    """core/calendar.py:114-135."""
    parts = str(date).split("-")
    if len(parts) != 2:
        raise ValueError("Day of year must be in the format 'MM-DD'.")
    return int(TimeAxis([year], [int(parts[0])], [int(parts[1])], calendar).doy[0])


def exceedance_tables(time: TimeAxis, seg, after_date=None, never_reached=None):
    """The per-period host tables of ``xh_degree_exceedance_date``: ``start`` (int64, P), the row of ``after_date`` inside the
    period (``index_of_date(..., max_idxs=1, default=0)`` on the period's own rows: the period's first row without a date), -1 for
    a period that does not hold the date; ``never`` (float64, P): NaN for None, the integer, or ``doy_from_string`` of the year of
    the period's first row."""
    seg = np.asarray(seg, np.int64)
    P = len(seg) - 1
    start, never = np.full(P, -1, np.int64), np.full(P, np.nan)
    if never_reached is not None and not isinstance(never_reached, str):
        if isinstance(never_reached, bool) or not isinstance(never_reached, (int, np.integer)):
            raise TypeError("never_reached must be None, an integer day of year or an 'MM-DD' string")
    for p in range(P):
        r0, r1 = int(seg[p]), int(seg[p + 1])
        if r1 <= r0:
            continue
        idx = index_of_date(time.subset(slice(r0, r1)), after_date, max_idxs=1, default=0)
        if idx.size:
            start[p] = r0 + int(idx[0])
        if isinstance(never_reached, str):
            never[p] = _doy_from_string(never_reached, int(time.year[r0]), time.calendar)
        elif never_reached is not None:
            never[p] = float(never_reached)
    return start, never


def degree_days_exceedance_date(tas, thresh: float = None, sum_thresh: float = 25.0, op: str = ">", after_date: str = None,
                                never_reached=None, freq: str = "YS", *, time: TimeAxis = None, units: str = "K", device=None,
                                keep: bool = False, mask_missing: bool = False):
    """_threshold.py:3215-3310: the day of year on which the sum of ``max(tas - thresh, 0)`` (``op`` ">": above; "<": ``thresh -
    tas``), started on ``after_date`` ("MM-DD"; default: the first day of the period), first exceeds ``sum_thresh`` K days;
    float64 ``(P, *cells)``.  ``thresh`` is in the ``units`` of the field ("K" / "degC"; default 0 degC).  Where the sum is never
    above ``sum_thresh``: ``never_reached``, an integer day of year or an "MM-DD" string (its day of year in the period's first
    year), NaN for None.  A period that does not hold ``after_date`` is NaN, and so is, as in the reference, a period whose every
    row is above ``sum_thresh`` (the exceedance on the period's first row, or a negative ``sum_thresh``: ``find_boundary_run``
    answers NaN when ``argmax == argmin``).  One launch of ``xh_degree_exceedance_date``."""
    who = "degree_days_exceedance_date"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    if units not in ("K", "degC"):
        raise ValueError(f"units must be one of ['K', 'degC'], got {units!r}")
    if op in _BELOW:
        below = True
    elif op in _ABOVE:
        below = False
    else:
        raise NotImplementedError(f"op: '{op}'.")
    if thresh is None:
        thresh = KELVIN_OFFSET if units == "K" else 0.0
    a = F.native(tas, "tas")
    T, cell_shape, C_ = F.shape_of({"tas": a})
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    start, never = exceedance_tables(time, seg, after_date, never_reached)
    if P == 0 or C_ == 0:
        return F.empty_result({"out": np.float64}, P, cell_shape, keep, device)["out"]
    dev = device or get_device()
    x = F.rows_on_device(dev, a, T, C_)
    out = K.degree_exceedance_date(dev, x, seg, start, never, time.doy, thresh=float(thresh), sum_thresh=float(sum_thresh), below=below)
    if keep:
        return out
    res = F.host_result({"out": out}, P, cell_shape)
    if mask_missing:
        res = _missing_any(res, dev, [x], seg, time, freq, cell_shape)
    return res["out"]


# ---- blowing_snow ------------------------------------------------------------------------------------------------------------
def blowing_snow_periods(seg):
    """``diff`` drops the first row of the series (_multivariate.py:1875), so the periods of the result are those of rows
    ``1 .. T - 1``: the index of the first period of ``seg`` that the result keeps (1 when row 0 is alone in its period)."""
    seg = np.asarray(seg, np.int64)
    return 1 if len(seg) > 1 and seg[1] <= 1 else 0


def blowing_snow(snd, sfcWind, snd_thresh: float = 0.05, sfcWind_thresh: float = 15.0 / 3.6, window: int = 3, freq: str = "YS-JUL", *,
                 time: TimeAxis = None, device=None, keep: bool = False, mask_missing: bool = False, **indexer):
    """_multivariate.py:1833-1884: the days of every period on which the snow depth gained at least ``snd_thresh`` over the last
    ``window`` days (the sum of ``window`` day-to-day differences) and the wind speed is at least ``sfcWind_thresh``; float64
    ``(P', *cells)``.  The thresholds are in the units of the fields (the defaults are the reference's 5 cm and 15 km/h for fields
    in m and m s-1).  ``**indexer`` (``season=`` / ``month=`` / ``doy_bounds=`` / ``date_bounds=``) selects rows after the window
    sum.  The periods are those of rows ``1 .. T - 1`` (:func:`blowing_snow_periods`).  One launch of ``xh_blowing_snow_days``."""
    who = "blowing_snow"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be an integer of at least 1, got {window!r}")
    if window > BS_MAX_WINDOW:
        raise NotServed(f"{who}: windows of up to {BS_MAX_WINDOW} rows are served, got {window}")
    f = F.native_set({"snd": snd, "sfcWind": sfcWind})
    T, cell_shape, C_ = F.shape_of(f)
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    first = blowing_snow_periods(seg)
    P = len(seg) - 1 if T > 1 else first
    flags = select_time_mask(time, **indexer) if any(v is not None for k, v in indexer.items() if k != "include_bounds") else None
    if P - first <= 0 or C_ == 0:
        return F.empty_result({"out": np.float64}, max(P - first, 0), cell_shape, keep, device)["out"]
    dev = device or get_device()
    x = {n: F.rows_on_device(dev, a, T, C_) for n, a in f.items()}
    out = K.blowing_snow_days(dev, x["snd"], x["sfcWind"], seg, flags, snd_thresh=float(snd_thresh), wind_thresh=float(sfcWind_thresh),
                              window=int(window))
    if first:   # the period that holds nothing but row 0 is absent from the reference's result
        kept = dev.wrap(out.ptr + C_ * 8, (P - 1, C_), np.float64)
        kept._owner = out
        out = kept
    if keep:
        return out
    res = F.host_result({"out": out}, P - first, cell_shape)
    if mask_missing:
        res = _missing_any(res, dev, x.values(), seg, time, freq, cell_shape, slice(first, None))
    return res["out"]


# ---- water_cycle_intensity ---------------------------------------------------------------------------------------------------
def water_cycle_intensity(pr, evspsbl, freq: str = "YS", *, time: TimeAxis = None, flux_units: str = "kg m-2 s-1", device=None,
                          keep: bool = False, mask_missing: bool = False):
    """_multivariate.py:1888-1918: the period sums of the daily amounts of ``pr + evspsbl`` (``rate2amount`` on a daily axis: the
    rate times the seconds of a day, or times 1 for "mm/d"), NaN terms skipped; float64 ``(P, *cells)``.  Both fields in
    ``flux_units``.  One launch of ``xh_pair_period_sum``: neither the sum field nor the amount field exists."""
    who = "water_cycle_intensity"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    scale = _per_day(flux_units)
    f = F.native_set({"pr": pr, "evspsbl": evspsbl})
    T, cell_shape, C_ = F.shape_of(f)
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return F.empty_result({"out": np.float64}, P, cell_shape, keep, device)["out"]
    dev = device or get_device()
    x = {n: F.rows_on_device(dev, a, T, C_) for n, a in f.items()}
    out = K.pair_period_sum(dev, x["pr"], x["evspsbl"], seg, scale)
    if keep:
        return out
    res = F.host_result({"out": out}, P, cell_shape)
    if mask_missing:
        res = _missing_any(res, dev, x.values(), seg, time, freq, cell_shape)
    return res["out"]


# ---- the xarray adapters (patch.install) -------------------------------------------------------------------------------------
# The replaced functions are defined in two modules of the reference and patch.install_mirror wants one defining module per mirror:
# two namespaces, each with its own ADAPTED and make_adapters.  make_adapters holds runners only.
def _same_dtype(v: dict):
    kinds = {np.dtype(a.dtype) for a in v.values()}
    if len(kinds) != 1 or not kinds <= {np.dtype(np.float32), np.dtype(np.float64)}:
        raise NotServed("integer fields or fields of mixed dtype")


def _number(env, q, like, **kw):
    """A scalar threshold (a string with units or a number) in the units of the DataArray ``like``."""
    if isinstance(q, str):
        return float(env.convert_units_to(q, like, **kw))
    if isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, bool):
        return float(q)
    raise NotServed("a threshold that is neither a string nor a number")


def _multivariate_adapters(env, originals: dict, device=None) -> dict:
    """The four compound counts, ``blowing_snow`` and ``water_cycle_intensity`` of ``xclim.indices._multivariate``: one launch each.
    The percentile tables pass ``convert_units_to(tas_per, tas)`` and ``convert_units_to(pr_per, pr, context="hydro")`` and must be
    DataArrays on ``dayofyear`` and the cell dimensions of the fields (a lone ``percentiles`` dimension of length 1 is dropped)."""
    from .xr_adapter import _tfirst_fields, forwarding_adapter, is_chunked, on_period_starts, served_fields, units_keyword

    DA = env.DataArray

    def table(per, like, a, **kw):
        if not isinstance(per, DA) or "dayofyear" not in per.dims or is_chunked(per):
            raise NotServed("a percentile table that is not an in-memory DataArray on dayofyear")
        per = env.convert_units_to(per, like, **kw)
        if "percentiles" in per.dims:
            if per.shape[per.dims.index("percentiles")] != 1:
                raise NotServed("a table of several percentiles")
            per = per.sel(percentiles=per["percentiles"].values[0])
        cells = tuple(d for d in a.dims if d != "time")
        if set(per.dims) != set(cells) | {"dayofyear"}:
            raise NotServed("a percentile table on other dimensions than the fields")
        per = per.transpose("dayofyear", *cells)
        doys = np.asarray(per["dayofyear"].values)
        return DoyPercentile(None, doys, [np.nan], per.shape[1:], dict(per.attrs), host=np.asarray(per.values, np.float64)[None],
                             device=device)

    def count(name, tables):
        def run(p):
            a, v, time = served_fields(DA, p, ("tas", "pr"))
            _same_dtype(v)
            per = dict(zip(tables, (table(p["tas_per"], p["tas"], a), table(p["pr_per"], p["pr"], a, context="hydro"))))
            out = compound_days(v["tas"], v["pr"], **per, outputs=(name,), freq=p["freq"], time=time, device=device)[name]
            return env.to_agg_units(on_period_starts(DA, a, out, p["freq"], {}), p["tas"], "count", deffreq="D")
        return run

    def _snow(p):
        indexer = p.get("indexer") or {}
        a, v, time = served_fields(DA, p, ("snd", "sfcWind"))
        _same_dtype(v)
        out = blowing_snow(v["snd"], v["sfcWind"], _number(env, p["snd_thresh"], p["snd"]), _number(env, p["sfcWind_thresh"], p["sfcWind"]),
                           p["window"], p["freq"], time=time, device=device, **indexer)
        whole = on_period_starts(DA, a.isel(time=slice(1, None)), out, p["freq"], {})
        return whole.assign_attrs(units=env.to_agg_units(whole, p["snd"], "count", deffreq="D"))

    def _wci(p):
        from .fields import FLUX_SPELLINGS

        flux = units_keyword(p["evspsbl"], FLUX_SPELLINGS, "evspsbl")
        if units_keyword(p["pr"], FLUX_SPELLINGS, "pr") != flux and _per_day(units_keyword(p["pr"], FLUX_SPELLINGS, "pr")) != _per_day(flux):
            raise NotServed("pr and evspsbl in different units")
        a, v = _tfirst_fields(DA, {"pr": p["pr"], "evspsbl": p["evspsbl"]})
        if any(x.shape != a.shape for x in v.values()):
            raise NotServed("fields on different dimensions")
        _same_dtype(v)
        from .xr_adapter import time_axis_of

        out = water_cycle_intensity(v["pr"], v["evspsbl"], p["freq"], time=time_axis_of(a), flux_units=flux, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": "mm" if flux.startswith("mm") else "kg m-2"})

    runners = {"cold_and_dry_days": count("cold_and_dry_days", ("tas_per_low", "pr_per_low")),
               "warm_and_dry_days": count("warm_and_dry_days", ("tas_per_high", "pr_per_low")),
               "warm_and_wet_days": count("warm_and_wet_days", ("tas_per_high", "pr_per_high")),
               "cold_and_wet_days": count("cold_and_wet_days", ("tas_per_low", "pr_per_high")),
               "blowing_snow": _snow, "water_cycle_intensity": _wci}
    return {n: forwarding_adapter(n, originals[n], runners[n]) for n in multivariate.ADAPTED}


def _threshold_adapters(env, originals: dict, device=None) -> dict:
    """``degree_days_exceedance_date`` of ``xclim.indices._threshold``: one launch of ``xh_degree_exceedance_date``; the result has
    ``units=""``, ``is_dayofyear`` and the calendar of the field (:3309)."""
    from .fields import T_SPELLINGS
    from .xr_adapter import forwarding_adapter, on_period_starts, served_fields, threshold_number, units_keyword

    DA = env.DataArray

    def _dded(p):
        a, v, time = served_fields(DA, p, ("tas",))
        _same_dtype(v)
        units = units_keyword(p["tas"], T_SPELLINGS, "tas")
        thresh = threshold_number(env, p["thresh"], units)
        sum_thresh = p["sum_thresh"]
        if isinstance(sum_thresh, str):
            sum_thresh = float(env.convert_units_to(sum_thresh, DA(np.zeros(1), dims=("x",), attrs={"units": "K days"})))
        elif isinstance(sum_thresh, bool) or not isinstance(sum_thresh, (int, float, np.integer, np.floating)):
            raise NotServed("a threshold that is neither a string nor a number")
        out = degree_days_exceedance_date(v["tas"], thresh, float(sum_thresh), p["op"], p["after_date"], p["never_reached"], p["freq"],
                                          time=time, units=units, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": "", "is_dayofyear": np.int32(1), "calendar": time.calendar})

    return {"degree_days_exceedance_date": forwarding_adapter("degree_days_exceedance_date", originals["degree_days_exceedance_date"], _dded)}


multivariate = types.SimpleNamespace(ADAPTED=("cold_and_dry_days", "warm_and_dry_days", "warm_and_wet_days", "cold_and_wet_days",
                                              "blowing_snow", "water_cycle_intensity"), make_adapters=_multivariate_adapters)
threshold = types.SimpleNamespace(ADAPTED=("degree_days_exceedance_date",), make_adapters=_threshold_adapters)
ADAPTED = multivariate.ADAPTED + threshold.ADAPTED


def make_adapters(env, originals: dict, device=None) -> dict:
    """Same-signature replacements of the seven functions (``ADAPTED``) on DataArrays with a time dimension: the adapters of both
    namespaces.  Chunked or time-less fields, integer fields and fields of mixed dtype, units this module has no keyword for,
    array-valued thresholds and everything :class:`NotServed` refuses go to the saved originals; no other exception is caught."""
    return {**_multivariate_adapters(env, originals, device), **_threshold_adapters(env, originals, device)}
