"""Host mirror of potential evapotranspiration and the water budget (reference: src/xclim/indices/converters.py:1890-2152,
2652-2740, with the solar geometry of src/xclim/indices/helpers.py:95-525).

The solar tables (extraterrestrial radiation Ra, day length) depend only on (day, latitude): ``xh_solar_table`` builds them
over the distinct latitudes of the field, from one day angle per row computed here (xarray's decimal year).  A regular
grid has one table column per latitude row; a curvilinear grid can have one per cell, and then the table is as large as
one float64 field.  The daily methods (BR65, HG85, MB05, FAO_PM98) run element-wise in ``xh_pet_daily``; the monthly
methods (TW48, DA02) march each cell down its months in ``xh_pet_monthly``, with per-(month, latitude) tables that
``xh_pet_month_table`` reduces from a daily table over WHOLE calendar months (the reference's ``_get_D_from_M``), even when
the data start or end inside a month.  See xclim_amd/csrc/pet.hip.

Inputs are time-first ``(T, *cells)`` numpy arrays (or ``(T, C)`` device arrays) in CF units: temperatures in K, ``hurs``
in %, radiation in W m-2, ``sfcWind`` in m s-1 (at 10 m), ``pr`` in kg m-2 s-1.  ``lat`` is in degrees north and
broadcasts to the cell shape.  ``time`` is a daily, gap-free :class:`~xclim_amd.timeaxis.TimeAxis`; its rows are stamped
at ``time_of_day`` hours (CMIP daily data is often stamped at 12:00, which moves the day angle by half a day).  Anything
else raises :class:`NotServed`.

Results are float64 in kg m-2 s-1, as the reference's are: every method mixes a float64 operand into its float32
fields (Ra or the day length, or the ``np.log`` wind factor under NEP 50).  float32 and float64 fields are read natively
and computed in float64 (the reference rounds some float32 intermediates); a mixed set is widened to float64, which is
exact.  ``XCLIM_AMD_FLOAT64`` does not apply: nothing is rounded.  The monthly methods return ``(values, months)`` with
the ``MS`` TimeAxis of the output rows.
"""

from __future__ import annotations

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import get_device
from .timeaxis import TimeAxis, _MLEN_NOLEAP

__all__ = ["NotServed", "potential_evapotranspiration", "water_budget", "extraterrestrial_solar_radiation", "day_lengths",
           "day_angle", "METHODS"]


NotServed = F.NotServed

# converters.py:1999-2147: the accepted spellings of each method
METHODS = {"baierrobertson65": "BR65", "BR65": "BR65", "hargreaves85": "HG85", "HG85": "HG85",
           "mcguinnessbordne05": "MB05", "MB05": "MB05", "thornthwaite48": "TW48", "TW48": "TW48",
           "allen98": "FAO_PM98", "FAO_PM98": "FAO_PM98", "droogersallen02": "DA02", "DA02": "DA02"}
_CALENDARS = ("standard", "gregorian", "proleptic_gregorian", "julian", "noleap", "365_day", "all_leap", "366_day",
              "360_day")
_SOLAR_CONSTANT = {"MB05": 1367.0}  # W m-2; 1361 otherwise (helpers.py:403, converters.py:2074)


def _canonical(method):
    m = METHODS.get(method) if isinstance(method, str) else None
    if m is None:
        raise NotImplementedError(f"'{method}' method is not implemented.")
    return m


def _leap(year, calendar):
    year = np.asarray(year)
    if calendar == "julian":
        return year % 4 == 0
    if calendar in ("noleap", "365_day", "360_day"):
        return np.zeros(year.shape, bool)
    if calendar in ("all_leap", "366_day"):
        return np.ones(year.shape, bool)
    return ((year % 4 == 0) & (year % 100 != 0)) | (year % 400 == 0)


def _days_in_month(year, month, calendar):
    if calendar == "360_day":
        return np.full(np.shape(year), 30, np.int64)
    return _MLEN_NOLEAP[np.asarray(month) - 1].astype(np.int64) + ((np.asarray(month) == 2) & _leap(year, calendar))


def _day_of_year(time: TimeAxis):
    if time.calendar == "360_day":
        return (time.month - 1) * 30 + time.day
    cum = np.concatenate([[0], np.cumsum(_MLEN_NOLEAP)])[:-1]
    return cum[time.month - 1] + time.day + ((time.month > 2) & _leap(time.year, time.calendar))


def _check_time(time: TimeAxis):
    if not isinstance(time, TimeAxis):
        raise TypeError("time must be a TimeAxis")
    if time.calendar not in _CALENDARS:
        raise NotServed(f"potential evapotranspiration: the calendar {time.calendar!r} is not served")
    if len(time) == 0:
        raise NotServed("potential evapotranspiration: an empty time axis is not served")
    y, m, d = time.year, time.month, time.day
    last = d == _days_in_month(y, m, time.calendar)
    ny = np.where(last & (m == 12), y + 1, y)
    nm = np.where(last, m % 12 + 1, m)
    nd = np.where(last, 1, d + 1)
    if not (np.array_equal(ny[:-1], y[1:]) and np.array_equal(nm[:-1], m[1:]) and np.array_equal(nd[:-1], d[1:])):
        raise NotServed("potential evapotranspiration: only daily, gap-free time axes are served")


def day_angle(time: TimeAxis, time_of_day: float = 0.0) -> np.ndarray:
    """helpers.py:95-116: ``(decimal_year % 1) * 2 pi`` with xarray's decimal year
    ``year + (dayofyear - 1 + time_of_day / 24) / days_in_year`` in the axis's calendar (float64, one per row)."""
    if time.calendar == "360_day":
        diy = np.full(len(time), 360.0)
    else:
        diy = 365.0 + _leap(time.year, time.calendar)
    dy = time.year + (_day_of_year(time) - 1 + float(time_of_day) / 24) / diy
    return (dy % 1) * 2 * np.pi


def _lat_table(lat, cell_shape):
    """The distinct latitudes (L) and each cell's int32 index into them (C)."""
    if lat is None:
        raise ValueError("potential evapotranspiration: lat is required")
    u, inv = np.unique(F.per_cell(lat, cell_shape, "lat"), return_inverse=True)
    return u, inv.astype(np.int32).reshape(-1)


def _solar(time, lat, what, time_of_day, solar_constant, device):
    lat = np.atleast_1d(np.asarray(lat, dtype=np.float64))
    if lat.ndim != 1:
        raise ValueError("lat must be 1-D")
    _check_time(time)
    dev = device or get_device()
    ra, dl = K.pet_solar_table(dev, day_angle(time, time_of_day), lat, solar_constant, ra=what == "ra", dl=what == "dl")
    return (ra if what == "ra" else dl).get()


def extraterrestrial_solar_radiation(time: TimeAxis, lat, *, solar_constant: float = 1361.0, time_of_day: float = 0.0,
                                     device=None) -> np.ndarray:
    """helpers.py:400-447 with method "spencer": ``(T, L)`` float64 in J m-2 d-1 for the latitudes ``lat`` (1-D,
    degrees north) and the daily rows of ``time``; ``solar_constant`` in W m-2."""
    return _solar(time, lat, "ra", time_of_day, solar_constant, device)


def day_lengths(time: TimeAxis, lat, *, time_of_day: float = 0.0, device=None) -> np.ndarray:
    """helpers.py:450-525 with method "spencer" and no infill: ``(T, L)`` float64 hours, NaN in the polar day and
    night."""
    return _solar(time, lat, "dl", time_of_day, 1361.0, device)


def _need(m, got, water):
    if m in ("MB05", "TW48"):
        if "tas" not in got and not {"tasmin", "tasmax"} <= set(got):
            raise ValueError(f"{m}: needs tas, or tasmin and tasmax")
    else:
        for n in ("tasmin", "tasmax"):
            if n not in got:
                raise ValueError(f"{m}: needs {n}")
    if m == "FAO_PM98":
        for n in ("hurs", "rsds", "rsus", "rlds", "rlus"):
            if n not in got:
                raise ValueError(f"FAO_PM98: needs {n}")
    if (m == "DA02" or water) and "pr" not in got:
        raise ValueError(f"{'DA02' if m == 'DA02' else 'the water budget'}: needs pr")


def _reads(m, has_tas, water):
    """The fields a method reads (converters.py:2000-2145): BR65 and FAO_PM98 ignore tas, MB05 and TW48 use it instead of
    tasmin / tasmax when given; pr only for DA02 and the water budget."""
    r = {"BR65": {"tasmin", "tasmax"}, "HG85": {"tasmin", "tasmax", "tas"}, "DA02": {"tasmin", "tasmax", "tas", "pr"},
         "FAO_PM98": {"tasmin", "tasmax", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind"}}.get(m)
    if r is None:
        r = {"tas"} if has_tas else {"tasmin", "tasmax"}
    return r | ({"pr"} if water else set())


def _months(time: TimeAxis):
    """The monthly frame: row offsets of each month of the data, the MS axis, and the daily axis over the whole months
    with its own month offsets (converters.py:1798-1812)."""
    seg, starts = time.segments("MS")
    y = np.array([s[0] for s in starts], np.int64)
    mo = np.array([s[1] for s in starts], np.int64)
    ndays = _days_in_month(y, mo, time.calendar)
    dseg = np.concatenate([[0], np.cumsum(ndays)]).astype(np.int64)
    cal = time.calendar
    days = TimeAxis(np.repeat(y, ndays), np.repeat(mo, ndays),
                    np.concatenate([np.arange(1, n + 1) for n in ndays]), cal)
    return seg, TimeAxis(y, mo, np.ones_like(y), cal), days, dseg, ndays


def _run(method, fields, time, lat, outputs, peta, petb, time_of_day, device, keep):
    m = _canonical(method)
    if m == "FAO_PM98" and fields.get("sfcWind") is None:
        raise ValueError("Wind speed is required for Allen98 method.")
    _need(m, {k for k, v in fields.items() if v is not None}, "wb" in outputs)
    fields = {k: v for k, v in fields.items() if k in _reads(m, fields.get("tas") is not None, "wb" in outputs)}
    got = F.native_set(fields)
    T, cell_shape, C_ = F.shape_of(got)
    if len(time) != T:
        raise ValueError(f"time has {len(time)} rows, the fields {T}")
    _check_time(time)
    if m == "DA02" and "wb" in outputs:  # converters.py:2718-2730 calls PET without pr, which DA02 needs
        raise NotServed("water_budget with DA02: the reference does not hand pr to potential_evapotranspiration")
    if C_ == 0 and m != "FAO_PM98":  # an empty grid: latitudes of no cell make no table for the kernels (FAO_PM98 has none and launches)
        months = None if m in K.PET_DAILY else _months(time)[1]
        rows = T if months is None else len(months)
        return F.empty_result(dict.fromkeys(outputs, np.float64), rows, cell_shape, keep, device), months
    lat_u, li = _lat_table(lat, cell_shape) if m != "FAO_PM98" else (None, None)
    dev = device or get_device()
    d = {n: F.rows_on_device(dev, a, T, C_) for n, a in got.items()}
    if m in K.PET_DAILY:
        months = ra = None
        if m != "FAO_PM98":
            ra, _ = K.pet_solar_table(dev, day_angle(time, time_of_day), lat_u, _SOLAR_CONSTANT.get(m, 1361.0))
        outs = K.pet_daily(dev, m, d, ra, li, peta=peta, petb=petb, outputs=outputs)
        rows = T
    else:
        seg, months, days, dseg, ndays = _months(time)
        ra, dl = K.pet_solar_table(dev, day_angle(days), lat_u, 1361.0, ra=m == "DA02", dl=m == "TW48")
        tab = K.pet_month_table(dev, dl if m == "TW48" else ra, dseg, 0 if m == "TW48" else 1)
        outs = K.pet_monthly(dev, m, d, seg, int(months.month[0]) - 1, tab, ndays * 86400.0, li, outputs=outputs)
        rows = len(months)
    return (outs if keep else F.host_result(outs, rows, cell_shape)), months


_FIELD_DOC = """``tasmin`` / ``tasmax`` / ``tas`` [K], ``hurs`` [%], ``rsds`` / ``rsus`` / ``rlds`` / ``rlus`` [W m-2], ``sfcWind``
    [m s-1], ``pr`` [kg m-2 s-1]: time-first fields of one shape."""


def potential_evapotranspiration(tasmin=None, tasmax=None, tas=None, lat=None, hurs=None, rsds=None, rsus=None, rlds=None,
                                 rlus=None, sfcWind=None, pr=None, *, time: TimeAxis, method: str = "BR65",
                                 peta: float = 0.00516409319477, petb: float = 0.0874972822289, time_of_day: float = 0.0,
                                 device=None, keep: bool = False):
    """converters.py:1890-2152: PET [kg m-2 s-1], float64 ``(T, *cells)`` (``(T, C)`` device array with ``keep=True``);
    TW48 / DA02 return ``(values, months)`` with ``(M, ...)`` values on the ``MS`` TimeAxis ``months``.  Unknown methods
    raise NotImplementedError, FAO_PM98 without ``sfcWind`` ValueError (the reference's errors)."""
    fields = dict(tasmin=tasmin, tasmax=tasmax, tas=tas, hurs=hurs, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus,
                  sfcWind=sfcWind, pr=pr)
    outs, months = _run(method, fields, time, lat, ("pet",), peta, petb, time_of_day, device, keep)
    return outs["pet"] if months is None else (outs["pet"], months)


def water_budget(pr, tasmin=None, tasmax=None, tas=None, lat=None, hurs=None, rsds=None, rsus=None, rlds=None, rlus=None,
                 sfcWind=None, *, time: TimeAxis, method: str = "BR65", peta: float = 0.00516409319477,
                 petb: float = 0.0874972822289, time_of_day: float = 0.0, device=None, keep: bool = False):
    """converters.py:2652-2740 with ``evspsblpot=None``: ``pr - PET`` [kg m-2 s-1] from the same launch as PET; for TW48 /
    DA02 ``pr`` is its NaN-skipping monthly mean and ``(values, months)`` is returned."""
    fields = dict(tasmin=tasmin, tasmax=tasmax, tas=tas, hurs=hurs, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus,
                  sfcWind=sfcWind, pr=pr)
    outs, months = _run(method, fields, time, lat, ("wb",), peta, petb, time_of_day, device, keep)
    return outs["wb"] if months is None else (outs["wb"], months)


potential_evapotranspiration.__doc__ += "\n\n    " + _FIELD_DOC
water_budget.__doc__ += "\n\n    " + _FIELD_DOC


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
_CF_UNITS = {"tasmin": "K", "tasmax": "K", "tas": "K", "hurs": "%", "rsds": "W m-2", "rsus": "W m-2", "rlds": "W m-2",
             "rlus": "W m-2", "sfcWind": "m s-1", "pr": "kg m-2 s-1"}


def make_adapters(env, orig_pet, orig_wb, gather_lat=None, device=None) -> dict:
    """Same-signature replacements of ``potential_evapotranspiration`` / ``water_budget`` (converters.py:1890-2152,
    2652-2740) on DataArrays with a time dimension.  Fields are converted to CF units with ``env.convert_units_to`` (a
    no-op for CF units); ``lat`` comes from ``gather_lat`` (the reference's ``_gather_lat``) when not passed.  Chunked
    fields, non-daily or gappy time axes (monthly inputs among them), ``evspsblpot`` and unknown methods go to the
    originals."""
    from .xr_adapter import _cell_dims, _tfirst_fields, _wrap_cells, time_axis_of

    DA = env.DataArray

    def _time_of_day(a):
        t = a["time"].dt
        try:
            h, mi, s = (np.asarray(getattr(t, k).values, np.float64) for k in ("hour", "minute", "second"))
        except (AttributeError, KeyError):
            return 0.0
        tod = h + mi / 60 + s / 3600
        if tod.size and np.any(tod != tod[0]):
            raise NotServed("potential evapotranspiration: rows stamped at different times of day")
        return float(tod[0]) if tod.size else 0.0

    def _lat_cells(lat, a):
        """lat (a DataArray over some cell dims, or array-like) as an array broadcast to the cell dims of ``a``."""
        dims = _cell_dims(a)
        if isinstance(lat, DA):
            if not set(lat.dims) <= set(dims):
                raise NotServed("lat: dimensions outside the field's cell dimensions")
            v = np.asarray(lat.transpose(*[d for d in dims if d in lat.dims]).values, np.float64)
            shape = [a.sizes[d] if d in lat.dims else 1 for d in dims] if hasattr(a, "sizes") else \
                [a.shape[a.dims.index(d)] if d in lat.dims else 1 for d in dims]
            return v.reshape(shape)
        return np.asarray(lat, np.float64)

    def _cf_units(k, v):
        return v if v.attrs.get("units") == _CF_UNITS[k] else env.convert_units_to(v, _CF_UNITS[k], context="hydro")

    def _serve(fields, lat, pr_first):
        named = {k: v for k, v in fields.items() if v is not None}
        a, conv = _tfirst_fields(DA, named, _cf_units)
        if lat is None:
            if gather_lat is None:
                raise NotServed("no lat")
            lat = gather_lat(named.get("tasmin") if named.get("tas") is None else named["tas"]) if not pr_first else \
                gather_lat(named["pr"])
        return a, conv, _lat_cells(lat, a), time_axis_of(a), _time_of_day(a)

    def _wrap(a, values, months, attrs):
        time = a["time"] if months is None else a["time"].resample(time="MS").first()["time"]
        return _wrap_cells(DA, a, values, time, attrs)

    def potential_evapotranspiration(tasmin=None, tasmax=None, tas=None, lat=None, hurs=None, rsds=None, rsus=None,
                                     rlds=None, rlus=None, sfcWind=None, pr=None, method="BR65", peta=0.00516409319477,
                                     petb=0.0874972822289):
        kw = dict(tasmin=tasmin, tasmax=tasmax, tas=tas, lat=lat, hurs=hurs, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus,
                  sfcWind=sfcWind, pr=pr, method=method, peta=peta, petb=petb)
        try:
            m = _canonical(method)
            if m == "FAO_PM98" and sfcWind is None:
                raise ValueError("Wind speed is required for Allen98 method.")
            if m != "DA02":
                pr = None
            a, x, latc, time, tod = _serve(dict(tasmin=tasmin, tasmax=tasmax, tas=tas, hurs=hurs, rsds=rsds, rsus=rsus,
                                               rlds=rlds, rlus=rlus, sfcWind=sfcWind, pr=pr), lat, False)
            out = _potential_evapotranspiration(**x, lat=latc if m != "FAO_PM98" else None, time=time, method=m,
                                                peta=peta, petb=petb, time_of_day=tod, device=device)
        except NotImplementedError:
            return orig_pet(**kw)
        values, months = out if isinstance(out, tuple) else (out, None)
        return _wrap(a, values, months, {"units": "kg m-2 s-1"})

    def water_budget(pr, evspsblpot=None, tasmin=None, tasmax=None, tas=None, lat=None, hurs=None, rsds=None, rsus=None,
                     rlds=None, rlus=None, sfcWind=None, method="BR65"):
        kw = dict(evspsblpot=evspsblpot, tasmin=tasmin, tasmax=tasmax, tas=tas, lat=lat, hurs=hurs, rsds=rsds, rsus=rsus,
                  rlds=rlds, rlus=rlus, sfcWind=sfcWind, method=method)
        try:
            if evspsblpot is not None:
                raise NotServed("evspsblpot given")
            m = _canonical(method)
            if m == "FAO_PM98" and sfcWind is None:
                raise ValueError("Wind speed is required for Allen98 method.")
            a, x, latc, time, tod = _serve(dict(pr=pr, tasmin=tasmin, tasmax=tasmax, tas=tas, hurs=hurs, rsds=rsds,
                                               rsus=rsus, rlds=rlds, rlus=rlus, sfcWind=sfcWind), lat, True)
            out = _water_budget(lat=latc if m != "FAO_PM98" else None, time=time, method=m, time_of_day=tod,
                                device=device, **x)
        except NotImplementedError:
            return orig_wb(pr, **kw)
        values, months = out if isinstance(out, tuple) else (out, None)
        return _wrap(a, values, months, {"units": "kg m-2 s-1"})

    potential_evapotranspiration.__wrapped__ = orig_pet
    water_budget.__wrapped__ = orig_wb
    return {"potential_evapotranspiration": potential_evapotranspiration, "water_budget": water_budget}


_potential_evapotranspiration = potential_evapotranspiration
_water_budget = water_budget
