"""Host mirror of the thermal-comfort end of the converters (reference: src/xclim/indices/converters.py:390-603, 2155-2635,
with the solar geometry of src/xclim/indices/helpers.py:60-397): ``saturation_vapor_pressure``, ``mean_radiant_temperature``,
``universal_thermal_climate_index`` and the ``cosine_of_solar_zenith_angle`` they stand on.

UTCI from seven fields is ONE launch (``xh_thermal_comfort``, xclim_amd/csrc/thermal.hip): the cosine of the zenith angle, the
direct fraction, the mean radiant temperature, ITS-90 e_sat and the polynomial stay in registers.  What depends on the row alone
(Spencer declination, UTC hour angle, interval, time correction, sun distance) is a small float64 table computed here, in the
reference's order of operations; what depends on the cell alone (latitude, longitude) is uploaded once.

Fields are time-first ``(R, *cells)`` numpy arrays (or ``(R, C)`` device arrays) in CF units: ``tas`` / ``mrt`` in K, ``hurs`` in %,
``sfcWind`` in m s-1, radiation in W m-2; ``lat`` / ``lon`` in degrees, broadcast to the cell shape.  ``time`` is the daily,
gap-free :class:`~xclim_amd.timeaxis.TimeAxis` of the DAYS.  A sub-daily field rides on it with ``subdaily=SubDaily(n)``, as
chill.py's hourly fields do: ``n * len(time)`` rows, row ``r`` being day ``r // n`` at ``offset + (r % n) * 86400 / n`` seconds
UTC, the start of its interval.  Daily rows are stamped at ``time_of_day`` hours.

float32 and float64 fields are read natively and computed in float64; a mixed set is widened to float64.  UTCI and e_sat come
back in the fields' dtype (the float64 result rounded once), the mean radiant temperature and the cosine as float64.

ASSUMPTIONS (none could be executed against xarray / pint here): xarray's decimal year is ``year + (dayofyear - 1 + hours / 24)
/ days_in_year`` (already the assumption of ``converters.day_angle``); pint's conversion factors are one multiplication; the
reference's float32 route (a float32 ``exp``, a float32 subtraction of 273.15, numba's float32 instance of ``_utci``) is not
reproduced: all arithmetic is float64 on the widened fields.

Not served (:class:`NotServed`): integer fields, chunked fields (the adapter's business), gappy or non-daily axes, the julian
calendar and calendars outside ``converters._CALENDARS``, a sub-daily field without ``lon`` or with fewer than three rows (the
reference treats those as daily), ``cosine_of_solar_zenith_angle`` with ``stat="integral"`` (``xh_solar_table`` serves the daily
integral) or with ``sunlit=False`` and "average", ``solar_declination(method="simple")``.
"""

from __future__ import annotations

import numpy as np

from . import _capi as capi
from . import fields as F
from . import kernels as K
from ._capi import DeviceArray, get_device
from .converters import NotServed, _check_time, day_angle
from .timeaxis import TimeAxis

__all__ = ["NotServed", "SubDaily", "solar_declination", "time_correction_for_solar_angle", "distance_from_sun", "solar_rows",
           "cosine_of_solar_zenith_angle", "saturation_vapor_pressure", "mean_radiant_temperature",
           "universal_thermal_climate_index", "ESAT_METHODS", "ADAPTED", "frame_of", "make_adapters"]

WHO = "thermal comfort"
ESAT_METHODS = tuple(capi.ESAT_METHODS)
_ESAT_VALID = ["sonntag90", "goffgratch46", "its90", "ecmwf", "tetens30", "wmo08", "buck81", "aerk96"]  # the reference's message
S_IN_D = 24 * 3600


class SubDaily:
    """``steps_per_day`` rows per day of the daily TimeAxis, the first of a day at ``offset_seconds`` UTC."""

    def __init__(self, steps_per_day: int, offset_seconds: int = 0):
        n, off = int(steps_per_day), int(offset_seconds)
        if n != steps_per_day or off != offset_seconds or n < 1 or S_IN_D % n:
            raise ValueError("SubDaily: steps_per_day must be a positive integer dividing 86400, offset_seconds an integer")
        if not 0 <= off < S_IN_D // n:
            raise ValueError(f"SubDaily: 0 <= offset_seconds < {S_IN_D // n}")
        self.steps_per_day, self.offset_seconds, self.interval_seconds = n, off, S_IN_D // n

    def seconds(self) -> np.ndarray:
        """Seconds of day of the ``steps_per_day`` rows of one day."""
        return self.offset_seconds + np.arange(self.steps_per_day, dtype=np.int64) * self.interval_seconds

    def __repr__(self):
        return f"SubDaily({self.steps_per_day}, {self.offset_seconds})"


def _wrap_radians(x):
    return ((x + np.pi) % (2 * np.pi)) - np.pi


def _time(time, subdaily):
    if not isinstance(time, TimeAxis):
        raise TypeError("time must be the daily TimeAxis of the days")
    try:
        _check_time(time)
    except NotServed as e:
        raise NotServed(str(e).replace("potential evapotranspiration", WHO)) from None
    if time.calendar == "julian":
        raise NotServed(f"{WHO}: the julian calendar is not served")
    if subdaily is not None:
        if not isinstance(subdaily, SubDaily):
            raise TypeError("subdaily must be a SubDaily")
        if subdaily.steps_per_day * len(time) < 3:
            raise NotServed(f"{WHO}: fewer than three sub-daily rows (the reference treats them as daily)")
    return len(time) * (subdaily.steps_per_day if subdaily is not None else 1)


def _day_angle(time, subdaily, time_of_day):
    """helpers.py:95-116 for every row: the day angle of the day at the row's hours."""
    if subdaily is None:
        return day_angle(time, time_of_day)
    n = subdaily.steps_per_day
    out = np.empty(len(time) * n)
    for k, s in enumerate(subdaily.seconds()):
        out[k::n] = day_angle(time, s / 3600)
    return out


def _seconds(time, subdaily, time_of_day):
    """Seconds of day of every row."""
    if subdaily is None:
        return np.full(len(time), float(time_of_day) * 3600)
    return np.tile(subdaily.seconds().astype(np.float64), len(time))


def solar_declination(time: TimeAxis, method: str = "spencer", *, subdaily=None, time_of_day: float = 0.0) -> np.ndarray:
    """helpers.py:119-163, "spencer": the wrapped declination [rad] of every row, float64."""
    if method != "spencer":
        if method == "simple":
            raise NotServed(f"{WHO}: solar_declination(method='simple') is not served")
        raise NotImplementedError("Method must be one of 'simple' or 'spencer'.")
    _time(time, subdaily)
    da = _day_angle(time, subdaily, time_of_day)
    sd = (0.006918 - 0.399912 * np.cos(da) + 0.070257 * np.sin(da) - 0.006758 * np.cos(2 * da) + 0.000907 * np.sin(2 * da)
          - 0.002697 * np.cos(3 * da) + 0.001480 * np.sin(3 * da))
    return _wrap_radians(sd)


def time_correction_for_solar_angle(time: TimeAxis, *, subdaily=None, time_of_day: float = 0.0) -> np.ndarray:
    """helpers.py:166-192: the wrapped time correction [rad] of every row, float64."""
    _time(time, subdaily)
    da = _day_angle(time, subdaily, time_of_day)
    tc = 0.004297 + 0.107029 * np.cos(da) - 1.837877 * np.sin(da) - 0.837378 * np.cos(2 * da) - 2.340475 * np.sin(2 * da)
    return _wrap_radians(tc * (np.pi / 180))


def distance_from_sun(time: TimeAxis, *, subdaily=None, time_of_day: float = 0.0) -> np.ndarray:
    """helpers.py:65-92: the sun-earth distance [au] of every row; days since 2000-01-01 12:00 in the axis's own calendar."""
    _time(time, subdaily)
    day0 = TimeAxis([2000], [1], [1], time.calendar).ordinal()[0]
    days = np.repeat(time.ordinal() - day0, subdaily.steps_per_day if subdaily is not None else 1)
    days_since = days + (_seconds(time, subdaily, time_of_day) / S_IN_D - 0.5)
    g = ((357.528 + 0.9856003 * days_since) % 360) * np.pi / 180
    return 1.00014 - 0.01671 * np.cos(g) - 0.00014 * np.cos(2.0 * g)


def solar_rows(time: TimeAxis, *, subdaily=None, time_of_day: float = 0.0) -> np.ndarray:
    """The per-row table of ``xh_thermal_comfort``: float64 (``capi.THERMAL_NROW``, R)."""
    R = _time(time, subdaily)
    dec = solar_declination(time, subdaily=subdaily, time_of_day=time_of_day)
    rows = np.zeros((capi.THERMAL_NROW, R))
    rows[capi.THERMAL_ROWS["sin_dec"]] = np.sin(dec)
    rows[capi.THERMAL_ROWS["cos_dec"]] = np.cos(dec)
    rows[capi.THERMAL_ROWS["tan_dec"]] = np.tan(dec)
    if subdaily is not None:
        s = _seconds(time, subdaily, time_of_day)
        rows[capi.THERMAL_ROWS["h_utc"]] = ((s % S_IN_D) / S_IN_D) * 2 * np.pi + np.pi
        rows[capi.THERMAL_ROWS["interval"]] = 2 * np.pi * subdaily.interval_seconds / S_IN_D
    rows[capi.THERMAL_ROWS["tcorr"]] = time_correction_for_solar_angle(time, subdaily=subdaily, time_of_day=time_of_day)
    rows[capi.THERMAL_ROWS["inv_d2"]] = distance_from_sun(time, subdaily=subdaily, time_of_day=time_of_day) ** (-2)
    return rows


def _cells(lat, lon, cell_shape, subdaily):
    if lat is None:
        raise ValueError(f"{WHO}: lat is required")
    if subdaily is not None and lon is None:
        raise NotServed(f"{WHO}: a sub-daily field without lon is not served")
    latr = _wrap_radians(F.per_cell(lat, cell_shape, "lat") * (np.pi / 180))
    lonr = None if subdaily is None else F.per_cell(lon, cell_shape, "lon") * (np.pi / 180)
    return latr, lonr


def _no_integers(fields):
    for n, a in fields.items():
        if a is not None and not isinstance(a, DeviceArray) and np.asarray(a).dtype.kind in "iub":
            raise NotServed(f"{WHO}: {n} is an integer field")


def _stat(stat):
    if stat not in ("sunlit", "instant"):
        raise NotImplementedError("Argument 'stat' must be one of 'instant' or 'sunlit'.")
    return stat


def _launch(fields, outputs, stat, lat, lon, time, subdaily, time_of_day, mask_invalid, wind_cap_min, device, keep):
    _no_integers(fields)
    got = F.native_set(fields)
    R, cell_shape, C_ = F.shape_of(got)
    sun = "mrt" not in got
    if sun:
        if time is None:
            raise ValueError(f"{WHO}: time is required")
        if _time(time, subdaily) != R:
            raise ValueError(f"time and subdaily give {_time(time, subdaily)} rows, the fields {R}")
    f64 = np.dtype(next(iter(got.values())).dtype) == np.float64
    dtypes = {o: (np.float64 if f64 or o != "utci" else np.float32) for o in outputs}
    if R == 0 or C_ == 0:
        res = F.empty_result(dtypes, R, cell_shape, keep, device)
        return res
    rows = latr = lonr = None
    if sun:
        rows = solar_rows(time, subdaily=subdaily, time_of_day=time_of_day)
        latr, lonr = _cells(lat, lon, cell_shape, subdaily)
    dev = device or get_device()
    d = {n: F.rows_on_device(dev, a, R, C_) for n, a in got.items()}
    outs = K.thermal_comfort(dev, d, rows, latr, lonr, mode="daily" if subdaily is None else "subdaily", stat=stat,
                             mask_invalid=mask_invalid, wind_cap_min=wind_cap_min, outputs=outputs)
    return outs if keep else F.host_result(outs, R, cell_shape)


def cosine_of_solar_zenith_angle(time: TimeAxis, lat, lon=0.0, stat: str = "average", sunlit: bool = True, *, subdaily=None,
                                 time_of_day: float = 0.0, device=None, keep: bool = False):
    """helpers.py:241-350 with the Spencer declination and time correction of ``time``: float64 ``(R, *cells)`` over the
    broadcast shape of ``lat`` and ``lon`` [degrees] (``(R, C)`` device array with ``keep``).  ``stat``: "average" (over the sunlit
    part of each interval: ``sunlit=True``) or "instant"."""
    if stat not in ("average", "integral", "instant"):
        raise NotImplementedError("Argument 'stat' must be one of 'integral', 'average' or 'instant'.")
    if stat == "integral":
        raise NotServed(f"{WHO}: cosine_of_solar_zenith_angle(stat='integral') is not served (extraterrestrial_solar_radiation is)")
    if stat == "average" and not sunlit:
        raise NotServed(f"{WHO}: cosine_of_solar_zenith_angle(stat='average', sunlit=False) is not served")
    R = _time(time, subdaily)
    cell_shape = np.broadcast_shapes(np.shape(lat), np.shape(lon))
    C_ = int(np.prod(cell_shape, dtype=np.int64))
    if C_ == 0:
        return F.empty_result({"csza": np.float64}, R, cell_shape, keep, device)["csza"]
    latr, lonr = _cells(lat, lon, cell_shape, subdaily)
    dev = device or get_device()
    out = K.thermal_comfort(dev, {}, solar_rows(time, subdaily=subdaily, time_of_day=time_of_day), latr, lonr,
                            mode="daily" if subdaily is None else "subdaily", stat="sunlit" if stat == "average" else "instant",
                            outputs=("csza",), shape=(R, C_, False))
    return out["csza"] if keep else F.host_result(out, R, cell_shape)["csza"]


def saturation_vapor_pressure(tas, ice_thresh=None, method: str = "sonntag90", interp_power=None, water_thresh: float = 273.15, *,
                              device=None, keep: bool = False):
    """converters.py:491-603: e_sat [Pa] of ``tas`` [K] in the dtype of ``tas``; the thresholds are plain numbers in K."""
    method = {"TE30": "tetens30", "GG46": "goffgratch46", "SO90": "sonntag90"}.get(method, method)
    method = method.casefold()
    if method not in capi.ESAT_METHODS:
        raise ValueError(f"Method {method} is not in {_ESAT_VALID}")
    if ice_thresh is None and interp_power is None:
        case = "water"
    elif interp_power is None:
        case = "binary"
    elif ice_thresh is None:
        raise ValueError("saturation_vapor_pressure: interp_power needs ice_thresh")
    else:
        case = "interp"
    _no_integers({"tas": tas})
    a = F.native(tas, "tas")
    R, cell_shape, C_ = F.shape_of({"tas": a})
    if R == 0 or C_ == 0:
        return F.empty_result({"e_sat": a.dtype}, R, cell_shape, keep, device)["e_sat"]
    dev = device or get_device()
    out = K.esat(dev, F.rows_on_device(dev, a, R, C_), method, case, 0.0 if ice_thresh is None else float(ice_thresh),
                 float(water_thresh), 1.0 if interp_power is None else float(interp_power))
    return out if keep else out.get().reshape((R,) + tuple(cell_shape))


def mean_radiant_temperature(rsds, rsus, rlds, rlus, stat: str = "sunlit", *, lat, lon=None, time: TimeAxis, subdaily=None,
                             time_of_day: float = 0.0, device=None, keep: bool = False):
    """converters.py:2537-2635: the mean radiant temperature [K], float64 ``(R, *cells)``."""
    fields = dict(rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus)
    return _launch(fields, ("mrt",), _stat(stat), lat, lon, time, subdaily, time_of_day, True, False, device, keep)["mrt"]


def universal_thermal_climate_index(tas, hurs, sfcWind, mrt=None, rsds=None, rsus=None, rlds=None, rlus=None, stat: str = "sunlit",
                                    mask_invalid: bool = True, wind_cap_min: bool = False, *, lat=None, lon=None, time=None,
                                    subdaily=None, time_of_day: float = 0.0, outputs=("utci",), device=None, keep: bool = False):
    """converters.py:2379-2489: UTCI [degC] in the dtype of the fields, ``(R, *cells)``.  Without ``mrt`` it comes from the four
    radiation fields in the same launch, and ``outputs=("utci", "mrt")`` returns both as a dict."""
    outputs = tuple(outputs)
    if not outputs or set(outputs) - {"utci", "mrt"}:
        raise ValueError("outputs: of 'utci' and 'mrt'")
    if mrt is not None:
        if "mrt" in outputs:
            raise ValueError("outputs: mrt is an input")
        fields = dict(tas=tas, hurs=hurs, sfcWind=sfcWind, mrt=mrt)
    else:
        fields = dict(tas=tas, hurs=hurs, sfcWind=sfcWind, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus)
        missing = [k for k, v in fields.items() if v is None]
        if missing:
            raise ValueError(f"universal_thermal_climate_index: without mrt, {', '.join(missing)} needed")
        _stat(stat)
    res = _launch(fields, outputs, stat if mrt is None else "sunlit", lat, lon, time, subdaily, time_of_day, mask_invalid,
                  wind_cap_min, device, keep)
    return res["utci"] if outputs == ("utci",) else res


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
ADAPTED = ("saturation_vapor_pressure", "mean_radiant_temperature", "universal_thermal_climate_index")
_CF_UNITS = {"tas": "K", "mrt": "K", "hurs": "%", "sfcWind": "m s-1", "rsds": "W m-2", "rsus": "W m-2", "rlds": "W m-2", "rlus": "W m-2"}


def frame_of(a):
    """``(TimeAxis of the days, SubDaily or None, time_of_day)`` of a DataArray's time coordinate: daily rows stamped at one time of
    day, or a uniform sub-daily coordinate (the same seconds of day on every day, evenly spaced over the whole day).
    :class:`NotServed` for anything else."""
    t = a["time"].dt
    y, m, d = (np.asarray(getattr(t, k).values, np.int64) for k in ("year", "month", "day"))
    try:
        s = sum(np.asarray(getattr(t, k).values, np.int64) * w for k, w in (("hour", 3600), ("minute", 60), ("second", 1)))
    except (AttributeError, KeyError):
        s = np.zeros(len(y), np.int64)
    cal = str(t.calendar)
    date = (y * 16 + m) * 32 + d
    n = int(np.argmax(date != date[0])) if np.any(date != date[0]) else len(date)
    if n == 1:
        if np.any(s != s[0]):
            raise NotServed(f"{WHO}: rows stamped at different times of day")
        return TimeAxis(y, m, d, cal), None, float(s[0]) / 3600
    if len(y) % n or S_IN_D % n or np.any(np.diff(s[:n]) != S_IN_D // n) or not 0 <= s[0] < S_IN_D // n:
        raise NotServed(f"{WHO}: the sub-daily time coordinate is not uniform")
    sub = SubDaily(n, int(s[0]))
    if np.any(date.reshape(-1, n) != date[::n, None]) or np.any(s.reshape(-1, n) != sub.seconds()[None, :]):
        raise NotServed(f"{WHO}: the sub-daily time coordinate is not uniform")
    return TimeAxis(y[::n], m[::n], d[::n], cal), sub, 0.0


def make_adapters(env, origs: dict, gather_lat=None, gather_lon=None, device=None) -> dict:
    """Same-signature replacements of the three functions of ``ADAPTED`` on DataArrays with a time dimension.  Fields go to CF units
    through ``env.convert_units_to``; ``lat`` / ``lon`` come from ``gather_lat`` / ``gather_lon`` (the reference's ``_gather_lat`` /
    ``_gather_lon``); a uniform sub-daily coordinate becomes a :class:`SubDaily`.  The results carry the reference's ``units``.
    Whatever raises :class:`NotServed` (chunked or time-less fields, gappy axes, a sub-daily field without ``lon`` ...) goes to the
    original with the arguments as they came."""
    from .xr_adapter import _cell_dims, _tfirst_fields, _wrap_cells

    DA = env.DataArray

    def _cf(k, v):
        return v if v.attrs.get("units") == _CF_UNITS[k] else env.convert_units_to(v, _CF_UNITS[k])

    def _cells_of(coord, a, what):
        dims = _cell_dims(a)
        if isinstance(coord, DA):
            if not set(coord.dims) <= set(dims):
                raise NotServed(f"{what}: dimensions outside the field's cell dimensions")
            v = np.asarray(coord.transpose(*[d for d in dims if d in coord.dims]).values, np.float64)
            return v.reshape([a.shape[a.dims.index(d)] if d in coord.dims else 1 for d in dims])
        return np.asarray(coord, np.float64)

    def _gather(fn, a, what, needed):
        try:
            if fn is None:
                raise ValueError(f"no {what}")
            return _cells_of(fn(a), a, what)
        except NotServed:
            raise
        except Exception:
            if needed:
                raise NotServed(f"{WHO}: no {what} on the field") from None
            return None

    def _kelvin(thr, tas_k):
        return float(thr) if isinstance(thr, (int, float)) else float(env.convert_units_to(thr, tas_k))

    def saturation_vapor_pressure(tas, ice_thresh=None, method="sonntag90", interp_power=None, water_thresh="0 °C"):
        try:
            a, x = _tfirst_fields(DA, {"tas": tas}, _cf)
            ak = _cf("tas", tas)
            out = _saturation_vapor_pressure(x["tas"], None if ice_thresh is None else _kelvin(ice_thresh, ak), method, interp_power,
                                             273.15 if water_thresh == "0 °C" else _kelvin(water_thresh, ak), device=device)
        except NotServed:
            return origs["saturation_vapor_pressure"](tas, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                                                      water_thresh=water_thresh)
        return _wrap_cells(DA, a, out, a["time"], {"units": "Pa"})

    def mean_radiant_temperature(rsds, rsus, rlds, rlus, stat="sunlit"):
        try:
            _stat(stat)
            a, x = _tfirst_fields(DA, dict(rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus), _cf)
            time, sub, tod = frame_of(a)
            out = _mean_radiant_temperature(**x, stat=stat, lat=_gather(gather_lat, rsds, "lat", True),
                                            lon=_gather(gather_lon, rsds, "lon", sub is not None), time=time, subdaily=sub, time_of_day=tod,
                                            device=device)
        except NotServed:
            return origs["mean_radiant_temperature"](rsds, rsus, rlds, rlus, stat=stat)
        return _wrap_cells(DA, a, out, a["time"], {"units": "K"})

    def universal_thermal_climate_index(tas, hurs, sfcWind, mrt=None, rsds=None, rsus=None, rlds=None, rlus=None, stat="sunlit",
                                        mask_invalid=True, wind_cap_min=False):
        try:
            named = dict(tas=tas, hurs=hurs, sfcWind=sfcWind, mrt=mrt) if mrt is not None else \
                dict(tas=tas, hurs=hurs, sfcWind=sfcWind, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus)
            if any(v is None for v in named.values()):
                raise NotServed(f"{WHO}: a field is missing")
            a, x = _tfirst_fields(DA, named, _cf)
            kw = {}
            if mrt is None:
                _stat(stat)
                time, sub, tod = frame_of(a)
                kw = dict(stat=stat, lat=_gather(gather_lat, rsds, "lat", True), lon=_gather(gather_lon, rsds, "lon", sub is not None),
                          time=time, subdaily=sub, time_of_day=tod)
            out = _universal_thermal_climate_index(**x, mask_invalid=mask_invalid, wind_cap_min=wind_cap_min, device=device, **kw)
        except NotServed:
            return origs["universal_thermal_climate_index"](tas, hurs, sfcWind, mrt=mrt, rsds=rsds, rsus=rsus, rlds=rlds, rlus=rlus,
                                                            stat=stat, mask_invalid=mask_invalid, wind_cap_min=wind_cap_min)
        return _wrap_cells(DA, a, out, a["time"], {"units": "degC"})

    out = {"saturation_vapor_pressure": saturation_vapor_pressure, "mean_radiant_temperature": mean_radiant_temperature,
           "universal_thermal_climate_index": universal_thermal_climate_index}
    for n, fn in out.items():
        fn.__wrapped__ = origs[n]
        fn.__doc__ = getattr(origs[n], "__doc__", None)
    return out


_saturation_vapor_pressure = saturation_vapor_pressure
_mean_radiant_temperature = mean_radiant_temperature
_universal_thermal_climate_index = universal_thermal_climate_index
