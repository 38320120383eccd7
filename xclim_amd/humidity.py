"""Host mirror of the humidity, heat-stress and wind conversions (reference: src/xclim/indices/converters.py:75-223, 272-387,
606-1084, 1659-1744, 2797-2902): ``humidex``, ``heat_index``, ``vapor_pressure``, ``vapor_pressure_deficit``, ``relative_humidity``,
``specific_humidity``, ``specific_humidity_from_dewpoint``, ``dewpoint_from_specific_humidity``, ``uas_vas_to_sfcwind``,
``sfcwind_to_uas_vas``, ``wind_chill_index`` and ``wind_power_potential`` with the reference's names, parameters and defaults, and
``saturation_vapor_pressure`` re-exported from :mod:`xclim_amd.thermal`.

Every humidity function is ONE launch of ``xh_air_moisture`` (xclim_amd/csrc/humidity.hip), and :func:`air_moisture` is the fused
form: any set of the nine results from one read of the fields, so ``air_moisture(tas=, tdps=, ps=, outputs=["hurs", "huss", "humidex",
"heat_index"])`` reads three fields and writes four.  An output that needs the relative humidity when no ``hurs`` field is given takes
the launch's own relative humidity (after ``invalid_values``, before any rounding to float32).  The wind functions are one launch
of ``xh_wind_map`` each.

Fields are numpy arrays of one shape (or ``(R, C)`` device arrays), float32 or float64, all of one dtype (a mixed set is widened to
float64; integers are not served).  ``tas`` and ``tdps`` are in ``units`` ("K" or "degC"), ``hurs`` in %, ``huss`` in kg/kg, ``ps`` in
Pa, winds in m s-1 (``wind_units="km/h"`` for the wind chill), air density in kg m-3.  Thresholds are plain numbers: ``ice_thresh`` /
``water_thresh`` in K (or a string "<number> K" / "<number> degC"), ``calm_wind_thresh``, ``cut_in``, ``rated``, ``cut_out`` in the
unit of the wind.  Results come back in the fields' dtype (the float64 result rounded once): humidex and the heat index in
``units``, the dewpoint in K.

ASSUMPTIONS, in line with the sibling units: a unit conversion is one multiplication or one offset (% to 1 is ``* 0.01``, m s-1 to
km/h is ``* 3.6``, degC to K is ``+ 273.15``); the device widens float32 fields and computes in float64 where the reference stays in
float32.  A threshold the reference compares with the raw float32 field is rounded to float32 first, as numpy >= 2 does.
``wind_power_potential`` of a NaN speed is 0, as the reference's ``_wind_power_factor`` returns it.

Not served (:class:`NotServed`): integer fields, fields of different shapes (nothing is broadcast), array-valued thresholds,
temperature units other than K / degC.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _capi as capi
from . import fields as F
from . import kernels as K
from ._capi import DeviceArray, get_device
from .fields import NotServed
from .thermal import _ESAT_VALID, saturation_vapor_pressure

__all__ = ["NotServed", "OUTPUTS", "air_moisture", "saturation_vapor_pressure", "humidex", "heat_index", "vapor_pressure",
           "vapor_pressure_deficit", "relative_humidity", "specific_humidity", "specific_humidity_from_dewpoint",
           "dewpoint_from_specific_humidity", "uas_vas_to_sfcwind", "sfcwind_to_uas_vas", "wind_chill_index", "wind_power_potential",
           "SERVED"]

WHO = "humidity"
OUTPUTS = tuple(capi.AM_OUTPUTS)
SERVED = ("humidex", "heat_index", "vapor_pressure", "vapor_pressure_deficit", "relative_humidity", "specific_humidity",
          "specific_humidity_from_dewpoint", "dewpoint_from_specific_humidity", "uas_vas_to_sfcwind", "sfcwind_to_uas_vas",
          "wind_chill_index", "wind_power_potential")
SFCWIND = namedtuple("SFCWIND", ["wind", "wind_from_dir"])
UAS_VAS = namedtuple("UAS_VAS", ["uas", "vas"])


def _kelvin(thr, what):
    """A threshold in K: a number, or "<number> K" / "<number> degC" (any spelling of ``fields.T_SPELLINGS``)."""
    if thr is None:
        return None
    if isinstance(thr, str):
        v, _, u = thr.strip().partition(" ")
        try:
            unit, v = F.T_SPELLINGS[u.strip()], float(v)
        except (KeyError, ValueError):
            raise NotServed(f"{WHO}: {what} = {thr!r} is not a number in K or degC") from None
        return v + F.KELVIN_OFFSET if unit == "degC" else v
    if np.ndim(thr) != 0:
        raise NotServed(f"{WHO}: an array-valued {what} is not served")
    return float(thr)


def _number(v, what):
    """A plain number, or the number of a string "<number> <unit>" (the unit is the caller's business)."""
    if isinstance(v, str):
        try:
            return float(v.strip().partition(" ")[0])
        except ValueError:
            raise NotServed(f"{WHO}: {what} = {v!r} is not a number") from None
    if np.ndim(v) != 0:
        raise NotServed(f"{WHO}: an array-valued {what} is not served")
    return float(v)


def _esat_kw(ice_thresh, method, interp_power, water_thresh):
    """saturation_vapor_pressure's parameters (converters.py:580-600) as the kernel takes them."""
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
    return dict(method=method, case=case, ice_thresh=0.0 if ice_thresh is None else _kelvin(ice_thresh, "ice_thresh"),
                water_thresh=_kelvin(water_thresh, "water_thresh"), interp_power=1.0 if interp_power is None else float(interp_power))


def _rule(invalid_values):
    if invalid_values not in ("clip", "mask", None):   # (the reference ignores any other word: so does the kernel's "none")
        return "none"
    return invalid_values or "none"


def _celsius(units):
    try:
        return F.T_SPELLINGS[units] == "degC"
    except KeyError:
        raise NotServed(f"{WHO}: temperatures in {units!r} are not served (K or degC)") from None


def _prepare(fields, device):
    """The fields that are given as ``(R, C)`` device arrays of one dtype, and the shape to give the results."""
    got = {n: a for n, a in fields.items() if a is not None}
    for n, a in got.items():
        if not isinstance(a, DeviceArray) and np.asarray(a).dtype.kind in "iub":
            raise NotServed(f"{WHO}: {n} is an integer field")
    got = F.native_set(got)
    shapes = {tuple(a.shape) for a in got.values()}
    if len(shapes) != 1:
        raise NotServed(f"{WHO}: the fields have different shapes {sorted(shapes)} (nothing is broadcast)")
    shape = shapes.pop()
    if any(isinstance(a, DeviceArray) for a in got.values()) and len(shape) != 2:
        raise TypeError(f"{WHO}: device arrays must be (R, C)")
    R, C_ = (1, int(np.prod(shape, dtype=np.int64))) if len(shape) < 2 else (int(shape[0]), int(np.prod(shape[1:], dtype=np.int64)))
    dtype = np.dtype(next(iter(got.values())).dtype)
    return got, shape, R, C_, dtype


def _finish(outs, names, shape, R, C_, dtype, keep, device):
    if R == 0 or C_ == 0:
        if keep:
            dev = device or get_device()
            return {n: dev.empty((R, C_), dtype) for n in names}
        return {n: np.empty(shape, dtype) for n in names}
    return outs if keep else {n: outs[n].get().reshape(shape) for n in names}


def air_moisture(tas=None, tdps=None, hurs=None, huss=None, ps=None, outputs=("hurs",), *, units: str = "K", ice_thresh=None,
                 method: str = "sonntag90", interp_power=None, water_thresh=273.15, invalid_values="clip", huss_invalid_values=None,
                 dew_method: str = "buck81", variant: str = "water", device=None, keep: bool = False) -> dict:
    """Any set of ``OUTPUTS`` from ONE launch over the given fields: ``{name: array}`` in the fields' shape and dtype (``(R, C)`` device
    arrays with ``keep``).  ``method``: an e_sat method, or "bohren98" for the relative humidity (the other outputs then take
    "sonntag90").  ``invalid_values`` is relative_humidity's, ``huss_invalid_values`` specific_humidity's; ``dew_method`` and ``variant``
    are dewpoint_from_specific_humidity's.  Each output is the reference function of its name on these inputs; "huss" is
    ``specific_humidity``, "huss_dew" ``specific_humidity_from_dewpoint``, "tdps" the dewpoint, "esat" and "vp" the two pressures."""
    outputs = tuple(outputs)
    if not outputs or set(outputs) - set(OUTPUTS) or len(set(outputs)) != len(outputs):
        raise ValueError(f"outputs: distinct names of {OUTPUTS}")
    rh_method = "esat"
    if method in ("bohren98", "BA90"):
        rh_method, method = "bohren98", "sonntag90"
    kw = _esat_kw(ice_thresh, method, interp_power, water_thresh)
    dm = dew_method.casefold()
    if dm not in capi.DEW_METHODS:
        raise KeyError(dm)
    if variant not in ("water", "ice"):
        raise KeyError(variant)
    celsius = _celsius(units)
    got, shape, R, C_, dtype = _prepare(dict(tas=tas, tdps=tdps, hurs=hurs, huss=huss, ps=ps), device)
    outs = None
    if R and C_:
        dev = device or get_device()
        d = {n: F.rows_on_device(dev, a, R, C_) for n, a in got.items()}
        outs = K.air_moisture(dev, d, outputs, celsius=celsius, rh_method=rh_method, invalid_rh=_rule(invalid_values),
                              invalid_q=_rule(huss_invalid_values), dew_method=dm, dew_variant=variant, **kw)
    return _finish(outs, outputs, shape, R, C_, dtype, keep, device)


def _one(name, **kw):
    return air_moisture(outputs=(name,), **kw)[name]


def humidex(tas, tdps=None, hurs=None, *, units: str = "K", device=None, keep: bool = False):
    """converters.py:75-172: the humidex in ``units``, from the dewpoint when ``tdps`` is given, otherwise from ``hurs`` [%]."""
    if tdps is None and hurs is None:
        raise ValueError("At least one of `tdps` or `hurs` must be given.")
    return _one("humidex", tas=tas, tdps=tdps, hurs=None if tdps is not None else hurs, units=units, device=device, keep=keep)


def heat_index(tas, hurs, *, units: str = "K", device=None, keep: bool = False):
    """converters.py:175-223: the heat index in ``units``; NaN unless ``tas`` > 20 degC."""
    return _one("heat_index", tas=tas, hurs=hurs, units=units, device=device, keep=keep)


def vapor_pressure(huss, ps, *, device=None, keep: bool = False):
    """converters.py:606-638: the vapour pressure [Pa] of ``huss`` [kg/kg] and ``ps`` [Pa]."""
    return _one("vp", huss=huss, ps=ps, device=device, keep=keep)


def vapor_pressure_deficit(tas, hurs, ice_thresh=None, method: str = "sonntag90", interp_power=None, water_thresh=273.15, *,
                           units: str = "K", device=None, keep: bool = False):
    """converters.py:641-691: the vapour pressure deficit [Pa]."""
    return _one("vpd", tas=tas, hurs=hurs, ice_thresh=ice_thresh, method=method, interp_power=interp_power, water_thresh=water_thresh,
                units=units, device=device, keep=keep)


def relative_humidity(tas, tdps=None, huss=None, ps=None, ice_thresh=None, method: str = "sonntag90", interp_power=None,
                      water_thresh=273.15, invalid_values="clip", *, units: str = "K", device=None, keep: bool = False):
    """converters.py:694-841: the relative humidity [%] from ``tas`` and ``tdps`` (which overrides) or ``huss`` and ``ps``."""
    if method in ("bohren98", "BA90"):
        if tdps is None:
            raise ValueError("To use method 'bohren98' (BA98), dewpoint must be given.")
    elif tdps is None and (huss is None or ps is None):
        raise ValueError("`huss` and `ps` must be provided if `tdps` is not given.")
    if tdps is not None:
        huss = ps = None
    return _one("hurs", tas=tas, tdps=tdps, huss=huss, ps=ps, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                water_thresh=water_thresh, invalid_values=invalid_values, units=units, device=device, keep=keep)


def specific_humidity(tas, hurs, ps, ice_thresh=None, method: str = "sonntag90", interp_power=None, water_thresh=273.15,
                      invalid_values=None, *, units: str = "K", device=None, keep: bool = False):
    """converters.py:844-948: the specific humidity [1] from ``tas``, ``hurs`` [%] and ``ps`` [Pa]."""
    return _one("huss", tas=tas, hurs=hurs, ps=ps, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                water_thresh=water_thresh, huss_invalid_values=invalid_values, units=units, device=device, keep=keep)


def specific_humidity_from_dewpoint(tdps, ps, ice_thresh=None, method: str = "sonntag90", interp_power=None, water_thresh=273.15, *,
                                    units: str = "K", device=None, keep: bool = False):
    """converters.py:951-1021: the specific humidity [1] from the dewpoint and ``ps`` [Pa]."""
    return _one("huss_dew", tdps=tdps, ps=ps, ice_thresh=ice_thresh, method=method, interp_power=interp_power, water_thresh=water_thresh,
                units=units, device=device, keep=keep)


def dewpoint_from_specific_humidity(huss, ps, method: str = "buck81", variant: str = "water", *, device=None, keep: bool = False):
    """converters.py:1024-1084: the dewpoint [K]; NaN where ``huss`` <= 0."""
    return _one("tdps", huss=huss, ps=ps, dew_method=method, variant=variant, device=device, keep=keep)


# ---- the wind functions (xh_wind_map) --------------------------------------------------------------------------------------------
def _wind(op, a, b, par, flags, outputs, device, keep):
    got, shape, R, C_, dtype = _prepare({"a": a, "b": b}, device)
    outs = None
    if R and C_:
        dev = device or get_device()
        d = {n: F.rows_on_device(dev, v, R, C_) for n, v in got.items()}
        outs = K.wind_map(dev, op, d["a"], d.get("b"), par, flags=flags, outputs=outputs)
    return _finish(outs, outputs, shape, R, C_, dtype, keep, device)


def uas_vas_to_sfcwind(uas, vas, calm_wind_thresh=0.5, *, device=None, keep: bool = False):
    """converters.py:272-333: ``SFCWIND(wind [m s-1], wind_from_dir [degree])``; 360 is north, 0 a wind below ``calm_wind_thresh``."""
    r = _wind("from_uv", uas, vas, [_number(calm_wind_thresh, "calm_wind_thresh")], (), (0, 1), device, keep)
    return SFCWIND(r[0], r[1])


def sfcwind_to_uas_vas(sfcWind, sfcWindfromdir, *, device=None, keep: bool = False):
    """converters.py:336-387: ``UAS_VAS(uas, vas)`` [m s-1] from the speed and the direction the wind blows from [degree]."""
    r = _wind("to_uv", sfcWind, sfcWindfromdir, None, (), (0, 1), device, keep)
    return UAS_VAS(r[0], r[1])


def wind_chill_index(tas, sfcWind, method: str = "CAN", mask_invalid: bool = True, *, units: str = "K", wind_units: str = "m s-1",
                     device=None, keep: bool = False):
    """converters.py:1659-1744: the wind chill index [degC]."""
    if method.upper() not in ("CAN", "US"):
        raise ValueError(f"`method` must be one of 'US' and 'CAN'. Got '{method}'.")
    if wind_units not in ("m s-1", "m/s", "km/h", "km h-1"):
        raise NotServed(f"{WHO}: winds in {wind_units!r} are not served (m s-1 or km/h)")
    flags = [f for f, on in (("celsius", _celsius(units)), ("kmh", wind_units in ("km/h", "km h-1")), ("us", method.upper() == "US"),
                             ("mask_invalid", bool(mask_invalid))) if on]
    return _wind("chill", tas, sfcWind, None, flags, (0,), device, keep)[0]


def wind_power_potential(wind_speed, air_density=None, cut_in=3.5, rated=13.0, cut_out=25.0, *, device=None, keep: bool = False):
    """converters.py:2797-2902: the power production factor [1]; ``cut_in`` < ``rated`` and ``cut_out`` in the unit of ``wind_speed``,
    ``air_density`` in kg m-3."""
    par = [_number(cut_in, "cut_in"), _number(rated, "rated"), _number(cut_out, "cut_out")]
    if not par[0] < par[1]:
        raise NotServed(f"{WHO}: wind_power_potential needs cut_in < rated")
    return _wind("power", wind_speed, air_density, par, (), (0,), device, keep)[0]


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------------------
ADAPTED = SERVED
_ONE = ("1", "", "kg/kg", "kg kg-1")
_MS, _KMH = ("m s-1", "m/s"), ("km/h", "km h-1")
_DENSITY = ("kg m-3", "kg/m3", "kg/m^3", "kg m^-3")


def make_adapters(env, origs: dict, device=None) -> dict:
    """Same-signature replacements of the twelve functions of ``ADAPTED`` on DataArrays of any dimensions.  Fields in the other unit of
    the same kind go through ``env.convert_units_to`` (hurs given as a fraction, huss in %, a wind in km/h), thresholds likewise; the
    results carry the reference's ``units`` and attributes and the dimensions and coordinates of the first field.  Whatever raises
    :class:`NotServed` goes to the original with the arguments as they came: chunked or integer fields, fields of different dtypes,
    operands on different dimensions or of different shapes (they would need broadcasting), Fahrenheit or any other unit outside
    K / degC / % / 1 / Pa / m s-1 / km/h (kg m-3 for the density), array-valued thresholds."""
    from .xr_adapter import is_chunked, threshold_number

    DA = env.DataArray

    def units_of(v):
        return str(v.attrs.get("units", "")).strip()

    def admitted(fields):
        """The fields that are not None: DataArrays, not chunked, float32 or float64 of one dtype, on the same dimensions in the same
        order and of one shape.  Returns the first one and ``{name: values}``."""
        got = {k: v for k, v in fields.items() if v is not None}
        first = next(iter(got.values()))
        for k, v in got.items():
            if not isinstance(v, DA) or is_chunked(v):
                raise NotServed(f"{WHO}: {k} is chunked or not a DataArray")
            if tuple(v.dims) != tuple(first.dims) or tuple(v.shape) != tuple(first.shape):
                raise NotServed(f"{WHO}: {k} would need broadcasting")
        vals = {k: np.asarray(v.values) for k, v in got.items()}
        if len({a.dtype for a in vals.values()}) != 1 or next(iter(vals.values())).dtype not in F.SERVED:
            raise NotServed(f"{WHO}: integer fields or fields of different dtypes")
        return first, vals

    def temperature_units(fields):
        """"K" or "degC", the one unit of the temperature fields given."""
        kinds = set()
        for k, v in fields.items():
            if v is not None:
                if not isinstance(v, DA) or units_of(v) not in F.T_SPELLINGS:
                    raise NotServed(f"{WHO}: {k} is not in K or degC")
                kinds.add(F.T_SPELLINGS[units_of(v)])
        if len(kinds) > 1:
            raise NotServed(f"{WHO}: temperatures in different units")
        return kinds.pop() if kinds else "K"

    def in_units(k, v, accepted, other, target):
        """``v`` as it is when its unit is one of ``accepted``, converted to ``target`` when it is one of ``other``."""
        if v is None:
            return None
        if not isinstance(v, DA) or is_chunked(v):
            raise NotServed(f"{WHO}: {k} is chunked or not a DataArray")
        if units_of(v) in accepted:
            return v
        if units_of(v) in other:
            return env.convert_units_to(v, target)
        raise NotServed(f"{WHO}: {k} in {units_of(v)!r}")

    def percent(v):
        return in_units("hurs", v, ("%",), _ONE, "%")

    def fraction(v):
        return in_units("huss", v, _ONE, ("%",), "1")

    def pascal(v):
        return in_units("ps", v, ("Pa",), (), "Pa")

    def metres_per_second(k, v):
        return in_units(k, v, _MS, _KMH, "m s-1")

    def wrap(a, values, attrs):
        return DA(np.asarray(values), coords=dict(a.coords), dims=tuple(a.dims), attrs=attrs)

    def esat_kw(ice_thresh, interp_power, water_thresh):
        return dict(ice_thresh=None if ice_thresh is None else threshold_number(env, ice_thresh, "K"), interp_power=interp_power,
                    water_thresh=273.15 if water_thresh == "0 °C" else threshold_number(env, water_thresh, "K"))

    def moisture(output, attrs, fields, **kw):
        a, vals = admitted(fields)
        return wrap(a, air_moisture(**vals, outputs=(output,), device=device, **kw)[output], attrs)

    def humidex(tas, tdps=None, hurs=None):
        try:
            if tdps is None and hurs is None:
                raise ValueError("At least one of `tdps` or `hurs` must be given.")
            units = temperature_units(dict(tas=tas, tdps=tdps))
            fields = dict(tas=tas, tdps=tdps) if tdps is not None else dict(tas=tas, hurs=percent(hurs))
            return moisture("humidex", {"units": tas.attrs["units"]}, fields, units=units)
        except NotServed:
            return origs["humidex"](tas, tdps=tdps, hurs=hurs)

    def heat_index(tas, hurs):
        try:
            return moisture("heat_index", {"units": tas.attrs["units"]} if isinstance(tas, DA) else {}, dict(tas=tas, hurs=percent(hurs)),
                            units=temperature_units(dict(tas=tas)))
        except NotServed:
            return origs["heat_index"](tas, hurs)

    def vapor_pressure(huss, ps):
        try:
            return moisture("vp", {"units": "Pa"}, dict(huss=fraction(huss), ps=pascal(ps)))
        except NotServed:
            return origs["vapor_pressure"](huss, ps)

    def vapor_pressure_deficit(tas, hurs, ice_thresh=None, method="sonntag90", interp_power=None, water_thresh="0 °C"):
        try:
            return moisture("vpd", {"units": "Pa"}, dict(tas=tas, hurs=percent(hurs)), units=temperature_units(dict(tas=tas)), method=method,
                            **esat_kw(ice_thresh, interp_power, water_thresh))
        except NotServed:
            return origs["vapor_pressure_deficit"](tas, hurs, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                                                   water_thresh=water_thresh)

    def relative_humidity(tas, tdps=None, huss=None, ps=None, ice_thresh=None, method="sonntag90", interp_power=None, water_thresh="0 °C",
                          invalid_values="clip"):
        try:
            if method in ("bohren98", "BA90"):
                if tdps is None:
                    raise ValueError("To use method 'bohren98' (BA98), dewpoint must be given.")
            elif tdps is None and (huss is None or ps is None):
                raise ValueError("`huss` and `ps` must be provided if `tdps` is not given.")
            fields = dict(tas=tas, tdps=tdps) if tdps is not None else dict(tas=tas, huss=fraction(huss), ps=pascal(ps))
            return moisture("hurs", {"units": "%"}, fields, units=temperature_units(dict(tas=tas, tdps=tdps)), method=method,
                            invalid_values=invalid_values, **esat_kw(ice_thresh, interp_power, water_thresh))
        except NotServed:
            return origs["relative_humidity"](tas, tdps=tdps, huss=huss, ps=ps, ice_thresh=ice_thresh, method=method,
                                              interp_power=interp_power, water_thresh=water_thresh, invalid_values=invalid_values)

    def specific_humidity(tas, hurs, ps, ice_thresh=None, method="sonntag90", interp_power=None, water_thresh="0 °C", invalid_values=None):
        try:
            return moisture("huss", {"units": ""}, dict(tas=tas, hurs=percent(hurs), ps=pascal(ps)), units=temperature_units(dict(tas=tas)),
                            method=method, huss_invalid_values=invalid_values, **esat_kw(ice_thresh, interp_power, water_thresh))
        except NotServed:
            return origs["specific_humidity"](tas, hurs, ps, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                                              water_thresh=water_thresh, invalid_values=invalid_values)

    def specific_humidity_from_dewpoint(tdps, ps, ice_thresh=None, method="sonntag90", interp_power=None, water_thresh="0 °C"):
        try:
            return moisture("huss_dew", {"units": ""}, dict(tdps=tdps, ps=pascal(ps)), units=temperature_units(dict(tdps=tdps)), method=method,
                            **esat_kw(ice_thresh, interp_power, water_thresh))
        except NotServed:
            return origs["specific_humidity_from_dewpoint"](tdps, ps, ice_thresh=ice_thresh, method=method, interp_power=interp_power,
                                                            water_thresh=water_thresh)

    def dewpoint_from_specific_humidity(huss, ps, method="buck81", variant="water"):
        try:
            return moisture("tdps", {"units": "K", "units_metadata": "temperature: on_scale"}, dict(huss=fraction(huss), ps=pascal(ps)),
                            dew_method=method, variant=variant)
        except NotServed:
            return origs["dewpoint_from_specific_humidity"](huss, ps, method=method, variant=variant)

    def wind(op, a, b, par, flags, attrs):
        first, vals = admitted({"a": a, "b": b})
        outputs = tuple(range(len(attrs)))
        res = _wind(op, vals["a"], vals.get("b"), par, flags, outputs, device, False)
        return [wrap(first, res[o], at) for o, at in zip(outputs, attrs)]

    def uas_vas_to_sfcwind(uas, vas, calm_wind_thresh="0.5 m/s"):
        try:
            w, d = wind("from_uv", metres_per_second("uas", uas), metres_per_second("vas", vas), [threshold_number(env, calm_wind_thresh, "m s-1")], (),
                        ({"units": "m s-1"}, {"units": "degree"}))
            return SFCWIND(w, d)
        except NotServed:
            return origs["uas_vas_to_sfcwind"](uas, vas, calm_wind_thresh=calm_wind_thresh)

    def sfcwind_to_uas_vas(sfcWind, sfcWindfromdir):
        try:
            if not isinstance(sfcWindfromdir, DA) or units_of(sfcWindfromdir) not in ("degree", "degrees", "deg", "°"):
                raise NotServed(f"{WHO}: sfcWindfromdir is not in degrees")
            u, v = wind("to_uv", metres_per_second("sfcWind", sfcWind), sfcWindfromdir, None, (), ({"units": "m s-1"}, {"units": "m s-1"}))
            return UAS_VAS(u, v)
        except NotServed:
            return origs["sfcwind_to_uas_vas"](sfcWind, sfcWindfromdir)

    def wind_chill_index(tas, sfcWind, method="CAN", mask_invalid=True):
        try:
            if method.upper() not in ("CAN", "US"):
                raise ValueError(f"`method` must be one of 'US' and 'CAN'. Got '{method}'.")
            ws = in_units("sfcWind", sfcWind, _MS + _KMH, (), "km/h")
            flags = [f for f, on in (("celsius", temperature_units(dict(tas=tas)) == "degC"), ("kmh", units_of(ws) in _KMH),
                                     ("us", method.upper() == "US"), ("mask_invalid", bool(mask_invalid))) if on]
            return wind("chill", tas, ws, None, flags, ({"units": "degC"},))[0]
        except NotServed:
            return origs["wind_chill_index"](tas, sfcWind, method=method, mask_invalid=mask_invalid)

    def wind_power_potential(wind_speed, air_density=None, cut_in="3.5 m/s", rated="13 m/s", cut_out="25 m/s"):
        try:
            ws = in_units("wind_speed", wind_speed, _MS + _KMH, (), "m s-1")
            rho = in_units("air_density", air_density, _DENSITY, (), "kg m-3")
            par = [threshold_number(env, q, units_of(ws)) for q in (cut_in, rated, cut_out)]
            if not par[0] < par[1]:
                raise NotServed(f"{WHO}: wind_power_potential needs cut_in < rated")
            return wind("power", ws, rho, par, (), ({"units": ""},))[0]
        except NotServed:
            return origs["wind_power_potential"](wind_speed, air_density=air_density, cut_in=cut_in, rated=rated, cut_out=cut_out)

    loc = locals()
    out = {n: loc[n] for n in ADAPTED}
    for n, fn in out.items():
        fn.__wrapped__ = origs[n]
        fn.__doc__ = getattr(origs[n], "__doc__", None)
    return out
