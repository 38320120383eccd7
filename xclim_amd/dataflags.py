"""Host mirror of the data-quality flags of the reference (src/xclim/core/dataflags.py): the thirteen check functions,
``data_flags``, ``ecad_compliant`` and ``DataQualityException``.  The kernels are in xclim_amd/csrc/dataflags.hip, their C ABI in
include/xclim_hip_flags.h.

The functions carry the reference's names, parameters and defaults, plus ``units`` (the units of the field: thresholds given as
``"<number> <unit>"`` strings are converted to them; plain numbers are taken as they are), ``time`` (a daily
:class:`~xclim_amd.timeaxis.TimeAxis`, needed only for ``freq`` and for the climatology check) and ``device``.  Inputs are numpy
arrays with TIME ON AXIS 0, float32 or float64; results are bool arrays.  A check function returns the ``(T, *cells)`` mask;
``data_flags`` returns an ordered mapping flag name -> bool array (``None`` where a companion variable is absent), aggregated as
``dims`` ("all", None, "time" or "cells") and ``freq`` say.

ONE launch of ``xh_data_flags`` evaluates the whole list of checks of a ``data_flags`` call (more than ``FLAGS_MAX_CHECKS``
checks, more than two companion variables or more than one climatology setting go in several), preceded by one launch of
``xh_doy_bounds`` when the climatology check is in the list.  Only the aggregated flag bytes come back to the host.

ASSUMPTIONS (xarray is neither needed nor used here).  A sample is widened to float64 and compared with the float64 threshold;
numpy >= 2 compares a float32 field with a Python float in float32, which differs only for thresholds that are not float32
values.  The climatology tables are those of ``xh_doy_bounds``: sums in float64 in (year, window) order, mean and deviation
rounded to the field's dtype, then ``mean -+ n * std`` in the field's dtype.  "mm d-1" becomes a rate per second as ``v / 86400``.
The descriptions print converted thresholds as Python floats.

:class:`NotServed` (the adapter forwards these to the reference): integer fields (any dtype but float32 and float64); fields of
mixed dtype in one call; array thresholds; units outside the table (temperature ``K`` / ``degC``, rates ``kg m-2 s-1`` / ``mm/s`` /
``mm d-1`` / ``mm/d``, speeds ``m s-1`` / ``m/s``; identical spellings always pass); a pair check whose variable under test is
neither of its operands; ``flags=None`` where ``xclim.core.VARIABLES`` cannot be imported and no ``variables`` table is given
(the table is the reference's data and is not restated here); and, with ``freq`` or the climatology check, non-daily or gappy
axes and a series that does not contain its calendar's last day of year (the reference then re-interpolates the day-of-year
tables).
"""

from __future__ import annotations

import re
from collections import OrderedDict

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import FLAGS_MAX_CHECKS, get_device
from .fields import KELVIN_OFFSET, NotServed, daily_axis
from .fields import per_day as _per_day
from .timeaxis import TimeAxis

__all__ = ["DataQualityException", "data_flags", "ecad_compliant", "negative_accumulation_values",
           "outside_n_standard_deviations_of_climatology", "percentage_values_outside_of_bounds", "specific_discharge_extremely_high",
           "tas_below_tasmin", "tas_exceeds_tasmax", "tasmax_below_tasmin", "temperature_extremely_high", "temperature_extremely_low",
           "values_op_thresh_repeating_for_n_or_more_days", "values_repeating_for_n_or_more_days", "very_large_precipitation_events",
           "wind_values_outside_of_bounds", "flag_name", "describe", "convert_threshold", "CHECK_NAMES", "NotServed", "FLAGS_MAX_CHECKS",
           "ADAPTED", "make_adapters"]

BINARY_OPS = {">": "gt", "<": "lt", ">=": "ge", "<=": "le", "==": "eq", "!=": "ne"}
_SYMBOL = {v: k for k, v in BINARY_OPS.items()}
_SWAPPED = {">": "<", "<": ">", ">=": "<=", "<=": ">=", "==": "==", "!=": "!="}
_NUMBER = re.compile(r"\s*([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)\s*(.*?)\s*")
_SPEEDS = ("m s-1", "m/s")
_RATES = dict(F.FLUX_SPELLINGS, **{"mm d-1": "mm/d"})


class DataQualityException(Exception):
    """Raised when any data evaluation check is flagged as True (core/dataflags.py:32-63).  ``flag_array``: a Dataset (its
    variables carry their ``description``) or a mapping flag name -> array with ``descriptions`` next to it."""

    flag_array = None

    def __init__(self, flag_array, message="Data quality flags indicate suspicious values. Flags raised are:\n  - ", descriptions=None):
        self.flag_array = flag_array
        self.message = message
        self.flags = []
        items = flag_array.data_vars.items() if hasattr(flag_array, "data_vars") else flag_array.items()
        for name, value in items:
            if value is None or not np.any(getattr(value, "values", value)):
                continue
            text = getattr(value, "attrs", {}).get("description", (descriptions or {}).get(name))
            if text is not None:
                self.flags.append(text)
        super().__init__(self.message)

    def __str__(self):
        nl = "\n  - "
        return f"{self.message}{nl.join(self.flags)}"


# ---- thresholds and names ----------------------------------------------------------------------------------------------------
def _split(q):
    """(magnitude, unit string or None) of a threshold: a number, or a "<number> <unit>" string."""
    if isinstance(q, bool):
        raise TypeError("a threshold must be a number or a string")
    if isinstance(q, (int, float, np.integer, np.floating)):
        return q, None
    if isinstance(q, str):
        m = _NUMBER.fullmatch(q)
        if m is None:
            raise NotServed(f"data_flags: threshold {q!r} is not '<number> <unit>'")
        text = m.group(1)
        return (int(text) if re.fullmatch(r"[-+]?\d+", text) else float(text)), (m.group(2) or None)
    raise NotServed("data_flags: array thresholds")


def convert_threshold(q, units) -> float:
    """A threshold as a float in the field's ``units`` (the module text lists the served conversions)."""
    mag, src = _split(q)
    mag = float(mag)
    if src is None or src == units:
        return mag
    if units is None:
        raise NotServed(f"data_flags: a threshold in {src!r} needs the units of the field")
    if src in F.T_SPELLINGS and units in F.T_SPELLINGS:
        a, b = F.T_SPELLINGS[src], F.T_SPELLINGS[units]
        return mag if a == b else (mag + KELVIN_OFFSET if b == "K" else mag - KELVIN_OFFSET)
    if src in _RATES and units in _RATES:
        a, b = _per_day(_RATES[src]), _per_day(_RATES[units])
        return mag if a == b else (mag / 86400.0 if a == 1.0 else mag * 86400.0)
    if src in _SPEEDS and units in _SPEEDS:
        return mag
    raise NotServed(f"data_flags: no conversion from {src!r} to {units!r}")


def _magnitude_text(q) -> str:
    """`_get_variable_name` (core/dataflags.py:655-665): integral magnitudes print as integers, "." -> "point", "-" -> "minus"."""
    mag, _ = _split(q)
    text = str(int(mag)) if mag == int(mag) else str(mag).replace(".", "point")
    return text.replace("-", "minus")


# name -> (name template, the variables it takes, {parameter: default}); a default of ... means "required"
_CHECKS = OrderedDict([
    ("tasmax_below_tasmin", (None, ("tasmax", "tasmin"), {})),
    ("tas_exceeds_tasmax", (None, ("tas", "tasmax"), {})),
    ("tas_below_tasmin", (None, ("tas", "tasmin"), {})),
    ("temperature_extremely_low", (None, ("da",), {"thresh": "-90 degC"})),
    ("temperature_extremely_high", (None, ("da",), {"thresh": "60 degC"})),
    ("negative_accumulation_values", (None, ("da",), {})),
    ("very_large_precipitation_events", (None, ("da",), {"thresh": "300 mm d-1"})),
    ("values_op_thresh_repeating_for_n_or_more_days", ("values_{op}_{thresh}_repeating_for_{n}_or_more_days", ("da",),
                                                       {"n": ..., "thresh": ..., "op": "=="})),
    ("wind_values_outside_of_bounds", (None, ("da",), {"lower": "0 m s-1", "upper": "46 m s-1"})),
    ("outside_n_standard_deviations_of_climatology", ("outside_{n}_standard_deviations_of_climatology", ("da",), {"n": ..., "window": 5})),
    ("values_repeating_for_n_or_more_days", ("values_repeating_for_{n}_or_more_days", ("da",), {"n": ...})),
    ("percentage_values_outside_of_bounds", (None, ("da",), {})),
    ("specific_discharge_extremely_high", (None, ("da",), {"thresh": "100 mm d-1"})),
])
CHECK_NAMES = tuple(_CHECKS)
_PAIR_OPS = {"tasmax_below_tasmin": "<", "tas_exceeds_tasmax": ">", "tas_below_tasmin": "<"}
_QUANTIFIED = ("thresh", "lower", "upper")


def _parameters(check, kwargs):
    if check not in _CHECKS:
        raise KeyError(check)
    defaults = _CHECKS[check][2]
    kwargs = dict(kwargs or {})
    extra = set(kwargs) - set(defaults)
    if extra:
        raise TypeError(f"{check}() got an unexpected keyword argument {sorted(extra)[0]!r}")
    p = {k: kwargs.get(k, d) for k, d in defaults.items()}
    missing = [k for k, v in p.items() if v is ...]
    if missing:
        raise TypeError(f"{check}() missing required keyword-only argument: {missing[0]!r}")
    return p


def flag_name(check: str, kwargs=None) -> str:
    """The name of a flag in the result of ``data_flags`` (`_get_variable_name`, core/dataflags.py:638-666)."""
    p = _parameters(check, kwargs)
    template = _CHECKS[check][0]
    if template is None:
        return check
    fmt = {}
    for k, v in p.items():
        if k == "op":
            fmt[k] = BINARY_OPS.get(v, v)
        elif k in _QUANTIFIED:
            fmt[k] = "array" if isinstance(v, np.ndarray) else _magnitude_text(v)
        else:
            fmt[k] = v
    return template.format(**fmt)


def _window(name, v, least=1):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name} must be an integer of at least {least}, got {v!r}")
    return int(v)


def _plan(check, kwargs, var, units, convert=None):
    """One check as ``(spec, description, has a units attribute)``; spec = ("cmp", op, a) | ("outside", a, b) | ("pair", op, the other
    variable's name) | ("repeat", op or None, a, n) | ("clim", n, window).  ``convert(threshold, units)`` makes a threshold a float in
    the field's units (:func:`convert_threshold` by default)."""
    p = _parameters(check, kwargs)
    who = var if var is not None else "None"
    conv = convert or convert_threshold
    if check in _PAIR_OPS:
        first, second = _CHECKS[check][1]
        op = _PAIR_OPS[check]
        if var not in (first, second):
            raise NotServed(f"data_flags: {check} on {who!r}, which is neither of its operands")
        spec = ("pair", op, second) if var == first else ("pair", _SWAPPED[op], first)
        text = {"tasmax_below_tasmin": "Maximum temperature values found below minimum temperatures.",
                "tas_exceeds_tasmax": "Mean temperature values found above maximum temperatures.",
                "tas_below_tasmin": "Mean temperature values found below minimum temperatures."}[check]
        return spec, text, True
    if check == "temperature_extremely_low":
        return ("cmp", "<", conv(p["thresh"], units)), f"Temperatures found below {p['thresh']} in {who}.", True
    if check == "temperature_extremely_high":
        return ("cmp", ">", conv(p["thresh"], units)), f"Temperatures found in excess of {p['thresh']} in {who}.", True
    if check == "negative_accumulation_values":
        return ("cmp", "<", 0.0), f"Negative values found for {who}.", True
    if check == "very_large_precipitation_events":
        return ("cmp", ">", conv(p["thresh"], units)), f"Precipitation events in excess of {p['thresh']} for {who}.", True
    if check == "specific_discharge_extremely_high":
        return ("cmp", ">", conv(p["thresh"], units)), f"One or multiple specific {who} found in excess of {p['thresh']}.", True
    if check == "values_op_thresh_repeating_for_n_or_more_days":
        op = _SYMBOL.get(p["op"], p["op"])
        if op not in BINARY_OPS:
            raise NotImplementedError(f"{p['op']}")
        thr, n = conv(p["thresh"], units), _window("n", p["n"])
        return ("repeat", op, thr, n), f"Repetitive values at {thr} for at least {n} days found for {who}.", True
    if check == "values_repeating_for_n_or_more_days":
        n = _window("n", p["n"])
        return ("repeat", None, 0.0, n), f"Runs of repetitive values for {n} or more days found for {who}.", True
    if check == "wind_values_outside_of_bounds":
        lo, hi = conv(p["lower"], units), conv(p["upper"], units)
        return ("outside", lo, hi), f"Percentage values exceeding bounds of {lo} and {hi} found for {who}.", True
    if check == "percentage_values_outside_of_bounds":
        return ("outside", 0.0, 100.0), f"Percentage values beyond bounds found for {who}.", False
    n, window = p["n"], _window("window", p["window"])
    if isinstance(n, bool) or not isinstance(n, (int, float, np.integer, np.floating)):
        raise TypeError("n must be a number")
    return (("clim", float(n), window),
            f"Values outside of {n} standard deviations from climatology found for {who} with moving window of {window} days.", True)


# ---- the launches ------------------------------------------------------------------------------------------------------------
def _field(a, what):
    a = np.asarray(a)
    if a.dtype not in F.SERVED:
        raise NotServed(f"data_flags: {what} is {a.dtype.name}; float32 and float64 fields are served")
    if a.ndim < 1:
        raise ValueError("fields must have a time axis (axis 0)")
    return a


def _clim_axis(time, T):
    """(tbase, tidx) of a daily axis that holds its calendar's last day of year."""
    daily_axis(time, T, "data_flags")
    tb, _, doys = time.doy_table()
    if T and int(doys.max()) != time.max_doy():
        raise NotServed("data_flags: a series without its calendar's last day of year (the reference re-interpolates the day-of-year tables)")
    return tb, np.searchsorted(doys, time.doy).astype(np.int32)


def _evaluate(x, specs, companions, seg, reduce_cells, time, device):
    """The flags of ``specs`` on the periods ``seg``: a list of bool arrays ``(P, *cells)``, or ``(P,)`` with ``reduce_cells``."""
    x = _field(x, "the field")
    T, cell_shape, C_ = x.shape[0], x.shape[1:], int(np.prod(x.shape[1:], dtype=np.int64))
    seg = np.asarray(seg, np.int64)
    P = len(seg) - 1
    others = {}
    for s in specs:
        if s[0] == "pair" and s[2] not in others:
            y = _field(companions[s[2]], s[2])
            if y.dtype != x.dtype:
                raise NotServed(f"data_flags: {s[2]} is {y.dtype.name}, the field {x.dtype.name}")
            if y.shape != x.shape:
                raise ValueError(f"{s[2]}: shape {y.shape} differs from {x.shape}")
            others[s[2]] = y
    shape = (P,) if reduce_cells else (P,) + tuple(cell_shape)
    clim = any(s[0] == "clim" for s in specs)
    if clim:
        tbase, tidx = _clim_axis(time, T)
    if T == 0 or C_ == 0 or P == 0 or not specs:
        return [np.zeros(shape, bool) for _ in specs]
    dev = device or get_device()
    dx = F.rows_on_device(dev, x, T, C_)
    dys = {}
    results = [None] * len(specs)
    todo = list(range(len(specs)))
    while todo:   # one launch takes at most FLAGS_MAX_CHECKS checks, two companions and one climatology setting
        batch, names, setting = [], [], None
        for i in list(todo):
            s = specs[i]
            if len(batch) == FLAGS_MAX_CHECKS:
                break
            if s[0] == "pair" and s[2] not in names:
                if len(names) == 2:
                    continue
                names.append(s[2])
            if s[0] == "clim":
                if setting not in (None, s[1:]):
                    continue
                setting = s[1:]
            batch.append(i)
            todo.remove(i)
        for nm in names:
            if nm not in dys:
                dys[nm] = F.rows_on_device(dev, others[nm], T, C_)
        lo = hi = None
        if setting is not None:
            lo, hi = K.doy_bounds(dev, dx, tbase, setting[1], setting[0])
        checks = []
        for i in batch:
            s = specs[i]
            if s[0] == "cmp":
                checks.append(K.flag_check("cmp", s[1], s[2]))
            elif s[0] == "outside":
                checks.append(K.flag_check("outside", None, s[1], s[2]))
            elif s[0] == "pair":
                checks.append(K.flag_check("pair", s[1], other=names.index(s[2])))
            elif s[0] == "repeat":
                checks.append(K.flag_check("repeat", s[1], s[2], n=s[3]))
            else:
                checks.append(K.flag_check("clim"))
        out = K.data_flags(dev, dx, checks, seg, y0=dys[names[0]] if names else None, y1=dys[names[1]] if len(names) > 1 else None,
                           tidx=tidx if setting is not None else None, lo=lo, hi=hi, reduce_cells=reduce_cells).get()
        for k, i in enumerate(batch):
            results[i] = out[k].reshape(shape).astype(bool)
    return results


def _single(check, var, fields, kwargs, units, time, device):
    """The element-wise mask of one check function: every row a period of its own."""
    spec, _, _ = _plan(check, kwargs, var, units)
    x = np.asarray(fields[var])
    T = x.shape[0] if x.ndim else 0
    return _evaluate(x, [spec], fields, np.arange(T + 1, dtype=np.int64), False, time, device)[0]


def tasmax_below_tasmin(tasmax, tasmin, *, device=None):
    """core/dataflags.py:124-158: ``tasmax < tasmin``."""
    return _single("tasmax_below_tasmin", "tasmax", {"tasmax": tasmax, "tasmin": tasmin}, None, None, None, device)


def tas_exceeds_tasmax(tas, tasmax, *, device=None):
    """core/dataflags.py:161-195: ``tas > tasmax``."""
    return _single("tas_exceeds_tasmax", "tas", {"tas": tas, "tasmax": tasmax}, None, None, None, device)


def tas_below_tasmin(tas, tasmin, *, device=None):
    """core/dataflags.py:198-229: ``tas < tasmin``."""
    return _single("tas_below_tasmin", "tas", {"tas": tas, "tasmin": tasmin}, None, None, None, device)


def temperature_extremely_low(da, *, thresh="-90 degC", units=None, device=None):
    """core/dataflags.py:232-266: ``da < thresh``."""
    return _single("temperature_extremely_low", "da", {"da": da}, {"thresh": thresh}, units, None, device)


def temperature_extremely_high(da, *, thresh="60 degC", units=None, device=None):
    """core/dataflags.py:269-303: ``da > thresh``."""
    return _single("temperature_extremely_high", "da", {"da": da}, {"thresh": thresh}, units, None, device)


def negative_accumulation_values(da, *, device=None):
    """core/dataflags.py:306-336: ``da < 0``."""
    return _single("negative_accumulation_values", "da", {"da": da}, None, None, None, device)


def very_large_precipitation_events(da, *, thresh="300 mm d-1", units=None, device=None):
    """core/dataflags.py:339-372: ``da > thresh``."""
    return _single("very_large_precipitation_events", "da", {"da": da}, {"thresh": thresh}, units, None, device)


def values_op_thresh_repeating_for_n_or_more_days(da, *, n, thresh, op="==", units=None, device=None):
    """core/dataflags.py:375-416: runs of at least ``n`` equal values that satisfy ``op thresh``."""
    return _single("values_op_thresh_repeating_for_n_or_more_days", "da", {"da": da}, {"n": n, "thresh": thresh, "op": op}, units, None, device)


def wind_values_outside_of_bounds(da, *, lower="0 m s-1", upper="46 m s-1", units=None, device=None):
    """core/dataflags.py:419-458: ``(da < lower) | (da > upper)``."""
    return _single("wind_values_outside_of_bounds", "da", {"da": da}, {"lower": lower, "upper": upper}, units, None, device)


def outside_n_standard_deviations_of_climatology(da, *, n, window=5, time: TimeAxis = None, device=None):
    """core/dataflags.py:464-516: outside ``mean -+ n * std`` of the day-of-year climatology over a centred ``window``."""
    return _single("outside_n_standard_deviations_of_climatology", "da", {"da": da}, {"n": n, "window": window}, None, time, device)


def values_repeating_for_n_or_more_days(da, *, n, device=None):
    """core/dataflags.py:519-549: runs of at least ``n`` equal values."""
    return _single("values_repeating_for_n_or_more_days", "da", {"da": da}, {"n": n}, None, None, device)


def percentage_values_outside_of_bounds(da, *, device=None):
    """core/dataflags.py:552-578: ``(da < 0) | (da > 100)``."""
    return _single("percentage_values_outside_of_bounds", "da", {"da": da}, None, None, None, device)


def specific_discharge_extremely_high(da, *, thresh="100 mm d-1", units=None, device=None):
    """core/dataflags.py:822-851: ``da > thresh``."""
    return _single("specific_discharge_extremely_high", "da", {"da": da}, {"thresh": thresh}, units, None, device)


# ---- data_flags --------------------------------------------------------------------------------------------------------------
def _flag_list(flags, name, variables):
    """The checks as a list of ``(check, kwargs)``: the reference's single dict, the list of dicts of ``VARIABLES``, or the
    defaults of ``name``; None where the table has no checks for the variable."""
    if flags is None:
        if variables is None:
            try:
                from xclim.core import VARIABLES as variables
            except ImportError:
                raise NotServed("data_flags: flags=None needs xclim.core.VARIABLES (or a `variables` table)") from None
        try:
            flags = variables.get(name)["data_flags"]
        except (KeyError, TypeError):
            return None
    if isinstance(flags, dict):
        flags = [flags]
    return [(check, kwargs) for entry in flags for check, kwargs in entry.items()]


def describe(name, flags=None, ds=(), units=None, variables=None, convert=None) -> OrderedDict:
    """flag name -> ``(spec, description, has a units attribute, check, kwargs)`` of the checks of a ``data_flags`` call, ``None`` for
    a flag whose companion variable is not among ``ds``; ``None`` altogether where the variable has no checks."""
    entries = _flag_list(flags, name, variables)
    if entries is None:
        return None
    out = OrderedDict()
    for check, kwargs in entries:
        label = flag_name(check, kwargs)
        needed = [v for v in _CHECKS[check][1] if v not in ("da", name)]
        out[label] = None if any(v not in ds for v in needed) else (*_plan(check, kwargs, name, units, convert), check, kwargs)
    return out


def _aggregation(dims, freq, time, T):
    """(row offsets of the periods, reduce over cells, drop the period axis) of ``dims`` and ``freq``."""
    if dims not in ("all", None, "time", "cells"):
        raise NotServed(f"data_flags: dims={dims!r}; 'all', None, 'time' and 'cells' are served")
    if freq is not None:
        F.check_freq(freq)
        daily_axis(time, T, "data_flags")
        return F.period_segments(time, freq), dims in ("all", "cells"), False
    if dims in ("all", "time"):
        return np.array([0, T], np.int64), dims == "all", True
    return np.arange(T + 1, dtype=np.int64), dims == "cells", False


def _run(plans, x, name, ds, dims, freq, time, device) -> OrderedDict:
    """The flags of :func:`describe`'s ``plans`` on the field ``x``: flag name -> bool array or None."""
    x = _field(x, name)
    seg, over_cells, squeeze = _aggregation(dims, freq, time, x.shape[0])
    served = [k for k, v in plans.items() if v is not None]
    fields = dict(ds)
    fields[name] = x
    masks = _evaluate(x, [plans[k][0] for k in served], fields, seg, over_cells, time, device)
    out = OrderedDict((k, None) for k in plans)
    for k, m in zip(served, masks):
        out[k] = m[0] if squeeze else m
    return out


def data_flags(da, ds=None, flags=None, dims="all", freq=None, raise_flags=False, *, name, time: TimeAxis = None, units=None,
               variables=None, device=None) -> OrderedDict:
    """core/dataflags.py:581-746 on numpy arrays.  ``da`` is the variable ``name``, ``ds`` a mapping name -> array of the other
    variables; ``flags`` the reference's dict, a list of such dicts, or None for the defaults of ``name`` (``variables``: the table
    to take them from instead of ``xclim.core.VARIABLES``).  ``dims``: "all" (time and cells), None, "time" or "cells"; with
    ``freq`` the time axis is aggregated per period instead.  Returns an ordered mapping flag name -> bool array (scalar,
    ``(*cells)``, ``(T or P,)`` or ``(T or P, *cells)``), ``None`` where a companion variable is absent."""
    ds = {} if ds is None else ds
    plans = describe(name, flags, ds, units, variables)
    if plans is None:
        if raise_flags:
            raise NotImplementedError(f"Data quality checks do not exist for '{name}' variable.")
        return OrderedDict()
    out = _run(plans, da, name, ds, dims, freq, time, device)
    if raise_flags and any(v is not None and v.any() for v in out.values()):
        raise DataQualityException(out, descriptions={k: v[1] for k, v in plans.items() if v is not None})
    return out


def ecad_compliant(ds, dims="all", raise_flags=False, *, time: TimeAxis = None, units=None, variables=None, device=None):
    """core/dataflags.py:749-819 on a mapping name -> array: the checks of every variable.  With ``raise_flags`` a
    :class:`DataQualityException` when any flag is raised and None otherwise; else the ``ecad_qc_flag`` array (True where no check
    is flagged).  ``units``: a mapping name -> units."""
    flags, texts = OrderedDict(), {}
    for var in ds:
        u = (units or {}).get(var)
        plans = describe(var, None, ds, u, variables)
        if plans is None:
            continue
        for label, m in _run(plans, ds[var], var, ds, dims, None, time, device).items():
            flags[f"{var}_{label}"] = m
            if plans[label] is not None:
                texts[f"{var}_{label}"] = plans[label][1]
    if raise_flags:
        if any(v is not None and v.any() for v in flags.values()):
            raise DataQualityException(flags, descriptions=texts)
        return None
    return ~np.logical_or.reduce([v for v in flags.values() if v is not None])


# ---- the xarray adapter (patch.install) --------------------------------------------------------------------------------------
ADAPTED = ("data_flags",)


def make_adapters(env, originals: dict, xarray=None, VARIABLES=None, registry=None, exc=None, device=None) -> dict:
    """The same-signature replacement of ``data_flags`` of ``xclim.core.dataflags`` (``ecad_compliant`` calls it through the module
    global and is thereby served).  ``xarray``, ``VARIABLES``, ``registry`` (``_REGISTRY``) and ``exc`` (``DataQualityException``) are
    the defining module's own.  ``dims`` is resolved against ``da.dims``; thresholds go through ``env.convert_units_to``; the result
    is an ``xarray.Dataset`` whose flags carry the reference's ``description`` and ``units`` attributes and, where the defining
    module has ``update_xclim_history``, the ``history`` entry it writes.  Chunked fields, a ``dims`` that names only some of the
    non-time dimensions, flags whose registry entry is not one of the reference's own thirteen functions as found at install
    time and everything :class:`NotServed` go to the saved original; no other exception is caught."""
    import inspect

    from .xr_adapter import forwarding_adapter, is_chunked, time_axis_of

    original = originals["data_flags"]
    registry = registry if registry is not None else {}
    own = {n: f for n, f in registry.items() if n in _CHECKS}
    stamp = getattr(inspect.unwrap(original), "__globals__", {}).get("update_xclim_history")

    def with_history(check, value, da, extras, kwargs):
        """The flag as the reference's decorated check returns it: a function of the check's name and signature that returns the
        device result, under the defining module's own ``update_xclim_history``."""
        if stamp is None:
            return value

        def result(*a, **k):
            return value

        result.__name__ = result.__qualname__ = check
        try:
            result.__signature__ = inspect.signature(own[check])
        except (TypeError, ValueError):
            pass
        if extras:
            return stamp(result)(**{da.name: da}, **extras, **(kwargs or {}))
        return stamp(result)(da, **(kwargs or {}))

    def run(p):
        da, ds, flags, dims, freq, raise_flags = (p[k] for k in ("da", "ds", "flags", "dims", "freq", "raise_flags"))
        name = str(da.name)
        if "time" not in da.dims or is_chunked(da):
            raise NotServed("data_flags: a chunked or time-less field")
        cells = tuple(d for d in da.dims if d != "time")
        wanted = set(da.dims) if dims == "all" else set() if dims is None else {dims} if isinstance(dims, str) else set(dims)
        if freq is not None:
            wanted -= {"time"}
        if wanted - set(da.dims) or (wanted & set(cells) and not set(cells) <= wanted):
            raise NotServed("data_flags: dims over a subset of the non-time dimensions")
        over_time, over_cells = "time" in wanted, bool(wanted & set(cells))
        entries = _flag_list(flags, name, VARIABLES)
        if entries is None:
            raise NotServed(f"data_flags: no checks for {name!r}")   # (the original logs or raises as the reference does)
        for check, _ in entries:
            if check not in own or registry.get(check) is not own[check]:
                raise NotServed(f"data_flags: {check} is not one of the reference's own checks")
        a = da.transpose("time", *cells)

        def convert(q, units):
            if isinstance(q, str):
                return float(env.convert_units_to(q, a))
            return convert_threshold(q, units)

        others = {}
        for v in ("tas", "tasmax", "tasmin"):
            if ds is not None and v != name and v in ds:
                if is_chunked(ds[v]) or set(ds[v].dims) != set(a.dims):
                    raise NotServed("data_flags: a companion that is chunked or on other dimensions")
                others[v] = np.ascontiguousarray(ds[v].transpose(*a.dims).values)
        plans = describe(name, [{c: k} for c, k in entries], others, a.attrs.get("units"), None, convert)
        mirror_dims = ("all" if over_cells or not cells else "time") if over_time else ("cells" if over_cells else None)
        got = _run(plans, np.ascontiguousarray(a.values), name, others, mirror_dims, freq, time_axis_of(a), device)
        coords, lead = {}, ()
        if not over_time:
            coords["time"] = a["time"].resample(time=freq).first()["time"] if freq is not None else a["time"]
            lead = ("time",)
        if not over_cells:
            coords.update({d: a[d] for d in cells if d in a.coords})
        data_vars = OrderedDict()
        for label, m in got.items():
            if m is None:
                data_vars[label] = None
                continue
            _, text, has_units, check, kwargs = plans[label]
            attrs = {"description": text, **({"units": ""} if has_units else {})}
            value = env.DataArray(m, dims=lead + (() if over_cells else cells), coords=coords, attrs=attrs, name=label)
            extras = {v: ds[v] for v in _CHECKS[check][1] if v not in ("da", name)}
            data_vars[label] = with_history(check, value, da, extras, kwargs)
        result = xarray.Dataset(data_vars=data_vars)
        if raise_flags and any(v is not None and np.any(v.values) for v in data_vars.values()):
            raise exc(result)
        return result

    return {"data_flags": forwarding_adapter("data_flags", original, run)}
