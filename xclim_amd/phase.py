"""Host mirror of the snow / rain partition and the period indices on it (reference: ``snowfall_approximation`` and
``rain_approximation`` of src/xclim/indices/converters.py:1088-1373; ``liquid_precip_ratio``, ``precip_accumulation``,
``precip_average``, ``rain_on_frozen_ground_days``, ``high_precip_low_temp`` and ``winter_rain_ratio`` of
src/xclim/indices/_multivariate.py:871-1171, :1797-1829; ``first_snowfall``, ``last_snowfall``, ``snowfall_frequency`` and
``snowfall_intensity`` of src/xclim/indices/_threshold.py:1701-1967).  The kernels are in xclim_amd/csrc/phase.hip, their C ABI in
include/xclim_hip_phase.h.

The functions carry the reference's names, parameters and defaults, with thresholds as plain numbers in the units of the data
(``None``: the reference's default, "0 degC" or "1 mm/d" ..., in those units), plus ``time``, ``units`` ("K" / "degC"),
``flux_units``, ``device``, ``keep`` and ``mask_missing``.  Inputs are numpy arrays (or ``(T, C)`` device arrays) with TIME ON AXIS 0
on a daily, gap-free :class:`~xclim_amd.timeaxis.TimeAxis`.  Period results are float64 ``(P, *cells)`` on the periods of
``time.segments(freq)``.  :func:`phase_indices` gives any set of the kernel's outputs from ONE launch of
``xh_precip_phase_period``; every period function here is one such launch and a line of numpy on ``(P, *cells)`` arrays.  The
``prsn`` field of the reference never exists.

ASSUMPTIONS (xarray is neither needed nor used here).  All arithmetic is float64 on the widened fields (a float32
"kg m-2 s-1" field is multiplied by 86400 in float64, where the reference goes on in float32), except that the "binary" method
is a select and its result is bit-identical to the reference's, the threshold rounded to float32 on a float32 field as numpy
does with a Python scalar.  Period sums are added in row order.  The thresholds on snow (``first_snowfall``, ``last_snowfall``,
``snowfall_frequency``, ``snowfall_intensity``) are compared on the daily amount in mm, where the reference compares in the
field's own units for ``snowfall_frequency`` and in mm/day for ``snowfall_intensity``.  ``rain_on_frozen_ground_days`` takes the
reference's window of 7 days only: the reference hard-codes ``rolling(time=8)`` and fails on every other window.  With a land
mask ARRAY the reference's inner calls drop ``clip_temp``; so does this module.

:class:`NotServed` (the adapters forward these to the reference): non-daily or gappy axes, integer fields, array-valued
thresholds, ``rain_on_frozen_ground_days`` with ``window != 7``.
"""

from __future__ import annotations

import types

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import PHASE_DAI_NTAB, PHASE_OUTPUTS, DeviceArray, get_device
from .fields import KELVIN_OFFSET, NotServed, daily_axis
from .fields import per_day as _per_day
from .timeaxis import TimeAxis

__all__ = ["snowfall_approximation", "rain_approximation", "phase_approximation", "precip_accumulation", "precip_average",
           "liquid_precip_ratio", "winter_rain_ratio", "high_precip_low_temp", "rain_on_frozen_ground_days", "first_snowfall",
           "last_snowfall", "snowfall_frequency", "snowfall_intensity", "phase_indices", "partition", "auer_table", "dai_table",
           "season_bytes", "winter_periods", "METHODS", "PHASE_OUTPUTS", "NotServed", "converters", "multivariate", "threshold"]

METHODS = ("binary", "brown", "auer", "dai_annual", "dai_seasonal")
SNOW_HIGH = 1e6 * 86400.0   # snowfall_frequency's "1E6 kg m-2 s-1" as a daily amount in mm

# the coefficients a, b, c, d of Dai (2008) as the reference holds them (converters.py:1200-1227, :1323-1350):
# [phase][land] -> annual (4,), seasonal (4 coefficients, 4 seasons DJF MAM JJA SON); phase 0 = snow, 1 = rain; land 0 = ocean
_DAI_ANNUAL = {(0, 1): (-48.2292, 0.7205, 1.1662, 1.0223), (0, 0): (-47.1472, 0.4049, 1.9280, 1.0203),
               (1, 1): (-47.8337, -0.6866, 1.4913, 1.0420), (1, 0): (-47.3041, -0.4263, 2.5687, 1.0784)}
_DAI_SEASONAL = {
    (0, 1): ((-48.2372, -48.2493, -46.4000, -48.3251), (0.7449, 0.6634, 0.7013, 0.7798), (1.0919, 1.3388, 0.8362, 1.1502),
             (1.0209, 1.0270, 1.0217, 1.0180)),
    (0, 0): ((-47.1823, -47.0035, -47.1472, -46.8494), (0.4003, 0.4090, 0.4049, 0.4162), (2.1735, 1.7372, 1.9280, 2.0474),
             (1.0255, 1.0226, 1.0203, 1.0155)),
    (1, 1): ((-47.5770, -47.9077, -46.8303, -48.0315), (-0.6856, -0.6603, -0.6595, -0.7663), (1.3942, 1.6927, 1.1582, 1.4640),
             (1.0438, 1.0358, 1.1056, 1.0412)),
    (1, 0): ((-47.0262, -47.2828, -47.3041, -47.2107), (-0.4360, -0.4299, -0.4263, -0.4280), (2.8572, 2.3397, 2.5687, 2.7118),
             (1.0731, 1.0800, 1.0784, 1.0911)),
}
_SEASON_OF_MONTH = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0], np.uint8)   # index = month: DJF, MAM, JJA, SON


def auer_table():
    """(nodes, values) of the "auer" method (converters.py:1181-1193): 103 nodes, the clipped degree-6 polynomial over 100, the
    first value forced to 1 and the last two to 0; float64."""
    t = np.concatenate([[-273.15], np.linspace(0, 6, 100, endpoint=False), [6, 1e10]])
    coeffs = [100, 4.6664, -15.038, -1.5089, 2.0399, -0.366, 0.0202]
    v = np.zeros_like(t) + coeffs[6]
    for deg in range(5, -1, -1):   # Horner, as xr.polyval
        v = v * t + coeffs[deg]
    v = np.clip(v, 0, 100) / 100
    v[0] = 1
    v[-2:] = 0
    return t, v


def dai_table(method: str, clip_temp=None) -> np.ndarray:
    """The coefficient table of the two dai methods, float64 ``(2 phases, 2 land, 4 seasons, 6)``: a, b, c, d, fmin, fmax - fmin.
    ``fmin`` / ``fmax`` are the fraction at ``clip_temp`` / ``-clip_temp`` (degC) for snow and the other way round for rain
    (converters.py:1235-1239, :1358-1362), NaN without ``clip_temp``."""
    tab = np.full((2, 2, 4, 6), np.nan)
    for phase in (0, 1):
        for land in (0, 1):
            if method == "dai_annual":
                k = np.repeat(np.array(_DAI_ANNUAL[phase, land], np.float64)[:, None], 4, axis=1)
            else:
                k = np.array(_DAI_SEASONAL[phase, land], np.float64)
            a, b, c, d = k
            tab[phase, land, :, :4] = k.T
            if clip_temp is not None:
                clip = np.float64(clip_temp)
                at_clip, at_minus = a * (np.tanh(b * (clip - c)) - d) / 100, a * (np.tanh(b * (-clip - c)) - d) / 100
                fmin, fmax = (at_clip, at_minus) if phase == 0 else (at_minus, at_clip)
                tab[phase, land, :, 4] = fmin
                tab[phase, land, :, 5] = fmax - fmin
    return tab


def season_bytes(time: TimeAxis) -> np.ndarray:
    """The season of every row as ``time.dt.season`` names it: 0 = DJF, 1 = MAM, 2 = JJA, 3 = SON; uint8 (T)."""
    return _SEASON_OF_MONTH[np.asarray(time.month, np.int64)]


def winter_periods(time: TimeAxis, freq: str) -> np.ndarray:
    """bool (P): the periods of ``time.segments(freq)`` whose label lies in December (``winter_rain_ratio``)."""
    try:
        starts = time.segments(freq)[1]
    except NotImplementedError as e:
        raise NotServed(str(e)) from None
    return np.array([s[1] == 12 for s in starts], bool)


def _scalar(name, v):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise NotServed(f"{name}: only scalar numbers are served, got {type(v).__name__}")
    return float(v)


def _units(units):
    if units not in ("K", "degC"):
        raise ValueError(f"units must be one of ['K', 'degC'], got {units!r}")
    return KELVIN_OFFSET if units == "K" else 0.0


def _round_like(dtype, v):
    """A Python scalar compared with a float32 field is rounded to float32 first (numpy >= 2)."""
    return float(np.float32(v)) if np.dtype(dtype) == np.float32 else float(v)


def partition(method: str = "binary", thresh=None, *, units: str = "K", dtype=np.float64, time: TimeAxis = None, clip_temp=None,
              landmask=True, cell_shape=(), device=None, thresh_degC=None, who: str = "snowfall") -> dict:
    """The partition parameters the two kernels take (``kernels.precip_phase_map`` / ``precip_phase_period``).  ``thresh`` in the
    units of ``tas`` (None: 0 degC); ``thresh_degC``: the same threshold in degC where the caller has converted it itself (else
    ``thresh`` less 273.15 for "K")."""
    if method == "given":
        return {"method": "given", "par": np.zeros(6), "tab": None, "season": None, "land": None}
    if not isinstance(method, str) or method not in METHODS:
        if isinstance(method, str) and method.startswith("dai"):
            raise ValueError(f"Unknown method {method} for {who} approximation.")
        raise ValueError(f"Method {method} not one of 'binary', 'brown', 'auer', 'dai_annual' or 'dai_seasonal'.")
    off = _units(units)
    if method == "brown" and thresh is not None and not np.isscalar(thresh):
        raise ValueError("Non-scalar `thresh` are not allowed with method `brown`.")
    thresh = _scalar("thresh", thresh)
    thresh = off if thresh is None else thresh
    par = np.zeros(6)
    part = {"method": method, "par": par, "tab": None, "season": None, "land": None}
    if method == "binary":
        par[0] = _round_like(dtype, thresh)
    elif method == "brown":
        c = (thresh - off) if thresh_degC is None else float(thresh_degC)
        par[0], par[1] = thresh, (c + 2) + off
    elif method == "auer":
        par[0], par[2] = thresh + (KELVIN_OFFSET - off), KELVIN_OFFSET - off   # convert_units_to(., "K") of thresh and of tas
        part["tab"] = np.concatenate(auer_table())
    else:
        par[3] = off
        is_array = not isinstance(landmask, (bool, np.bool_))
        clip = None if is_array else _scalar("clip_temp", clip_temp)   # (the reference's inner calls drop clip_temp)
        par[4] = clip is not None
        part["tab"] = dai_table(method, clip).reshape(-1)
        assert part["tab"].size == PHASE_DAI_NTAB
        if method == "dai_seasonal":
            if not isinstance(time, TimeAxis):
                raise TypeError("dai_seasonal needs time, the TimeAxis of the rows")
            part["season"] = season_bytes(time)
        if is_array:
            try:
                m = np.broadcast_to(np.asarray(landmask), cell_shape)
            except ValueError:
                raise ValueError(f"landmask: shape {np.shape(landmask)} does not broadcast to the cell shape {tuple(cell_shape)}") from None
            dev = device or get_device()
            part["land"] = dev.to_device(np.ascontiguousarray(m.astype(bool)).reshape(-1).view(np.uint8))
        else:
            par[5] = bool(landmask)
    return part


def _fields(pr, second, names):
    for n, a in zip(names, (pr, second)):
        if not isinstance(a, DeviceArray) and np.asarray(a).dtype.kind in "iub":
            raise NotServed(f"{n}: integer fields are not served")
    a = F.native_set(dict(zip(names, (pr, second))))
    T, cell_shape, C_ = F.shape_of(a)
    return a[names[0]], a[names[1]], T, cell_shape, C_


def phase_approximation(pr, tas, thresh=None, method: str = "binary", clip_temp=None, landmask=True, *, time: TimeAxis = None,
                        units: str = "K", device=None, keep: bool = False, outputs=("snow", "rain")):
    """``(snowfall_approximation, rain_approximation)`` from ONE launch of ``xh_precip_phase_map`` and one read of ``pr`` and
    ``tas``: ``(T, *cells)`` in the units of ``pr``, the dtype of ``pr`` for "binary" and float64 otherwise."""
    a, t, T, cell_shape, C_ = _fields(pr, tas, ("pr", "tas"))
    if time is not None:
        daily_axis(time, T, "phase_approximation")
    part = partition(method, thresh, units=units, dtype=a.dtype, time=time, clip_temp=clip_temp, landmask=landmask,
                     cell_shape=cell_shape, device=device)
    dtype = np.dtype(a.dtype) if method == "binary" else np.dtype(np.float64)
    if T == 0 or C_ == 0:
        res = F.empty_result(dict.fromkeys(outputs, dtype), T, cell_shape, keep, device)
    else:
        dev = device or get_device()
        res = K.precip_phase_map(dev, F.rows_on_device(dev, a, T, C_), F.rows_on_device(dev, t, T, C_), part, outputs)
        res = res if keep else F.host_result(res, T, cell_shape)
    return tuple(res[o] for o in outputs)


def snowfall_approximation(pr, tas, thresh=None, method: str = "binary", clip_temp=None, landmask=True, **kw):
    """converters.py:1088-1251: the solid part of ``pr`` by ``tas``."""
    return phase_approximation(pr, tas, thresh, method, clip_temp, landmask, outputs=("snow",), **kw)[0]


def rain_approximation(pr, tas, thresh=None, method: str = "binary", clip_temp=None, landmask=True, **kw):
    """converters.py:1255-1373: the liquid part of ``pr`` by ``tas`` (for the dai methods its own fraction, not ``pr - snow``)."""
    if isinstance(method, str) and method.startswith("dai") and method not in METHODS:
        raise ValueError(f"Unknown method {method} for rain approximation.")
    return phase_approximation(pr, tas, thresh, method, clip_temp, landmask, outputs=("rain",), **kw)[0]


def phase_indices(pr, tas=None, *, prsn=None, outputs, method: str = "binary", thresh=None, clip_temp=None, landmask=True,
                  freq: str = "YS", snow_low: float = 0.0, snow_high: float = SNOW_HIGH, snow_thresh: float = 1.0, pr_thresh=None,
                  tas_thresh=None, rofg_thresh=None, window: int = 7, time: TimeAxis = None, units: str = "K",
                  flux_units: str = "kg m-2 s-1", per_day=None, device=None, keep: bool = False, mask_missing: bool = False,
                  thresh_degC=None) -> dict:
    """Any set of ``PHASE_OUTPUTS`` per period of ``freq`` from ONE launch: ``{name: (P, *cells) float64}``.  The snow of a day is
    ``prsn`` where it is given and the ``method`` partition of ``pr`` by ``tas`` otherwise.  ``snow_low``, ``snow_high`` and
    ``snow_thresh`` are daily amounts in mm; ``pr_thresh`` / ``tas_thresh`` (high_precip_low_temp: None = 0.4 mm/d, -0.2 degC) and
    ``rofg_thresh`` (rain on frozen ground: None = 1 mm/d) are in the units of the fields.  ``per_day`` overrides the factor of
    ``flux_units`` (1.0: sums in the field's own units)."""
    who = "phase_indices"
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    outputs = list(outputs)
    if not outputs or set(outputs) - set(PHASE_OUTPUTS):
        raise ValueError(f"outputs must be a non-empty subset of {', '.join(PHASE_OUTPUTS)}")
    given = prsn is not None
    if not given and tas is None:
        raise KeyError("prsn or tas must be supplied.")
    a, t, T, cell_shape, C_ = _fields(pr, prsn if given else tas, ("pr", "prsn" if given else "tas"))
    daily_axis(time, T, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    pd = _per_day(flux_units) if per_day is None else float(per_day)
    off = _units(units)
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be an integer of at least 1, got {window!r}")
    if "rofg_days" in outputs and window != 7:
        raise NotServed("rain_on_frozen_ground_days: the reference serves window = 7 only")
    part = partition("given" if given else method, thresh, units=units, dtype=a.dtype, time=time, clip_temp=clip_temp,
                     landmask=landmask, cell_shape=cell_shape, device=device, thresh_degC=thresh_degC)
    limits = {"snow_low": _scalar("low", snow_low), "snow_high": _scalar("high", snow_high), "snow_thresh": _scalar("thresh", snow_thresh)}
    if not given:
        pr_thresh, tas_thresh, rofg_thresh = (_scalar(n, v) for n, v in (("pr_thresh", pr_thresh), ("tas_thresh", tas_thresh),
                                                                         ("thresh", rofg_thresh)))
        limits.update(hplt_pr=_round_like(a.dtype, 0.4 / _per_day(flux_units) if pr_thresh is None else pr_thresh),
                      hplt_tas=_round_like(a.dtype, -0.2 + off if tas_thresh is None else tas_thresh),
                      rofg_pr=_round_like(a.dtype, 1.0 / _per_day(flux_units) if rofg_thresh is None else rofg_thresh),
                      rofg_frz=_round_like(a.dtype, off))
    wanted = list(outputs) + [n for n in ("pr_n", "tas_n") if mask_missing and n not in outputs]
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(outputs, np.float64), P, cell_shape, keep, device)
    dev = device or get_device()
    x = F.rows_on_device(dev, a, T, C_)
    outs = K.precip_phase_period(dev, x, x if t is a else F.rows_on_device(dev, t, T, C_), seg, part, wanted, per_day=pd, doy=time.doy,
                                 window=int(window), **limits)
    if keep:
        return {o: outs[o] for o in outputs}
    res = F.host_result(outs, P, cell_shape)
    if mask_missing:   # MissingAny on both fields: a period whose rows with a value are not all the days of the period
        expected = np.asarray(time.expected_count(freq)).reshape((P,) + (1,) * len(cell_shape))
        bad = (res["pr_n"] != expected) | (res["tas_n"] != expected)
        res = {o: np.where(bad, np.nan, res[o]) for o in outputs}
    return {o: res[o] for o in outputs}


def _phase_of(phase):
    if phase not in (None, "liquid", "solid"):
        raise ValueError(f"phase must be None, 'liquid' or 'solid', got {phase!r}")
    return {None: "pr", "liquid": "liquid", "solid": "solid"}[phase]


def _accumulate(pr, tas, phase, thresh, freq, method, mean, kw):
    name = _phase_of(phase)
    if name != "pr" and tas is None:
        raise ValueError("a phase needs tas")
    outputs = [name + "_sum"] + ([name + "_n"] if mean else [])
    if name == "pr" and tas is None:   # no partition: pr is its own second field, which the "given" method only carries along
        r = phase_indices(pr, prsn=pr, outputs=outputs, freq=freq, **kw)
    else:
        r = phase_indices(pr, tas, outputs=outputs, method=method, thresh=thresh, freq=freq, **kw)
    return r


def precip_accumulation(pr, tas=None, phase=None, thresh=None, freq: str = "YS", *, method: str = "binary", **kw):
    """_multivariate.py:930-990: the total (``phase`` None), liquid or solid precipitation of every period in mm (xclim's
    ``prcptot``, ``liquidprcptot``, ``solidprcptot``).  ``method``: any partition; the reference has "binary" only."""
    return _accumulate(pr, tas, phase, thresh, freq, method, False, kw)[_phase_of(phase) + "_sum"]


def precip_average(pr, tas=None, phase=None, thresh=None, freq: str = "YS", *, method: str = "binary", **kw):
    """_multivariate.py:994-1054: the mean daily amount of every period in mm, NaN for a period without a value."""
    _no_keep(kw)
    r = _accumulate(pr, tas, phase, thresh, freq, method, True, kw)
    name = _phase_of(phase)
    with np.errstate(invalid="ignore", divide="ignore"):
        return r[name + "_sum"] / r[name + "_n"]


def _no_keep(kw):
    if kw.get("keep"):
        raise ValueError("keep=True: this index is finished on the host; phase_indices keeps the kernel's outputs on the device")


def liquid_precip_ratio(pr, prsn=None, tas=None, thresh=None, freq: str = "QS-DEC", *, method: str = "binary", **kw):
    """_multivariate.py:871-926: ``(sum(pr) - sum(prsn)) / sum(pr)`` per period, the sums in the field's own units as in the
    reference; ``prsn`` from ``tas`` by ``method`` where it is not given."""
    _no_keep(kw)
    r = phase_indices(pr, tas, prsn=prsn, outputs=("pr_sum", "solid_sum"), method=method, thresh=thresh, freq=freq, per_day=1.0, **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (r["pr_sum"] - r["solid_sum"]) / r["pr_sum"]


def winter_rain_ratio(*, pr, prsn=None, tas=None, freq: str = "QS-DEC", time: TimeAxis = None, **kw):
    """_multivariate.py:1797-1829: :func:`liquid_precip_ratio` on the periods whose label lies in December
    (:func:`winter_periods`), ``(P_winter, *cells)``."""
    ratio = liquid_precip_ratio(pr, prsn, tas, freq=freq, time=time, **kw)
    return ratio[winter_periods(time, freq)]


def high_precip_low_temp(pr, tas, pr_thresh=None, tas_thresh=None, freq: str = "YS", **kw):
    """_multivariate.py:1128-1171: days with ``pr >= pr_thresh`` and ``tas < tas_thresh`` (None: 0.4 mm/d, -0.2 degC)."""
    return phase_indices(pr, tas, outputs=("hplt_days",), pr_thresh=pr_thresh, tas_thresh=tas_thresh, freq=freq, **kw)["hplt_days"]


def rain_on_frozen_ground_days(pr, tas, thresh=None, window: int = 7, freq: str = "YS", **kw):
    """_multivariate.py:1059-1119: days with ``pr > thresh`` (None: 1 mm/d) and ``tas`` above 0 degC after ``window`` days at or
    below it (a NaN ``tas`` counts as frozen, as in the reference)."""
    return phase_indices(pr, tas, outputs=("rofg_days",), rofg_thresh=thresh, window=window, freq=freq, **kw)["rofg_days"]


def _snow(prsn, pr, tas, outputs, freq, kw, **limits):
    """The snowfall indices on ``prsn``, or on the ``method`` partition of ``pr`` by ``tas`` (``phase_thresh``: its freezing point
    in the units of ``tas``; the indices' own ``thresh`` is the snow amount in mm)."""
    kw = dict(kw)
    phase_thresh = kw.pop("phase_thresh", None)
    if prsn is not None:
        return phase_indices(prsn, prsn=prsn, outputs=outputs, freq=freq, **limits, **kw)
    if pr is None or tas is None:
        raise KeyError("prsn, or pr and tas, must be supplied.")
    return phase_indices(pr, tas, outputs=outputs, thresh=phase_thresh, freq=freq, **limits, **kw)


def first_snowfall(prsn=None, thresh: float = 1.0, freq: str = "YS-JUL", *, pr=None, tas=None, **kw):
    """_threshold.py:1701-1758: the day of year of the first day with at least ``thresh`` mm of snow, NaN without one."""
    return _snow(prsn, pr, tas, ("first_snow",), freq, kw, snow_thresh=thresh)["first_snow"]


def last_snowfall(prsn=None, thresh: float = 1.0, freq: str = "YS-JUL", *, pr=None, tas=None, **kw):
    """_threshold.py:1762-1819: the day of year of the last day with at least ``thresh`` mm of snow, NaN without one."""
    return _snow(prsn, pr, tas, ("last_snow",), freq, kw, snow_thresh=thresh)["last_snow"]


def snowfall_frequency(prsn=None, thresh: float = 1.0, freq: str = "YS-JUL", *, pr=None, tas=None, **kw):
    """_threshold.py:1864-1912: the percentage of the days with a value that have at least ``thresh`` mm of snow."""
    _no_keep(kw)
    r = _snow(prsn, pr, tas, ("snow_days", "solid_n"), freq, kw, snow_low=thresh, snow_high=SNOW_HIGH)
    with np.errstate(invalid="ignore", divide="ignore"):
        return r["snow_days"] / r["solid_n"] * 100


def snowfall_intensity(prsn=None, thresh: float = 1.0, freq: str = "YS-JUL", *, pr=None, tas=None, **kw):
    """_threshold.py:1916-1967: the mean snow amount in mm/day of the days with at least ``thresh`` mm, 0 without one."""
    _no_keep(kw)
    r = _snow(prsn, pr, tas, ("snow_sum_over", "snow_n_over"), freq, kw, snow_thresh=thresh)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(r["snow_n_over"] > 0, r["snow_sum_over"] / r["snow_n_over"], 0.0)


# ---- the xarray adapters (patch.install) -----------------------------------------------------------------------------
# The replaced functions are defined in three modules of the reference and patch.install_mirror wants one defining module per
# mirror: three namespaces, each with its own ADAPTED and make_adapters.  make_adapters holds runners only.
def _adapter_tools(env):
    from .fields import FLUX_SPELLINGS, T_SPELLINGS
    from .xr_adapter import on_period_starts, served_fields, threshold_number, units_keyword

    DA = env.DataArray

    def temperature(p, name, tas_units):
        """A temperature threshold in the units of tas, and in degC."""
        return threshold_number(env, p[name], tas_units), threshold_number(env, p[name], "degC")

    def two(p, names):
        a, v, time = served_fields(DA, p, names)
        return a, v, time, units_keyword(p[names[0]], FLUX_SPELLINGS, names[0])

    return types.SimpleNamespace(DA=DA, env=env, temperature=temperature, two=two, T_SPELLINGS=T_SPELLINGS, FLUX_SPELLINGS=FLUX_SPELLINGS,
                                 units_keyword=units_keyword, threshold_number=threshold_number, on_period_starts=on_period_starts,
                                 served_fields=served_fields)


def _wrap_like(DA, a, values, attrs):
    return DA(values, dims=a.dims, coords=a.coords, attrs=attrs)


def _converters_adapters(env, originals: dict, device=None) -> dict:
    """``snowfall_approximation`` and ``rain_approximation`` of ``xclim.indices.converters``: one launch of ``xh_precip_phase_map``;
    the result has the dimensions, coordinates and units of ``pr``."""
    from .xr_adapter import forwarding_adapter

    t = _adapter_tools(env)

    def runner(fn):
        def run(p):
            a, v, time, _ = t.two(p, ("pr", "tas"))
            units = t.units_keyword(p["tas"], t.T_SPELLINGS, "tas")
            method = p["method"]
            thresh = None
            if method in ("binary", "brown", "auer"):
                if method == "brown" and not np.isscalar(p["thresh"]):
                    raise ValueError("Non-scalar `thresh` are not allowed with method `brown`.")
                thresh = t.threshold_number(env, p["thresh"], units)
            clip = None if p["clip_temp"] is None else t.threshold_number(env, p["clip_temp"], "degC")
            land = p["landmask"]
            if not isinstance(land, (bool, np.bool_)):   # a mask on the cell dimensions of the field, in their order
                if not isinstance(land, t.DA) or tuple(land.dims) != tuple(a.dims[1:]):
                    raise NotServed("landmask: not a DataArray on the cell dimensions of the field")
                land = np.asarray(land.values).astype(bool)
            out = fn(v["pr"], v["tas"], thresh, method, clip, land, time=time, units=units, device=device)
            return _wrap_like(t.DA, a, out, {"units": p["pr"].attrs["units"]})
        return run

    runners = {"snowfall_approximation": runner(snowfall_approximation), "rain_approximation": runner(rain_approximation)}
    return {n: forwarding_adapter(n, originals[n], runners[n]) for n in converters.ADAPTED}


def _multivariate_adapters(env, originals: dict, device=None) -> dict:
    """The six period functions of ``xclim.indices._multivariate``: one launch of ``xh_precip_phase_period`` each."""
    from .xr_adapter import forwarding_adapter

    t = _adapter_tools(env)

    def second(p):
        """(names of the two fields, is prsn given)"""
        if p.get("prsn") is not None:
            return ("pr", "prsn"), True
        if p.get("tas") is None:
            raise KeyError("prsn or tas must be supplied.")
        return ("pr", "tas"), False

    def ratio_values(p):
        names, given = second(p)
        a, v, time, flux = t.two(p, names)
        kw = {"time": time, "flux_units": flux, "device": device}
        if given:
            return a, time, liquid_precip_ratio(v["pr"], prsn=v["prsn"], freq=p["freq"], **kw)
        units = t.units_keyword(p["tas"], t.T_SPELLINGS, "tas")
        thresh = t.threshold_number(env, p.get("thresh", "0 degC"), units)
        return a, time, liquid_precip_ratio(v["pr"], tas=v["tas"], thresh=thresh, freq=p["freq"], units=units, **kw)

    def _ratio(p):
        a, _, out = ratio_values(p)
        return t.on_period_starts(t.DA, a, out, p["freq"], {"units": ""})

    def _winter(p):
        a, time, out = ratio_values(p)
        whole = t.on_period_starts(t.DA, a, out, p["freq"], {"units": ""})
        return whole.isel(time=np.flatnonzero(winter_periods(time, p["freq"])))

    def totals(fn):
        def run(p):
            if p["phase"] not in (None, "liquid", "solid"):
                raise NotServed("phase")
            names = ("pr",) if p["tas"] is None else ("pr", "tas")
            if p["phase"] is not None and p["tas"] is None:
                raise NotServed("a phase without tas")
            a, v, time = t.served_fields(t.DA, p, names)
            flux = t.units_keyword(p["pr"], t.FLUX_SPELLINGS, "pr")
            kw = {"time": time, "flux_units": flux, "device": device}
            if p["tas"] is not None:
                kw["units"] = t.units_keyword(p["tas"], t.T_SPELLINGS, "tas")
                kw["thresh"] = t.threshold_number(env, p["thresh"], kw["units"])
            out = fn(v["pr"], v.get("tas"), p["phase"], freq=p["freq"], **kw)
            return t.on_period_starts(t.DA, a, out, p["freq"], {"units": "mm"})   # rate2amount of a daily flux
        return run

    def _hplt(p):
        a, v, time, flux = t.two(p, ("pr", "tas"))
        units = t.units_keyword(p["tas"], t.T_SPELLINGS, "tas")
        pr_thresh = float(env.convert_units_to(p["pr_thresh"], p["pr"], context="hydro")) if isinstance(p["pr_thresh"], str) else _scalar("pr_thresh", p["pr_thresh"])
        out = high_precip_low_temp(v["pr"], v["tas"], pr_thresh, t.threshold_number(env, p["tas_thresh"], units), p["freq"], time=time,
                                   units=units, flux_units=flux, device=device)
        return env.to_agg_units(t.on_period_starts(t.DA, a, out, p["freq"], {}), p["pr"], "count")

    def _rofg(p):
        if p["window"] != 7:
            raise NotServed("rain_on_frozen_ground_days: the reference serves window = 7 only")
        a, v, time, flux = t.two(p, ("pr", "tas"))
        units = t.units_keyword(p["tas"], t.T_SPELLINGS, "tas")
        thresh = float(env.convert_units_to(p["thresh"], p["pr"], context="hydro")) if isinstance(p["thresh"], str) else _scalar("thresh", p["thresh"])
        out = rain_on_frozen_ground_days(v["pr"], v["tas"], thresh, 7, p["freq"], time=time, units=units, flux_units=flux, device=device)
        return env.to_agg_units(t.on_period_starts(t.DA, a, out, p["freq"], {}), p["tas"], "count")

    runners = {"liquid_precip_ratio": _ratio, "winter_rain_ratio": _winter, "precip_accumulation": totals(precip_accumulation),
               "precip_average": totals(precip_average), "high_precip_low_temp": _hplt, "rain_on_frozen_ground_days": _rofg}
    return {n: forwarding_adapter(n, originals[n], runners[n]) for n in multivariate.ADAPTED}


def _threshold_adapters(env, originals: dict, device=None) -> dict:
    """The four snowfall indices of ``xclim.indices._threshold`` on ``prsn``: one launch of ``xh_precip_phase_period`` each."""
    from .xr_adapter import forwarding_adapter

    t = _adapter_tools(env)

    def snow(fn, finish):
        def run(p):
            a, v, time = t.served_fields(t.DA, p, ("prsn",))
            flux = t.units_keyword(p["prsn"], t.FLUX_SPELLINGS, "prsn")
            out = fn(v["prsn"], t.threshold_number(env, p["thresh"], "mm/d"), p["freq"], time=time, flux_units=flux, device=device)
            return finish(t.on_period_starts(t.DA, a, out, p["freq"], {}), p["prsn"], time)
        return run

    def date(out, prsn, time):
        return out.assign_attrs(units="", is_dayofyear=np.int32(1), calendar=time.calendar)

    def freq_(out, prsn, time):
        return env.to_agg_units(out, prsn, "count").assign_attrs(units="%")

    def intensity(out, prsn, time):
        return out.assign_attrs(units="mm/d")

    runners = {"first_snowfall": snow(first_snowfall, date), "last_snowfall": snow(last_snowfall, date),
               "snowfall_frequency": snow(snowfall_frequency, freq_), "snowfall_intensity": snow(snowfall_intensity, intensity)}
    return {n: forwarding_adapter(n, originals[n], runners[n]) for n in threshold.ADAPTED}


converters = types.SimpleNamespace(ADAPTED=("snowfall_approximation", "rain_approximation"), make_adapters=_converters_adapters)
multivariate = types.SimpleNamespace(ADAPTED=("liquid_precip_ratio", "precip_accumulation", "precip_average", "rain_on_frozen_ground_days",
                                              "high_precip_low_temp", "winter_rain_ratio"), make_adapters=_multivariate_adapters)
threshold = types.SimpleNamespace(ADAPTED=("first_snowfall", "last_snowfall", "snowfall_frequency", "snowfall_intensity"),
                                  make_adapters=_threshold_adapters)
