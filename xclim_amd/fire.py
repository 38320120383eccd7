"""Host mirror of the Canadian Forest Fire Weather Index System (reference: src/xclim/indices/fire/_cffwis.py).

The whole daily iteration of ``_fire_weather_calc`` (:655-880) — the three moisture codes, ISI / BUI / FWI / DSR, the fire
season (computed or given), overwintering of the drought code and the dry starts — is ONE launch of ``xh_fire_weather``
(xclim_amd/csrc/fire.hip): one lane per cell carries the state down the time-major field.

Inputs are numpy arrays (or float32 device arrays) with TIME ON AXIS 0, ``(T, *cells)``, already in the units of the FWI
equations: tas [degC], pr [mm/day], hurs [%], sfcWind [km/h], snd [m].  Per-cell inputs (lat, dc0, dmc0, ffmc0, winter_pr)
have the cell shape (they are broadcast to it).  The months come from a :class:`~xclim_amd.timeaxis.TimeAxis` (``time=``).
Outputs are numpy ``(T, *cells)`` float32 (the season mask bool, ``winter_pr`` ``(*cells)``), or device arrays with
``keep=True``.  No CPU fallback: a form the kernel does not serve (``dry_start="GFWED"`` with ``snd``, GFWED season
windows over 7 days) raises NotImplementedError; float64 fields follow ``XCLIM_AMD_FLOAT64`` (no float64 twin).
"""

from __future__ import annotations

from collections import namedtuple
from collections.abc import Sequence

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import DeviceArray, get_device, handle_float64
from .calendar import _flatten
from .timeaxis import TimeAxis

__all__ = ["default_params", "fire_weather_ufunc", "cffwis_indices", "drought_code", "duff_moisture_code", "fire_season",
           "overwintering_drought_code", "GFWED_MAX_WINDOW"]

# _cffwis.py:162-179; parameters with units in the reference carry them as (value, units)
default_params: dict = {
    "temp_start_thresh": (12.0, "degC"),
    "temp_end_thresh": (5.0, "degC"),
    "snow_thresh": (0.01, "m"),
    "temp_condition_days": 3,
    "snow_condition_days": 3,
    "carry_over_fraction": 0.75,
    "wetting_efficiency_fraction": 0.75,
    "dc_start": 15,
    "dmc_start": 6,
    "ffmc_start": 85,
    "prec_thresh": (1.0, "mm/d"),
    "dc_dry_factor": 5,
    "dmc_dry_factor": 2,
    "snow_cover_days": 60,
    "snow_min_cover_frac": 0.75,
    "snow_min_mean_depth": (0.1, "m"),
}

GFWED_MAX_WINDOW = 7  # the kernel's GFWED season means: numpy sums shorter windows in order
_ORDER = ["DC", "DMC", "FFMC", "ISI", "BUI", "FWI", "DSR"]

CFFWISIndices = namedtuple("CFFWISIndices", ["DC", "DMC", "FFMC", "ISI", "BUI", "FWI"])


def _cells(a, cell_shape, dev, dtype, name):
    """A per-cell input broadcast to the cell shape, flattened and uploaded (None stays None)."""
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        if a.dtype != np.dtype(dtype) or int(np.prod(a.shape, dtype=np.int64)) != int(np.prod(cell_shape, dtype=np.int64)):
            raise TypeError(f"{name}: device array must be {np.dtype(dtype).name} with the cell shape {tuple(cell_shape)}")
        return a.reshape(-1)
    arr = np.asarray(a)
    if dtype == np.float32:
        handle_float64(arr, name)
    return dev.to_device(np.ascontiguousarray(np.broadcast_to(arr, cell_shape), dtype=dtype).reshape(-1))


def _mask_u8(season_mask, dev, T, C_):
    if isinstance(season_mask, DeviceArray):
        if season_mask.dtype != np.uint8:
            raise TypeError("season_mask: a device mask must be uint8 (0 / 1)")
        return season_mask.reshape(T, C_)
    m = np.asarray(season_mask)
    m16 = m.astype(np.int16)  # what _fire_weather_calc does with the mask (:720)
    if m16.size and (m16.min() < 0 or m16.max() > 1):
        raise ValueError("season_mask must be boolean (0 / 1)")
    return dev.to_device(np.ascontiguousarray(m16.reshape(T, C_), dtype=np.uint8))


def _merged_params(params: dict) -> dict:
    kw = {k: v[0] if isinstance(v, tuple) else v for k, v in default_params.items()}
    kw.update(params)
    return kw


def fire_weather_ufunc(  # noqa: C901
    *,
    tas,
    pr,
    hurs=None,
    sfcWind=None,
    snd=None,
    lat=None,
    dc0=None,
    dmc0=None,
    ffmc0=None,
    winter_pr=None,
    season_mask=None,
    start_dates=None,  # noqa: ARG001  (unused, as in the reference)
    indexes: Sequence[str] | None = None,
    season_method: str | None = None,
    overwintering: bool = False,
    dry_start: str | None = None,
    initial_start_up: bool = True,
    time: TimeAxis | None = None,
    device=None,
    keep: bool = False,
    **params,
) -> dict:
    """_cffwis.py:882-1051: the fire weather indexes of ``indexes`` (closed over their dependencies), plus "season_mask"
    when a ``season_method`` computes it and "winter_pr" with ``overwintering``.  Same arguments, defaults and errors as
    the reference; ``time`` gives the months (needed for DC and DMC)."""
    idx = set(indexes or _ORDER)
    if "DSR" in idx:
        idx.update({"FWI"})
    if "FWI" in idx:
        idx.update({"ISI", "BUI"})
    if "BUI" in idx:
        idx.update({"DC", "DMC"})
    if "ISI" in idx:
        idx.update({"FFMC"})
    unknown = idx - set(_ORDER)
    if unknown:
        raise ValueError(f"unknown fire weather indexes {sorted(unknown)}")
    idx = sorted(idx, key=_ORDER.index)
    month = time.month if time is not None else None
    needed = ((tas, "tas", ["DC", "DMC", "FFMC", "WF93", "LA08"]), (pr, "pr", ["DC", "DMC", "FFMC"]),
              (hurs, "hurs", ["DMC", "FFMC"]), (sfcWind, "sfcWind", ["FFMC"]), (snd, "snd", ["LA08"]),
              (month, "month", ["DC", "DMC"]), (lat, "lat", ["DC", "DMC"]))
    for arg, name, usedby in needed:
        if any(i in idx + [season_method] for i in usedby) and arg is None:
            raise TypeError(f"Missing input argument {name} for index combination {idx} "
                            f"with fire season method '{season_method}'.")
    if snd is not None and dry_start == "GFWED":
        dry_start = "GFWED+SNOW"
    elif dry_start not in [None, "CFS", "GFWED"]:
        raise ValueError("'dry_start' must be one of None, 'CFS' or 'GFWED'.")
    if season_mask is not None:
        season_method = "mask"
    elif season_method not in (None, "WF93", "LA08", "GFWED"):
        raise ValueError("`method` must be one of 'WF93', 'LA08' or 'GFWED'.")
    if season_method == "GFWED" and snd is None:
        raise TypeError(f"Missing input argument snd for index combination {idx} with fire season method 'GFWED'.")
    if overwintering and season_method is None:
        raise ValueError("If overwintering is activated, either `season_method` or `season_mask` must be given.")
    kw = _merged_params(params)
    if dry_start == "GFWED+SNOW":
        raise NotImplementedError("dry_start='GFWED' with snow depth (the 60-day snow-cover start) is not implemented on the GPU")
    if season_method == "GFWED" and max(kw["temp_condition_days"], kw["snow_condition_days"]) > GFWED_MAX_WINDOW:
        raise NotImplementedError(f"GFWED fire season windows over {GFWED_MAX_WINDOW} days are not implemented on the GPU")

    dev = device or get_device()
    fields, cell_shape, T = {}, None, None
    reads = {"tas": bool(set(idx) & {"DC", "DMC", "FFMC"}) or season_method in ("WF93", "LA08", "GFWED"),
             "pr": bool(set(idx) & {"DC", "DMC", "FFMC"}) or dry_start is not None,
             "hurs": bool(set(idx) & {"DMC", "FFMC"}), "sfcWind": bool(set(idx) & {"FFMC", "ISI"}),
             "snd": season_method in ("LA08", "GFWED")}
    for name, arr in (("tas", tas), ("pr", pr), ("hurs", hurs), ("sfcWind", sfcWind), ("snd", snd)):
        if arr is None or not reads[name]:
            continue
        d, cs = _flatten(arr, dev)
        if cell_shape is None:
            cell_shape, T = tuple(cs), d.shape[0]
        elif tuple(cs) != cell_shape or d.shape[0] != T:
            raise ValueError(f"{name}: shape {(d.shape[0],) + tuple(cs)} differs from tas {(T,) + cell_shape}")
        fields[name] = d
    if cell_shape is None:
        shp = tas.shape if tas is not None else pr.shape
        T, cell_shape = int(shp[0]), tuple(shp[1:])
    C_ = int(np.prod(cell_shape, dtype=np.int64))
    if month is not None:
        month = np.asarray(month)
        if month.shape != (T,):
            raise ValueError(f"time has {month.shape[0]} steps, the fields {T}")
    else:
        month = np.ones(T, dtype=np.int32)
    d_lat = _cells(lat, cell_shape, dev, np.float64, "lat") if set(idx) & {"DC", "DMC"} else None
    starts = {"dc0": _cells(dc0, cell_shape, dev, np.float32, "dc0"), "dmc0": _cells(dmc0, cell_shape, dev, np.float32, "dmc0"),
              "ffmc0": _cells(ffmc0, cell_shape, dev, np.float32, "ffmc0")}
    if overwintering:
        starts["winter_pr"] = _cells(winter_pr if winter_pr is not None else np.zeros((), np.float32), cell_shape, dev,
                                     np.float32, "winter_pr")
    d_mask = _mask_u8(season_mask, dev, T, C_) if season_method == "mask" else None
    want_mask = season_method not in (None, "mask")
    outs = K.fire_weather(dev, fields, month, d_lat, starts, idx, kw, season_method=season_method, season_mask=d_mask,
                          overwintering=overwintering, dry_start=dry_start, initial_start_up=initial_start_up,
                          want_mask=want_mask, want_winter_pr=bool(overwintering))
    if keep:
        return outs
    res = F.host_result({n: d for n, d in outs.items() if n != "winter_pr"}, T, cell_shape)
    if "season_mask" in res:
        res["season_mask"] = res["season_mask"].astype(bool)
    if "winter_pr" in outs:
        res["winter_pr"] = outs["winter_pr"].get().reshape(cell_shape)
    return res


def _convert_parameters(params: dict, funcname: str = "fire weather indices") -> dict:
    """_cffwis.py:1107-1120 without units: the inputs here are already in the FWI units."""
    for param in params:
        if param not in default_params:
            raise ValueError(f"{param} is not a valid parameter for {funcname}. "
                             "See the docstring of the function and the list in xc.indices.fire.default_params.")
    return params


def cffwis_indices(tas, pr, sfcWind, hurs, lat, snd=None, ffmc0=None, dmc0=None, dc0=None, season_mask=None,
                   season_method=None, overwintering=False, dry_start=None, initial_start_up=True, *, time: TimeAxis,
                   device=None, keep=False, **params) -> CFFWISIndices:
    """_cffwis.py:1134-1265: DC, DMC, FFMC, ISI, BUI and FWI as a named tuple."""
    out = fire_weather_ufunc(tas=tas, pr=pr, hurs=hurs, sfcWind=sfcWind, lat=lat, dc0=dc0, dmc0=dmc0, ffmc0=ffmc0, snd=snd,
                             indexes=["DC", "DMC", "FFMC", "ISI", "BUI", "FWI"], season_mask=season_mask,
                             season_method=season_method, overwintering=overwintering, dry_start=dry_start,
                             initial_start_up=initial_start_up, time=time, device=device, keep=keep,
                             **_convert_parameters(params))
    return CFFWISIndices(out["DC"], out["DMC"], out["FFMC"], out["ISI"], out["BUI"], out["FWI"])


def drought_code(tas, pr, lat, snd=None, dc0=None, season_mask=None, season_method=None, overwintering=False, dry_start=None,
                 initial_start_up=True, *, time: TimeAxis, device=None, keep=False, **params):
    """_cffwis.py:1268-1362."""
    out = fire_weather_ufunc(tas=tas, pr=pr, lat=lat, dc0=dc0, snd=snd, indexes=["DC"], season_mask=season_mask,
                             season_method=season_method, overwintering=overwintering, dry_start=dry_start,
                             initial_start_up=initial_start_up, time=time, device=device, keep=keep,
                             **_convert_parameters(params, "drought_code"))
    return out["DC"]


def duff_moisture_code(tas, pr, hurs, lat, snd=None, dmc0=None, season_mask=None, season_method=None, dry_start=None,
                       initial_start_up=True, *, time: TimeAxis, device=None, keep=False, **params):
    """_cffwis.py:1365-1455."""
    out = fire_weather_ufunc(tas=tas, pr=pr, hurs=hurs, lat=lat, dmc0=dmc0, snd=snd, indexes=["DMC"], season_mask=season_mask,
                             season_method=season_method, dry_start=dry_start, initial_start_up=initial_start_up, time=time,
                             device=device, keep=keep, **_convert_parameters(params, "duff_moisture_code"))
    return out["DMC"]


def fire_season(tas, snd=None, method: str = "WF93", freq: str | None = None, temp_start_thresh=12.0, temp_end_thresh=5.0,
                temp_condition_days: int = 3, snow_condition_days: int = 3, snow_thresh=0.01, *, time: TimeAxis | None = None,
                device=None, keep=False):
    """_cffwis.py:1458-1546 (and _fire_season, :570-652): the boolean fire season mask, ``(T, *cells)``.  With ``freq``
    only the longest run of every period is kept (``rl.keep_longest_run`` per ``resample(time=freq)``, on the device)."""
    if not all(np.isscalar(v) for v in [temp_start_thresh, temp_end_thresh, snow_thresh]):
        raise ValueError("Thresholds must be scalar.")
    if method not in ("WF93", "LA08", "GFWED"):
        raise ValueError("`method` must be one of 'WF93', 'LA08' or 'GFWED'.")
    if method != "WF93" and snd is None:
        raise TypeError(f"fire_season: method '{method}' needs snd")
    if method == "GFWED" and max(temp_condition_days, snow_condition_days) > GFWED_MAX_WINDOW:
        raise NotImplementedError(f"GFWED fire season windows over {GFWED_MAX_WINDOW} days are not implemented on the GPU")
    if freq is not None and time is None:
        raise TypeError("fire_season: freq needs time=")
    dev = device or get_device()
    d_tas, cell_shape = _flatten(tas, dev)
    fields = {"tas": d_tas}
    if method != "WF93":
        d_snd, cs = _flatten(snd, dev)
        if tuple(cs) != tuple(cell_shape) or d_snd.shape != d_tas.shape:
            raise ValueError("fire_season: tas and snd must have one shape")
        fields["snd"] = d_snd
    T = d_tas.shape[0]
    kw = _merged_params({"temp_start_thresh": float(temp_start_thresh), "temp_end_thresh": float(temp_end_thresh),
                         "snow_thresh": float(snow_thresh), "temp_condition_days": int(temp_condition_days),
                         "snow_condition_days": int(snow_condition_days)})
    outs = K.fire_weather(dev, fields, np.ones(T, np.int32), None, {}, [], kw, season_method=method, want_mask=True)
    mask = outs["season_mask"]
    if freq is not None:
        # season_mask.resample(time=freq).map(rl.keep_longest_run): every period on its own (runs do not cross a period
        # boundary), so each period is one keep_longest_run over its own rows
        seg, _ = time.segments(freq)
        m32 = K.mask_to_f32(dev, mask)
        C_ = m32.shape[1]
        mf = dev.empty((T, C_), np.float32)
        for t0, t1 in zip(seg[:-1], seg[1:]):
            if t1 > t0:
                rows = dev.wrap(m32.ptr + int(t0) * C_ * 4, (int(t1 - t0), C_), np.float32)
                part = K.keep_longest_run(dev, rows, np.array([0, t1 - t0], dtype=np.int64))
                dev.copy_d2d(mf.ptr + int(t0) * C_ * 4, part.ptr, part.nbytes)
        if keep:
            return mf
        return mf.get().reshape((T,) + tuple(cell_shape)).astype(bool)
    if keep:
        return mask
    return mask.get().reshape((T,) + tuple(cell_shape)).astype(bool)


def overwintering_drought_code(last_dc, winter_pr, carry_over_fraction=default_params["carry_over_fraction"],
                               wetting_efficiency_fraction=default_params["wetting_efficiency_fraction"],
                               min_dc=default_params["dc_start"], *, device=None, keep=False):
    """_cffwis.py:1054-1104 on arrays (winter_pr in mm); scalar parameters; float32 result of the broadcast shape."""
    if not all(np.isscalar(v) for v in (carry_over_fraction, wetting_efficiency_fraction, min_dc)):
        raise TypeError("overwintering_drought_code: the parameters must be scalars here")
    dev = device or get_device()
    a, b = np.asarray(last_dc), np.asarray(winter_pr)
    handle_float64(a, "last_dc")
    handle_float64(b, "winter_pr")
    a, b = np.broadcast_arrays(a, b)
    shape = a.shape
    da = dev.to_device(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    db = dev.to_device(np.ascontiguousarray(b, dtype=np.float32).reshape(-1))
    out = K.overwintering_dc(dev, da, db, carry_over_fraction, wetting_efficiency_fraction, min_dc)
    if keep:
        return out.reshape(shape) if shape else out
    return out.get().reshape(shape)


# ---- the adapter callees (patch.install): the reference's numpy iterators, time LAST ---------------------------------
_Forward = F.Forward


def _tfirst(a, shape, name):
    """(…, T) numpy array -> (T, C) float32 device upload; the transposed view xarray hands over is uploaded without a copy."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.shape != shape or a.dtype != np.float32:
        raise _Forward(name)
    return F.time_first(a)


def _cells_f32(a, cell_shape, name):
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise _Forward(name)
    try:
        return np.ascontiguousarray(np.broadcast_to(a, cell_shape)).reshape(-1)
    except ValueError:
        raise _Forward(name) from None


def fire_weather_calc(tas, pr, rh, ws, snd, mth, lat, season_mask, dc0, dmc0, ffmc0, winter_pr, *, device=None, **params):
    """Drop-in for ``_fire_weather_calc`` (_cffwis.py:655-880) on the numpy arrays ``xr.apply_ufunc`` passes (time LAST).
    Returns what the reference returns: one array, or the tuple of ``params["outputs"]``, time last (views).  Raises
    ``_Forward`` for what the device path does not take (float64 fields, GFWED+SNOW, GFWED windows over 7 days, inputs
    broadcast against the cells)."""
    outputs = list(params["outputs"])
    season_method = params.get("season_method")
    dry_start = params.get("dry_start")
    if dry_start not in FIRE_DRY_SERVED or season_method not in (None, "mask", "WF93", "LA08", "GFWED"):
        raise _Forward("dry_start / season_method")
    if season_method == "GFWED" and max(params["temp_condition_days"], params["snow_condition_days"]) > GFWED_MAX_WINDOW:
        raise _Forward("GFWED window")
    tas = np.asarray(tas)
    shape = tas.shape
    if tas.ndim < 1:
        raise _Forward("tas")
    T, cell_shape = shape[-1], shape[:-1]
    idx = [o for o in outputs if o in _ORDER]
    fields = {"tas": _tfirst(tas, shape, "tas"), "pr": _tfirst(pr, shape, "pr"), "hurs": _tfirst(rh, shape, "hurs"),
              "sfcWind": _tfirst(ws, shape, "sfcWind"),
              "snd": _tfirst(snd, shape, "snd") if season_method in ("LA08", "GFWED") else None}
    month = np.ones(T, np.int32)
    if mth is not None:
        m = np.asarray(mth)
        if m.size != T or m.shape[-1] != T:
            raise _Forward("month")  # (a month per cell and day: not a TimeAxis-shaped input)
        month = m.reshape(T).astype(np.int32)
    lat_c = None
    if lat is not None and set(idx) & {"DC", "DMC"}:
        try:
            lat_c = F.per_cell(lat, cell_shape, "lat")
        except ValueError:
            raise _Forward("lat") from None
    starts = {"dc0": _cells_f32(dc0, cell_shape, "dc0"), "dmc0": _cells_f32(dmc0, cell_shape, "dmc0"),
              "ffmc0": _cells_f32(ffmc0, cell_shape, "ffmc0")}
    if params.get("overwintering"):
        starts["winter_pr"] = _cells_f32(winter_pr, cell_shape, "winter_pr")
    mask = None
    if season_method == "mask":
        m = np.asarray(season_mask)
        if m.shape != shape:
            raise _Forward("season_mask")
        m16 = m.astype(np.int16)
        if m16.size and (m16.min() < 0 or m16.max() > 1):
            raise _Forward("season_mask values")
        mask = F.time_first(m16.astype(np.uint8))
    dev = device or get_device()
    d = {k: dev.to_device(v) for k, v in fields.items() if v is not None}
    ds = {k: (dev.to_device(v) if v is not None else None) for k, v in starts.items()}
    outs = K.fire_weather(dev, d, month, dev.to_device(lat_c) if lat_c is not None else None, ds, idx, params,
                          season_method=season_method, season_mask=dev.to_device(mask) if mask is not None else None,
                          overwintering=bool(params.get("overwintering")), dry_start=dry_start,
                          initial_start_up=params.get("initial_start_up", True),
                          want_mask="season_mask" in outputs and season_method not in (None, "mask"),
                          want_winter_pr="winter_pr" in outputs and bool(params.get("overwintering")))
    res = []
    for name in outputs:
        if name == "season_mask":
            if season_method is None:
                res.append(np.full(shape, True))
            elif season_method == "mask":
                res.append(season_mask)
            else:
                res.append(F.time_last(outs[name].get().view(bool), cell_shape))
        elif name == "winter_pr":
            res.append(outs[name].get().reshape(cell_shape) if name in outs else np.asarray(winter_pr).copy())
        else:
            res.append(F.time_last(outs[name].get(), cell_shape))
    return res[0] if len(res) == 1 else tuple(res)


FIRE_DRY_SERVED = (None, "CFS", "GFWED")


def fire_season_np(tas, snd=None, method="WF93", temp_start_thresh=12.0, temp_end_thresh=5.0, temp_condition_days=3,
                   snow_condition_days=3, snow_thresh=0.01, *, device=None):
    """Drop-in for ``_fire_season`` (_cffwis.py:570-652): (…, T) float32 arrays -> (…, T) bool, time last.  Raises
    ``_Forward`` for what the device path does not take."""
    if method not in ("WF93", "LA08", "GFWED"):
        raise _Forward("method")
    if method == "GFWED" and max(temp_condition_days, snow_condition_days) > GFWED_MAX_WINDOW:
        raise _Forward("GFWED window")
    if not all(np.isscalar(v) for v in (temp_start_thresh, temp_end_thresh, snow_thresh)):
        raise _Forward("thresholds")
    tas = np.asarray(tas)
    if tas.ndim < 1:
        raise _Forward("tas")
    shape = tas.shape
    T = shape[-1]
    fields = {"tas": _tfirst(tas, shape, "tas")}
    if method != "WF93":
        if snd is None:
            raise _Forward("snd")
        fields["snd"] = _tfirst(snd, shape, "snd")
    dev = device or get_device()
    kw = _merged_params({"temp_start_thresh": float(temp_start_thresh), "temp_end_thresh": float(temp_end_thresh),
                         "snow_thresh": float(snow_thresh), "temp_condition_days": int(temp_condition_days),
                         "snow_condition_days": int(snow_condition_days)})
    outs = K.fire_weather(dev, {k: dev.to_device(v) for k, v in fields.items()}, np.ones(T, np.int32), None, {}, [], kw,
                          season_method=method, want_mask=True)
    return F.time_last(outs["season_mask"].get().view(bool), shape[:-1])


def make_adapters(orig_calc, orig_season):
    """The two module attributes patch.install() puts into xclim.indices.fire._cffwis: each forwards to the saved
    original for the forms the device path does not take."""

    def _fire_weather_calc(tas, pr, rh, ws, snd, mth, lat, season_mask, dc0, dmc0, ffmc0, winter_pr, **params):
        try:
            return fire_weather_calc(tas, pr, rh, ws, snd, mth, lat, season_mask, dc0, dmc0, ffmc0, winter_pr, **params)
        except _Forward:
            return orig_calc(tas, pr, rh, ws, snd, mth, lat, season_mask, dc0, dmc0, ffmc0, winter_pr, **params)

    def _fire_season(tas, snd=None, method="WF93", temp_start_thresh=default_params["temp_start_thresh"][0],
                     temp_end_thresh=default_params["temp_end_thresh"][0],
                     temp_condition_days=default_params["temp_condition_days"],
                     snow_condition_days=default_params["snow_condition_days"], snow_thresh=default_params["snow_thresh"][0]):
        kw = dict(method=method, temp_start_thresh=temp_start_thresh, temp_end_thresh=temp_end_thresh,
                  temp_condition_days=temp_condition_days, snow_condition_days=snow_condition_days, snow_thresh=snow_thresh)
        try:
            return fire_season_np(tas, snd, **kw)
        except _Forward:
            return orig_season(tas, snd, **kw)

    _fire_weather_calc.__wrapped__ = orig_calc
    _fire_season.__wrapped__ = orig_season
    return {"_fire_weather_calc": _fire_weather_calc, "_fire_season": _fire_season}
