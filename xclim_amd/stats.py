"""Host mirror of the standardized indices of ``indices/stats.py`` (reference: src/xclim/indices/stats.py:770-1197).

``standardized_index_fit_params`` and ``standardized_index`` take a daily (or already resampled) field with TIME ON AXIS 0,
``(T, *cells)``, as a numpy array or a device array, plus its :class:`~xclim_amd.timeaxis.TimeAxis`.  The chain:

1. preprocess (:770-852): the ``MS`` means (``xh_resample_reduce``, NaN skipped) and the trailing
   ``rolling(time=window).mean(skipna=False)`` (``xh_rolling_reduce``, a NaN anywhere in the window gives NaN);
2. the fits, one lane per (cell, group) in float64 (``xh_si_fit``, xclim_amd/csrc/stdidx.hip): month groups for ``MS``,
   day-of-year groups (day 366 included) for ``D``;
3. the transform (``xh_si_apply``): cdf, the zero-inflated mixture, ``norm.ppf``, clipped to +-8.21; float64 out.

Float64 fields follow ``XCLIM_AMD_FLOAT64``.  Under ``native`` (a float64 host field or device array, e.g. the
``water_budget(..., keep=True)`` of :mod:`xclim_amd.converters`) every step runs on the float64 twins:
``xh_resample_reduce_f64`` (the month sums added in row order), ``xh_rolling_reduce_f64`` (the window added first row to
last), ``xh_si_fit_f64`` and ``xh_si_apply_f64``; nothing is rounded to float32.  Under ``raise`` (the default) a float64
host field raises :class:`~xclim_amd._capi.Float64FieldError`, under ``round`` it is rounded with a PrecisionWarning; a
float64 device array outside ``native`` is a TypeError.

Served: ``dist`` "gamma" / "fisk", ``method`` "APP" (with ``fitkwargs={"floc": v}``) and "ML" with or without ``floc``.
Refused with :class:`NotServed` (a NotImplementedError; the xarray adapter forwards these to the reference): weekly groups,
other distributions and ``rv_continuous`` objects, the PWM / MM / MSE methods, ``fscale`` and other fit keywords, time
selections (``**indexer``), day-of-year parameters whose calendar differs from the data's (the reference interpolates them,
``adjust_doy_calendar``).

Differences from the reference, all where the reference itself fails:
* gamma ML with ``floc`` and a value at or below ``floc``: NaN parameters (scipy raises FitDataError);
* a Nelder–Mead fit that ends off the parameter domain: NaN parameters (scipy raises FitError);
* the fits see the float32 preprocessed values widened to float64 (the reference hands scipy the float32 slices, so its
  start values are float32 means); the means of step 1 are float64 sums rounded once to float32, as every float32 mean of
  this package;
* float64 fields: the rolling mean is the window sum added in order, divided by the window; xarray's own rolling mean
  (bottleneck's running sum, or numpy's sum of the window view) can differ from it in the last bit.
"""

from __future__ import annotations

import json
import warnings

import numpy as np

from . import kernels as K
from ._capi import DISTFIT_MAX_Q, DISTFIT_STATUS, DeviceArray, float64_native, float64_policy, get_device, handle_float64
from .calendar import _flatten
from .fields import NotServed
from .timeaxis import TimeAxis

__all__ = ["NotServed", "SIParams", "standardized_index_fit_params", "standardized_index", "preprocessed_time", "Fitted", "fit",
           "parametric_quantile", "parametric_cdf", "parametric_pdf", "fa", "frequency_analysis"]

DIST_PARAMS = {"gamma": ("a", "loc", "scale"), "fisk": ("c", "loc", "scale")}
_MAX_DOY = {"360_day": 360, "noleap": 365, "365_day": 365}  # every other calendar: 366


class SIParams:
    """The fitted parameters of :func:`standardized_index_fit_params`.

    ``values``: ``(group, dparams, *cells)`` float64 (dparams = shape, loc, scale); ``number_of_zeros`` /
    ``number_of_notnull``: ``(group, *cells)`` float64 when the fit was zero-inflated, else None (NaN for a group absent from
    the calibration rows); ``group_values``: the labels (months 1..12 or days of year 1..366); ``attrs``: the reference's
    keys.  The tables stay on the device (``d_params`` ...) until one of the host properties is read."""

    def __init__(self, d_params, d_nzeros, d_nnotnull, cell_shape, attrs: dict, present=None):
        self.d_params, self.d_nzeros, self.d_nnotnull = d_params, d_nzeros, d_nnotnull
        self.cell_shape = tuple(cell_shape)
        self.attrs = dict(attrs)
        G = int(d_params.shape[0])
        self.present = np.ones(G, bool) if present is None else np.asarray(present, bool)  # groups the fit saw
        self.group_values = np.arange(1, G + 1)
        self.dparams = DIST_PARAMS[self.attrs["scipy_dist"]]

    def _host(self, a, lead):
        return None if a is None else a.get().reshape(*lead, *self.cell_shape)

    @property
    def values(self) -> np.ndarray:
        return self._host(self.d_params, (self.d_params.shape[0], 3))

    @property
    def number_of_zeros(self):
        return self._host(self.d_nzeros, (self.d_params.shape[0],))

    @property
    def number_of_notnull(self):
        return self._host(self.d_nnotnull, (self.d_params.shape[0],))

    @classmethod
    def from_arrays(cls, values, attrs: dict, number_of_zeros=None, number_of_notnull=None, present=None, *,
                    device=None) -> "SIParams":
        """Parameters given as host arrays: ``values`` (G, 3, *cells) with G = 12 for month groups, 366 for days of year;
        ``present`` (G) bool: the groups the fit saw (default: every group with a finite parameter somewhere)."""
        dev = device or get_device()
        v = np.asarray(values, dtype=np.float64)
        G = {"time.month": 12, "time.dayofyear": 366}.get(attrs.get("group"))
        if G is None or v.ndim < 2 or v.shape[0] != G or v.shape[1] != 3:
            raise ValueError(f"params: expected ({G}, 3, *cells) for group {attrs.get('group')!r}, got {v.shape}")
        if (number_of_zeros is None) != (number_of_notnull is None):
            raise ValueError("params: number_of_zeros and number_of_notnull go together")
        cells = v.shape[2:]
        C = int(np.prod(cells, dtype=np.int64))
        up = lambda a, lead: None if a is None else dev.to_device(np.asarray(a, np.float64).reshape(*lead, C))  # noqa: E731
        if present is None:
            present = np.isfinite(v.reshape(G, -1)).any(axis=1)
        return cls(up(v, (G, 3)), up(number_of_zeros, (G,)), up(number_of_notnull, (G,)), cells, attrs, present)


def _refuse_unserved(dist, method, fitkwargs, indexer, freq):
    if indexer:
        raise NotServed(f"standardized indices: time selections ({sorted(indexer)}) are not served")
    if freq is not None and freq not in ("MS", "D"):
        if freq.startswith("W"):
            raise NotServed("standardized indices: weekly groups are not served")
        raise ValueError(f"The input (following resampling if applicable) has a frequency `{freq}` "
                         "which is not supported for standardized indices.")
    if not isinstance(dist, str) or dist not in DIST_PARAMS:
        raise NotServed(f"standardized indices: the distribution {dist!r} is not served (gamma, fisk)")
    if method is not None and method not in ("ML", "MLE", "APP"):
        raise NotServed(f"standardized indices: the method {method!r} is not served (ML, APP)")
    extra = set(fitkwargs) - {"floc"}
    if extra:
        raise NotServed(f"standardized indices: fit keywords {sorted(extra)} are not served (floc only)")


def _check_dist_method(dist, method, fitkwargs):
    """The argument checks of standardized_index_fit_params (stats.py:912-936)."""
    if method == "APP" and "floc" not in fitkwargs:
        raise ValueError("The APP method is only supported for two-parameter distributions with `gamma`, `fisk`, "
                         "`lognorm`, or `genextreme` with `loc` being fixed. Pass a value for `floc` in `fitkwargs`.")
    dist_and_methods = {"gamma": ["ML", "APP"], "fisk": ["ML", "APP"], "genextreme": ["ML", "APP"], "lognorm": ["ML", "APP"]}
    if isinstance(dist, str):
        if dist not in dist_and_methods:
            raise NotImplementedError(f"The distribution `{dist}` is not supported.")
        if method not in dist_and_methods[dist]:
            raise NotImplementedError(f"The method `{method}` is not supported for distribution `{dist}`.")


def _is_monthly(t: TimeAxis) -> bool:
    if len(t) == 0:
        return False
    m = t.year * 12 + t.month
    return bool(np.all(t.day == 1) and np.all(np.diff(m) == 1))


def _is_daily(t: TimeAxis) -> bool:
    return len(t) > 0 and bool(np.all(np.diff(t.ordinal()) == 1))


def _group_of(freq, time: TimeAxis) -> str:
    """preprocess_standardized_index's group (stats.py:798-818); ``freq=None`` takes it from the (already resampled) axis."""
    final = freq
    if final is None:
        final = "MS" if _is_monthly(time) else ("D" if _is_daily(time) else None)
        if final is None:
            warnings.warn("No resampling frequency was specified and a frequency for the dataset could not be identified "
                          "with ``xr.infer_freq``")
            return "time.dayofyear"
    return "time.month" if final == "MS" else "time.dayofyear"


def preprocessed_time(time: TimeAxis, freq: str | None) -> TimeAxis:
    """The time axis of the preprocessed series (and of the standardized index): month starts for ``MS``."""
    if freq == "MS" and not _is_monthly(time):
        _, starts = time.segments("MS")
        return TimeAxis([y for y, _ in starts], [m for _, m in starts], np.ones(len(starts), np.int64), time.calendar)
    if freq == "D" and not _is_daily(time):
        raise NotServed("standardized indices: freq='D' needs a daily time axis")
    return time


def _preprocess(dev, x: DeviceArray, time: TimeAxis, freq, window: int):
    """Resample (MS means) and roll (trailing mean, NaN-propagating): (T', C) on the device in the field's dtype (float32,
    or float64 under ``native``) + its axis."""
    if window is None or int(window) < 1:
        raise ValueError(f"window must be an integer >= 1, got {window!r}")
    if len(time) != x.shape[0]:
        raise ValueError(f"time axis has {len(time)} steps, the field {x.shape[0]}")
    t2 = preprocessed_time(time, freq)
    if t2 is not time:
        seg_off, _ = time.segments("MS")
        x, _ = K.resample_reduce(dev, x, "mean", seg_off, skipna=True, want_valid=False)
    if int(window) > 1:
        x = K.rolling_reduce(dev, x, int(window), "mean", center=False)
    return x, t2


def _groups(time: TimeAxis, group: str) -> tuple[np.ndarray, int]:
    if group == "time.month":
        return (time.month - 1).astype(np.int32), 12
    return (time.doy - 1).astype(np.int32), 366


def _date_key(s: str | None, end: bool):
    if s is None:
        return None
    parts = [int(p) for p in str(s)[:10].split("-")]
    y = parts[0]
    m = parts[1] if len(parts) > 1 else (12 if end else 1)
    d = parts[2] if len(parts) > 2 else (31 if end else 1)
    return y * 10000 + m * 100 + d


def _cal_rows(time: TimeAxis, cal_start, cal_end) -> np.ndarray:
    """Rows of ``da.sel(time=slice(cal_start, cal_end))`` (date strings, partial dates as pandas reads them)."""
    key = time.year * 10000 + time.month * 100 + time.day
    keep = np.ones(len(time), bool)
    lo, hi = _date_key(cal_start, False), _date_key(cal_end, True)
    if lo is not None:
        keep &= key >= lo
    if hi is not None:
        keep &= key <= hi
    return keep


def _zero_options(prob_zero_interpolation, plotting_position_zero):
    """stats.py:1088-1101."""
    interp = {"center": 1 / 2, "upper": 1}.get(prob_zero_interpolation, None) if isinstance(prob_zero_interpolation, str) else None
    if interp is None:
        if isinstance(prob_zero_interpolation, str):
            raise ValueError("Accepted strings for `prob_zero_interpolation` are: ['center', 'upper']")
        interp = prob_zero_interpolation
    ab = {"ecdf": (0, 1), "weibull": (0, 0)}.get(plotting_position_zero, None) if isinstance(plotting_position_zero, str) else None
    if ab is None:
        if isinstance(plotting_position_zero, str):
            raise ValueError("Accepted strings for `plotting_position_zero` are: ['ecdf', 'weibull']")
        ab = plotting_position_zero
    return float(interp), float(ab[0]), float(ab[1])


def _refuse_float64(da):
    """The XCLIM_AMD_FLOAT64 refusal before any device work (``round`` warns once, in _flatten; ``native`` uploads the
    field as it is, _flatten(..., f64=True))."""
    if not isinstance(da, DeviceArray) and getattr(da, "dtype", None) == np.float64 and float64_policy() == "raise":
        handle_float64(np.asarray(da), "standardized_index")


def _fit(dev, x, t2, group, dist, method, zero_inflated, fitkwargs, keep_rows, attrs, staging="auto"):
    gidx, G = _groups(t2, group)
    gidx = np.where(keep_rows, gidx, -1).astype(np.int32)
    floc = fitkwargs.get("floc")
    params, nz, nn, _ = K.si_fit(dev, x, gidx, G, dist, "APP" if method == "APP" else "ML",
                                 floc=None if floc is None else float(floc), zero_inflated=zero_inflated, staging=staging)
    present = np.zeros(G, bool)
    present[gidx[gidx >= 0]] = True
    return params, nz, nn, present


def standardized_index_fit_params(da, time: TimeAxis, freq: str | None, window: int, dist="gamma", method: str = "ML",
                                  zero_inflated: bool = False, fitkwargs: dict | None = None, *, device=None,
                                  **indexer) -> SIParams:
    """stats.py:855-964: the per-group parameters of ``dist`` fitted to the preprocessed ``da``."""
    fitkwargs = dict(fitkwargs or {})
    _check_dist_method(dist, method, fitkwargs)
    _refuse_unserved(dist, method, fitkwargs, indexer, freq)
    _refuse_float64(da)
    dev = device or get_device()
    x, cells = _flatten(da, dev, f64=float64_native())  # native: the _f64 twins (xh_si_fit_f64 / xh_si_apply_f64)
    x, t2 = _preprocess(dev, x, time, freq, window)
    group = _group_of(freq, t2)
    params, nz, nn, present = _fit(dev, x, t2, group, dist, method, zero_inflated, fitkwargs, np.ones(len(t2), bool), None)
    cal = (_iso(t2, 0), _iso(t2, -1)) if len(t2) else ("", "")
    attrs = {"calibration_period": cal, "freq": freq or "", "window": window, "scipy_dist": dist, "method": method,
             "group": group, "units": "", "time_indexer": json.dumps(indexer)}
    return SIParams(params, nz, nn, cells, attrs, present)


def _iso(t: TimeAxis, i: int) -> str:
    return f"{int(t.year[i]):04d}-{int(t.month[i]):02d}-{int(t.day[i]):02d}"


def standardized_index(da, time: TimeAxis, freq: str | None, window: int | None, dist="gamma", method: str | None = "ML",
                       zero_inflated: bool | None = False, fitkwargs: dict | None = None, cal_start: str | None = None,
                       cal_end: str | None = None, params: SIParams | None = None, prob_zero_interpolation="upper",
                       plotting_position_zero="ecdf", *, device=None, keep: bool = False, **indexer):
    """stats.py:967-1197: the standardized index (T', *cells) float64 on the axis ``preprocessed_time(time, freq)``
    (``keep=True``: the (T', C) float64 DeviceArray).  ``params`` (from :func:`standardized_index_fit_params`) overrides
    ``freq``, ``window`` and ``dist``, and the calibration dates."""
    fitkwargs = dict(fitkwargs or {})
    if params is None and None in [window, dist, method, zero_inflated]:
        raise ValueError("If `params` is `None`, `window`, `dist`, `method` and `zero_inflated` must be given.")
    if params is not None:
        if not isinstance(params, SIParams):
            raise NotServed("standardized_index: params must be an SIParams table")
        freq, window, dist = params.attrs["freq"], params.attrs["window"], params.attrs["scipy_dist"]
        freq = None if freq == "" else freq
        indexer = json.loads(params.attrs["time_indexer"]) or indexer
        if cal_start or cal_end:
            warnings.warn("Expected either `cal_{start|end}` or `params`, got both. The `params` input overrides other inputs."
                          "If `cal_start`, `cal_end`, `freq`, `window`, and/or `dist` were given as input, they will be ignored.")
    interp, alpha, beta = _zero_options(prob_zero_interpolation, plotting_position_zero)
    if params is None:
        _check_dist_method(dist, method, fitkwargs)
    _refuse_unserved(dist, method if params is None else None, fitkwargs if params is None else {}, indexer, freq)
    _refuse_float64(da)
    dev = device or get_device()
    x, cells = _flatten(da, dev, f64=float64_native())  # native: the _f64 twins (xh_si_fit_f64 / xh_si_apply_f64)
    x, t2 = _preprocess(dev, x, time, freq, window)
    if params is None:
        group = _group_of(None, t2)  # the fit runs on the preprocessed series with freq=None (stats.py:1105-1113)
        d_params, nz, nn, present = _fit(dev, x, t2, group, dist, method, bool(zero_inflated), fitkwargs,
                                         _cal_rows(t2, cal_start, cal_end), None)
    else:
        group = params.attrs["group"]
        if group not in ("time.month", "time.dayofyear"):
            raise NotServed(f"standardized_index: parameters grouped by {group!r} are not served")
        if params.cell_shape != tuple(cells):
            raise NotServed(f"standardized_index: params cells {params.cell_shape} differ from the field's {tuple(cells)}")
        if group == "time.dayofyear":
            maxdoy = int(np.flatnonzero(params.present)[-1]) + 1 if params.present.any() else 0
            if maxdoy != _MAX_DOY.get(time.calendar, 366):
                raise NotServed("standardized_index: day-of-year parameters of another calendar (adjust_doy_calendar)")
        d_params, nz, nn = params.d_params, params.d_nzeros, params.d_nnotnull
    gidx, _ = _groups(t2, group)
    out = K.si_apply(dev, x, gidx, d_params, dist, nz, nn, alpha=alpha, beta=beta, interp=interp)
    if keep:
        return out
    return out.get().reshape(len(t2), *cells)


# ---- xarray adapter (patch.install() puts these into indices/stats.py, _agro.py and _hydrology.py) --------------------------
_GROUP_DIM = {"time.month": "month", "time.dayofyear": "dayofyear"}


def _params_table(params, da_cell_dims, cell_shape, dev):
    """A reference params DataArray ``(group, dparams, *cells)`` -> SIParams (full 12 / 366 group tables, NaN for the
    groups it does not hold, as its reindexing gives); None when its form is not served."""
    group = params.attrs.get("group")
    gdim = _GROUP_DIM.get(group)
    if gdim is None or params.attrs.get("scipy_dist") not in DIST_PARAMS or "dparams" not in params.dims:
        return None
    if "number_of_zeros" not in params.coords and "prob_of_zero" in params.coords:
        return None  # parameters of an old version (stats.py:1115-1129): the reference's own path
    if set(params.dims) != {gdim, "dparams", *da_cell_dims}:
        return None
    p = params.transpose(gdim, "dparams", *da_cell_dims)
    G = 12 if gdim == "month" else 366
    labels = np.asarray(p[gdim].values).astype(np.int64)
    if labels.min() < 1 or labels.max() > G or tuple(p.shape[2:]) != tuple(cell_shape):
        return None
    vals = np.full((G, 3) + tuple(cell_shape), np.nan)
    vals[labels - 1] = np.asarray(p.values, np.float64)
    present = np.zeros(G, bool)
    present[labels - 1] = True
    counts = [None, None]
    if "number_of_zeros" in params.coords:
        for k, name in enumerate(("number_of_zeros", "number_of_notnull")):
            c = np.full((G,) + tuple(cell_shape), np.nan)
            c[labels - 1] = np.asarray(params.coords[name].transpose(gdim, *da_cell_dims).values, np.float64)
            counts[k] = c
    return SIParams.from_arrays(vals, dict(params.attrs), counts[0], counts[1], present, device=dev)


def make_adapters(env, orig_index, orig_fit, device=None) -> dict:
    """Same-signature replacements of ``standardized_index`` / ``standardized_index_fit_params`` (stats.py:855-1197) on
    DataArrays (time may be anywhere; results come back time first).  Forms the device does not serve (:class:`NotServed`,
    float64 fields outside ``XCLIM_AMD_FLOAT64=native``, chunked fields, parameters in an unserved layout) go to
    ``orig_index`` / ``orig_fit``."""
    from ._capi import Float64FieldError
    from .xr_adapter import _cell_coords, _cell_dims, _tfirst, time_axis_of

    DA = env.DataArray

    def _field(da):
        if not isinstance(da, DA) or "time" not in da.dims:
            return None
        a, x = _tfirst(da)
        return None if x is None else (a, x)

    def _time_out(a, freq, t2, time):
        if t2 is time:
            return a["time"]
        return a["time"].resample(time=freq).first()["time"]

    def _wrap(a, data, time_coord, attrs):
        coords = dict(_cell_coords(a))
        coords["time"] = time_coord
        return DA(np.asarray(data), coords=coords, dims=("time",) + _cell_dims(a), attrs=attrs)

    def fit_params(da, freq, window, dist, method, zero_inflated=False, fitkwargs=None, **indexer):
        f = _field(da)
        if f is None:
            return orig_fit(da, freq, window, dist, method, zero_inflated=zero_inflated, fitkwargs=fitkwargs, **indexer)
        a, x = f
        try:
            p = standardized_index_fit_params(x, time_axis_of(a), freq, window, dist, method, zero_inflated, fitkwargs,
                                              device=device, **indexer)
        except (NotServed, Float64FieldError):
            return orig_fit(da, freq, window, dist, method, zero_inflated=zero_inflated, fitkwargs=fitkwargs, **indexer)
        gdim = _GROUP_DIM[p.attrs["group"]]
        labels = np.flatnonzero(p.present) + 1
        cdims = _cell_dims(a)
        coords = dict(_cell_coords(a))
        coords[gdim] = labels
        coords["dparams"] = list(DIST_PARAMS[dist])
        if p.d_nzeros is not None:
            nz, nn = p.number_of_zeros[labels - 1], p.number_of_notnull[labels - 1]
            ccoords = {k: v for k, v in coords.items() if k != "dparams"}
            coords["number_of_zeros"] = DA(nz.astype(np.int64), coords=ccoords, dims=(gdim,) + cdims)
            coords["number_of_notnull"] = DA(nn.astype(np.int64), coords=ccoords, dims=(gdim,) + cdims)
            with np.errstate(all="ignore"):
                coords["prob_of_zero"] = DA(nz / nn, coords=ccoords, dims=(gdim,) + cdims)
        return DA(p.values[labels - 1], coords=coords, dims=(gdim, "dparams") + cdims, attrs=dict(p.attrs))

    def standardized_index_(da, freq, window, dist, method, zero_inflated, fitkwargs, cal_start, cal_end, params=None,
                            prob_zero_interpolation="upper", plotting_position_zero="ecdf", **indexer):
        def forward():
            return orig_index(da, freq, window, dist, method, zero_inflated, fitkwargs, cal_start, cal_end, params=params,
                              prob_zero_interpolation=prob_zero_interpolation,
                              plotting_position_zero=plotting_position_zero, **indexer)

        f = _field(da)
        if f is None:
            return forward()
        a, x = f
        time = time_axis_of(a)
        sip = None
        try:
            if params is not None:
                _refuse_float64(x)
                sip = _params_table(params, _cell_dims(a), x.shape[1:], device or get_device())
                if sip is None:
                    return forward()
            si = standardized_index(x, time, freq, window, dist, method, zero_inflated, fitkwargs, cal_start, cal_end,
                                    params=sip, prob_zero_interpolation=prob_zero_interpolation,
                                    plotting_position_zero=plotting_position_zero, device=device, **indexer)
        except (NotServed, Float64FieldError):
            return forward()
        if sip is not None:
            attrs = dict(sip.attrs)
            freq, window = sip.attrs["freq"] or None, sip.attrs["window"]
        else:  # the attrs of the fit on the calibration rows (stats.py:1105-1113: freq=None, window=1)
            t2 = preprocessed_time(time, freq)
            rows = np.flatnonzero(_cal_rows(t2, cal_start, cal_end))
            cal = (_iso(t2, int(rows[0])), _iso(t2, int(rows[-1]))) if len(rows) else ("", "")
            attrs = {"calibration_period": cal, "freq": "", "window": 1, "scipy_dist": dist, "method": method,
                     "group": _group_of(None, t2), "units": "", "time_indexer": "{}"}
        t2 = preprocessed_time(time, freq)
        inferred = "MS" if _is_monthly(t2) else ("D" if _is_daily(t2) else None)
        attrs.update(freq=(freq or inferred) or "undefined", window=window, units="")
        return _wrap(a, si, _time_out(a, freq, t2, time), attrs)

    standardized_index_.__wrapped__ = orig_index
    fit_params.__wrapped__ = orig_fit
    return {"standardized_index": standardized_index_, "standardized_index_fit_params": fit_params}


# ==== distribution fits and return levels (stats.py:45-548; xclim_amd/csrc/distfit.hip) ==================================================
# fit, parametric_quantile / _cdf / _pdf, fa and frequency_analysis on arrays with TIME ON AXIS 0.  One launch per call (xh_dist_fit,
# xh_dist_eval); fa and frequency_analysis take their levels from the fit launch itself.
#
# Served: ``dist`` one of FIT_DISTS, by name or as the scipy singleton of that name; ``method`` ML / MLE (lognorm only with
# ``floc``) and APP (genextreme, gamma, fisk, lognorm; for norm and gumbel_r the reference itself raises KeyError); ``floc`` for
# gamma, fisk and lognorm.  Refused with NotServed: other distributions and rv_continuous objects, the methods MM / PWM / MSE /
# MPS, lognorm ML without floc, floc for norm / gumbel_r / genextreme, every other fit keyword, integer fields.
#
# ASSUMPTION: all arithmetic is float64 on the widened values.  The reference hands scipy a float32 slice of a float32 field, so
# its start values are float32 means; this unit does not reproduce that.
#
# Differences from the reference, all where scipy itself fails for the cell (and the reference with it, for the whole call): NaN
# parameters where brentq finds no sign change or meets a NaN function value (gumbel_r on identical values, where scipy returns
# (inf, tiny)), where gamma with floc has a value at or below floc, where lognorm with floc ends with a shape of zero, and where a
# Nelder–Mead fit ends off the parameter domain.  gamma's isf(q) is ppf(1 - q).  No ``history`` attribute is written.
FIT_DISTS = {"norm": ("loc", "scale"), "gumbel_r": ("loc", "scale"), "genextreme": ("c", "loc", "scale"),
             "gamma": ("a", "loc", "scale"), "fisk": ("c", "loc", "scale"), "lognorm": ("s", "loc", "scale")}
_METHOD_NAME = {"ML": "maximum likelihood", "MM": "method of moments", "MLE": "maximum likelihood",
                "MSE": "maximum product of spacings", "MPS": "maximum product of spacings", "PWM": "probability weighted moments",
                "APP": "approximative method"}
_FLOC_DISTS = ("gamma", "fisk", "lognorm")


class Fitted:
    """The result of :func:`fit`: ``values`` (nparams, *cells) float64 (``keep=True``: the (nparams, C) DeviceArray), ``attrs``
    (the reference's), ``dist``, ``cell_shape``, and per cell ``nfev`` (objective evaluations) and ``status``
    (``_capi.DISTFIT_STATUS``) as host arrays.  Unpacks as ``values, attrs = fit(...)``."""

    def __init__(self, values, attrs, dist, cell_shape, nfev, status):
        self.values, self.attrs, self.dist, self.cell_shape = values, attrs, dist, tuple(cell_shape)
        self.nfev, self.status = nfev, status

    def __iter__(self):
        return iter((self.values, self.attrs))


def dist_name(dist) -> str:
    """The name of a served distribution given by name or as the scipy singleton of that name; NotServed otherwise."""
    if isinstance(dist, str):
        if dist in FIT_DISTS:
            return dist
        raise NotServed(f"distribution fits: the distribution {dist!r} is not served ({', '.join(FIT_DISTS)})")
    name = getattr(dist, "name", None)
    if name in FIT_DISTS:
        import sys

        sst = sys.modules.get("scipy.stats")   # (an rv_continuous object exists only where scipy.stats was imported)
        if sst is not None and getattr(sst, name, None) is dist:
            return name
    raise NotServed(f"distribution fits: {dist!r} is not one of scipy's {', '.join(FIT_DISTS)}")


def _check_fit(dist, method, fitkwargs):
    """(name, the method in capitals, "ML" | "APP" for the kernel, floc or None) of a served fit; ValueError for an unknown method, NotServed for the rest."""
    method = method.upper()
    if method not in _METHOD_NAME:
        raise ValueError(f"Fitting method not recognized: {method}")
    name = dist_name(dist)
    if method not in ("ML", "MLE", "APP"):
        raise NotServed(f"distribution fits: the method {method} is not served (ML, MLE, APP)")
    extra = set(fitkwargs) - {"floc"}
    if extra:
        raise NotServed(f"distribution fits: fit keywords {sorted(extra)} are not served (floc only)")
    floc = fitkwargs.get("floc")
    if floc is not None:
        if name not in _FLOC_DISTS:
            raise NotServed(f"distribution fits: floc is not served for {name}")
        floc = float(floc)
    if method == "APP" and name in ("norm", "gumbel_r"):
        raise NotServed(f"distribution fits: the reference has no APP method for {name}")
    if name == "lognorm" and method != "APP" and floc is None:
        raise NotServed("distribution fits: lognorm by maximum likelihood is served with floc only")
    return name, method, ("APP" if method == "APP" else "ML"), floc


def _fit_field(da, dev):
    """(DeviceArray (T, C) float32 or float64, cell shape): float fields only, float64 read natively."""
    if not isinstance(da, DeviceArray):
        da = np.asarray(da)
        if da.dtype.kind != "f":
            raise NotServed(f"distribution fits: {da.dtype.name} fields are not served (float32, float64)")
        if da.dtype not in (np.float32, np.float64):
            da = da.astype(np.float32)
    if len(da.shape) < 1:
        raise ValueError("distribution fits: the field needs a time axis")
    return _flatten(da, dev, f64=True)


def fit_attrs(name: str, method: str, attrs: dict | None = None) -> dict:
    """The attributes of the reference's fit (stats.py:203-217, without ``history``)."""
    out = {}
    for k, v in (attrs or {}).items():
        out[f"original_{k}" if k in ("standard_name", "long_name", "units", "description") else k] = v
    out.update(long_name=f"{name} parameters", description=f"Parameters of the {name} distribution", method=method,
               estimator=_METHOD_NAME[method].capitalize(), scipy_dist=name, units="")
    return out


def _raise_support(name, status):
    # lognorm_gen.fit raises FitDataError (a ValueError) for the whole call; scipy's text
    if name == "lognorm" and (status == DISTFIT_STATUS["support"]).any():
        raise ValueError("Invalid values in `data`.  Maximum likelihood estimation with 'lognorm' requires that 0.0 < "
                         "(x - loc)/scale  < inf for each x in `data`.")


def fit(da, dist="norm", method: str = "ML", *, attrs: dict | None = None, device=None, keep: bool = False, **fitkwargs) -> Fitted:
    """stats.py:115-218 on a (T, *cells) field: the parameters (nparams, *cells) float64 of ``dist`` for every cell.  NaN values
    of a cell are dropped; fewer than two values, or a NaN parameter, make all of the cell's parameters NaN."""
    name, method, kmethod, floc = _check_fit(dist, method, fitkwargs)
    dev = device or get_device()
    x, cells = _fit_field(da, dev)
    params, nfev, status, _ = K.dist_fit(dev, x, name, kmethod, floc)
    st = status.get()
    _raise_support(name, st)
    values = params if keep else params.get().reshape(len(FIT_DISTS[name]), *cells)
    return Fitted(values, fit_attrs(name, method, attrs), name, cells, nfev.get(), st)


def _params_of(p, dist, dev):
    """(DeviceArray (nparams, C), name, cell shape) of a Fitted, a DeviceArray (nparams, C) or a host array (nparams, *cells)."""
    if isinstance(p, Fitted):
        name = dist_name(dist or p.attrs["scipy_dist"])
        v, cells = p.values, p.cell_shape
    else:
        if dist is None:
            raise ValueError("parametric functions of a plain array need `dist`")
        name, v = dist_name(dist), p
        cells = None
    n = len(FIT_DISTS[name])
    if isinstance(v, DeviceArray):
        if np.dtype(v.dtype) != np.float64 or v.shape[0] != n:
            raise TypeError(f"{name} parameters must be float64 ({n}, C), got {np.dtype(v.dtype).name} {v.shape}")
        cells = tuple(v.shape[1:]) if cells is None else cells
        return v.reshape(n, -1), name, cells
    v = np.asarray(v)
    if v.dtype.kind != "f":
        raise NotServed(f"distribution fits: {v.dtype.name} parameters are not served")
    if v.ndim < 1 or v.shape[0] != n:
        raise ValueError(f"{name} has {n} parameters, got an array of shape {v.shape}")
    return dev.to_device(v.reshape(n, -1), dtype=np.float64), name, tuple(v.shape[1:])


def _parametric(p, v, dist, func, device, keep):
    dev = device or get_device()
    d, name, cells = _params_of(p, dist, dev)
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    if v.ndim != 1:
        raise ValueError("`v` must be one-dimensional.")
    out = K.dist_eval(dev, d, name, func, v)
    return out if keep else out.get().reshape(len(v), *cells)


def quantile_route(q) -> tuple[str, np.ndarray]:
    """The switch of parametric_quantile (stats.py:254-262): ("isf", 1 - q) when every q > 0.5, else ("ppf", q)."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    return ("isf", 1 - q) if np.all(q > 0.5) else ("ppf", q)


def parametric_quantile(p, q, dist=None, *, device=None, keep: bool = False):
    """stats.py:221-292: (nq, *cells) float64, the quantiles ``q`` of the fitted distribution of every cell."""
    func, arg = quantile_route(q)
    return _parametric(p, arg, dist, func, device, keep)


def parametric_cdf(p, v, dist=None, *, device=None, keep: bool = False):
    """stats.py:297-360: (nv, *cells) float64."""
    return _parametric(p, v, dist, "cdf", device, keep)


def parametric_pdf(p, v, dist=None, *, device=None, keep: bool = False):
    """stats.py:363-426: (nv, *cells) float64."""
    return _parametric(p, v, dist, "pdf", device, keep)


def _return_quantiles(t, mode):
    t = np.atleast_1d(t)
    if mode in ["max", "high"]:
        return t, 1 - 1.0 / t
    if mode in ["min", "low"]:
        return t, 1.0 / t
    raise ValueError(f"Mode `{mode}` should be either 'max' or 'min'.")


def fa(da, t, dist="norm", mode: str = "max", method: str = "ML", *, device=None, keep: bool = False):
    """stats.py:429-482: (nt, *cells) float64, the value with return period ``t`` from the maximized / minimized ``da``
    (T, *cells).  Fit and levels are ONE launch for up to ``_capi.DISTFIT_MAX_Q`` periods."""
    name, method, kmethod, floc = _check_fit(dist, method, {})
    t, q = _return_quantiles(t, mode)
    func, arg = quantile_route(q)
    dev = device or get_device()
    x, cells = _fit_field(da, dev)
    if len(arg) <= DISTFIT_MAX_Q:
        _, _, _, out = K.dist_fit(dev, x, name, kmethod, floc, q=arg, qfunc=func)
    else:
        params, _, _, _ = K.dist_fit(dev, x, name, kmethod, floc)
        out = K.dist_eval(dev, params, name, func, arg)
    return out if keep else out.get().reshape(len(arg), *cells)


def frequency_analysis(da, mode: str, t, dist, time: TimeAxis = None, window: int = 1, freq: str | None = None,
                       method: str = "ML", *, device=None, keep: bool = False, **indexer):
    """stats.py:485-548 on a daily (T, *cells) field with its TimeAxis: the trailing rolling mean (``skipna=False``), the
    period extremes (``generic.select_resample_op``; ``freq=None``: ``generic.default_freq(**indexer)``), kept on the device,
    and :func:`fa` on them."""
    from . import generic
    from .calendar import _flatten as flatten

    if time is None:
        raise TypeError("frequency_analysis needs the field's TimeAxis (time=)")
    _check_fit(dist, method, {})
    _return_quantiles(t, mode)
    if mode not in ("max", "min"):
        raise NotServed(f"frequency_analysis: the resampling operator {mode!r} is not served (max, min)")
    dev = device or get_device()
    if int(window) > 1:
        x, cells = flatten(da, dev, f64=float64_native() and not indexer)
        da = K.rolling_reduce(dev, x, int(window), "mean", center=False)
    else:
        cells = tuple(da.shape[1:])
    freq = freq or generic.default_freq(**indexer)
    sel = generic.select_resample_op(da, mode, time, freq, device=dev, keep=True, **indexer)
    out = fa(sel, t, dist, mode, method, device=dev, keep=True)
    return out if keep else out.get().reshape(out.shape[0], *cells)


FIT_ADAPTED = ("fit", "parametric_quantile", "parametric_cdf", "parametric_pdf", "fa", "frequency_analysis")


def make_fit_adapters(env, origs: dict, device=None) -> dict:
    """Same-signature replacements of the six functions of FIT_ADAPTED on DataArrays (``dim`` may be anywhere; ``dparams``,
    ``quantile`` / ``return_period``, ``cdf`` and ``v`` land where the reference transposes them).  NotServed forms, chunked
    fields and float64 refusals go to ``origs``."""
    from ._capi import Float64FieldError
    from .xr_adapter import is_chunked, time_axis_of

    DA = env.DataArray

    def _moved(a, dim):
        """(values with `dim` first, the position of `dim`, the other dims, the coordinates without `dim`)"""
        ax = a.dims.index(dim)
        rest = tuple(d for d in a.dims if d != dim)
        vals = np.ascontiguousarray(a.transpose(dim, *rest).values)
        coords = {k: v for k, v in a.coords.items() if dim not in getattr(v, "dims", ())}
        return vals, ax, rest, coords

    def _put(values, ax, rest, coords, newdim, labels, attrs):
        coords = dict(coords)
        coords[newdim] = labels
        dims = rest[:ax] + (newdim,) + rest[ax:]
        return DA(np.moveaxis(np.asarray(values), 0, ax), coords=coords, dims=dims, attrs=attrs)

    def _ok(da, dim):
        return isinstance(da, DA) and dim in da.dims and not is_chunked(da)

    def fit_(da, dist="norm", method="ML", dim="time", **fitkwargs):
        if not _ok(da, dim):
            return origs["fit"](da, dist, method, dim, **fitkwargs)
        try:
            vals, ax, rest, coords = _moved(da, dim)
            p = fit(vals, dist, method, attrs=da.attrs, device=device, **fitkwargs)
        except (NotServed, Float64FieldError):
            return origs["fit"](da, dist, method, dim, **fitkwargs)
        return _put(p.values, ax, rest, coords, "dparams", list(FIT_DISTS[p.dist]), p.attrs)

    def _unprefixed(attrs):
        out = {}
        for k, v in attrs.items():
            if k in ("original_units", "original_standard_name"):
                out[k[len("original_"):]] = v
            elif k not in out:
                out[k] = v
        return out

    def _param_call(fn, p, arg, dist, newdim, label, cell_methods, what):
        if not _ok(p, "dparams") or not (dist or "scipy_dist" in p.attrs):
            return None
        arg_da = arg if isinstance(arg, DA) else None
        if arg_da is not None and len(arg_da.dims) > 1:
            raise ValueError("`v` must be one-dimensional.")
        a = np.atleast_1d(np.asarray(arg_da.values if arg_da is not None else arg, dtype=np.float64))
        try:
            dname = dist_name(dist or p.attrs["scipy_dist"])
            vals, ax, rest, coords = _moved(p, "dparams")
            out = fn(vals, a, dname, device=device)
        except (NotServed, Float64FieldError):
            return None
        attrs = _unprefixed(p.attrs)
        attrs.update(long_name=f"{dname} {label}", description=f"{what} estimated by the {dname} distribution",
                     cell_methods=cell_methods)
        labels = a if arg_da is None else DA(a, dims=(newdim,), attrs=arg_da.attrs)
        return _put(out, ax, rest, coords, newdim, labels, attrs)

    def parametric_quantile_(p, q, dist=None):
        out = _param_call(parametric_quantile, p, q, dist, "quantile", "quantiles", "dparams: ppf", "Quantiles")
        return origs["parametric_quantile"](p, q, dist) if out is None else out

    def parametric_cdf_(p, v, dist=None):
        out = _param_call(parametric_cdf, p, v, dist, "cdf", "cdf", "dparams: cdf", "CDF")
        return origs["parametric_cdf"](p, v, dist) if out is None else out

    def parametric_pdf_(p, v, dist=None):
        out = _param_call(parametric_pdf, p, v, dist, "v", "PDF", "dparams: v", "PDF")
        return origs["parametric_pdf"](p, v, dist) if out is None else out

    def fa_(da, t, dist="norm", mode="max", method="ML"):
        if not _ok(da, "time"):
            return origs["fa"](da, t, dist, mode, method)
        try:
            vals, ax, rest, coords = _moved(da, "time")
            out = fa(vals, t, dist, mode, method, device=device)
            attrs = _unprefixed(fit_attrs(dist_name(dist), method.upper(), da.attrs))
        except (NotServed, Float64FieldError):
            return origs["fa"](da, t, dist, mode, method)
        dname = attrs["scipy_dist"]
        attrs.update(long_name=f"{dname} quantiles", description=f"Quantiles estimated by the {dname} distribution",
                     cell_methods="dparams: ppf", mode=mode)
        return _put(out, ax, rest, coords, "return_period", np.atleast_1d(t), attrs)

    def frequency_analysis_(da, mode, t, dist, window=1, freq=None, method="ML", **indexer):
        if not _ok(da, "time"):
            return origs["frequency_analysis"](da, mode, t, dist, window, freq, method, **indexer)
        try:
            vals, ax, rest, coords = _moved(da, "time")
            out = frequency_analysis(vals, mode, t, dist, time_axis_of(da), window, freq, method, device=device, **indexer)
            attrs = _unprefixed(fit_attrs(dist_name(dist), method.upper(), da.attrs))
        except (NotServed, Float64FieldError):
            return origs["frequency_analysis"](da, mode, t, dist, window, freq, method, **indexer)
        dname = attrs["scipy_dist"]
        attrs.update(long_name=f"{dname} quantiles", description=f"Quantiles estimated by the {dname} distribution",
                     cell_methods="dparams: ppf", mode=mode)
        return _put(out, ax, rest, coords, "return_period", np.atleast_1d(t), attrs)

    adapters = {"fit": fit_, "parametric_quantile": parametric_quantile_, "parametric_cdf": parametric_cdf_,
                "parametric_pdf": parametric_pdf_, "fa": fa_, "frequency_analysis": frequency_analysis_}
    for n, fn in adapters.items():
        fn.__wrapped__ = origs[n]
        fn.__name__ = n
    return adapters
