"""Host mirror of the streamflow and snow-melt indices (reference: src/xclim/indices/_hydrology.py ``base_flow_index`` :50-90,
``rb_flashiness_index`` :94-129, ``snow_melt_we_max`` :371-400, ``melt_and_precip_max`` :404-440, ``flow_index`` :577-603,
``high_flow_frequency`` :607-636, ``low_flow_frequency`` :640-669, ``antecedent_precipitation_index`` :673-706,
``aridity_index`` :772-814, ``sen_slope`` :894-944, ``sen_slope_ratio`` :949-993, ``base_flow_index_seasonal_ratio`` :997-1038,
and ``split_time_to_season_year`` of src/xclim/core/calendar.py:1775-1802).  The kernels are in xclim_amd/csrc/hydro.hip, their
C ABI in include/xclim_hip_hydro.h.

The functions carry the reference's names, parameters and defaults, plus ``time``, ``flux_units``, ``device``, ``keep`` and, for
the period functions, ``mask_missing``.  Inputs are numpy arrays (or ``(T, C)`` device arrays) with TIME ON AXIS 0 on a daily,
gap-free :class:`~xclim_amd.timeaxis.TimeAxis`; discharge and snow amount stay in their own units (every index here is a ratio
or keeps the units of ``snw``), ``flux_units`` of a precipitation rate is one of "kg m-2 s-1", "mm/s", "mm/d".  Results are
float64 ``(P, *cells)`` on the periods of ``time.segments(freq)`` (``(T, *cells)`` for the antecedent precipitation index), or
device arrays with ``keep=True`` (which needs ``mask_missing=False``).

ASSUMPTIONS (neither xarray nor pymannkendall is needed, or used, here).  All arithmetic of the new kernels is float64 on
the widened field.  A NaN discharge is skipped by the period mean and sum and makes the seven-day means around it NaN; a
period without a seven-day mean or without a value gives NaN.  The seven-day mean adds its seven values in row order, the
melt window its ``window`` totals in row order, the antecedent precipitation index its ``window`` products in window order
(where xarray runs on bottleneck its running sums round differently, and its ``dot`` leaves the order to BLAS).  The Sen
slope is the median of the pair slopes over the ORIGINAL year positions with NaN years left out (``np.nanmedian``), the
Mann-Kendall score and variance are those of the series with the NaN years dropped, and fewer than two values give NaN for
both.  The thresholds of the two flow frequencies are float64 (``threshold_factor`` times the float64 median / the mean in the
field's dtype) and the comparison is made in float64.

``mask_missing=True``: a period whose count of rows with every field present differs from ``time.expected_count(freq)`` is NaN.
The default is False, the reference's index functions.

:class:`NotServed` (the adapter forwards these to the reference): non-daily or gappy axes, windows beyond
``HYDRO_MAX_WINDOW`` rows, ``sen_slope`` on more than ``SEN_MAX_YEARS`` years or with a ``freq`` that is not one of "MS", "QS-*",
"YS-*", quantiles of series beyond the selection kernels' length.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import fields as F
from . import kernels as K
from ._capi import HYDRO_MAX_WINDOW, SEN_MAX_YEARS, get_device
from .fields import FLUX_SPELLINGS, NotServed, daily_axis
from .fields import per_day as _per_day
from .timeaxis import MONTHS, TimeAxis, parse_freq

__all__ = ["base_flow_index", "rb_flashiness_index", "flow_stats", "snow_melt_we_max", "melt_and_precip_max",
           "antecedent_precipitation_index", "sen_slope", "sen_slope_ratio", "base_flow_index_seasonal_ratio", "flow_index",
           "high_flow_frequency", "low_flow_frequency", "aridity_index", "season_year_table", "api_weights", "FlowStats", "SenSlope",
           "SenSlopeRatio", "SeasonalBFI", "NotServed", "HYDRO_MAX_WINDOW", "SEN_MAX_YEARS"]

FlowStats = namedtuple("FlowStats", ["base_flow_index", "rb_flashiness_index"])
SenSlope = namedtuple("SenSlope", ["sen_slope", "p_value", "seasons"])
SenSlopeRatio = namedtuple("SenSlopeRatio", ["sen_slope", "p_value", "sen_slope_sim", "p_value_sim", "ratio", "seasons"])
SeasonalBFI = namedtuple("SeasonalBFI", ["bfi", "ratio", "seasons", "years"])


def _open(fields, time, who):
    """The admitted fields: ``(native fields, T, cell_shape, C)`` on a daily, gap-free axis."""
    got = F.native_set(fields)
    T, cell_shape, C_ = F.shape_of(got)
    daily_axis(time, T, who)
    return got, T, cell_shape, C_


def _window(window, who):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"{who}: window must be an integer of at least 1, got {window!r}")
    if window > HYDRO_MAX_WINDOW:
        raise NotServed(f"{who}: windows of up to {HYDRO_MAX_WINDOW} rows are served, got {window}")
    return int(window)


def _masked(res, valid, time, freq):
    """The MissingAny rule on downloaded results: ``valid`` (P, *cells) against the expected count of every period."""
    return F.mask_incomplete(res, valid, time.expected_count(freq))


# ---- base_flow_index / rb_flashiness_index ----------------------------------------------------------------------------
def _flow(names, q, freq, time, device, keep, mask_missing, who):
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    got, T, cell_shape, C_ = _open(dict(q=q), time, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return F.empty_result(dict.fromkeys(names, np.float64), P, cell_shape, keep, device)
    dev = device or get_device()
    outs = K.flow_period_stats(dev, F.rows_on_device(dev, got["q"], T, C_), seg, outputs=list(names) + (["valid"] if mask_missing else []))
    if keep:
        return {n: outs[n] for n in names}
    res = F.host_result(outs, P, cell_shape)
    return _masked({n: res[n] for n in names}, res["valid"], time, freq) if mask_missing else res


def base_flow_index(q, freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False, mask_missing: bool = False):
    """_hydrology.py:50-90: the minimum over the period of the centred seven-day mean flow over the period's mean flow, float64
    ``(P, *cells)``.  The seven-day window reads across period boundaries and is NaN within three rows of either end of the
    series."""
    return _flow(("bfi",), q, freq, time, device, keep, mask_missing, "base_flow_index")["bfi"]


def rb_flashiness_index(q, freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False, mask_missing: bool = False):
    """_hydrology.py:94-129: the sum of the absolute day-to-day changes of the period over the period's total flow, float64
    ``(P, *cells)``."""
    return _flow(("rbi",), q, freq, time, device, keep, mask_missing, "rb_flashiness_index")["rbi"]


def flow_stats(q, freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False, mask_missing: bool = False) -> FlowStats:
    """``FlowStats(base_flow_index, rb_flashiness_index)`` of the same ``q`` and ``freq`` from ONE launch (``q`` is read once)."""
    out = _flow(("bfi", "rbi"), q, freq, time, device, keep, mask_missing, "flow_stats")
    return FlowStats(out["bfi"], out["rbi"])


# ---- snow_melt_we_max / melt_and_precip_max ---------------------------------------------------------------------------
def _melt(snw, pr, window, freq, time, per_day, device, keep, mask_missing, who):
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    got, T, cell_shape, C_ = _open(dict(snw=snw, pr=pr), time, who)
    window = _window(window, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return F.empty_result({"out": np.float64}, P, cell_shape, keep, device)["out"]
    dev = device or get_device()
    d = {n: F.rows_on_device(dev, a, T, C_) for n, a in got.items()}
    out = K.melt_period_max(dev, d["snw"], seg, d.get("pr"), window=window, per_day=per_day)
    if keep:
        return out
    res = out.get().reshape((P,) + tuple(cell_shape))
    if mask_missing:
        valid = None
        for a in d.values():      # the rows with a value, field by field (xh_resample_reduce): every field must be complete
            v = K.resample_reduce(dev, a, "count", seg, want_valid=False)[0].get()
            valid = v if valid is None else np.minimum(valid, v)
        res = _masked({"out": res}, valid.reshape(res.shape), time, freq)["out"]
    return res


def snow_melt_we_max(snw, window: int = 3, freq: str = "YS-JUL", *, time: TimeAxis = None, device=None, keep: bool = False,
                     mask_missing: bool = False):
    """_hydrology.py:371-400: the largest snow melt (the decrease of ``snw``) accumulated over ``window`` days in each period, in the
    units of ``snw``, float64 ``(P, *cells)``."""
    return _melt(snw, None, window, freq, time, 1.0, device, keep, mask_missing, "snow_melt_we_max")


def melt_and_precip_max(snw, pr, window: int = 3, freq: str = "YS-JUL", *, time: TimeAxis = None, flux_units: str = "kg m-2 s-1",
                        device=None, keep: bool = False, mask_missing: bool = False):
    """_hydrology.py:404-440: the largest snow melt plus precipitation accumulated over ``window`` days in each period, float64
    ``(P, *cells)`` [kg m-2 with ``snw`` in kg m-2].  ``pr`` is a rate in ``flux_units``."""
    if pr is None:
        raise TypeError("melt_and_precip_max: pr is required")
    return _melt(snw, pr, window, freq, time, _per_day(flux_units), device, keep, mask_missing, "melt_and_precip_max")


# ---- antecedent_precipitation_index -----------------------------------------------------------------------------------
def api_weights(window: int, p_exp: float) -> np.ndarray:
    """The weights exactly as the reference builds them (:700-703)."""
    return np.asarray(list(reversed([p_exp ** (idx - 1) for idx in range(1, window + 1)])), np.float64)


def antecedent_precipitation_index(pr, window: int = 7, p_exp: float = 0.935, *, time: TimeAxis = None,
                                   flux_units: str = "kg m-2 s-1", device=None, keep: bool = False):
    """_hydrology.py:673-706: the trailing sum of the last ``window`` daily precipitation amounts [mm] weighted by
    ``p_exp ** age``, float64 ``(T, *cells)``; NaN until the window is full and where one of its days is NaN.  ``time`` (optional)
    is only checked to be daily and gap-free."""
    who = "antecedent_precipitation_index"
    per_day = _per_day(flux_units)
    a = F.native(pr, "pr")
    T, cell_shape, C_ = F.shape_of({"pr": a})
    if time is not None:
        daily_axis(time, T, who)
    window = _window(window, who)
    if T == 0 or C_ == 0:
        return F.empty_result({"api": np.float64}, T, cell_shape, keep, device)["api"]
    dev = device or get_device()
    out = K.antecedent_precip(dev, F.rows_on_device(dev, a, T, C_), api_weights(window, p_exp), per_day=per_day)
    return out if keep else out.get().reshape((T,) + tuple(cell_shape))


# ---- sen_slope / sen_slope_ratio / base_flow_index_seasonal_ratio -----------------------------------------------------
def season_year_table(time: TimeAxis, freq: str):
    """``split_time_to_season_year`` (core/calendar.py:1775-1802) of the periods of ``time.segments(freq)`` as a host table:
    ``(period_of (Y, K) int64, seasons, years)`` — the period that is year y of season k (-1 for none), the season labels in
    the order the reference's unstack gives them (sorted), the years ascending.  A year runs from the anchor month of ``freq``;
    ``freq`` is "MS", "QS-*" or "YS-*" (anything else: :class:`NotServed`)."""
    try:
        base, par = parse_freq(freq)
    except NotImplementedError as e:
        raise NotServed(str(e)) from None
    if base not in ("Y", "Q", "M"):
        raise NotServed(f"split_time_to_season_year: periods of {freq!r} are not served")
    _, starts = time.segments(freq)
    base_month = 1 if base == "M" else par
    letters = "JFMAMJJASOND"
    labels, years = [], []
    for y, m in starts:
        if base == "Y":
            labels.append("annual")
        elif base == "Q":
            labels.append("".join(letters[(m - 1 + i) % 12] for i in range(3)))
        else:
            labels.append(MONTHS[m - 1])
        years.append(y - 1 if m < base_month else y)
    seasons = sorted(set(labels))
    ys = np.arange(min(years), max(years) + 1) if years else np.zeros(0, np.int64)
    period_of = np.full((len(ys), len(seasons)), -1, np.int64)
    for p, (lab, y) in enumerate(zip(labels, years)):
        period_of[y - ys[0], seasons.index(lab)] = p
    return period_of, seasons, ys


def sen_slope(q, freq: str = "YS", *, time: TimeAxis = None, device=None, keep: bool = False) -> SenSlope:
    """_hydrology.py:894-944: the Theil-Sen slope and the Mann-Kendall p value of the period means of ``q`` (computed in the
    field's dtype), per season of ``freq``: ``SenSlope(sen_slope, p_value, seasons)`` with two float64 ``(K, *cells)`` arrays and
    the K season labels ("annual" for a yearly ``freq``).  Does not need pymannkendall."""
    who = "sen_slope"
    F.check_freq(freq)
    got, T, cell_shape, C_ = _open(dict(q=q), time, who)
    period_of, seasons, _ = season_year_table(time, freq)
    Y, K_ = period_of.shape
    if Y > SEN_MAX_YEARS:
        raise NotServed(f"{who}: series of up to {SEN_MAX_YEARS} years are served, got {Y}")
    if K_ == 0 or C_ == 0:
        e = F.empty_result({"slope": np.float64, "p": np.float64}, K_, cell_shape, keep, device)
        return SenSlope(e["slope"], e["p"], seasons)
    dev = device or get_device()
    means, _ = K.resample_reduce(dev, F.rows_on_device(dev, got["q"], T, C_), "mean", F.period_segments(time, freq), want_valid=False)
    outs = K.sen_slope(dev, means, period_of)
    if keep:
        return SenSlope(outs["slope"], outs["p"], seasons)
    res = F.host_result(outs, K_, cell_shape)
    return SenSlope(res["slope"], res["p"], seasons)


def sen_slope_ratio(q, qsim, freq: str = "YS", *, time: TimeAxis = None, device=None) -> SenSlopeRatio:
    """_hydrology.py:949-993: :func:`sen_slope` of the observed and of the simulated flow, and the ratio of the two slopes."""
    obs = sen_slope(q, freq, time=time, device=device)
    sim = sen_slope(qsim, freq, time=time, device=device)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = obs.sen_slope / sim.sen_slope
    return SenSlopeRatio(obs.sen_slope, obs.p_value, sim.sen_slope, sim.p_value, ratio, obs.seasons)


def base_flow_index_seasonal_ratio(q, freq: str = "QS-DEC", numerator: str = "DJF", denominator: str = "JJA", *,
                                   time: TimeAxis = None, device=None, mask_missing: bool = False) -> SeasonalBFI:
    """_hydrology.py:997-1038: the base flow index per season and year, ``bfi`` ``(K, Y, *cells)`` (NaN where the series has no
    such period), and ``ratio`` ``(Y, *cells)`` of the ``numerator`` season over the ``denominator`` season where the latter is
    positive; with the season labels and the years."""
    bfi = base_flow_index(q, freq, time=time, device=device, mask_missing=mask_missing)
    period_of, seasons, years = season_year_table(time, freq)
    for s in (numerator, denominator):
        if s not in seasons:
            raise KeyError(f"season {s!r} is not one of {seasons}")
    Y, K_ = period_of.shape
    split = np.full((K_, Y) + bfi.shape[1:], np.nan)
    for k in range(K_):
        has = period_of[:, k] >= 0
        split[k, has] = bfi[period_of[has, k]]
    den = split[seasons.index(denominator)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = split[seasons.index(numerator)] / np.where(den > 0, den, np.nan)
    return SeasonalBFI(split, ratio, seasons, years)


# ---- the indices built from the project's existing kernels --------------------------------------------------------------
_QUANTILE_MAX = {np.dtype(np.float64): 4096}      # xh_nan_quantile_f64: N <= 4096 samples per cell


def _series_quantiles(dev, x, qs, who):
    T = int(x.shape[0])
    if T > _QUANTILE_MAX.get(np.dtype(x.dtype), np.inf):
        raise NotServed(f"{who}: whole-series quantiles of float64 fields are served up to {_QUANTILE_MAX[np.dtype(x.dtype)]} rows")
    return K.nan_quantile(dev, x, qs, alpha=1.0, beta=1.0)


def flow_index(q, p: float = 0.95, *, device=None):
    """_hydrology.py:577-603: the ``p`` quantile of the whole series over its median (both NaN-skipping, linear interpolation,
    from one ``xh_nan_quantile`` call), float64 ``(*cells)``."""
    a = F.native(q, "q")
    T, cell_shape, C_ = F.shape_of({"q": a})
    if T == 0 or C_ == 0:
        return np.full(tuple(cell_shape), np.nan)
    dev = device or get_device()
    qq = _series_quantiles(dev, F.rows_on_device(dev, a, T, C_), [float(p), 0.5], "flow_index").get()
    with np.errstate(divide="ignore", invalid="ignore"):
        return (qq[0] / qq[1]).reshape(tuple(cell_shape))


def _flow_frequency(q, op, threshold_of, freq, time, device, keep, mask_missing, who):
    F.check_freq(freq)
    F.no_keep_with_mask(keep, mask_missing)
    got, T, cell_shape, C_ = _open(dict(q=q), time, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return F.empty_result({"n": np.int32}, P, cell_shape, keep, device)["n"]
    dev = device or get_device()
    x = F.rows_on_device(dev, got["q"], T, C_)
    # one threshold per cell: a one-row table that every step indexes with 0 (the day-of-year form of xh_threshold_count).  The
    # ``full=`` form would need the (1, C) row repeated into a (T, C) float64 table, twice the bytes of a float32 field.  The
    # zero index is uploaded here, as a device array, so that the call stays asynchronous
    thr = dev.to_device(np.ascontiguousarray(threshold_of(dev, x), dtype=np.float64).reshape(1, C_))
    tidx = dev.to_device(np.zeros(T, np.int32))
    count, valid = K.threshold_count(dev, x, op, seg, doy_table=thr, tidx=tidx, want_valid=mask_missing)
    if keep:
        dev.sync()      # (the two tables above are released on return)
        return count
    res = count.get().reshape((P,) + tuple(cell_shape))
    return _masked({"n": res}, valid.get().reshape(res.shape), time, freq)["n"] if mask_missing else res


def high_flow_frequency(q, threshold_factor: int = 9, freq: str = "YS-OCT", *, time: TimeAxis = None, device=None,
                        keep: bool = False, mask_missing: bool = False):
    """_hydrology.py:607-636: the days of each period with a flow above ``threshold_factor`` times the whole-series median, int32
    ``(P, *cells)`` (float64 with NaN under ``mask_missing``)."""
    who = "high_flow_frequency"
    return _flow_frequency(q, ">", lambda dev, x: threshold_factor * _series_quantiles(dev, x, [0.5], who).get()[0], freq, time, device,
                           keep, mask_missing, who)


def low_flow_frequency(q, threshold_factor: float = 0.2, freq: str = "YS-OCT", *, time: TimeAxis = None, device=None,
                       keep: bool = False, mask_missing: bool = False):
    """_hydrology.py:640-669: the days of each period with a flow below ``threshold_factor`` times the whole-series mean, int32
    ``(P, *cells)`` (float64 with NaN under ``mask_missing``)."""

    def threshold_of(dev, x):
        mean, _ = K.resample_reduce(dev, x, "mean", np.array([0, x.shape[0]], np.int64), want_valid=False)
        return threshold_factor * mean.get()[0].astype(np.float64)

    return _flow_frequency(q, "<", threshold_of, freq, time, device, keep, mask_missing, "low_flow_frequency")


def aridity_index(pr, evspsblpot, freq: str = "YS", *, time: TimeAxis = None, device=None, mask_missing: bool = False):
    """_hydrology.py:772-814: the period mean of ``pr`` over the period mean of ``evspsblpot`` (both in the same units; the means
    by ``xh_resample_reduce`` in the fields' dtype, the division on the host in float64), ``(P, *cells)``."""
    who = "aridity_index"
    F.check_freq(freq)
    got, T, cell_shape, C_ = _open(dict(pr=pr, evspsblpot=evspsblpot), time, who)
    seg = F.period_segments(time, freq)
    P = len(seg) - 1
    if P == 0 or C_ == 0:
        return np.empty((P,) + tuple(cell_shape))
    dev = device or get_device()
    means, valid = {}, None
    for n, a in got.items():
        m, v = K.resample_reduce(dev, F.rows_on_device(dev, a, T, C_), "mean", seg, want_valid=mask_missing)
        means[n] = m.get().astype(np.float64)
        if mask_missing:
            valid = v.get() if valid is None else np.minimum(valid, v.get())
    with np.errstate(divide="ignore", invalid="ignore"):
        ai = (means["pr"] / means["evspsblpot"]).reshape((P,) + tuple(cell_shape))
    return _masked({"ai": ai}, valid.reshape(ai.shape), time, freq)["ai"] if mask_missing else ai


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
ADAPTED = ("base_flow_index", "rb_flashiness_index", "snow_melt_we_max", "melt_and_precip_max", "antecedent_precipitation_index",
           "flow_index", "high_flow_frequency", "low_flow_frequency", "aridity_index", "sen_slope", "sen_slope_ratio",
           "base_flow_index_seasonal_ratio")


def make_adapters(env, originals: dict, device=None) -> dict:
    """Same-signature replacements of the functions of ``xclim.indices._hydrology`` listed in ``ADAPTED`` on DataArrays with a time
    dimension.  The precipitation's ``units`` attribute picks the kernel's ``flux_units`` (the reference's ``rate2amount`` /
    ``convert_units_to(..., "mm")`` for a daily series); the result keeps the cell dimensions and coordinates of the first
    field, has the period starts of ``resample(time=freq)`` as its time coordinate (the field's own for the antecedent
    precipitation index; for the Sen slopes a trailing ``season`` dimension with the attributes of ``add_season_coord``; for the
    seasonal base flow index a trailing yearly ``time`` — (year, anchor month, 1) in the field's calendar, as
    ``split_time_to_season_year`` labels it — and ``season``) and the units and attributes the reference gives it.
    Chunked or time-less fields, fields on different dimensions, units this module has no keyword for and everything
    :class:`NotServed` refuses go to the saved originals."""
    import re

    from .xr_adapter import _cell_coords, _cell_dims, _wrap_cells, forwarding_adapter, on_period_starts, served_fields, units_keyword

    DA = env.DataArray

    def _cells(a, values, attrs, tail=None):
        """``values`` (*cells, *tail) on the cell dimensions of ``a`` followed by the trailing ``(dim, coordinate)`` pairs: the
        reference's ``unstack`` puts the yearly ``time`` and ``season`` behind the dimensions the field had."""
        tail = tail or []
        coords = dict(_cell_coords(a))
        coords.update({d: c for d, c in tail})
        return DA(np.asarray(values), coords=coords, dims=_cell_dims(a) + tuple(d for d, _ in tail), attrs=attrs)

    def _bfi(p):
        a, v, t = served_fields(DA, p, ("q",))
        return on_period_starts(DA, a, base_flow_index(v["q"], p["freq"], time=t, device=device), p["freq"], {"units": ""})

    def _rbi(p):
        a, v, t = served_fields(DA, p, ("q",))
        return on_period_starts(DA, a, rb_flashiness_index(v["q"], p["freq"], time=t, device=device), p["freq"], {"units": ""})

    def _swe(p):
        a, v, t = served_fields(DA, p, ("snw",))
        return on_period_starts(DA, a, snow_melt_we_max(v["snw"], p["window"], p["freq"], time=t, device=device), p["freq"],
                                {"units": p["snw"].attrs.get("units", "")})

    def _mpm(p):
        a, v, t = served_fields(DA, p, ("snw", "pr"))
        flux = units_keyword(p["pr"], FLUX_SPELLINGS, "pr")
        out = melt_and_precip_max(v["snw"], v["pr"], p["window"], p["freq"], time=t, flux_units=flux, device=device)
        return on_period_starts(DA, a, out, p["freq"], {"units": p["snw"].attrs.get("units", "")})

    def _api(p):
        a, v, t = served_fields(DA, p, ("pr",))
        flux = units_keyword(p["pr"], FLUX_SPELLINGS, "pr")
        out = antecedent_precipitation_index(v["pr"], p["window"], p["p_exp"], time=t, flux_units=flux, device=device)
        return _wrap_cells(DA, a, out, a["time"], {"units": "mm"})

    def _fi(p):
        a, v, _ = served_fields(DA, p, ("q",))
        return _cells(a, flow_index(v["q"], p["p"], device=device), {"units": "1"})

    def _hff(p):
        a, v, t = served_fields(DA, p, ("q",))
        out = on_period_starts(DA, a, high_flow_frequency(v["q"], p["threshold_factor"], p["freq"], time=t, device=device), p["freq"], {})
        return env.to_agg_units(out, p["q"], "count")

    def _lff(p):
        a, v, t = served_fields(DA, p, ("q",))
        out = on_period_starts(DA, a, low_flow_frequency(v["q"], p["threshold_factor"], p["freq"], time=t, device=device), p["freq"], {})
        return env.to_agg_units(out, p["q"], "count")

    def _ai(p):
        a, v, t = served_fields(DA, p, ("pr", "evspsblpot"))
        if str(p["pr"].attrs.get("units", "")).strip() != str(p["evspsblpot"].attrs.get("units", "")).strip():
            raise NotServed("pr and evspsblpot in different units")
        return on_period_starts(DA, a, aridity_index(v["pr"], v["evspsblpot"], p["freq"], time=t, device=device), p["freq"], {"units": ""})

    def _split_freq(freq):
        """(base, anchor) of a start-anchored ``freq`` the season split serves ("MS", "QS[-MMM]", "YS[-MMM]" / "AS[-MMM]")."""
        m = re.fullmatch(r"(MS)|(?:(QS|YS|AS)(?:-([A-Z]{3}))?)", str(freq).upper())
        if m is None or (m.group(3) is not None and m.group(3) not in MONTHS):
            raise NotServed(f"split_time_to_season_year: {freq!r}")
        return ("M" if m.group(1) else m.group(2)[0].replace("A", "Y")), (m.group(3) or "JAN")

    def _season(seasons, freq):
        """The ``season`` coordinate with the attributes of ``add_season_coord`` (core/calendar.py:1770-1772)."""
        base, anchor = _split_freq(freq)
        attrs = dict(mult=1, base=base, isstart=True, anchor=anchor, season_length=len(seasons[0]) if base != "M" else 1)
        return ("season", DA(np.asarray(seasons, dtype=object), dims=("season",), attrs=attrs))

    def _years(a, freq, n):
        """The yearly ``time`` coordinate of ``split_time_to_season_year`` (:1796-1802): (year, anchor month, 1) in the calendar of
        the field, which is what a yearly resampling from the anchor month labels its bins with."""
        _, anchor = _split_freq(freq)
        years = a["time"].resample(time=f"YS-{anchor}").first()["time"]
        if len(years.values) != n:
            raise NotServed("split_time_to_season_year: years")
        return ("time", years)

    def _last(x, n=1):
        """The ``n`` leading axes of a mirror's result moved behind the cell axes."""
        return np.moveaxis(np.asarray(x), list(range(n)), list(range(-n, 0)))

    def _sen(p):
        a, v, t = served_fields(DA, p, ("q",))
        _split_freq(p["freq"])
        s = sen_slope(v["q"], p["freq"], time=t, device=device)
        season = _season(s.seasons, p["freq"])
        return tuple(_cells(a, _last(x), {"units": ""}, [season]) for x in (s.sen_slope, s.p_value))

    def _senr(p):
        a, v, t = served_fields(DA, p, ("q", "qsim"))
        _split_freq(p["freq"])
        s = sen_slope_ratio(v["q"], v["qsim"], p["freq"], time=t, device=device)
        season = _season(s.seasons, p["freq"])
        return tuple(_cells(a, _last(x), {"units": ""}, [season]) for x in s[:5])

    def _bfis(p):
        a, v, t = served_fields(DA, p, ("q",))
        _split_freq(p["freq"])
        seasons = season_year_table(t, p["freq"])[1]
        if p["numerator"] not in seasons or p["denominator"] not in seasons:
            raise NotServed("a season the series does not have: the reference raises its own error")
        s = base_flow_index_seasonal_ratio(v["q"], p["freq"], p["numerator"], p["denominator"], time=t, device=device)
        years = _years(a, p["freq"], len(s.years))
        bfi = _cells(a, _last(np.swapaxes(s.bfi, 0, 1), 2), {"units": ""}, [years, _season(s.seasons, p["freq"])])
        ratio = _cells(a, _last(s.ratio), {"units": "", "denominator": p["denominator"], "numerator": p["numerator"]}, [years])
        return bfi, ratio

    runners = {"base_flow_index": _bfi, "rb_flashiness_index": _rbi, "snow_melt_we_max": _swe, "melt_and_precip_max": _mpm,
               "antecedent_precipitation_index": _api, "flow_index": _fi, "high_flow_frequency": _hff, "low_flow_frequency": _lff,
               "aridity_index": _ai, "sen_slope": _sen, "sen_slope_ratio": _senr, "base_flow_index_seasonal_ratio": _bfis}

    return {name: forwarding_adapter(name, originals[name], runners[name]) for name in ADAPTED}
