"""numpy restatement of ``rain_season`` (reference: src/xclim/indices/_agro.py:796-980) and ``hardiness_zones`` (:1388-1433 with
``get_zones``, src/xclim/indices/generic.py:1611-1708), written from reading them — the oracle of tests/test_rain_cpu.py and
tests/test_gpu_rain.py (test infrastructure only; the reference's own code needs xarray, which the tests do not).

It follows the reference step by step, whole arrays at a time, on top of the oracle's ``rle`` and ``runs_with_holes``
(oracle/run_length.py): per period a ``select_time`` of the amounts, one or two rolling sums, ``runs_with_holes``, ``rle``,
``_get_first_run`` (argmax against argmin over the rows inside the date bounds), a masked copy, a second ``rle`` or rolling sum,
``_get_first_run`` again.  Fields are (T, C) with time on axis 0; the date selections are made per period with
``xclim_amd.calendar.select_time_mask`` on the period's own rows, as ``resample(time=freq).map`` does.

A rolling sum adds its window in row order from its first term (the repository's standing choice; where xarray runs on
bottleneck its running sum rounds differently), in float64 on the widened field."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import run_length as orl  # noqa: E402
from xclim_amd.calendar import select_time_mask  # noqa: E402

DAY = 86400.0
PER_DAY = {"kg m-2 s-1": DAY, "mm/s": DAY, "mm/d": 1.0}
DEFAULTS = dict(thresh_wet_start=25.0, window_wet_start=3, window_not_dry_start=30, thresh_dry_start=1.0, window_dry_start=7,
                method_dry_start="per_day", date_min_start="05-01", date_max_start="12-31", thresh_dry_end=0.0, window_dry_end=20,
                method_dry_end="per_day", date_min_end="09-01", date_max_end="12-31")


def rollsum(a, w):
    """``rolling(time=w).sum()`` with ``min_periods = w``: NaN for the first w - 1 rows and wherever a term is NaN; the terms
    are added oldest first."""
    n = a.shape[0]
    out = np.full(a.shape, np.nan)
    if n >= w:
        acc = a[0:n - w + 1].astype(np.float64)
        for k in range(1, w):
            acc = acc + a[k:n - w + 1 + k]
        out[w - 1:] = acc
    return out


def first_run(pos, inb):
    """``_get_first_run``: ``pos`` (n, C) bool, ``inb`` (n) the rows inside the date bounds.  argmax over the rows in bounds
    where it differs from argmin, NaN otherwise (no true row, or no false one)."""
    idx = np.flatnonzero(inb)
    if idx.size == 0:
        raise ValueError("no row inside the date bounds: xarray's argmax raises on an all-NaN slice")
    v = pos[idx]
    amax, amin = idx[np.argmax(v, axis=0)], idx[np.argmin(v, axis=0)]
    return np.where(amax != amin, amax.astype(np.float64), np.nan)


def rain_season_period(a, m_window, m_start, m_end, *, thresh_wet_start=25.0, window_wet_start=3, window_not_dry_start=30,
                       thresh_dry_start=1.0, window_dry_start=7, method_dry_start="per_day", thresh_dry_end=0.0, window_dry_end=20,
                       method_dry_end="per_day"):
    """One period: ``a`` (n, C) daily amounts in mm, the three row masks (n).  Returns the ROW of the start and of the end within
    the period and the length, float64 (C) with NaN."""
    a = np.asarray(a, np.float64)
    n, C = a.shape
    P = np.where(m_window[:, None], a, np.nan)                                     # _agro.py:906
    with np.errstate(invalid="ignore"):
        wet = rollsum(P, window_wet_start) >= thresh_wet_start                      # :909
        if method_dry_start == "per_day":                                           # :912-914
            stop, window_dry = P <= thresh_dry_start, window_dry_start
        elif method_dry_start == "total":                                           # :915-919
            late = rollsum(P, window_dry_start) <= thresh_dry_start
            stop = np.zeros((n, C), bool)
            k = window_dry_start - 1
            if n > k:
                stop[:n - k] = late[k:]                                             # shift(-(window - 1), fill_value=False)
            window_dry = 1
        else:
            raise ValueError(f"Unknown method_dry_start: {method_dry_start}.")
        events = orl.runs_with_holes(wet, 1, stop, window_dry)                      # :924
        pos = orl.rle(events) >= (window_not_dry_start + window_wet_start)         # :925
    start = first_run(pos, m_start)                                                 # :927
    rows = np.arange(n)[:, None]
    with np.errstate(invalid="ignore"):
        a2 = np.where(rows > start[None, :], a, np.nan)                             # :950-957 (NaN start: nothing is kept)
        if method_dry_end == "per_day":                                             # :932-934
            pos2 = orl.rle(a2 <= thresh_dry_end) >= window_dry_end
        elif method_dry_end == "total":                                             # :935-936
            pos2 = rollsum(a2, window_dry_end) <= thresh_dry_end
        else:
            raise ValueError(f"Unknown method_dry_end: {method_dry_end}.")
    end = first_run(pos2, m_end)                                                    # :939
    length = np.where(np.isnan(end), n - start, end - start)                        # :959
    return start, end, length


def period_masks(time, rows, date_min_start, date_max_start, date_min_end, date_max_end):
    """The three selections of one period, made on the period's own rows: inside (date_min_start, the month-day of the last
    row), inside the start bounds, inside the end bounds."""
    sub = time.subset(rows)
    last = f"{int(sub.month[-1]):02d}-{int(sub.day[-1]):02d}"                       # :905
    return (select_time_mask(sub, date_bounds=(date_min_start, last)), select_time_mask(sub, date_bounds=(date_min_start, date_max_start)),
            select_time_mask(sub, date_bounds=(date_min_end, date_max_end)))


def rain_season(pr, time, freq="YS-JAN", flux_units="mm/d", **kw):
    """(start, end, length), float64 (P, C): the day of year of the start and of the end, and the length in days."""
    p = dict(DEFAULTS, **kw)
    dates = {k: p.pop(k) for k in ("date_min_start", "date_max_start", "date_min_end", "date_max_end")}
    a = np.asarray(pr).astype(np.float64) * PER_DAY[flux_units]                    # rate2amount
    seg = np.asarray(time.segments(freq)[0])
    out = np.full((3, len(seg) - 1, a.shape[1]), np.nan)
    for k in range(len(seg) - 1):
        rows = slice(int(seg[k]), int(seg[k + 1]))
        if rows.stop == rows.start:
            continue
        mw, ms, me = period_masks(time, rows, **dates)
        start, end, length = rain_season_period(a[rows], mw, ms, me, **p)
        doy = time.doy[rows].astype(np.float64)
        for j, v in enumerate((start, end)):
            ok = ~np.isnan(v)
            out[j, k, ok] = doy[v[ok].astype(int)]                                  # lazy_indexing(dayofyear, ...)  :962-964
        out[2, k] = length
    return out[0], out[1], out[2]


def rain_season_flags(pr, seg, flags, doy, flux_units="mm/d", **kw):
    """The same from the kernel's own inputs: the flag byte (bit 0 the start window, bit 1 the start bounds, bit 2 the end bounds)
    and the day of year of every row."""
    p = dict({k: v for k, v in DEFAULTS.items() if not k.startswith("date_")}, **kw)
    a = np.asarray(pr).astype(np.float64) * PER_DAY[flux_units]
    flags, doy = np.asarray(flags), np.asarray(doy, np.float64)
    out = np.full((3, len(seg) - 1, a.shape[1]), np.nan)
    for k in range(len(seg) - 1):
        rows = slice(int(seg[k]), int(seg[k + 1]))
        if rows.stop == rows.start:
            continue
        f = flags[rows]
        start, end, length = rain_season_period(a[rows], (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, **p)
        for j, v in enumerate((start, end)):
            ok = ~np.isnan(v)
            out[j, k, ok] = doy[rows][v[ok].astype(int)]
        out[2, k] = length
    return out[0], out[1], out[2]


def margin(pr, seg, flags, flux_units, **kw):
    """Per column: the smallest relative distance |s - t| / |t| between a threshold t (non-zero) and any sum s the decisions
    compare with it — every window sum of the start window's amounts and of the amounts, and every single amount where the method
    is "per_day".  An answer cannot depend on the order or the precision of the additions while this stays above their error."""
    p = dict({k: v for k, v in DEFAULTS.items() if not k.startswith("date_")}, **kw)
    a = np.asarray(pr).astype(np.float64) * PER_DAY[flux_units]
    best = np.full(a.shape[1], np.inf)
    for k in range(len(seg) - 1):
        rows = slice(int(seg[k]), int(seg[k + 1]))
        if rows.stop == rows.start:
            continue
        x = a[rows]
        P = np.where(((np.asarray(flags)[rows] & 1) != 0)[:, None], x, np.nan)
        pairs = [(rollsum(P, p["window_wet_start"]), p["thresh_wet_start"]),
                 (rollsum(P, p["window_dry_start"]) if p["method_dry_start"] == "total" else P, p["thresh_dry_start"]),
                 (rollsum(x, p["window_dry_end"]) if p["method_dry_end"] == "total" else x, p["thresh_dry_end"])]
        for s, t in pairs:
            assert t != 0
            d = np.abs(s - t) / abs(t)
            best = np.minimum(best, np.where(np.isnan(d), np.inf, d).min(axis=0, initial=np.inf))
    return best


# ---- hardiness_zones ------------------------------------------------------------------------------------------------------
KELVIN_OFFSET = 273.15


def zone_edges(method, units):
    """The bin edges of ``_get_zone_bins`` in ``units`` ("K" or "degC"): -60 .. 70 degF or -15 .. 20 degC in steps of 5."""
    if method.lower() == "usda":
        f = np.arange(-60.0, 70.0 + 5.0, 5.0)
        k = (f + 459.67) * 5.0 / 9.0
        return k if units == "K" else k - KELVIN_OFFSET
    if method.lower() == "anbg":
        c = np.arange(-15.0, 20.0 + 5.0, 5.0)
        return c + KELVIN_OFFSET if units == "K" else c
    raise NotImplementedError(f"Method must be one of `usda` or `anbg`. Got {method}.")


def get_zones(x, edges):
    """generic.py:1698-1706 with the defaults: digitize - 1, the last zone closed on the right, NaN outside the edges."""
    x = np.asarray(x, np.float64)
    edges = np.asarray(edges, np.float64)
    z = (np.digitize(x, edges) - 1).astype(np.float64)
    z = np.where(x != edges[-1], z, np.digitize(edges[-2], edges) - 1)
    keep = (z != np.digitize(edges[0] - 1, edges) - 1) & (z != np.digitize(edges[-1], edges) - 1)
    return np.where(keep, z, np.nan)


def rolling_zones(x, window, edges):
    """The zones of the mean of the last ``window`` rows of ``x`` (P, C): the sum in row order over ``window``."""
    return get_zones(rollsum(np.asarray(x).astype(np.float64), window) / window, edges)


def period_min(x, seg):
    """``tn_min``: the NaN-skipping minimum of every period, in the field's dtype; NaN for a period without a value."""
    x = np.asarray(x)
    out = np.full((len(seg) - 1, x.shape[1]), np.nan, x.dtype)
    for k in range(len(seg) - 1):
        rows = x[int(seg[k]):int(seg[k + 1])]
        has = (~np.isnan(rows)).any(axis=0)
        if rows.shape[0] and has.any():
            out[k, has] = np.nanmin(rows[:, has], axis=0)
    return out


def hardiness_zones(tasmin, time, window=30, method="usda", freq="YS", units="K"):
    edges = zone_edges(method, units)
    return rolling_zones(period_min(tasmin, time.segments(freq)[0]), window, edges)
