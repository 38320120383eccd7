"""numpy restatement of the seven bodies of the compound-extreme unit, written from reading them — ``cold_and_dry_days``,
``warm_and_dry_days``, ``warm_and_wet_days``, ``cold_and_wet_days`` (reference: src/xclim/indices/_multivariate.py:162-423),
``degree_days_exceedance_date`` (src/xclim/indices/_threshold.py:3215-3310), ``blowing_snow`` (_multivariate.py:1833-1884) and
``water_cycle_intensity`` (:1888-1918) — the oracle of tests/test_compound_cpu.py and tests/test_gpu_compound.py (test
infrastructure only; the reference's own code needs xarray, which the tests do not).

It follows the reference step by step, whole arrays at a time, on the oracle's time axis (``oracle.timeutil.OTime``) and on the
pieces the oracle already restates: ``oracle.calendar.resample_doy`` (the (T, cells) float64 threshold field the reference
makes), ``oracle.calendar.select_time_mask``, ``oracle.run_length.first_run_after_date`` (with ``find_boundary_run``'s
``argmax != argmin``) and its ``index_of_date``.  Fields are (T, C) with time on axis 0.

Sums are float64 on the widened fields and are added in row order: ``np.nancumsum`` along axis 0, a rolling sum from its first
term (the repository's standing choice; where xarray runs on bottleneck its running sum rounds differently), the period sum of
``water_cycle_intensity`` one row after the other."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import calendar as ocal  # noqa: E402
from oracle import run_length as orl  # noqa: E402
from oracle.timeutil import OTime, groups  # noqa: E402

DAY = 86400.0
PER_DAY = {"kg m-2 s-1": DAY, "mm/s": DAY, "mm/d": 1.0}
# name -> (compare of tas with its table, compare of pr with its table)
COMPOUND = {"cold_and_dry_days": (np.less, np.less), "warm_and_dry_days": (np.greater, np.less),
            "warm_and_wet_days": (np.greater, np.greater), "cold_and_wet_days": (np.less, np.greater)}
_BELOW, _ABOVE = ("<", "lt", "<=", "le"), (">", "gt", ">=", "ge")
_CUM = np.array([0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334])


def otime(calendar, start, n) -> OTime:
    """The oracle's axis of ``n`` days from ``start`` ("YYYY-MM-DD"; other calendars than standard start on a 1 January)."""
    if calendar == "standard":
        return OTime.standard(start, n)
    y, m, d = (int(v) for v in start.split("-"))
    assert (m, d) == (1, 1), "the oracle's noleap / 360_day axes start on a 1 January"
    return OTime.noleap(y, n, calendar)


def isel(time: OTime, idx) -> OTime:
    return time.isel(idx)


def doy_from_string(date, year, calendar):
    """core/calendar.py:114-135."""
    parts = date.split("-")
    if len(parts) != 2:
        raise ValueError("Day of year must be in the format 'MM-DD'.")
    m, d = int(parts[0]), int(parts[1])
    if calendar == "360_day":
        return (m - 1) * 30 + d
    leap = calendar == "standard" and ((year % 4 == 0 and year % 100 != 0) or year % 400 == 0)
    return int(_CUM[m - 1]) + d + (1 if leap and m > 2 else 0)


def compound_days(name, tas, pr, tas_per, pr_per, time: OTime, freq="YS", tas_doys=None, pr_doys=None):
    """_multivariate.py:208-219 (and the three siblings): ``resample_doy`` of both tables, two compares (a NaN on either side is
    False), ``logical_and``, ``resample(freq).sum``.  ``tas_per`` / ``pr_per``: (ndoy, C) float64 on the days of year
    ``tas_doys`` / ``pr_doys`` (default 1 .. ndoy).  float64 (P, C)."""
    t_op, p_op = COMPOUND[name]
    tas_doys = np.arange(1, len(tas_per) + 1) if tas_doys is None else np.asarray(tas_doys)
    pr_doys = np.arange(1, len(pr_per) + 1) if pr_doys is None else np.asarray(pr_doys)
    with np.errstate(invalid="ignore"):
        a = t_op(np.asarray(tas), ocal.resample_doy(np.asarray(tas_per, np.float64), tas_doys, time))
        b = p_op(np.asarray(pr), ocal.resample_doy(np.asarray(pr_per, np.float64), pr_doys, time))
    both = np.logical_and(a, b)
    return np.stack([both[idx].sum(axis=0) for _, idx in groups(time, freq)]).astype(np.float64)


def degree_days_exceedance_date(tas, time: OTime, thresh, sum_thresh=25.0, op=">", after_date=None, never_reached=None, freq="YS"):
    """_threshold.py:3277-3310 with ``thresh`` in the units of ``tas``: per period ``index_of_date`` (a period without the date
    is NaN), ``where(time >= start).cumsum`` (NaN skipped), ``first_run_after_date(cumsum > sum_thresh, window=1, date=None)`` as
    a day of year, and the ``never_reached`` replacement where ``cumsum <= sum_thresh`` on ALL rows.  float64 (P, C)."""
    x = np.asarray(tas).astype(np.float64)
    if op in _BELOW:
        c = thresh - x
    elif op in _ABOVE:
        c = x - thresh
    else:
        raise NotImplementedError(f"op: '{op}'.")
    with np.errstate(invalid="ignore"):
        c = np.where(c < 0, 0.0, c)    # clip(0): NaN stays NaN
    rows = []
    for _, idx in groups(time, freq):
        grp, t = c[idx], time.isel(idx)
        strt = orl._date_index(t, after_date)
        strt = np.array([0]) if strt is None else strt
        if strt.size == 0 or len(idx) == 0:
            rows.append(np.full(c.shape[1:], np.nan))
            continue
        assert strt.size == 1, "max_idxs=1"
        g = grp.copy()
        g[:strt[0]] = np.nan
        cumsum = np.nancumsum(g, axis=0)
        first = orl.first_run_after_date((cumsum > sum_thresh).astype(np.float64), 1, None, t)
        out = np.full(first.shape, np.nan)
        ok = ~np.isnan(first)
        out[ok] = np.asarray(t.doy)[first[ok].astype(np.int64)]
        if never_reached is not None:
            val = doy_from_string(never_reached, int(t.year[0]), time.calendar) if isinstance(never_reached, str) else never_reached
            out = np.where((cumsum <= sum_thresh).all(axis=0), float(val), out)
        rows.append(out)
    return np.stack(rows)


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


def blowing_snow_sums(snd, window):
    """``snd.diff("time").rolling(time=window).sum()`` on the rows 1 .. T - 1 (:1875)."""
    return rollsum(np.diff(np.asarray(snd).astype(np.float64), axis=0), window)


def blowing_snow(snd, sfcWind, time: OTime, snd_thresh, sfcWind_thresh, window=3, freq="YS-JUL", **indexer):
    """_multivariate.py:1871-1884 with the thresholds in the units of the fields: the window sums of the differences,
    ``select_time`` on both sides (unselected rows become NaN, after the sum), two compares, a product, ``resample(freq).sum`` over
    the rows 1 .. T - 1, which are the rows of ``diff``.  float64 (P', C)."""
    snow = blowing_snow_sums(snd, window)
    w = np.asarray(sfcWind).astype(np.float64)
    if indexer:
        m = ocal.select_time_mask(time, **indexer)
        snow = np.where(m[1:, None], snow, np.nan)
        w = np.where(m[:, None], w, np.nan)
    with np.errstate(invalid="ignore"):
        cond = (snow >= snd_thresh) * (w[1:] >= sfcWind_thresh) * 1
    t1 = time.isel(slice(1, None))
    return np.stack([cond[idx].sum(axis=0) for _, idx in groups(t1, freq)]).astype(np.float64) if len(t1) else np.zeros((0,) + cond.shape[1:])


def water_cycle_intensity(pr, evspsbl, time: OTime, freq="YS", flux_units="kg m-2 s-1"):
    """_multivariate.py:1912-1918 for fields in one unit: ``(pr + evspsbl)``, ``rate2amount`` on a daily axis (times the seconds of
    a day), ``resample(freq).sum`` (NaN skipped, 0 without a term).  float64 (P, C), added row after row."""
    amount = (np.asarray(pr).astype(np.float64) + np.asarray(evspsbl).astype(np.float64)) * PER_DAY[flux_units]
    rows = []
    for _, idx in groups(time, freq):
        s = np.zeros(amount.shape[1:])
        for i in idx:
            s = s + np.where(np.isnan(amount[i]), 0.0, amount[i])
        rows.append(s)
    return np.stack(rows)


# ---- the conditions of the fixtures ------------------------------------------------------------------------------------------
def _rel_gap(a, b):
    """The smallest |a - b| / max(|a|, |b|) over the pairs that are not NaN (inf without one)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    ok = ~(np.isnan(a) | np.isnan(b))
    if not ok.any():
        return np.inf
    scale = np.maximum(np.abs(a[ok]), np.abs(b[ok]))
    scale[scale == 0] = 1.0
    return float((np.abs(a[ok] - b[ok]) / scale).min())


def compound_margin(tas, pr, tables: dict, time: OTime):
    """The smallest relative gap between a field value and its table value: ``tables`` {"tas_lo" / "tas_hi" / "pr_lo" / "pr_hi":
    (ndoy, C)} on the days of year 1 .. ndoy."""
    gaps = []
    for k, tab in tables.items():
        thr = ocal.resample_doy(np.asarray(tab, np.float64), np.arange(1, len(tab) + 1), time)
        gaps.append(_rel_gap(np.asarray(tas if k.startswith("tas") else pr), thr))
    return min(gaps)


def exceedance_margin(tas, time: OTime, thresh, sum_thresh, op=">", after_date=None, freq="YS"):
    """The smallest relative gap between a running sum and ``sum_thresh``, over every row from the start of every period."""
    x = np.asarray(tas).astype(np.float64)
    c = thresh - x if op in _BELOW else x - thresh
    with np.errstate(invalid="ignore"):
        c = np.where(c < 0, 0.0, c)
    gaps = []
    for _, idx in groups(time, freq):
        strt = orl._date_index(time.isel(idx), after_date)
        strt = np.array([0]) if strt is None else strt
        if strt.size == 0 or len(idx) == 0:
            continue
        gaps.append(_rel_gap(np.nancumsum(c[idx][strt[0]:], axis=0), sum_thresh))
    return min(gaps)


def blowing_snow_margin(snd, sfcWind, snd_thresh, sfcWind_thresh, window):
    """The smallest relative gap between a window sum and ``snd_thresh`` and between a wind speed and ``sfcWind_thresh``."""
    return min(_rel_gap(blowing_snow_sums(snd, window), snd_thresh), _rel_gap(np.asarray(sfcWind), sfcWind_thresh))
