"""Writes tests/golden/rain_vectors.npz from the numpy restatement tests/raincpu.py: precipitation columns built for the decisions
of ``rain_season`` (one family per decision), the flag byte of every row, and the restatement's start, end and length.  Run from
the repository root: ``python tests/golden/make_rain_golden.py``.

Every amount of the built families lies on a 0.25 mm grid in "mm/d": every window sum is then exact in any order and in either
precision, so the expected values do not depend on the order of the additions or on float32 arithmetic.  The last family is
random float32 "kg m-2 s-1" fields; for it the generator keeps only columns whose every window sum (and every single amount
compared with a per-day threshold) stays 1e-6 relative away from its threshold (``raincpu``-side check: ``margin``).

Families (``family`` in the meta of a case; the columns of a case are listed in ``columns``):
  reach     wet spells followed by dry sequences one row short of, and exactly reaching, window_dry_start (at the row that makes
            the event run one row short of, and exactly, window_not_dry_start + window_wet_start), and the same for window_dry_end
  nan       a NaN row inside the wet window, inside the dry sequence of the start and inside the dry sequence of the end
  same_row  a stop and a start marker on the same rows (the wet amounts are themselves below thresh_dry_start)
  bounds    hand-made flags: candidates on rows outside the start bounds followed by one inside; a single row in bounds that is
            a candidate (argmax == argmin); a dry sequence that ends the season before date_min_end followed by one after it
  none      no start at all; a start without an end
  random    random float32 fields in kg m-2 s-1
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import raincpu as R  # noqa: E402
from xclim_amd import rainseason  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

AXES = {
    # one period; three periods with a leap year and a short last one; a July year with wrapping bounds and a 29 February
    "one": dict(start="2001-01-01", T=365, calendar="standard", freq="YS-JAN",
                dates=dict(date_min_start="02-10", date_max_start="09-30", date_min_end="06-01", date_max_end="12-31")),
    "three": dict(start="1999-01-01", T=365 + 366 + 200, calendar="standard", freq="YS-JAN",
                  dates=dict(date_min_start="02-10", date_max_start="06-30", date_min_end="04-15", date_max_end="12-31")),
    "july": dict(start="1999-07-01", T=366 + 365 + 150, calendar="standard", freq="YS-JUL",
                 dates=dict(date_min_start="08-15", date_max_start="03-15", date_min_end="10-01", date_max_end="06-30")),
    "noleap": dict(start="2001-01-01", T=365, calendar="noleap", freq="YS-JAN",
                   dates=dict(date_min_start="01-01", date_max_start="12-31", date_min_end="01-01", date_max_end="12-31")),
}


def params(ww=3, wnd=10, wd=7, we=5, ms="per_day", me="per_day", tw=25.0, td=1.0, te=0.5):
    return dict(thresh_wet_start=tw, window_wet_start=ww, window_not_dry_start=wnd, thresh_dry_start=td, window_dry_start=wd,
                method_dry_start=ms, thresh_dry_end=te, window_dry_end=we, method_dry_end=me)


PSETS = {"default": params(3, 30, 7, 20, te=0.0)}
for _ms in ("per_day", "total"):
    for _me in ("per_day", "total"):
        PSETS[f"{_ms}.{_me}"] = params(ms=_ms, me=_me)
for _w in (1, 2, 32):
    PSETS[f"ww{_w}"] = params(ww=_w, tw=25.0 if _w < 32 else 100.0)     # (32 moist rows must not add up to a wet window)
    PSETS[f"wd{_w}.total"] = params(wd=_w, ms="total")
    PSETS[f"we{_w}.total"] = params(we=_w, me="total")
    PSETS[f"wd{_w}.per_day"] = params(wd=_w)
PSETS["wd33.per_day"] = params(wd=33, we=6)          # a per-day dry window beyond the ring: the decision row is read twice
PSETS["wd40.we40.per_day"] = params(wd=40, we=40)
PSETS["all32.total"] = params(ww=32, wd=32, we=32, ms="total", me="total", tw=100.0)   # the largest ring


def up4(x):
    return np.ceil(x * 4 - 1e-9) / 4


class Blocks:
    """Rows on the 0.25 mm grid for one parameter set."""

    def __init__(self, p):
        self.p = p
        self.ww, self.wd, self.we = p["window_wet_start"], p["window_dry_start"], p["window_dry_end"]
        self.N = p["window_not_dry_start"] + self.ww
        self.hw = float(up4(p["thresh_wet_start"] / self.ww))                 # ww of them reach thresh_wet_start
        self.m = max(p["thresh_dry_start"], p["thresh_dry_end"]) + 0.25      # neither dry for the start nor for the end
        self.end_from = self.end_pos = 0

    def wet(self):
        return [self.hw] * self.ww

    def moist(self, k):
        return [self.m] * max(k, 0)

    def dry_start(self, k):
        """k rows that are a dry sequence for the start when k == wd: each <= thresh_dry_start / their sum == thresh_dry_start."""
        if self.p["method_dry_start"] == "per_day":
            return [self.p["thresh_dry_start"]] * k
        return ([self.p["thresh_dry_start"]] + [0.0] * (k - 1)) if k else []

    def dry_end(self, k):
        if self.p["method_dry_end"] == "per_day":
            return [self.p["thresh_dry_end"]] * k
        return ([0.0] * (k - 1) + [self.p["thresh_dry_end"]]) if k else []


def column(n, at, rows):
    """n rows of NaN with ``rows`` from row ``at`` on (cut at the period's end)."""
    c = np.full(n, np.nan)
    rows = np.asarray(rows, np.float64)[:max(n - at, 0)]
    c[at:at + len(rows)] = rows
    return c


def season(b, n, at, run=None, stop=None, gap=6, end=None, tail=True):
    """A wet spell at ``at``; an event run that a dry sequence of ``stop`` rows cuts at ``run`` rows (None: no cut before the
    run has N + gap rows); then, not before row ``b.end_from``, a dry sequence of ``end`` rows for the end (``b.end_pos`` is its
    first row afterwards); moist rows to the end of the period."""
    rows = b.wet()
    if run is not None:
        rows += b.moist(run - 1) + b.dry_start(stop) + b.moist(3)
    else:
        rows += b.moist(b.N + gap)
    if end is not None:
        rows += b.moist(b.end_from - at - len(rows))
        b.end_pos = at + len(rows)
        rows += b.dry_end(end) + b.moist(2)
    if tail:
        rows += b.moist(n)
    return column(n, at, rows)


def family_reach(b, n, s0):
    cols = {}
    cols["run N-1: cut one row early"] = season(b, n, s0, run=b.N - 1, stop=b.wd, end=b.we)
    cols["run N: cut on the row after"] = season(b, n, s0, run=b.N, stop=b.wd, end=b.we)
    cols["dry sequence one row short"] = season(b, n, s0, run=max(b.N - 3, 1), stop=b.wd - 1, end=b.we)
    cols["end one row short"] = season(b, n, s0, end=b.we - 1)
    cols["end exact"] = season(b, n, s0, end=b.we)
    cols["end one row longer"] = season(b, n, s0, end=b.we + 1)
    cols["failed candidate, then a season"] = np.where(np.arange(n) < s0 + b.ww + b.N + b.wd + 4,
                                                       season(b, n, s0, run=b.N - 1, stop=b.wd, tail=False),
                                                       season(b, n, s0 + b.ww + b.N + b.wd + 4, end=b.we))
    return cols


def family_nan(b, n, s0):
    cols = {}
    c = season(b, n, s0, end=b.we)
    c[s0 + b.ww // 2] = np.nan
    cols["NaN in the wet window"] = c
    c = season(b, n, s0, run=max(b.N - 2, 1), stop=b.wd, end=b.we)
    c[s0 + b.ww + max(b.N - 2, 1) - 1 + b.wd // 2] = np.nan
    cols["NaN in the dry sequence of the start"] = c
    c = season(b, n, s0, end=b.we)
    c[b.end_pos + b.we // 2] = np.nan
    cols["NaN in the dry sequence of the end"] = c
    c = season(b, n, s0, end=b.we)
    c[s0 + b.ww + 2] = np.nan
    cols["NaN in the run"] = c
    return cols


def family_none(b, n, s0):
    return {"no start: never wet": column(n, s0, b.moist(n)), "no start: all NaN": np.full(n, np.nan),
            "no end": season(b, n, s0), "no end: all dry after a short run": season(b, n, s0, run=2, stop=n, tail=False),
            "season to the last row": season(b, n, max(n - b.ww - b.N, 0), gap=0)}


def build(axis, pset, families, dtype="float64", flux="mm/d"):
    """One case: every family's columns in every period of the axis (shifted a little from period to period)."""
    ax, p = AXES[axis], PSETS[pset]
    time = TimeAxis.daily(ax["start"], ax["T"], ax["calendar"])
    seg = np.asarray(time.segments(ax["freq"])[0])
    flags = rainseason.rain_flags(time, seg, **ax["dates"])
    b = Blocks(p)
    names, per_period = None, []
    for k in range(len(seg) - 1):
        r0, n = int(seg[k]), int(seg[k + 1] - seg[k])
        inb = np.flatnonzero(flags[r0:r0 + n] & 2)
        s0 = int(inb[0]) + 2 + k                                   # the wet spell starts a few rows inside the start bounds
        b.end_from = int(np.flatnonzero(flags[r0:r0 + n] & 4)[0]) + 1 + k        # the dry sequence of the end inside the end bounds
        cols = {}
        for fam in families:
            cols.update({f"{fam.__name__[7:]}: {name}": c for name, c in fam(b, n, s0).items()})
        names = list(cols)
        per_period.append(np.stack([cols[c] for c in names], axis=1))
    pr = np.concatenate(per_period, axis=0).astype(dtype)
    return dict(axis=axis, pset=pset, params=p, dates=ax["dates"], flux_units=flux, dtype=dtype, columns=names,
                time=dict(start=ax["start"], calendar=ax["calendar"], freq=ax["freq"]),
                family=[f.__name__[7:] for f in families]), time, seg, flags, pr


def case_same_row():
    """The wet amounts are below thresh_dry_start: wet[i] and stop[i] are both true until fewer than wd such rows are left."""
    p = params(ww=3, wnd=4, wd=5, we=3, tw=25.0, td=12.5, te=0.0)
    n = 365
    cols, names = [], []
    for k in (5, 6, 9, 20):                 # rows of 10 mm, then 15 mm (not dry), then a dry end
        names.append(f"same_row: {k} rows wet and dry at once")
        cols.append(column(n, 60, [10.0] * k + [15.0] * 12 + [0.0] * 4 + [15.0] * n))
    names.append("same_row: wet and dry to the end")
    cols.append(column(n, 60, [10.0] * n))
    return p, np.stack(cols, axis=1), names


def case_bounds():
    """Hand-made flags on 200 rows: the start window is rows 20 .. 199; the start bounds are rows 90 .. 120, or the single row 42;
    the end bounds are rows 150 .. 199."""
    p = params(ww=3, wnd=5, wd=4, we=3)
    b, n = Blocks(p), 200
    b.end_from = 152
    out = []
    base = np.zeros(n, np.uint8)
    base[20:] |= 1
    f = base.copy()
    f[90:121] |= 2
    f[150:] |= 4
    early = season(b, n, 40, run=b.N + 3, stop=b.wd, tail=False)      # a candidate at row 42, outside the bounds
    both = np.where(np.arange(n) < 80, early, season(b, n, 95, end=b.we))
    both2 = both.copy()
    both2[130:140] = b.dry_end(3) + b.moist(7)                          # the season ends before the end bounds: not counted ...
    late = np.where(np.arange(n) < 80, early, season(b, n, 125, end=b.we))   # the second candidate is past the bounds as well
    cols = np.stack([early, both, both2, late, season(b, n, 88, end=b.we), season(b, n, 87, end=b.we)], axis=1)
    names = ["bounds: one candidate, outside", "bounds: a candidate outside, then one inside", "bounds: an end before date_min_end, then one after",
             "bounds: candidates before and after the bounds", "bounds: a candidate on the first row in bounds", "bounds: a candidate one row before"]
    out.append(("bounds_window", p, f, cols, names))
    g = base.copy()
    g[42] |= 2                                                          # ONE row in bounds: a candidate there is argmax == argmin
    g[150:] |= 4
    cols = np.stack([early, season(b, n, 50, end=b.we)], axis=1)
    out.append(("bounds_single_row", p, g, cols, ["bounds: the only row in bounds is a candidate", "bounds: the only row in bounds is not"]))
    h = base.copy()
    h[30:100] |= 2
    h[150:153] |= 4                                                     # every row of the end bounds is marked ("total"): no end
    pt = params(ww=3, wnd=5, wd=4, we=3, me="total")
    cols = np.stack([column(n, 40, Blocks(pt).wet() + Blocks(pt).moist(60) + [0.0] * n),
                     column(n, 40, Blocks(pt).wet() + Blocks(pt).moist(60) + [0.0] * 49 + [5.0] + [0.0] * n)], axis=1)
    out.append(("bounds_every_end_row", pt, h, cols, ["bounds: every row of the end bounds is marked", "bounds: all but one"]))
    return out


def case_random(seed, axis, pset, C=24):
    ax, p = AXES[axis], dict(PSETS[pset])
    p.update(thresh_wet_start=20.0, thresh_dry_start=1.0, thresh_dry_end=0.3)
    time = TimeAxis.daily(ax["start"], ax["T"], ax["calendar"])
    seg = np.asarray(time.segments(ax["freq"])[0])
    flags = rainseason.rain_flags(time, seg, **ax["dates"])
    rng = np.random.default_rng(seed)
    keep = []
    while len(keep) < C:
        T = len(time)
        wet = rng.random((T, 64)) < np.where((time.doy > 100) & (time.doy < 290), 0.75, 0.08)[:, None]
        x = np.where(wet, rng.gamma(0.9, 9.0, (T, 64)), np.where(rng.random((T, 64)) < 0.3, rng.random((T, 64)) * 0.6, 0.0))
        x[rng.random((T, 64)) < 0.002] = np.nan
        x = (x / R.DAY).astype(np.float32)
        ok = R.margin(x, seg, flags, "kg m-2 s-1", **p) > 1e-6
        keep += [x[:, j] for j in np.flatnonzero(ok)]
    pr = np.stack(keep[:C], axis=1)
    meta = dict(axis=axis, pset=pset, params=p, dates=ax["dates"], flux_units="kg m-2 s-1", dtype="float32",
                columns=[f"random: {j}" for j in range(C)], family=["random"],
                time=dict(start=ax["start"], calendar=ax["calendar"], freq=ax["freq"]))
    return meta, time, seg, flags, pr


def main():
    arrays, meta = {}, {}

    def add(name, m, time, seg, flags, pr):
        doy = time.doy if time is not None else np.arange(1, len(flags) + 1)
        s, e, ln = R.rain_season_flags(pr, seg, flags, doy, m["flux_units"], **m["params"])
        arrays[f"{name}/pr"], arrays[f"{name}/flags"], arrays[f"{name}/seg"], arrays[f"{name}/doy"] = pr, flags, np.asarray(seg, np.int64), np.asarray(doy, np.int32)
        arrays[f"{name}/start"], arrays[f"{name}/end"], arrays[f"{name}/length"] = s, e, ln
        m["found"] = [int((~np.isnan(s)).sum()), int((~np.isnan(e)).sum()), int(s.size)]
        meta[name] = m

    fams = (family_reach, family_nan, family_none)
    for pset in PSETS:
        axis = {"default": "three", "per_day.per_day": "july", "total.total": "july", "per_day.total": "three", "total.per_day": "one",
                "all32.total": "three", "wd33.per_day": "july"}.get(pset, "one")
        dtype = "float32" if pset in ("total.total", "ww2", "wd33.per_day", "we32.total") else "float64"
        add(f"built.{pset}", *build(axis, pset, fams, dtype))
    add("built.noleap", *build("noleap", "per_day.per_day", fams))
    p, cols, names = case_same_row()
    t = TimeAxis.daily("2001-01-01", 365)
    seg = np.array([0, 365])
    m = dict(axis="one", pset=None, params=p, dates=AXES["noleap"]["dates"], flux_units="mm/d", dtype="float64", columns=names, family=["same_row"],
             time=dict(start="2001-01-01", calendar="standard", freq="YS-JAN"))
    add("same_row", m, t, seg, rainseason.rain_flags(t, seg, **AXES["noleap"]["dates"]), cols)
    for name, p, flags, cols, names in case_bounds():
        m = dict(axis=None, pset=None, params=p, dates=None, time=None, flux_units="mm/d", dtype="float64", columns=names, family=["bounds"])
        add(name, m, None, np.array([0, len(flags)]), flags, cols)
    add("random.three", *case_random(7, "three", "per_day.per_day"))
    add("random.july", *case_random(8, "july", "total.total"))
    arrays["meta"] = np.array(json.dumps(meta))

    # hardiness zones: 31 periods of minima in degC and K: every bin edge, one ulp above and below it, the outer edges, NaN
    for method in ("usda", "anbg"):
        for units in ("degC", "K"):
            e = R.zone_edges(method, units)
            vals = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [e[0] - 40.0, e[-1] + 40.0, np.nan], (e[:-1] + e[1:]) / 2])
            rng = np.random.default_rng(len(vals))
            x = np.stack([np.full(31, v) for v in vals], axis=1)                       # constant columns: the mean is the value itself
            noisy = rng.uniform(e[0] - 8, e[-1] + 8, (31, 12))
            noisy[13, :4] = np.nan                                                      # a NaN period inside a window
            x = np.concatenate([x, noisy], axis=1)
            arrays[f"zones.{method}.{units}/x"] = x
            for w in (1, 2, 30):
                arrays[f"zones.{method}.{units}/w{w}"] = R.rolling_zones(x, w, e)
    out = os.path.join(HERE, "rain_vectors.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    for k, m in meta.items():
        print(f"{k:28s} start/end found {m['found'][0]:4d}/{m['found'][1]:4d} of {m['found'][2]:4d}")


if __name__ == "__main__":
    main()
