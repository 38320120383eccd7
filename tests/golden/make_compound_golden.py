"""Writes tests/golden/compound_known_answers.json and tests/golden/compound_vectors.npz.  Run from the repository root:
``python tests/golden/make_compound_golden.py``.

compound_known_answers.json records the known answers of the reference's own tests of the seven bodies, with the recipe of their
inputs: tests/test_preciptemp.py (all four classes: the first month has 10 / 20 / 20 / 10 compound days at ``freq="MS"``),
tests/test_indices.py:3405-3415 (exceedance dates 151, 151 and 256 with ``after_date="04-15"``), :3735-3740 (blowing snow, ``[1]``)
and ``TestWaterCycleIntensity`` (:4548-4554).  The ``never_reached`` cases of tests/test_temperature.py:1333 all read a data file
(FWI/GFWED_sample_2017.nc) that is not available, so none of them is recorded; the three kinds of ``never_reached`` are families of
the vectors instead.

compound_vectors.npz holds inputs and the results of the numpy restatement tests/compoundcpu.py.  Every result of this unit is an
integer, a day of year or NaN (the water-cycle sums are exact sums), so the device must equal the restatement EXACTLY.  To make
that independent of summation order and precision, the built families lie on grids: temperatures on 0.25 K, snow depths on 1/64 m,
winds on 0.25, fluxes on 2^-22 kg m-2 s-1, so that every sum is exact in float32 and float64.  Each kernel also has one random float32
family; for those the generator ASSERTS a relative gap of at least 1e-6 between every running or window sum and its threshold and
between every field value and its table value (a condition of the fixture, not a tolerance).

One family per decision (the columns of a case; ``columns`` in its meta):
  compound   generic | a NaN in tas | a NaN in pr | a NaN in a table row | equality with the table value on each side | doy 366 of a
             leap year against a 366-row table (case ``*.tab366``) and a 365-row table (``*.tab365``, interpolated) | a noleap axis
  exceedance generic | reached exactly (== then >) | on the first row of a period (the reference's NaN) | on the last row (doy 366) |
             a NaN run across the start row | never reached (all three kinds of ``never_reached``) | ``after_date`` absent from the
             first ("02-01") and from the last period ("06-15"), and from every non-leap year ("02-29")
  snow       generic | a NaN one row inside and one row outside the window | the halo across a period start | the first ``window``
             rows of the series | equality with both thresholds | an indexer that removes rows inside a window; windows 1, 2, 3, 32
  wci        generic with NaN terms and an all-NaN period
Periods are cut at both ends of the series (it runs from 1999-03-10 to 2002-03-09); every case is recorded at ``MS``, ``YS``,
``YS-JUL`` and ``QS-DEC`` (the ``after_date`` cases at the annual ones)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import compoundcpu as CC  # noqa: E402

FREQS = ("MS", "YS", "YS-JUL", "QS-DEC")
ANNUAL = ("YS", "YS-JUL")
AXES = {"std": dict(calendar="standard", start="1999-03-10", T=1096), "noleap": dict(calendar="noleap", start="2001-01-01", T=1095)}
FLUX = 2.0 ** -22          # the grid of the fluxes in kg m-2 s-1
K2C_TEST = 273             # tests/test_preciptemp.py:8
K2C = 273.15               # tests/test_indices.py


def axis(name):
    a = AXES[name]
    return CC.otime(a["calendar"], a["start"], a["T"])


def row_of(t, y, m, d):
    return int(np.flatnonzero((t.year == y) & (t.month == m) & (t.day == d))[0])


def grid(x, step):
    return np.round(np.asarray(x) / step) * step


# ---- the reference's known answers --------------------------------------------------------------------------------------------
def known_answers():
    quad = []
    for name, t_edit, p_edit, t_per, p_per, want in (
            ("cold_and_dry_days", [10, 20, -10], [10, 20, "=0"], 25, 25, 10), ("warm_and_dry_days", [10, 30, 10], [10, 30, "=0"], 75, 25, 20),
            ("warm_and_wet_days", [10, 30, 10], [10, 30, 20], 75, 75, 20)):
        quad.append(dict(function=name, source="tests/test_preciptemp.py", start="2000-07-01", n=365 * 4, tas_fill=20 + K2C_TEST,
                         tas_edits=[t_edit], pr_fill=10, pr_edits=[p_edit], window=5, tas_per=t_per, pr_per=p_per, freq="MS",
                         first_value=want))
    quad.append(dict(function="cold_and_wet_days", source="tests/test_preciptemp.py", start="2000-07-01", n=365 * 4, tas_fill=20 + K2C_TEST,
                     tas_edits=[[10, 25, -20]], pr_fill=10, pr_edits=[[15, 30, 20]], window=5, tas_per=75, pr_per=75, freq="MS",
                     first_value=10))
    dded = [dict(source="tests/test_indices.py:3405-3415", start="2000-01-01", n=366, tas_fill=1 + K2C, thresh_K=t, op=op, sum_thresh=150.0,
                 after_date=after, first_value=want)
            for t, op, after, want in ((0 + K2C, ">", None, 151), (2 + K2C, "<", None, 151), (2 + K2C, "<", "04-15", 256))]
    snow = dict(source="tests/test_indices.py:3735-3740", start="2000-07-01", snd=[0, 0.1, 0.2, 0, 0, 0.1, 0.3, 0.5, 0.7, 0],
                sfcWind=[9, 0, 0, 0, 0, 1, 1, 0, 5, 0], snd_thresh_m=0.5, sfcWind_thresh_kmh=4.0, window=3, freq="YS-JUL", value=[1])
    wci = dict(source="tests/test_indices.py:4548-4554", start="2000-07-01", n=31, pr_fill=1.0, evspsbl_fill=1.0, freq="MS",
               value=2 * 60 * 60 * 24 * 31)
    return dict(compound=quad, degree_days_exceedance_date=dded, blowing_snow=snow, water_cycle_intensity=wci,
                not_recorded=["tests/test_temperature.py:1333 (never_reached): reads FWI/GFWED_sample_2017.nc"])


# ---- compound days ------------------------------------------------------------------------------------------------------------
COMPOUND_COLUMNS = ("generic", "nan_tas", "nan_pr", "nan_table", "equal", "doy366", "generic2", "generic3")


def compound_case(axis_name, ndoy, seed, random=False):
    t = axis(axis_name)
    T, C = len(t), len(COMPOUND_COLUMNS)
    rng = np.random.default_rng(seed)
    doy = np.asarray(t.doy)
    base = 283.0 + 9.0 * np.sin(2 * np.pi * (doy - 110) / 365.25)
    dbase = 283.0 + 9.0 * np.sin(2 * np.pi * (np.arange(1, ndoy + 1) - 110) / 365.25)
    if random:
        tas = (base[:, None] + rng.normal(0, 4, (T, C))).astype(np.float32)
        pr = np.where(rng.random((T, C)) < 0.45, rng.gamma(0.8, 6e-5, (T, C)), 0.0).astype(np.float32)
        tabs = dict(tas_lo=dbase[:, None] - 2.5 + rng.normal(0, 0.3, (ndoy, C)), tas_hi=dbase[:, None] + 2.5 + rng.normal(0, 0.3, (ndoy, C)),
                    pr_lo=rng.uniform(5e-6, 2e-5, (ndoy, C)), pr_hi=rng.uniform(5e-5, 2e-4, (ndoy, C)))
        for k, tab in tabs.items():   # the condition of the random family: no sample within 1e-6 relative of its threshold
            x = tas if k.startswith("tas") else pr
            thr = tab[doy - 1]
            close = np.abs(x - thr) < 2e-6 * np.maximum(np.abs(x), np.abs(thr))
            x[close] = x[close] * np.float32(1.001)
        assert CC.compound_margin(tas, pr, tabs, t) >= 1e-6
        return t, tas, pr, tabs
    tas = grid(base[:, None] + rng.normal(0, 4, (T, C)), 0.25)
    pr = np.where(rng.random((T, C)) < 0.45, np.round(rng.gamma(0.8, 250.0, (T, C))), 0.0) * FLUX
    col = np.arange(C)[None, :]
    d = np.arange(ndoy)[:, None]
    tabs = dict(tas_lo=grid(dbase[:, None] - 2.5, 0.25) + 0.125 + 0.25 * (col % 3), tas_hi=grid(dbase[:, None] + 2.5, 0.25) + 0.125 - 0.25 * (col % 2),
                pr_lo=(40 + d % 7 + col + 0.5) * FLUX, pr_hi=(400 + d % 11 + 3 * col + 0.5) * FLUX)
    tabs = {k: np.array(np.broadcast_to(v, (ndoy, C)), dtype=np.float64) for k, v in tabs.items()}
    c = COMPOUND_COLUMNS.index
    plain = {n: CC.compound_days(n, tas, pr, tabs[CC_TABLES[n][0]], tabs[CC_TABLES[n][1]], t, "YS") for n in CC.COMPOUND}
    # a NaN in tas / in pr on rows that count: the count must fall
    hit = np.flatnonzero((tas[:, c("nan_tas")] < tabs["tas_lo"][np.minimum(doy, ndoy) - 1, c("nan_tas")]) & (pr[:, c("nan_tas")] < tabs["pr_lo"][np.minimum(doy, ndoy) - 1, c("nan_tas")]))
    tas[hit[::3], c("nan_tas")] = np.nan
    hit = np.flatnonzero((tas[:, c("nan_pr")] > tabs["tas_hi"][np.minimum(doy, ndoy) - 1, c("nan_pr")]) & (pr[:, c("nan_pr")] < tabs["pr_lo"][np.minimum(doy, ndoy) - 1, c("nan_pr")]))
    pr[hit[::3], c("nan_pr")] = np.nan
    assert len(hit) > 6
    # a NaN in a table row
    tabs["tas_lo"][40:60, c("nan_table")] = np.nan
    tabs["pr_hi"][200:230, c("nan_table")] = np.nan
    # equality with the table value on each side: tables on the fields' grids, and the samples of every fifth row ON them
    e = c("equal")
    tabs["tas_lo"][:, e] -= 0.125
    tabs["tas_hi"][:, e] -= 0.125
    tabs["pr_lo"][:, e] -= 0.5 * FLUX
    tabs["pr_hi"][:, e] -= 0.5 * FLUX
    rows = np.arange(0, T, 5)
    drow = np.minimum(doy[rows], ndoy) - 1
    tas[rows[0::2], e] = tabs["tas_lo"][drow[0::2], e]
    tas[rows[1::2], e] = tabs["tas_hi"][drow[1::2], e]
    pr[rows[0::4], e] = tabs["pr_lo"][drow[0::4], e]
    pr[rows[2::4], e] = tabs["pr_hi"][drow[2::4], e]
    # doy 366: a sample that is cold only against the table's row 366 and wet only against it
    if axis_name == "std":
        r, k = row_of(t, 2000, 12, 31), c("doy366")
        assert doy[r] == 366
        if ndoy == 366:
            tabs["tas_lo"][365, k], tabs["tas_lo"][364, k], tabs["tas_lo"][0, k] = tas[r, k] + 1.125, tas[r, k] - 0.875, tas[r, k] - 0.875
            tabs["pr_hi"][365, k], tabs["pr_hi"][364, k], tabs["pr_hi"][0, k] = 100.5 * FLUX, 900.5 * FLUX, 900.5 * FLUX
            pr[r, k] = 500 * FLUX
    changed = {n: CC.compound_days(n, tas, pr, tabs[CC_TABLES[n][0]], tabs[CC_TABLES[n][1]], t, "YS") for n in CC.COMPOUND} if ndoy == 366 else plain
    if ndoy == 366:
        assert (changed["cold_and_dry_days"][:, c("nan_tas")] < plain["cold_and_dry_days"][:, c("nan_tas")]).any()
        assert (changed["warm_and_dry_days"][:, c("nan_pr")] < plain["warm_and_dry_days"][:, c("nan_pr")]).any()
        assert (changed["cold_and_dry_days"][:, c("nan_table")] < plain["cold_and_dry_days"][:, c("nan_table")]).any()
    return t, tas, pr, tabs


CC_TABLES = {"cold_and_dry_days": ("tas_lo", "pr_lo"), "warm_and_dry_days": ("tas_hi", "pr_lo"), "warm_and_wet_days": ("tas_hi", "pr_hi"),
             "cold_and_wet_days": ("tas_lo", "pr_hi")}


def add_compound(arrays, meta):
    for name, axis_name, ndoy, seed, random in (("compound.tab366", "std", 366, 11, False), ("compound.tab365", "std", 365, 12, False),
                                               ("compound.noleap", "noleap", 365, 13, False), ("compound.random", "std", 366, 14, True)):
        t, tas, pr, tabs = compound_case(axis_name, ndoy, seed, random)
        if name == "compound.tab365":   # the interpolated thresholds must stay clear of the samples: the two interpolations round differently
            from oracle import calendar as ocal

            for k, tab in tabs.items():
                thr = ocal.resample_doy(tab, np.arange(1, 366), t)
                x = tas if k.startswith("tas") else pr
                e = COMPOUND_COLUMNS.index("equal")
                keep = np.ones(x.shape[1], bool)
                keep[e] = False
                gap = np.abs(x[:, keep] - thr[:, keep]) / np.maximum(np.maximum(np.abs(x[:, keep]), np.abs(thr[:, keep])), 1e-300)
                assert np.nanmin(gap) >= 1e-6, (k, np.nanmin(gap))
        arrays[f"{name}/tas"], arrays[f"{name}/pr"] = tas, pr
        for k, tab in tabs.items():
            arrays[f"{name}/{k}"] = tab
        cols = list(range(len(COMPOUND_COLUMNS)))
        if name == "compound.tab365":
            cols.remove(COMPOUND_COLUMNS.index("equal"))   # an interpolated table has no exact equality to offer
        for freq in FREQS:
            for n in CC.COMPOUND:
                a, b = CC_TABLES[n]
                arrays[f"{name}/{freq}/{n}"] = CC.compound_days(n, tas, pr, tabs[a], tabs[b], t, freq)
        meta[name] = dict(kind="compound", axis=axis_name, ndoy=ndoy, random=random, columns=list(COMPOUND_COLUMNS), use=cols, freqs=list(FREQS))


# ---- exceedance dates ---------------------------------------------------------------------------------------------------------
DDED_COLUMNS = ("generic", "exact", "first_row", "last_row", "nan_run", "never", "never_equal", "generic2")
DDED_THRESH, DDED_SUM = 278.0, 200.0
DDED_SETS = {"plain": dict(op=">", after_date=None, never_reached=None), "apr15": dict(op=">", after_date="04-15", never_reached=None),
             "below.oct01.300": dict(op="<", after_date="10-01", never_reached=300), "feb01.dec01": dict(op=">", after_date="02-01", never_reached="12-01"),
             "jun15.200": dict(op=">", after_date="06-15", never_reached=200), "feb29": dict(op=">", after_date="02-29", never_reached="12-01"),
             "plain.300": dict(op="ge", after_date=None, never_reached=300)}


def dded_fields(random=False):
    t = axis("std")
    T, C = len(t), len(DDED_COLUMNS)
    rng = np.random.default_rng(21)
    doy = np.asarray(t.doy)
    base = 280.0 + 10.0 * np.sin(2 * np.pi * (doy - 110) / 365.25)
    if random:
        return t, (base[:, None] + rng.normal(0, 4, (T, C))).astype(np.float32)
    tas = grid(base[:, None] + rng.normal(0, 4, (T, C)), 0.25)
    c = DDED_COLUMNS.index
    tas[:, c("exact")] = DDED_THRESH + 1.0                   # the running sum is the day count: == 200 on day 200, > on day 201
    tas[:, c("first_row")] = DDED_THRESH - 5.0
    for y, m in ((2000, 1), (2000, 7), (2000, 12), (2001, 1)):   # the first row of a YS / MS, YS-JUL, QS-DEC period is above at once
        tas[row_of(t, y, m, 1), c("first_row")] = DDED_THRESH + 500.0
    tas[row_of(t, 2001, 4, 15), c("first_row")] = DDED_THRESH + 500.0   # ... and the start row of after_date="04-15", which is not the first
    tas[:, c("last_row")] = DDED_THRESH - 5.0
    for y, m, d in ((2000, 6, 30), (2000, 12, 31), (2001, 12, 31)):    # the last row of a YS-JUL year, doy 366 (of December 2000), of a YS year
        tas[row_of(t, y, m, d), c("last_row")] = DDED_THRESH + 500.0
    for y, m, d in ((1999, 4, 15), (2000, 4, 15), (2000, 10, 1), (2001, 2, 1), (2000, 2, 29), (2000, 1, 1)):
        r = row_of(t, y, m, d)
        tas[max(r - 3, 0):r + 4, c("nan_run")] = np.nan
    tas[:, c("never")] = DDED_THRESH - 0.25                  # never a degree day above; always one below
    tas[:, c("never_equal")] = DDED_THRESH
    r = row_of(t, 2000, 1, 1)
    tas[r + 10:r + 210, c("never_equal")] = DDED_THRESH + 1.0   # 200 degree days in 2000: == sum_thresh on every later row, never above
    return t, tas


def add_dded(arrays, meta):
    for name, random in (("dded.built", False), ("dded.random", True)):
        t, tas = dded_fields(random)
        thresh, sum_thresh = (DDED_THRESH, DDED_SUM) if not random else (278.15, 150.3)
        arrays[f"{name}/tas"] = tas
        sets = {}
        for sname, p in DDED_SETS.items():
            freqs = FREQS if p["after_date"] is None else ANNUAL
            sets[sname] = dict(p, freqs=list(freqs))
            for freq in freqs:
                if random:
                    assert CC.exceedance_margin(tas, t, thresh, sum_thresh, p["op"], p["after_date"], freq) >= 1e-6, (sname, freq)
                arrays[f"{name}/{sname}/{freq}"] = CC.degree_days_exceedance_date(tas, t, thresh, sum_thresh, freq=freq, **p)
        meta[name] = dict(kind="dded", axis="std", random=random, columns=list(DDED_COLUMNS), thresh=thresh, sum_thresh=sum_thresh, sets=sets)
    b = lambda s, f: arrays[f"dded.built/{s}/{f}"]  # noqa: E731  (the decisions are really taken)
    c = DDED_COLUMNS.index
    assert b("plain", "YS")[1, c("exact")] == 201 and np.isnan(b("plain", "YS")[1:3, c("first_row")]).all()
    assert b("plain", "YS")[2, c("last_row")] == 365 and b("plain", "YS-JUL")[1, c("last_row")] == 182 and b("plain", "MS")[21, c("last_row")] == 366
    assert b("apr15", "YS")[2, c("first_row")] == 105 and np.isnan(b("plain", "YS")[:, c("never")]).all()
    assert (b("plain.300", "YS")[:, c("never")] == 300).all() and b("plain.300", "YS")[1, c("never_equal")] == 300
    assert b("feb01.dec01", "YS")[:, c("never")].tolist()[1:] == [336.0, 335.0, 335.0] and np.isnan(b("feb01.dec01", "YS")[0]).all()
    assert np.isnan(b("jun15.200", "YS")[3]).all() and not np.isnan(b("jun15.200", "YS")[0]).all()
    assert np.isnan(b("feb29", "YS")[[0, 2, 3]]).all() and not np.isnan(b("feb29", "YS")[1]).all()


# ---- blowing snow -------------------------------------------------------------------------------------------------------------
SNOW_COLUMNS = ("generic", "nan_inside", "nan_outside", "halo", "first_rows", "equal", "generic2", "generic3")
SNOW_THRESH, WIND_THRESH = 0.5, 4.0
SNOW_INDEXERS = {"all": {}, "winter": dict(month=[12, 1, 2]), "dates": dict(date_bounds=["11-15", "03-15"])}


def snow_fields(window, random=False):
    t = axis("std")
    T, C = len(t), len(SNOW_COLUMNS)
    rng = np.random.default_rng(30 + window)
    if random:
        snd = np.abs(np.cumsum(rng.normal(0, 0.2, (T, C)), axis=0)).astype(np.float32)
        wind = rng.uniform(0, 9, (T, C)).astype(np.float32)
        sums = CC.blowing_snow_sums(snd, window)
        assert CC.blowing_snow_margin(snd, wind, 0.513, 4.07, window) >= 1e-6
        del sums
        return t, snd, wind
    step = rng.integers(-24, 25, (T, C)) / 64.0
    snd = np.maximum(np.cumsum(step, axis=0), 0.0)           # on the 1/64 m grid
    wind = grid(rng.uniform(0, 9, (T, C)), 0.25)
    c = SNOW_COLUMNS.index
    gain = SNOW_THRESH / window if window <= 2 else grid(SNOW_THRESH / window, 1 / 64) + 1 / 64

    def event(col, r, exact=False):
        """A snow gain of at least the threshold over the ``window`` days that end on row r, on flat ground, with wind."""
        snd[max(r - window - 2, 0):r + 3, col] = 1.0
        for k in range(window):
            if r - k >= 0:
                snd[r - k:r + 3, col] += gain
        if exact:
            assert window in (1, 2)
        wind[max(r - 2, 0):r + 3, col] = 0.0
        wind[r, col] = WIND_THRESH if exact else WIND_THRESH + 1.0

    for col in ("nan_inside", "nan_outside", "halo", "first_rows", "equal"):
        snd[:, c(col)] = 1.0
        wind[:, c(col)] = 0.0
    for k, r in enumerate(range(60, T - 40, 97)):
        event(c("nan_inside"), r)
        snd[r - window, c("nan_inside")] = np.nan             # d[r - window + 1] is NaN: inside the window of row r
        event(c("nan_outside"), r)
        if r - window - 1 >= 0:
            snd[r - window - 1, c("nan_outside")] = np.nan     # d[r - window] is NaN: one row outside it
    for y, m in ((2000, 1), (2000, 7), (2000, 12), (2001, 1), (2001, 7), (2001, 12), (1999, 12)):
        event(c("halo"), row_of(t, y, m, 1))                  # the window of a period's first row lies in the period before
    for r in range(0, window + 2):                            # gains from row 0 on: only rows >= window have a full window
        snd[r:, c("first_rows")] += 1.0
        wind[r, c("first_rows")] = WIND_THRESH + 1.0
    if window <= 2:
        for r in range(50, T - 10, 61):
            event(c("equal"), r, exact=True)                  # sum == snd_thresh and wind == sfcWind_thresh: both >= hold
    else:
        for r in range(50, T - 10, 61):
            event(c("equal"), r)
    return t, snd, wind


def add_snow(arrays, meta):
    for window in (1, 2, 3, 32):
        name = f"snow.w{window}"
        t, snd, wind = snow_fields(window)
        arrays[f"{name}/snd"], arrays[f"{name}/sfcWind"] = snd, wind
        for iname, indexer in SNOW_INDEXERS.items():
            for freq in FREQS:
                arrays[f"{name}/{iname}/{freq}"] = CC.blowing_snow(snd, wind, t, SNOW_THRESH, WIND_THRESH, window, freq, **indexer)
        meta[name] = dict(kind="snow", axis="std", random=False, window=window, columns=list(SNOW_COLUMNS), snd_thresh=SNOW_THRESH,
                          sfcWind_thresh=WIND_THRESH, indexers=SNOW_INDEXERS, freqs=list(FREQS))
        c = SNOW_COLUMNS.index
        ys = arrays[f"{name}/all/YS"]
        assert ys[:, c("nan_outside")].sum() > ys[:, c("nan_inside")].sum() == 0, (window, ys[:, c("nan_outside")], ys[:, c("nan_inside")])
        # (at window 32 the events of 1 December and 1 January overlap, and the later one flattens the ground under the earlier)
        assert ys[:, c("halo")].sum() >= 5 and (arrays[f"{name}/all/MS"][:, c("halo")] == 1).sum() >= 5
        assert ys[0, c("first_rows")] == 2, (window, ys[:, c("first_rows")])   # rows window and window + 1 of rows 0 .. window + 1
        assert ys[:, c("equal")].sum() > 10
        # 1 July is not selected; 1 December is, and the rows of its window in November are not: they still count in the sum
        assert 0 < arrays[f"{name}/winter/YS"][:, c("halo")].sum() < ys[:, c("halo")].sum()
    t, snd, wind = snow_fields(3, random=True)
    arrays["snow.random/snd"], arrays["snow.random/sfcWind"] = snd, wind
    for iname, indexer in SNOW_INDEXERS.items():
        for freq in FREQS:
            arrays[f"snow.random/{iname}/{freq}"] = CC.blowing_snow(snd, wind, t, 0.513, 4.07, 3, freq, **indexer)
    meta["snow.random"] = dict(kind="snow", axis="std", random=True, window=3, columns=list(SNOW_COLUMNS), snd_thresh=0.513, sfcWind_thresh=4.07,
                               indexers=SNOW_INDEXERS, freqs=list(FREQS))


# ---- water cycle intensity ----------------------------------------------------------------------------------------------------
def add_wci(arrays, meta):
    t = axis("std")
    T, C = len(t), 8
    for name, random in (("wci.built", False), ("wci.random", True)):
        rng = np.random.default_rng(41 + random)
        if random:
            pr, ev = rng.gamma(0.8, 6e-5, (T, C)).astype(np.float32), rng.gamma(2.0, 1e-5, (T, C)).astype(np.float32)
        else:
            pr, ev = np.round(rng.gamma(0.8, 250.0, (T, C))) * FLUX, np.round(rng.gamma(2.0, 40.0, (T, C))) * FLUX
        pr[5:9, 1] = np.nan
        ev[7:12, 2] = np.nan
        r0, r1 = row_of(t, 2000, 2, 1), row_of(t, 2000, 3, 1)
        pr[r0:r1, 3] = np.nan                                  # February 2000 without a term: 0
        arrays[f"{name}/pr"], arrays[f"{name}/evspsbl"] = pr, ev
        for freq in FREQS:
            arrays[f"{name}/{freq}"] = CC.water_cycle_intensity(pr, ev, t, freq)
        assert arrays[f"{name}/MS"][11, 3] == 0.0
        meta[name] = dict(kind="wci", axis="std", random=random, flux_units="kg m-2 s-1", freqs=list(FREQS))


def main():
    with open(os.path.join(HERE, "compound_known_answers.json"), "w") as f:
        json.dump(known_answers(), f, indent=1)
        f.write("\n")
    arrays, meta = {}, {}
    add_compound(arrays, meta)
    add_dded(arrays, meta)
    add_snow(arrays, meta)
    add_wci(arrays, meta)
    arrays["meta"] = np.array(json.dumps(dict(axes=AXES, cases=meta)))
    path = os.path.join(HERE, "compound_vectors.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(meta)} cases, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
