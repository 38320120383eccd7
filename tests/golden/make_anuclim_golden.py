"""Writes tests/golden/anuclim_vectors.npz: the ANUCLIM variables BIO1-BIO19 of small fields, float32 and float64.

The bodies of the reference's indices/_anuclim.py are xarray plumbing; where this file is written there is no xarray, so the
expected values come from the numpy restatement tests/anuclimcpu.py (sequential sums in row order, exact windows, two-pass
standard deviations).  Before anything is written the restatement must reproduce EVERY known answer of the reference's own
tests (tests/test_indices.py:2797-3085: TestTemperatureSeasonality, TestPrecipSeasonality, TestPrecipWettestDriestQuarter,
TestTempWetDryPrecipWarmColdQuarter, TestTempWarmestColdestQuarter, TestPrcptot, TestPrecipWettestDriestPeriod,
TestIsothermality) to the 6 decimals they are asserted with, on inputs regenerated from their recipes — the seeded ones from
the seed of tests/conftest.py:34-35.  Those are stored as cases ("ka_*") with their answers.

It ASSERTS that in every (cell, period, criterion) of every case the best and the runner-up quarter differ by more than 1e-9
relative or are exactly equal (a tie goes to the first index), so that no test hides behind a coin toss.

"cv_single_pass_dev" is the largest relative distance, over every case, of Welford's single-pass BIO4 / BIO15 (numpy float64,
the formula of the kernel) from the two-pass value; the device is tested at four times that, and the formula would be rejected
above 1e-10.

    python tests/golden/make_anuclim_golden.py
"""
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import anuclimcpu as A  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

K2C = 273.15
DAY = 86400.0
SEED = [120189, 120094, 120211, 120097, 120212, 120106]   # tests/conftest.py:35 of the reference, as code points
OUT = os.path.join(HERE, "anuclim_vectors.npz")
FIELDS = ("tas", "tasmin", "tasmax", "pr")

store, meta, worst_cv, worst_gap = {}, {}, 0.0, np.inf


def axis(kind, start, T, calendar="standard"):
    """(TimeAxis, days per row) of a daily / weekly / monthly axis."""
    if kind == "D":
        t = TimeAxis.daily(start, T, calendar)
        return t, np.ones(T)
    if kind == "W":
        t = TimeAxis.daily(start, 7 * T, calendar).subset(slice(None, None, 7))
        return t, np.full(T, 7.0)
    y, m, _ = (int(p) for p in start.split("-"))
    mo = y * 12 + m - 1 + np.arange(T)
    t = TimeAxis(mo // 12, mo % 12 + 1, np.ones(T, np.int64), calendar)
    return t, t.days_in_month().astype(np.float64)


def add_case(name, fields, kind, start, freqs, calendar="standard", per_day=DAY, cv_scale=DAY, kelvin=0.0, thresh=0.0, answers=None):
    """Compute, check the gaps and the single-pass distance, and store one case; returns {freq: outputs}."""
    global worst_cv, worst_gap
    T = len(next(iter(fields.values())))
    t, days = axis(kind, start, T, calendar)
    res = {}
    for freq in freqs:
        so, sr, ss, W = A.tables(t.year, t.month, kind, freq)
        args = (fields, so, per_day * days, sr, ss, W, kind == "D", kelvin, cv_scale, thresh)
        out = A.bioclim(*args, want_gap=True)
        one = A.bioclim(*args, single_pass=True)
        gap = out.pop("min_gap")
        assert gap > 1e-9, f"{name} {freq}: the best and the runner-up quarter are {gap:.2e} apart: change the seed"
        worst_gap = min(worst_gap, gap)
        for k in ("bio4", "bio15"):
            if k in out:
                a, b = one[k], out[k]
                ok = ~np.isnan(b)
                assert np.array_equal(np.isnan(a), np.isnan(b))
                dev = np.where(b[ok] == 0, np.where(a[ok] == 0, 0.0, np.inf), np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300))
                worst_cv = max(worst_cv, float(dev.max(initial=0.0)))
        for k, v in out.items():
            store[f"{name}/{freq}/{k}"] = v
        res[freq] = out
    for k, v in fields.items():
        store[f"{name}/{k}"] = v
    meta[name] = dict(kind=kind, start=start, T=T, calendar=calendar, freqs=list(freqs), per_day=per_day, cv_scale=cv_scale,
                      kelvin=kelvin, thresh=thresh, dtype=str(next(iter(fields.values())).dtype), answers=answers or {})
    for key, want in (answers or {}).items():
        np.testing.assert_array_almost_equal(res[freqs[0]][key][:, 0], want, decimal=6, err_msg=f"{name}: {key}")
    return res


# ---- the known answers of the reference's tests ---------------------------------------------------------------------------
def col(x):
    return np.asarray(x, np.float64).reshape(-1, 1)


def binned(x, idx, kind, how):
    """The reference's tests resample their daily series to "7D" / "MS" before the call: mean or sum per bin."""
    x = np.asarray(x, np.float64)
    if kind == "D":
        return x
    edges = np.arange(0, len(x), 7) if kind == "W" else np.flatnonzero(np.r_[True, np.diff(idx.month) != 0])
    tot = np.add.reduceat(x, edges)
    return tot / np.diff(np.r_[edges, len(x)]) if how == "mean" else tot


def season(idx, name):
    return np.isin(idx.month, {"DJF": (12, 1, 2), "MAM": (3, 4, 5), "JJA": (6, 7, 8), "SON": (9, 10, 11)}[name])


def known_answers():
    # TestTemperatureSeasonality
    idx = pd.date_range("1971-01-01", periods=365)
    for tag, base, kelvin in (("K", K2C, 0.0), ("degC", 0.0, K2C)):
        a = np.zeros(365) + base
        for s, d in (("DJF", -15), ("MAM", -5), ("JJA", 22), ("SON", 2)):
            a[season(idx, s)] += d
        add_case(f"ka_tseas_{tag}", dict(tas=col(a)), "D", "1971-01-01", ["YS"], kelvin=kelvin, answers=dict(bio4=[4.940925]))
        if tag == "K":
            add_case("ka_tseas_weekly", dict(tas=col(binned(a, idx, "W", "mean"))), "W", "1971-01-01", ["YS"],
                     answers=dict(bio4=[4.87321337]))
    # TestPrecipSeasonality
    a = np.zeros(365)
    for m, d in ((12, 2), (8, 10), (1, 5)):
        a[idx.month == m] += d / 3600 / 24
    add_case("ka_pseas", dict(pr=col(a)), "D", "1971-01-01", ["YS"], answers=dict(bio15=[206.29127187]))
    add_case("ka_pseas_weekly", dict(pr=col(binned(a * DAY, idx, "W", "sum"))), "W", "1971-01-01", ["YS"], per_day=1 / 7, cv_scale=1.0,
             answers=dict(bio15=[197.25293501]))
    add_case("ka_pseas_monthly", dict(pr=col(binned(a * DAY, idx, "M", "sum"))), "M", "1971-01-01", ["YS"], per_day=12 / 365.25,
             cv_scale=1.0, answers=dict(bio15=[208.71994117]))
    # TestPrecipWettestDriestQuarter
    idx = pd.date_range("1971-01-01", periods=731)
    a = np.ones(731)
    a[idx.month == 9] += 5
    a[idx.month == 3] += -1
    add_case("ka_wetdry", dict(pr=col(a)), "D", "1971-01-01", ["YS"], per_day=1.0, cv_scale=1.0, answers=dict(bio16=[241, 241], bio17=[60, 60]))
    add_case("ka_wetdry_weekly", dict(pr=col(binned(a, idx, "W", "sum"))), "W", "1971-01-01", ["YS"], per_day=1 / 7, cv_scale=1.0,
             answers=dict(bio16=[241, 241], bio17=[60, 60]))
    add_case("ka_wetdry_monthly", dict(pr=col(binned(a, idx, "M", "mean"))), "M", "1971-01-01", ["YS"], per_day=1.0, cv_scale=1.0,
             answers=dict(bio16=[242, 242], bio17=[58, 59]))
    # TestTempWetDryPrecipWarmColdQuarter (seeded)
    times = pd.date_range("2000-01-01", "2001-12-31")
    cycle = np.sin(2 * np.pi * (times.dayofyear.values / 365.25 - 0.28)).reshape(-1, 1)
    rng = np.random.default_rng(seed=SEED)
    tas = (10 + 15 * cycle + 3 * rng.standard_normal((cycle.size, 1)) + K2C).squeeze()[:730]
    pr = 15 * cycle + 10 + 10 * rng.standard_normal((cycle.size, 1))
    pr = pr / 3600 / 24
    pr[pr < 0] = 0
    pr = pr.squeeze()[:730]
    idx = pd.date_range("2001-01-01", periods=730)
    want = {"D": dict(bio8=[296.138132, 295.823782], bio9=[271.8105, 269.993252], bio18=[2042.826039, 2131.651904],
                      bio19=[246.965006, 229.86537]),
            "M": dict(bio8=[296.429311, 296.192342], bio9=[271.655305, 269.736969], bio18=[2085.393869, 2193.985419],
                      bio19=[245.550801, 233.847277])}
    want["W"] = want["D"]
    for kind in "DWM":
        add_case(f"ka_random_{kind}", dict(tas=col(binned(tas, idx, kind, "mean")), pr=col(binned(pr, idx, kind, "mean"))), kind,
                 "2001-01-01", ["YS"], answers=want[kind])
    # TestIsothermality (seeded)
    rng = np.random.default_rng(seed=SEED)
    tn = (10 + 15 * cycle + 3 * rng.standard_normal((cycle.size, 1)) + K2C).squeeze()[:730]
    tx = (10 + 15 * cycle + 10 + 3 * rng.standard_normal((cycle.size, 1)) + K2C).squeeze()[:730]
    for kind, exp in (("D", [19.798229, 19.559826]), ("W", [23.835284, 24.15181]), ("M", [25.260527, 26.647243])):
        add_case(f"ka_iso_{kind}", dict(tasmin=col(binned(tn, idx, kind, "mean")), tasmax=col(binned(tx, idx, kind, "mean"))), kind,
                 "2001-01-01", ["YS"], answers=dict(bio3=exp))
    # TestTempWarmestColdestQuarter
    idx = pd.date_range("1971-01-01", periods=730)
    a = np.zeros(730) + K2C
    a[season(idx, "JJA") & (idx.year == 1971)] += 22
    a[season(idx, "SON") & (idx.year == 1972)] += 25
    a[season(idx, "DJF") & (idx.year == 1971)] += -15
    a[season(idx, "MAM") & (idx.year == 1972)] += -10
    add_case("ka_warmcold", dict(tas=col(a)), "D", "1971-01-01", ["YS"],
             answers=dict(bio10=[294.66648352, 298.15], bio11=[263.42472527, 263.25989011]))
    add_case("ka_warmcold_weekly", dict(tas=col(binned(a, idx, "W", "mean"))), "W", "1971-01-01", ["YS"],
             answers=dict(bio11=[263.42472527, 263.25989011]))
    add_case("ka_warmcold_monthly", dict(tas=col(binned(a, idx, "M", "mean"))), "M", "1971-01-01", ["YS"], answers=dict(bio11=[263.15, 263.15]))
    a = np.zeros(730)
    a[season(idx, "JJA") & (idx.year == 1971)] += 22
    a[season(idx, "SON") & (idx.year == 1972)] += 25
    a[(idx.month >= 1) & (idx.month <= 3) & (idx.year == 1971)] += -15
    a[season(idx, "MAM") & (idx.year == 1972)] += -10
    add_case("ka_warmcold_degC", dict(tas=col(a)), "D", "1971-01-01", ["YS"], kelvin=K2C,
             answers=dict(bio10=[21.51648352, 25], bio11=[-14.835165, -9.89011]))
    # TestPrcptot, TestPrecipWettestDriestPeriod
    idx = pd.date_range("1971-01-01", periods=731)
    a = np.ones(731)
    a[0:7] += 10
    a[-7:] += 11
    for kind, b12, b13, b14 in (("D", [435.0, 443.0], [11.0, 12.0], [1, 1]), ("W", [441.0, 485.0], [77, 84], [7, 7]),
                                ("M", [435.0, 443.0], [101, 108], [28, 29])):
        add_case(f"ka_prcptot_{kind}", dict(pr=col(binned(a, idx, kind, "mean"))), kind, "1971-01-01", ["YS"], per_day=1.0, cv_scale=1.0,
                 answers=dict(bio12=b12, bio13=b13, bio14=b14))


# ---- seeded fields ----------------------------------------------------------------------------------------------------------
def synth(seed, t, C, dtype, kind="D", spread=3.0):
    """tas, tasmin, tasmax [K] and pr [kg m-2 s-1] with an annual cycle, on the axis t."""
    rng = np.random.default_rng(seed)
    T = len(t)
    doy = t.doy[:, None].astype(np.float64)
    tas = 283 + 10 * np.sin(2 * np.pi * (doy - 100) / 365) + rng.normal(0, spread, (T, C)) + np.linspace(-3, 3, C)[None, :]
    tn, tx = tas - rng.uniform(2, 6, (T, C)), tas + rng.uniform(2, 6, (T, C))
    pr = np.maximum(rng.normal(2 + np.cos(2 * np.pi * doy / 365), 4, (T, C)), 0) / DAY
    return {k: v.astype(dtype) for k, v in dict(tas=tas, tasmin=tn, tasmax=tx, pr=pr).items()}


def seeded():
    t, _ = axis("D", "1999-03-15", 1002)   # bins anchored at March 15; 1002 = 143 * 7 + 1: a last bin of one day
    f = synth(1, t, 3, np.float64)
    add_case("midyear_f64", f, "D", "1999-03-15", ["YS", "YS-JUL"])
    add_case("midyear_thresh_f64", dict(pr=f["pr"]), "D", "1999-03-15", ["YS"], thresh=2.5 / DAY)
    f = synth(2, t, 6, np.float32)
    f["tas"][10, 1] = f["pr"][11, 1] = np.nan                 # a NaN day inside a week
    f["tasmin"][300, 1] = np.nan
    f["tas"][399:406, 2] = f["pr"][399:406, 2] = np.nan       # an all-NaN week (rows 399 .. 405 are step 57): tas NaN for 13 quarters, pr 0
    for k in FIELDS:
        f[k][:, 3] = np.nan                                   # an all-NaN cell
    f["tas"][200:700, 4] = np.nan                             # every tas quarter of 2000 is NaN: the criterion of BIO10 / 11 / 18 / 19
    add_case("midyear_nan_f32", f, "D", "1999-03-15", ["YS", "YS-JUL"])    # is all NaN, and the wettest quarter's tas is NaN
    t, _ = axis("D", "2001-02-01", 80)
    add_case("short_f64", synth(3, t, 2, np.float64), "D", "2001-02-01", ["YS"])
    t, _ = axis("D", "2001-01-01", 730, "noleap")
    add_case("noleap_f32", synth(4, t, 3, np.float32), "D", "2001-01-01", ["YS"], calendar="noleap")
    t, _ = axis("D", "2001-01-01", 720, "360_day")
    add_case("360day_f64", synth(5, t, 2, np.float64), "D", "2001-01-01", ["YS-JUL"], calendar="360_day")
    t, _ = axis("W", "2000-01-03", 110)
    f = synth(6, t, 3, np.float64, spread=1.0)
    f["pr"] = f["pr"] * DAY * 7                               # mm/week
    f["pr"][40, 1] = np.nan                                   # a NaN row is a NaN step here
    add_case("weekly_f64", f, "W", "2000-01-03", ["YS"], per_day=1 / 7, cv_scale=1.0)
    t, _ = axis("M", "2000-01-01", 36)
    f = synth(7, t, 3, np.float32, spread=1.0)
    f["pr"] = (f["pr"] * np.float32(DAY)).astype(np.float32)  # mm/d
    add_case("monthly_f32", f, "M", "2000-01-01", ["YS", "QS-DEC"], per_day=1.0, cv_scale=1.0)
    T = 730
    const = dict(tas=np.full((T, 2), 280.0), tasmin=np.full((T, 2), 275.0), tasmax=np.full((T, 2), 285.0), pr=np.full((T, 2), 2.0))
    add_case("constant_f64", const, "D", "2001-01-01", ["YS"], per_day=1.0, cv_scale=1.0)   # ties: the first index wins
    rng = np.random.default_rng(8)
    trop = dict(tas=300 + rng.uniform(-0.3, 0.3, (T, 3)), pr=5 + rng.uniform(-0.005, 0.005, (T, 3)))
    trop["tasmin"], trop["tasmax"] = trop["tas"] - 0.2, trop["tas"] + 0.2
    add_case("tropical_f64", trop, "D", "2001-01-01", ["YS"], per_day=1.0, cv_scale=1.0)     # a naive sum of squares fails here


if __name__ == "__main__":
    known_answers()
    seeded()
    assert worst_cv <= 1e-10, f"Welford's single pass is {worst_cv:.2e} from the two-pass value: rejected"
    store["cv_single_pass_dev"] = np.float64(worst_cv)
    store["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print(f"{OUT}: {len(meta)} cases, {size} bytes; smallest quarter gap {worst_gap:.2e}; single-pass distance {worst_cv:.2e}")
