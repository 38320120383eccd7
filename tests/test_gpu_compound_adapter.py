"""The xarray adapters of the compound-extreme unit, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like the
reference — ``xclim.indices._multivariate`` defines the four compound counts, ``blowing_snow`` and ``water_cycle_intensity``,
``xclim.indices._threshold`` defines ``degree_days_exceedance_date`` (all with the reference's signatures) and ``xclim.indices``
re-exports the same objects — with the DataArray stand-in of tests/fakexr.py and the units of tests/fakeunits.py.  The stand-in
originals only record that they were reached (the forwarded forms)."""

import types

import numpy as np
import pytest

import fakexr
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)
from xclim_amd import compound, patch
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu
COUNT_SIG = "tas, pr, tas_per, pr_per, freq='YS'"
# the reference's signatures (_multivariate.py:162-168 ..., 1833-1841, 1888; _threshold.py:3215-3223): the adapters bind against them
SIGS = {
    "xclim.indices._multivariate": {
        "cold_and_dry_days": COUNT_SIG, "warm_and_dry_days": COUNT_SIG, "warm_and_wet_days": COUNT_SIG, "cold_and_wet_days": COUNT_SIG,
        "blowing_snow": "snd, sfcWind, snd_thresh='5 cm', sfcWind_thresh='15 km/h', window=3, freq='YS-JUL', **indexer",
        "water_cycle_intensity": "pr, evspsbl, freq='YS'"},
    "xclim.indices._threshold": {
        "degree_days_exceedance_date": "tas, thresh='0 degC', sum_thresh='25 K days', op='>', after_date=None, never_reached=None, freq='YS'"},
}
KEPT = ("multiday_temperature_swing", "daily_pr_intensity")
T = 365 * 3 + 1
TIME = TimeAxis.daily("2000-01-01", T)


def _modules(reached):
    pkg = types.ModuleType("xclim.indices")
    mods, originals = {"xclim.indices": pkg}, {}
    for modname, sigs in SIGS.items():
        mod = mods[modname] = types.ModuleType(modname)
        for name, sig in sigs.items():
            ns = {"reached": reached}
            exec(f"def {name}({sig}):\n    reached.append({name!r})\n    return 'original {name}'\n", ns)
            originals[name] = ns[name]
            setattr(mod, name, ns[name])
            setattr(pkg, name, ns[name])
    for name in KEPT:                                                         # not replaced by this unit
        fn = lambda *a, _n=name, **k: "original " + _n  # noqa: E731
        setattr(mods["xclim.indices._multivariate"], name, fn)
        setattr(pkg, name, fn)
    return mods, originals


def _env():
    """The stand-in environment, with the one quantity of this unit that tests/fakeunits.py does not parse: a degree-day sum."""
    env = fakexr.make_env()
    plain = env.convert_units_to

    def convert_units_to(thr, data, context=None):
        if isinstance(thr, str) and thr.strip().endswith(" days") and getattr(data, "attrs", {}).get("units") == "K days":
            value, unit = thr.strip()[:-len(" days")].split(" ", 1)
            assert unit in ("K", "degC")          # a temperature DIFFERENCE: the same number in both
            return float(value)
        return plain(thr, data, context=context)

    env.convert_units_to = convert_units_to
    return env


@pytest.fixture()
def wired(dev):
    import xclim_amd._capi as capi

    reached = []
    mods, originals = _modules(reached)
    old = capi._default_device
    capi._default_device = dev
    names = patch.install(_env(), mods)
    try:
        yield mods, names, reached, originals
    finally:
        patch.uninstall()
        capi._default_device = old


def _fields(dtype=np.float32, ny=3, nx=2):
    rng = np.random.default_rng(7)
    base = 283.0 + 9.0 * np.sin(2 * np.pi * (TIME.doy - 110) / 365.25)
    dbase = 283.0 + 9.0 * np.sin(2 * np.pi * (np.arange(1, 367) - 110) / 365.25)
    f = {"tas": np.round((base[:, None, None] + rng.normal(0, 4, (T, ny, nx))) * 4) / 4,
         "pr": np.where(rng.random((T, ny, nx)) < 0.45, np.round(rng.gamma(0.8, 250.0, (T, ny, nx))), 0.0) * 2.0 ** -22,
         "evspsbl": np.round(rng.gamma(2.0, 40.0, (T, ny, nx))) * 2.0 ** -22,
         "snd": np.maximum(np.cumsum(rng.integers(-24, 25, (T, ny, nx)) / 64.0, axis=0), 0.0),
         "sfcWind": np.round(rng.uniform(0, 9, (T, ny, nx)) * 4) / 4}
    f = {k: v.astype(dtype) for k, v in f.items()}
    units = {"tas": "K", "pr": "kg m-2 s-1", "evspsbl": "kg m-2 s-1", "snd": "m", "sfcWind": "m s-1"}
    da = {k: fakexr.field(v, TIME, attrs={"units": units[k]}) for k, v in f.items()}
    tabs = {"tas_lo": dbase[:, None, None] - 2.4 + np.zeros((1, ny, nx)), "tas_hi": dbase[:, None, None] + 2.6 + np.zeros((1, ny, nx)),
            "pr_lo": np.full((366, ny, nx), 40.5 * 2.0 ** -22), "pr_hi": np.full((366, ny, nx), 400.5 * 2.0 ** -22)}
    coords = {"dayofyear": np.arange(1, 367), "lat": np.arange(ny), "lon": np.arange(nx)}
    dt = {k: fakexr.DataArray(v, coords=coords, dims=("dayofyear", "lat", "lon"), attrs={"units": "K" if k.startswith("tas") else "kg m-2 s-1"})
          for k, v in tabs.items()}
    return f, da, tabs, dt


def _on_period_starts(got, freq, time=TIME):
    """One label per period of ``resample(time=freq)``.  (The stand-in labels a period by its first row, xarray by the period's
    start: the same wherever the series does not cut the period.)"""
    first = np.asarray(time.segments(freq)[0][:-1])
    assert len(got["time"].values) == len(first)
    np.testing.assert_array_equal(got["time"].dt.year.values, time.year[first])
    np.testing.assert_array_equal(got["time"].dt.month.values, time.month[first])


def _traced(dev, call):
    trace = dev.start_trace()
    try:
        out = call()
    finally:
        dev.stop_trace()
    return out, [n for n, _ in trace if n.startswith("xh_") and n != "xh_memcpy_d2d"]


def test_install_replaces_the_seven_functions_where_defined_and_where_re_exported(wired):
    mods, names, _, originals = wired
    assert set(originals) == set(compound.ADAPTED) and len(originals) == 7
    for modname, sigs in SIGS.items():
        for n in sigs:
            for where in (modname, "xclim.indices"):
                assert f"{where}.{n}" in names
                fn = getattr(mods[where], n)
                assert fn is not originals[n] and fn.__wrapped__ is originals[n] and fn.__name__ == n
            assert getattr(mods["xclim.indices"], n) is getattr(mods[modname], n)
    assert not any(n.split(".")[-1] in KEPT for n in names)
    assert mods["xclim.indices"].daily_pr_intensity() == "original daily_pr_intensity"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_the_compound_counts_are_one_launch_each_with_the_reference_s_units(dev, wired, dtype):
    mods, _, reached, _ = wired
    f, da, tabs, dt = _fields(dtype)
    tables = {"cold_and_dry_days": ("tas_lo", "pr_lo"), "warm_and_dry_days": ("tas_hi", "pr_lo"), "warm_and_wet_days": ("tas_hi", "pr_hi"),
              "cold_and_wet_days": ("tas_lo", "pr_hi")}
    fused = compound.compound_days(f["tas"], f["pr"], tabs["tas_lo"], tabs["tas_hi"], tabs["pr_lo"], tabs["pr_hi"], freq="MS", time=TIME, device=dev)
    for where in ("xclim.indices._multivariate", "xclim.indices"):
        for n, (a, b) in tables.items():
            got, launches = _traced(dev, lambda: getattr(mods[where], n)(da["tas"], da["pr"], dt[a], dt[b], freq="MS"))
            assert launches == ["xh_compound_doy_days"]
            assert got.dims == ("time", "lat", "lon") and got.attrs == {"units": "days"} and set(got.coords) >= {"lat", "lon", "time"}
            assert got.values.dtype == np.float64 and got.values.sum() > 0
            np.testing.assert_array_equal(got.values, fused[n])
            _on_period_starts(got, "MS")
    # another dimension order of the fields and of a table, and a table with a percentiles dimension of length one
    swapped = da["tas"].transpose("lon", "time", "lat")
    per = fakexr.DataArray(np.moveaxis(tabs["tas_lo"], 0, -1)[..., None], coords={"dayofyear": np.arange(1, 367), "lat": np.arange(3), "lon": np.arange(2),
                                                                             "percentiles": [25]},
                           dims=("lat", "lon", "dayofyear", "percentiles"), attrs={"units": "K"})
    got = mods["xclim.indices"].cold_and_dry_days(swapped, da["pr"].transpose("lon", "time", "lat"), per, dt["pr_lo"])
    want = compound.cold_and_dry_days(f["tas"], f["pr"], tabs["tas_lo"], tabs["pr_lo"], time=TIME, device=dev)
    assert got.dims == ("time", "lon", "lat")
    np.testing.assert_array_equal(got.values, np.moveaxis(want, 2, 1))
    _on_period_starts(got, "YS")
    assert not reached


def test_the_exceedance_date_has_the_reference_s_attributes(dev, wired):
    mods, _, reached, _ = wired
    f, da, _, _ = _fields(np.float32)
    fn = mods["xclim.indices"].degree_days_exceedance_date
    calls = [
        (lambda: fn(da["tas"], thresh="5 degC", sum_thresh="200 K days"), dict(thresh=278.15, sum_thresh=200.0), "YS"),
        (lambda: fn(da["tas"], "278 K", "150 degC days", "<", "10-01", 300, "YS-JUL"),
         dict(thresh=278.0, sum_thresh=150.0, op="<", after_date="10-01", never_reached=300, freq="YS-JUL"), "YS-JUL"),
        (lambda: mods["xclim.indices._threshold"].degree_days_exceedance_date(da["tas"], 280.0, 2000.0, never_reached="12-01"),
         dict(thresh=280.0, sum_thresh=2000.0, never_reached="12-01"), "YS"),
    ]
    for call, kw, freq in calls:
        got, launches = _traced(dev, call)
        assert launches == ["xh_degree_exceedance_date"]
        want = compound.degree_days_exceedance_date(f["tas"], time=TIME, device=dev, **kw)
        attrs = {"units": "", "is_dayofyear": np.int32(1), "calendar": "standard"}
        assert got.dims == ("time", "lat", "lon") and got.attrs == attrs and type(got.attrs["is_dayofyear"]) is np.int32
        np.testing.assert_array_equal(got.values, want)
        assert not np.isnan(want).all()
        _on_period_starts(got, freq)
    celsius = fakexr.field(f["tas"] - np.float32(273.0), TIME, attrs={"units": "degC"})
    got = fn(celsius, thresh="278 K", sum_thresh=200.0)          # the threshold in the units of the field: 4.85 degC
    np.testing.assert_array_equal(got.values, compound.degree_days_exceedance_date(f["tas"] - np.float32(273.0), 278.0 - 273.15, 200.0, time=TIME,
                                                                                   units="degC", device=dev))
    assert not reached


def test_blowing_snow_and_the_water_cycle_intensity(dev, wired):
    mods, _, reached, _ = wired
    f, da, _, _ = _fields(np.float64)
    pkg = mods["xclim.indices"]
    for call, kw, freq in (
            (lambda: pkg.blowing_snow(da["snd"], da["sfcWind"]), dict(snd_thresh=0.05, sfcWind_thresh=15.0 / 3.6), "YS-JUL"),
            (lambda: pkg.blowing_snow(da["snd"], da["sfcWind"], "50 cm", "4 m/s", 5, "MS", month=[12, 1, 2]),
             dict(snd_thresh=0.5, sfcWind_thresh=4.0, window=5, freq="MS", month=[12, 1, 2]), "MS")):
        got, launches = _traced(dev, call)
        assert launches == ["xh_blowing_snow_days"]
        want = compound.blowing_snow(f["snd"], f["sfcWind"], time=TIME, device=dev, **kw)
        np.testing.assert_array_equal(got.values, want)
        assert want.sum() > 0 and got.dims == ("time", "lat", "lon")
        # the reference assigns the DataArray that to_agg_units returns as the ``units`` attribute (_multivariate.py:1883): so does this
        assert isinstance(got.attrs["units"], fakexr.DataArray) and got.attrs["units"].attrs["units"] == "days"
        _on_period_starts(got, freq)
    # a series that begins on the last day of a month: diff drops row 0 and its period with it
    late = slice(30, None)
    snd, wind = (fakexr.field(f[k][late], TIME.subset(late), attrs={"units": u}) for k, u in (("snd", "m"), ("sfcWind", "m s-1")))
    got = pkg.blowing_snow(snd, wind, "50 cm", "4 m/s", freq="MS")
    assert len(got["time"].values) == len(TIME.segments("MS")[1]) - 1 and (got["time"].dt.month.values[0], got["time"].dt.year.values[0]) == (2, 2000)
    np.testing.assert_array_equal(got.values, compound.blowing_snow(f["snd"][late], f["sfcWind"][late], 0.5, 4.0, freq="MS", time=TIME.subset(late), device=dev))
    got, launches = _traced(dev, lambda: pkg.water_cycle_intensity(da["pr"], da["evspsbl"], freq="QS-DEC"))
    assert launches == ["xh_pair_period_sum"] and got.attrs == {"units": "kg m-2"}
    np.testing.assert_array_equal(got.values, compound.water_cycle_intensity(f["pr"], f["evspsbl"], "QS-DEC", time=TIME, device=dev))
    _on_period_starts(got, "QS-DEC")
    per_day = {k: fakexr.field(f[k], TIME, attrs={"units": "mm/d"}) for k in ("pr", "evspsbl")}
    got = pkg.water_cycle_intensity(**per_day)
    assert got.attrs == {"units": "mm"}
    np.testing.assert_array_equal(got.values, compound.water_cycle_intensity(f["pr"], f["evspsbl"], time=TIME, flux_units="mm/d", device=dev))
    assert not reached


def test_what_is_not_served_goes_to_the_originals(dev, wired):
    mods, _, reached, _ = wired
    pkg = mods["xclim.indices"]
    f, da, tabs, dt = _fields(np.float32)
    chunked = {k: fakexr.field(v, TIME, attrs=da[k].attrs, chunks={"lat": 1}) for k, v in f.items()}
    ints = {k: fakexr.field((v * 64).astype(np.int32), TIME, attrs=da[k].attrs) for k, v in f.items()}
    f64 = {k: fakexr.field(v.astype(np.float64), TIME, attrs=da[k].attrs) for k, v in f.items()}
    months = TimeAxis([2000 + k // 12 for k in range(36)], [k % 12 + 1 for k in range(36)], [1] * 36)
    monthly = {k: fakexr.field(v[:36], months, attrs=da[k].attrs) for k, v in f.items()}
    keep = np.r_[0:40, 50:T]
    gaps = TimeAxis(TIME.year[keep], TIME.month[keep], TIME.day[keep])
    gappy = {k: fakexr.field(v[keep], gaps, attrs=da[k].attrs) for k, v in f.items()}
    n = 0
    for bad in (chunked, ints, monthly, gappy):
        for name in ("cold_and_dry_days", "warm_and_wet_days"):
            assert getattr(pkg, name)(bad["tas"], bad["pr"], dt["tas_lo"], dt["pr_lo"]) == f"original {name}"
        assert pkg.degree_days_exceedance_date(bad["tas"]) == "original degree_days_exceedance_date"
        assert pkg.blowing_snow(bad["snd"], bad["sfcWind"]) == "original blowing_snow"
        assert pkg.water_cycle_intensity(bad["pr"], bad["evspsbl"]) == "original water_cycle_intensity"
        n += 5
    # mixed dtypes
    assert pkg.warm_and_dry_days(da["tas"], f64["pr"], dt["tas_hi"], dt["pr_lo"]) == "original warm_and_dry_days"
    assert pkg.blowing_snow(f64["snd"], da["sfcWind"]) == "original blowing_snow"
    assert pkg.water_cycle_intensity(da["pr"], f64["evspsbl"]) == "original water_cycle_intensity"
    # array-valued thresholds, windows beyond 32, units outside the tables
    assert pkg.blowing_snow(da["snd"], da["sfcWind"], snd_thresh=da["snd"]) == "original blowing_snow"
    assert pkg.blowing_snow(da["snd"], da["sfcWind"], window=33) == "original blowing_snow"
    assert pkg.degree_days_exceedance_date(da["tas"], thresh=da["tas"]) == "original degree_days_exceedance_date"
    assert pkg.degree_days_exceedance_date(da["tas"], sum_thresh=np.ones(3)) == "original degree_days_exceedance_date"
    fahrenheit = fakexr.field(f["tas"], TIME, attrs={"units": "degF"})
    assert pkg.degree_days_exceedance_date(fahrenheit) == "original degree_days_exceedance_date"
    inches = fakexr.field(f["pr"], TIME, attrs={"units": "inch/d"})
    assert pkg.water_cycle_intensity(inches, da["evspsbl"]) == "original water_cycle_intensity"
    assert pkg.water_cycle_intensity(fakexr.field(f["pr"], TIME, attrs={"units": "mm/d"}), da["evspsbl"]) == "original water_cycle_intensity"
    # tables: not on dayofyear, several percentiles, other dimensions, a table that does not cover the year, plain arrays
    two = fakexr.DataArray(np.stack([tabs["tas_lo"]] * 2, -1), coords={"dayofyear": np.arange(1, 367), "lat": np.arange(3), "lon": np.arange(2), "percentiles": [10, 25]},
                           dims=("dayofyear", "lat", "lon", "percentiles"), attrs={"units": "K"})
    flat = fakexr.DataArray(tabs["tas_lo"][:, 0], coords={"dayofyear": np.arange(1, 367), "lon": np.arange(2)}, dims=("dayofyear", "lon"), attrs={"units": "K"})
    holed = fakexr.DataArray(np.delete(tabs["tas_lo"], 59, 0), coords={"dayofyear": np.delete(np.arange(1, 367), 59), "lat": np.arange(3), "lon": np.arange(2)},
                             dims=("dayofyear", "lat", "lon"), attrs={"units": "K"})
    for per in (two, flat, holed, tabs["tas_lo"], da["tas"]):
        assert pkg.cold_and_wet_days(da["tas"], da["pr"], per, dt["pr_hi"]) == "original cold_and_wet_days"
    assert pkg.cold_and_wet_days(da["tas"], f["pr"], dt["tas_lo"], dt["pr_hi"]) == "original cold_and_wet_days"     # not a DataArray
    assert len(reached) == n + 3 + 7 + 6
    # ... and what the reference itself refuses is the caller's: no forwarding of a ValueError
    with pytest.raises(NotImplementedError, match="op: '=='"):
        pkg.degree_days_exceedance_date(da["tas"], op="==")
    with pytest.raises(ValueError, match="MM-DD"):
        pkg.degree_days_exceedance_date(da["tas"], never_reached="2000-12-01")


def test_uninstall_puts_the_originals_back(dev):
    reached = []
    mods, originals = _modules(reached)
    patch.install(_env(), mods)
    patch.uninstall()
    for modname, sigs in SIGS.items():
        for n in sigs:
            assert getattr(mods[modname], n) is originals[n] and getattr(mods["xclim.indices"], n) is originals[n]
