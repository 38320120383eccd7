"""The xarray adapter of the hydrology functions, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like the
reference — ``xclim.indices._hydrology`` defines the functions (with the reference's signatures) and ``xclim.indices`` re-exports
the same objects — with the DataArray stand-in of tests/fakexr.py and the units of tests/fakeunits.py.  The stand-in originals
only record that they were reached (the forwarded forms)."""

import types

import numpy as np
import pytest

import fakexr
from xclim_amd import hydrology, patch
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
DAY = 86400.0
# the reference's signatures (_hydrology.py:50, 94, 371, 404, 577, 607, 640, 673, 772, 894, 949, 997): the adapters bind against them
SIGS = {
    "base_flow_index": "q, freq='YS'",
    "rb_flashiness_index": "q, freq='YS'",
    "snow_melt_we_max": "snw, window=3, freq='YS-JUL'",
    "melt_and_precip_max": "snw, pr, window=3, freq='YS-JUL'",
    "antecedent_precipitation_index": "pr, window=7, p_exp=0.935",
    "flow_index": "q, p=0.95",
    "high_flow_frequency": "q, threshold_factor=9, freq='YS-OCT'",
    "low_flow_frequency": "q, threshold_factor=0.2, freq='YS-OCT'",
    "aridity_index": "pr, evspsblpot, freq='YS'",
    "sen_slope": "q, freq='YS'",
    "sen_slope_ratio": "q, qsim, freq='YS'",
    "base_flow_index_seasonal_ratio": "q, freq='QS-DEC', numerator='DJF', denominator='JJA'",
}
KEPT = ("runoff_ratio", "lag_snowpack_flow_peaks", "snd_max", "snw_max", "snd_max_doy", "snw_max_doy", "standardized_streamflow_index")


def _modules(reached, with_hydro=True):
    mod, pkg = types.ModuleType("xclim.indices._hydrology"), types.ModuleType("xclim.indices")
    originals = {}
    if with_hydro:
        for name, sig in SIGS.items():
            ns = {"reached": reached}
            exec(f"def {name}({sig}):\n    reached.append({name!r})\n    return 'original {name}'\n", ns)
            originals[name] = ns[name]
            setattr(mod, name, ns[name])
            setattr(pkg, name, ns[name])
    for name in KEPT:                                                         # not replaced by this unit
        fn = lambda *a, _n=name, **k: "original " + _n  # noqa: E731
        setattr(mod, name, fn)
        setattr(pkg, name, fn)
    return {"xclim.indices._hydrology": mod, "xclim.indices": pkg}, originals


@pytest.fixture()
def wired(dev):
    import xclim_amd._capi as capi

    reached = []
    mods, originals = _modules(reached)
    old = capi._default_device
    capi._default_device = dev
    names = patch.install(fakexr.make_env(), mods)
    try:
        yield mods, names, reached, originals
    finally:
        patch.uninstall()
        capi._default_device = old


def _fields(T=800, start="2000-01-01", ny=3, nx=2, pr_units="kg m-2 s-1"):
    rng = np.random.default_rng(12)
    t = TimeAxis.daily(start, T)
    doy = t.doy[:, None, None]
    f = {"q": 40 + 30 * np.sin(2 * np.pi * (doy - 120) / 365) ** 2 + rng.gamma(2.0, 6.0, (T, ny, nx)),
         "snw": np.maximum(60 * np.cos(2 * np.pi * (doy - 30) / 365) + rng.normal(0, 4.0, (T, ny, nx)), 0),
         "pr": np.where(rng.random((T, ny, nx)) < 0.4, rng.gamma(0.8, 8.0, (T, ny, nx)), 0.0) / (DAY if pr_units == "kg m-2 s-1" else 1.0)}
    f["evspsblpot"] = f["pr"] * 0.5 + f["pr"].mean()
    f = {k: v.astype(np.float64 if k == "q" else np.float32) for k, v in f.items()}      # (a float64 discharge, float32 land fields)
    f["q"][5, 0, 0] = np.nan
    units = {"q": "m3 s-1", "snw": "kg m-2", "pr": pr_units, "evspsblpot": pr_units}
    return t, f, {k: fakexr.field(v, t, attrs={"units": units[k], "standard_name": k}) for k, v in f.items()}


def test_install_replaces_the_functions_where_defined_and_where_re_exported(wired):
    mods, names, _, originals = wired
    for modname, m in mods.items():
        for n, fn in originals.items():
            assert f"{modname}.{n}" in names
            assert getattr(m, n) is not fn and getattr(m, n).__wrapped__ is fn and getattr(m, n).__name__ == n
    assert set(originals) == set(hydrology.ADAPTED)
    assert not any(n.split(".")[-1] in KEPT for n in names)
    assert mods["xclim.indices"].runoff_ratio() == "original runoff_ratio"


@pytest.mark.parametrize("pr_units", ["kg m-2 s-1", "mm/d"])
def test_served_calls_are_one_launch_each_with_the_reference_s_units(dev, wired, pr_units):
    mods, _, reached, _ = wired
    m, pkg = mods["xclim.indices._hydrology"], mods["xclim.indices"]
    t, f, da = _fields(pr_units=pr_units)
    kw = dict(time=t, device=dev)
    fkw = dict(flux_units=pr_units, **kw)
    calls = [
        # (the call through the patched module, the mirror's value, units, the entry points it may reach, the period frequency)
        (lambda: m.base_flow_index(da["q"]), hydrology.base_flow_index(f["q"], **kw), "", ["xh_flow_period_stats"], "YS"),
        (lambda: pkg.base_flow_index(da["q"], freq="QS-DEC"), hydrology.base_flow_index(f["q"], "QS-DEC", **kw), "", ["xh_flow_period_stats"], "QS-DEC"),
        (lambda: m.rb_flashiness_index(da["q"], "YS-OCT"), hydrology.rb_flashiness_index(f["q"], "YS-OCT", **kw), "", ["xh_flow_period_stats"], "YS-OCT"),
        (lambda: m.snow_melt_we_max(da["snw"]), hydrology.snow_melt_we_max(f["snw"], **kw), "kg m-2", ["xh_melt_period_max"], "YS-JUL"),
        (lambda: pkg.melt_and_precip_max(da["snw"], da["pr"], window=5), hydrology.melt_and_precip_max(f["snw"], f["pr"], 5, **fkw), "kg m-2",
         ["xh_melt_period_max"], "YS-JUL"),
        (lambda: m.antecedent_precipitation_index(da["pr"], window=5), hydrology.antecedent_precipitation_index(f["pr"], 5, **fkw), "mm",
         ["xh_antecedent_precip"], None),
        (lambda: m.high_flow_frequency(da["q"], 1.2), hydrology.high_flow_frequency(f["q"], 1.2, **kw), "days",
         ["xh_nan_quantile_f64", "xh_threshold_count_f64"], "YS-OCT"),
        (lambda: m.low_flow_frequency(da["q"], 0.8, freq="YS"), hydrology.low_flow_frequency(f["q"], 0.8, "YS", **kw), "days",
         ["xh_resample_reduce_f64", "xh_threshold_count_f64"], "YS"),
        (lambda: pkg.aridity_index(da["pr"], da["evspsblpot"]), hydrology.aridity_index(f["pr"], f["evspsblpot"], **kw), "",
         ["xh_resample_reduce", "xh_resample_reduce"], "YS"),
    ]
    for call, want, units, entry_points, freq in calls:
        trace = dev.start_trace()
        try:
            out = call()
        finally:
            dev.stop_trace()
        assert [n for n, _ in trace if n.startswith("xh_")] == entry_points
        assert out.dims == ("time", "lat", "lon") and out.attrs["units"] == units, (out.dims, out.attrs)
        np.testing.assert_array_equal(out.values, want)
        assert set(out.coords) >= {"lat", "lon", "time"}
        if freq is None:
            np.testing.assert_array_equal(out["time"].values, da["pr"]["time"].values)
        else:
            starts = t.segments(freq)[1]            # (the stand-in labels a period by its first row: the partial first one is left out)
            assert len(out["time"].values) == len(starts)
            np.testing.assert_array_equal(out["time"].dt.year.values[1:], [y for y, _ in starts[1:]])
            np.testing.assert_array_equal(out["time"].dt.month.values[1:], [mm for _, mm in starts[1:]])
    assert not reached


def test_the_series_functions_keep_the_cell_dimensions(dev, wired):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._hydrology"]
    t, f, da = _fields()
    kw = dict(time=t, device=dev)
    trace = dev.start_trace()
    try:
        fi = m.flow_index(da["q"], 0.9)
        slope, p = m.sen_slope(da["q"], freq="QS-DEC")
        five = m.sen_slope_ratio(da["q"], da["q"], "YS")
        bfi, ratio = m.base_flow_index_seasonal_ratio(da["q"])
    finally:
        dev.stop_trace()
    assert [n for n, _ in trace if n.startswith("xh_")] == (["xh_nan_quantile_f64"] + ["xh_resample_reduce_f64", "xh_sen_slope"] * 3
                                                             + ["xh_flow_period_stats"])
    assert fi.dims == ("lat", "lon") and fi.attrs["units"] == "1"
    np.testing.assert_array_equal(fi.values, hydrology.flow_index(f["q"], 0.9, device=dev))
    # the reference's layout: unstack puts the yearly time and the season BEHIND the dimensions the field had
    want = hydrology.sen_slope(f["q"], "QS-DEC", **kw)
    assert slope.dims == p.dims == ("lat", "lon", "season") and list(slope["season"].values) == want.seasons == ["DJF", "JJA", "MAM", "SON"]
    assert slope["season"].attrs == dict(mult=1, base="Q", isstart=True, anchor="DEC", season_length=3)
    np.testing.assert_array_equal(slope.values, np.moveaxis(want.sen_slope, 0, -1))
    np.testing.assert_array_equal(p.values, np.moveaxis(want.p_value, 0, -1))
    assert slope.attrs["units"] == p.attrs["units"] == ""
    assert len(five) == 5 and all(x.dims == ("lat", "lon", "season") for x in five) and (five[4].values[~np.isnan(five[4].values)] == 1.0).all()
    assert five[0]["season"].attrs == dict(mult=1, base="Y", isstart=True, anchor="JAN", season_length=6) and list(five[0]["season"].values) == ["annual"]
    want = hydrology.base_flow_index_seasonal_ratio(f["q"], **kw)
    assert bfi.dims == ("lat", "lon", "time", "season") and ratio.dims == ("lat", "lon", "time")
    np.testing.assert_array_equal(bfi.values, np.moveaxis(want.bfi, [0, 1], [-1, -2]))
    np.testing.assert_array_equal(ratio.values, np.moveaxis(want.ratio, 0, -1))
    assert ratio.attrs == {"units": "", "denominator": "JJA", "numerator": "DJF"}
    assert bfi["season"].attrs["anchor"] == "DEC" and list(bfi["season"].values) == want.seasons
    for out in (bfi, ratio):        # dates, not year numbers (the stand-in labels a bin by its first row: the partial first year is left out)
        tc = out["time"]
        assert tc.dt.calendar == "standard" and len(tc.values) == len(want.years) == 3
        np.testing.assert_array_equal(tc.dt.year.values[1:], want.years[1:])
        assert (tc.dt.month.values[1:] == 12).all() and (tc.dt.day.values[1:] == 1).all()
    assert not reached


@pytest.mark.parametrize("start,freq,month", [("1999-12-01", "QS-DEC", 12), ("2000-01-01", "QS", 1), ("2000-03-01", "QS-MAR", 3)])
def test_the_yearly_time_of_the_seasonal_ratio_is_the_reference_s(dev, wired, start, freq, month):
    """split_time_to_season_year (core/calendar.py:1796-1802) labels a year with the date (year, anchor month, 1) in the field's
    calendar.  On series that start on the anchor every label is exact in the stand-in too: year, month and day of all of them."""
    mods, _, reached, _ = wired
    t, f, da = _fields(T=800, start=start)
    num, den = {"QS-DEC": ("DJF", "JJA"), "QS": ("JFM", "JAS"), "QS-MAR": ("MAM", "SON")}[freq]
    bfi, ratio = mods["xclim.indices"].base_flow_index_seasonal_ratio(da["q"], freq, num, den)
    want = hydrology.base_flow_index_seasonal_ratio(f["q"], freq, num, den, time=t, device=dev)
    y0 = int(start[:4])
    assert list(want.years) == [y0, y0 + 1, y0 + 2]
    for out in (bfi, ratio):
        tc = out["time"]
        np.testing.assert_array_equal(tc.dt.year.values, want.years)
        np.testing.assert_array_equal(tc.dt.month.values, [month] * 3)
        np.testing.assert_array_equal(tc.dt.day.values, [1] * 3)
        assert tc.dt.calendar == "standard" and tc.values.dtype != object and not np.array_equal(tc.values, want.years)
    np.testing.assert_array_equal(ratio.values, np.moveaxis(want.ratio, 0, -1))
    assert bfi["season"].attrs == dict(mult=1, base="Q", isstart=True, anchor=freq[3:] or "JAN", season_length=3)
    assert not reached


@pytest.mark.parametrize("form", ["chunked", "gappy", "units", "dims", "array", "window", "freq", "different_units", "season", "end_anchored"])
def test_forwarded_forms_reach_the_original(wired, form):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._hydrology"]
    t, f, da = _fields(T=400)
    if form == "chunked":
        q = fakexr.field(f["q"], t, attrs={"units": "m3 s-1"}, chunks={"lat": 2})
        assert m.base_flow_index(q) == "original base_flow_index"
    elif form == "gappy":
        keep = np.r_[0:10, 11:400]
        assert m.rb_flashiness_index(fakexr.field(f["q"][keep], t.subset(keep), attrs={"units": "m3 s-1"})) == "original rb_flashiness_index"
    elif form == "units":       # a precipitation unit this module has no keyword for
        pr = fakexr.field(f["pr"], t, attrs={"units": "in/d"})
        assert m.melt_and_precip_max(da["snw"], pr) == "original melt_and_precip_max"
    elif form == "dims":
        pr = fakexr.field(f["pr"][:, :, :1], t, attrs={"units": "kg m-2 s-1"})
        assert m.melt_and_precip_max(da["snw"], pr) == "original melt_and_precip_max"
    elif form == "array":
        assert m.snow_melt_we_max(f["snw"]) == "original snow_melt_we_max"
    elif form == "window":      # beyond the LDS ring of the kernels
        assert m.antecedent_precipitation_index(da["pr"], window=hydrology.HYDRO_MAX_WINDOW + 1) == "original antecedent_precipitation_index"
    elif form == "freq":        # a season split the host table does not serve
        assert m.sen_slope(da["q"], freq="7D") == "original sen_slope"
    elif form == "season":      # a season the series does not have: the reference raises its own error
        assert m.base_flow_index_seasonal_ratio(da["q"], numerator="JFM") == "original base_flow_index_seasonal_ratio"
    elif form == "end_anchored":   # the anchor of an end-anchored freq is another month in the reference's season attributes
        assert m.sen_slope(da["q"], freq="QE-NOV") == "original sen_slope"
    else:
        pet = fakexr.field(f["evspsblpot"], t, attrs={"units": "mm/d"})
        assert m.aridity_index(da["pr"], pet) == "original aridity_index"
    assert len(reached) == 1


def test_uninstall_restores_by_identity(wired):
    mods, _, _, originals = wired
    patch.uninstall()
    for m in mods.values():
        for n, fn in originals.items():
            assert getattr(m, n) is fn


def test_install_on_modules_without_every_name_replaces_nothing_new(dev):
    """Replaced only when all are present: a module that lacks one of the functions keeps the others."""
    reached = []
    mods, originals = _modules(reached)
    for m in mods.values():
        delattr(m, "sen_slope_ratio")
    try:
        names = patch.install(fakexr.make_env(), mods)
        assert not [n for n in names if n.split(".")[-1] in hydrology.ADAPTED]
        assert mods["xclim.indices._hydrology"].base_flow_index is originals["base_flow_index"]
    finally:
        patch.uninstall()
