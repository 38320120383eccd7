"""The xarray adapter of rain_season and hardiness_zones, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like
the reference — ``xclim.indices._agro`` defines the two functions (with the reference's signatures) and ``xclim.indices`` re-exports
the same objects — with the DataArray stand-in of tests/fakexr.py and the units of tests/fakeunits.py.  The stand-in originals
only record that they were reached (the forwarded forms)."""

import types

import numpy as np
import pytest

import fakexr
from xclim_amd import patch, rainseason
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
DAY = 86400.0
# the reference's signatures (_agro.py:796-812, 1388-1390): the adapters bind against them
SIGS = {
    "rain_season": ("pr, thresh_wet_start='25.0 mm', window_wet_start=3, window_not_dry_start=30, thresh_dry_start='1.0 mm', "
                    "window_dry_start=7, method_dry_start='per_day', date_min_start='05-01', date_max_start='12-31', "
                    "thresh_dry_end='0.0 mm', window_dry_end=20, method_dry_end='per_day', date_min_end='09-01', date_max_end='12-31', "
                    "freq='YS-JAN'"),
    "hardiness_zones": "tasmin, window=30, method='usda', freq='YS'",
}
KEPT = ("corn_heat_units", "qian_weighted_mean_average", "dryness_index_of_another_module")


def _modules(reached, names=tuple(SIGS)):
    mod, pkg = types.ModuleType("xclim.indices._agro"), types.ModuleType("xclim.indices")
    originals = {}
    for name in names:
        ns = {"reached": reached}
        exec(f"def {name}({SIGS[name]}):\n    reached.append({name!r})\n    return 'original {name}'\n", ns)
        originals[name] = ns[name]
        setattr(mod, name, ns[name])
        setattr(pkg, name, ns[name])
    for name in KEPT:                                                         # not replaced by this unit
        fn = lambda *a, _n=name, **k: "original " + _n  # noqa: E731
        setattr(mod, name, fn)
        setattr(pkg, name, fn)
    return {"xclim.indices._agro": mod, "xclim.indices": pkg}, originals


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


def _fields(T=365 * 3 + 1, start="2000-01-01", ny=3, nx=2, pr_units="mm/d"):
    """A wet season from May to October: amounts in mm per day on a 0.25 mm grid (exact in float32)."""
    rng = np.random.default_rng(21)
    t = TimeAxis.daily(start, T)
    wet = (t.doy > 125) & (t.doy < 290)
    amount = np.where(wet[:, None, None] & (rng.random((T, ny, nx)) < 0.8), np.round(rng.gamma(1.5, 8.0, (T, ny, nx)) * 4) / 4, 0.0)
    amount[np.flatnonzero(wet)[:3]] = 12.0
    pr = amount.astype(np.float32)
    tasmin = (15 + 8 * np.cos(2 * np.pi * (t.doy - 200) / 365.25)[:, None, None] + rng.normal(0, 2, (T, ny, nx))).astype(np.float64)
    return t, {"pr": pr, "tasmin": tasmin}, {"pr": fakexr.field(pr, t, attrs={"units": pr_units, "standard_name": "precipitation_flux"}),
                                             "tasmin": fakexr.field(tasmin, t, attrs={"units": "degC", "standard_name": "air_temperature"})}


def test_install_replaces_both_functions_where_defined_and_where_re_exported(wired):
    mods, names, _, originals = wired
    for modname, m in mods.items():
        for n, fn in originals.items():
            assert f"{modname}.{n}" in names
            assert getattr(m, n) is not fn and getattr(m, n).__wrapped__ is fn and getattr(m, n).__name__ == n
    assert set(originals) == set(rainseason.ADAPTED)
    assert not any(n.split(".")[-1] in KEPT for n in names)
    assert mods["xclim.indices"].corn_heat_units() == "original corn_heat_units"


def test_rain_season_is_one_launch_with_the_reference_s_attributes(dev, wired):
    mods, _, reached, _ = wired
    m, pkg = mods["xclim.indices._agro"], mods["xclim.indices"]
    t, f, da = _fields(pr_units="mm/d")
    kw = dict(time=t, device=dev, flux_units="mm/d")
    calls = [
        (lambda: m.rain_season(da["pr"], window_not_dry_start=10, window_dry_end=8),
         rainseason.rain_season(f["pr"], window_not_dry_start=10, window_dry_end=8, **kw), "YS-JAN"),
        (lambda: pkg.rain_season(da["pr"], "20 mm", 2, 10, "0.5 mm", 5, "total", thresh_dry_end="1 mm", window_dry_end=6, method_dry_end="total"),
         rainseason.rain_season(f["pr"], 20.0, 2, 10, 0.5, 5, "total", thresh_dry_end=1.0, window_dry_end=6, method_dry_end="total", **kw), "YS-JAN"),
        (lambda: m.rain_season(da["pr"], thresh_wet_start="2 cm", window_not_dry_start=10, date_min_start="03-01", date_min_end="06-01", freq="YS-JAN"),
         rainseason.rain_season(f["pr"], 20.0, window_not_dry_start=10, date_min_start="03-01", date_min_end="06-01", **kw), "YS-JAN"),
    ]
    for call, want, freq in calls:
        trace = dev.start_trace()
        try:
            out = call()
        finally:
            dev.stop_trace()
        assert [n for n, _ in trace if n.startswith("xh_")] == ["xh_rain_season"]
        assert isinstance(out, tuple) and len(out) == 3
        assert not np.isnan(want.rain_season_start).all() and not np.isnan(want.rain_season_end).all()
        for got, w, attrs in zip(out, want, ({"units": "", "is_dayofyear": np.int32(1)},) * 2 + ({"units": "days"},)):
            assert got.dims == ("time", "lat", "lon") and got.attrs == attrs and set(got.coords) >= {"lat", "lon", "time"}
            assert all(type(got.attrs[k]) is type(v) for k, v in attrs.items())
            np.testing.assert_array_equal(got.values, w)
            starts = t.segments(freq)[1]
            assert len(got["time"].values) == len(starts)
            np.testing.assert_array_equal(got["time"].dt.year.values, [y for y, _ in starts])
            np.testing.assert_array_equal(got["time"].dt.month.values, [mm for _, mm in starts])
    assert not reached


def test_a_rate_in_kg_m2_s_is_an_amount_per_day(dev, wired):
    """rate2amount: the flux units come from the ``units`` attribute.  The rate is the amount over 86400 rounded to float32; the
    thresholds are chosen between the grid values, so the rounding of the rate cannot move an answer."""
    mods, _, reached, _ = wired
    t, f, da = _fields(pr_units="mm/d")
    rate = (f["pr"].astype(np.float64) / DAY).astype(np.float32)
    out = mods["xclim.indices._agro"].rain_season(fakexr.field(rate, t, attrs={"units": "kg m-2 s-1"}), "19.9 mm", window_not_dry_start=10,
                                                  thresh_dry_start="0.9 mm", thresh_dry_end="0.1 mm", window_dry_end=8)
    want = rainseason.rain_season(f["pr"], 19.9, window_not_dry_start=10, thresh_dry_start=0.9, thresh_dry_end=0.1, window_dry_end=8, time=t,
                                  flux_units="mm/d", device=dev)
    for got, w in zip(out, want):
        np.testing.assert_array_equal(got.values, w)
    assert not np.isnan(want.rain_season_start).all() and not reached


def test_hardiness_zones_is_the_period_minimum_and_one_zone_launch(dev, wired):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._agro"]
    t, f, da = _fields(T=365 * 6)
    for call, want, freq in [
        (lambda: m.hardiness_zones(da["tasmin"], 3), rainseason.hardiness_zones(f["tasmin"], 3, time=t, units="degC", device=dev), "YS"),
        (lambda: m.hardiness_zones(da["tasmin"], window=2, method="anbg", freq="YS-JUL"),
         rainseason.hardiness_zones(f["tasmin"], 2, "anbg", "YS-JUL", time=t, units="degC", device=dev), "YS-JUL"),
    ]:
        trace = dev.start_trace()
        try:
            out = call()
        finally:
            dev.stop_trace()
        assert [n for n, _ in trace if n.startswith("xh_")] == ["xh_resample_reduce_f64", "xh_rolling_zones"]
        assert out.dims == ("time", "lat", "lon") and out.attrs == {"units": ""}
        np.testing.assert_array_equal(out.values, want)
        assert not np.isnan(want[-1]).any() and len(out["time"].values) == len(t.segments(freq)[1])
    kelvin = fakexr.field(f["tasmin"] + 273.15, t, attrs={"units": "K"})
    np.testing.assert_array_equal(m.hardiness_zones(kelvin, 3).values,
                                  rainseason.hardiness_zones(f["tasmin"] + 273.15, 3, time=t, units="K", device=dev))
    assert not reached


@pytest.mark.parametrize("form", ["chunked", "gappy", "units", "array", "window", "no_bounds", "zones_chunked", "zones_units", "zones_gappy"])
def test_forwarded_forms_reach_the_original(wired, form):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._agro"]
    t, f, da = _fields(T=400)
    keep = np.r_[0:10, 11:400]
    if form == "chunked":
        assert m.rain_season(fakexr.field(f["pr"], t, attrs={"units": "mm/d"}, chunks={"lat": 2})) == "original rain_season"
    elif form == "gappy":
        assert m.rain_season(fakexr.field(f["pr"][keep], t.subset(keep), attrs={"units": "mm/d"}), date_min_start="01-01",
                             date_min_end="01-01") == "original rain_season"
    elif form == "units":       # a precipitation unit this module has no keyword for
        assert m.rain_season(fakexr.field(f["pr"], t, attrs={"units": "in/d"})) == "original rain_season"
    elif form == "array":
        assert m.rain_season(f["pr"]) == "original rain_season"
    elif form == "window":      # a sum window beyond the ring of the kernel
        assert m.rain_season(da["pr"], window_wet_start=rainseason.RAIN_MAX_WINDOW + 1, date_min_start="01-01", date_min_end="01-01") == "original rain_season"
    elif form == "no_bounds":   # the 34 rows of 2001 have no row in the default bounds: xarray raises there, the reference answers
        assert m.rain_season(da["pr"]) == "original rain_season"
    elif form == "zones_chunked":
        assert m.hardiness_zones(fakexr.field(f["tasmin"], t, attrs={"units": "degC"}, chunks={"lat": 2})) == "original hardiness_zones"
    elif form == "zones_units":
        assert m.hardiness_zones(fakexr.field(f["tasmin"], t, attrs={"units": "degF"})) == "original hardiness_zones"
    else:
        assert m.hardiness_zones(fakexr.field(f["tasmin"][keep], t.subset(keep), attrs={"units": "degC"})) == "original hardiness_zones"
    assert len(reached) == 1


def test_errors_of_the_reference_are_raised_not_forwarded(wired):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._agro"]
    t, f, da = _fields(T=366)
    with pytest.raises(ValueError, match="Unknown method_dry_start: weekly."):
        m.rain_season(da["pr"], method_dry_start="weekly")
    with pytest.raises(NotImplementedError, match="Method must be one of `usda` or `anbg`. Got rhs."):
        m.hardiness_zones(da["tasmin"], method="rhs")
    assert not reached


def test_uninstall_restores_by_identity(wired):
    mods, _, _, originals = wired
    patch.uninstall()
    for m in mods.values():
        for n, fn in originals.items():
            assert getattr(m, n) is fn


def test_install_on_modules_without_both_names_replaces_neither(dev):
    """Replaced only when both are present: a module that lacks hardiness_zones keeps its rain_season."""
    reached = []
    mods, originals = _modules(reached, names=("rain_season",))
    try:
        names = patch.install(fakexr.make_env(), mods)
        assert not [n for n in names if n.split(".")[-1] in rainseason.ADAPTED]
        assert mods["xclim.indices._agro"].rain_season is originals["rain_season"]
    finally:
        patch.uninstall()
