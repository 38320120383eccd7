"""The xarray adapter of the six agroclimatic period functions, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired
like the reference — ``xclim.indices._agro`` defines the functions (with the reference's signatures) and ``_gather_lat``, and
``xclim.indices`` re-exports the same objects — with the DataArray stand-in of tests/fakexr.py and the units of
tests/fakeunits.py.  The stand-in originals only record that they were reached (the forwarded forms)."""

import types

import numpy as np
import pytest

import fakexr
from xclim_amd import agro, patch
from xclim_amd.calendar import select_time_mask
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
DAY = 86400.0
# the reference's signatures (_agro.py:151-161, 275-288, 447-451, 532-538, 728-733, 1292-1301): the adapters bind against them
SIGS = {
    "huglin_index": "tas, tasmax, lat=None, thresh='10 degC', method='smoothed', cap_value=1.0, start_date='04-01', end_date='10-01', freq='YS'",
    "biologically_effective_degree_days": "tasmin, tasmax, lat=None, thresh_tasmin='10 degC', method='gladstones', cap_value=1.0, "
                                          "low_dtr='10 degC', high_dtr='13 degC', max_daily_degree_days='9 degC', start_date='04-01', "
                                          "end_date='11-01', freq='YS'",
    "cool_night_index": "tasmin, lat=None, freq='YS'",
    "dryness_index": "pr, evspsblpot, lat=None, wo='200 mm', freq='YS'",
    "latitude_temperature_index": "tas, lat=None, lat_factor=75, freq='YS'",
    "effective_growing_degree_days": "tasmax, tasmin, *, thresh='5 degC', method='bootsma', after_date='07-01', dim='time', freq='YS'",
}
LATS = np.array([-52.0, 38.0, 47.0])


def _modules(reached, with_agro=True):
    mod, pkg = types.ModuleType("xclim.indices._agro"), types.ModuleType("xclim.indices")
    originals = {}
    if with_agro:
        for name, sig in SIGS.items():
            ns = {"reached": reached}
            exec(f"def {name}({sig}):\n    reached.append({name!r})\n    return 'original {name}'\n", ns)
            originals[name] = ns[name]
            setattr(mod, name, ns[name])
            setattr(pkg, name, ns[name])
        mod._gather_lat = lambda da: fakexr.DataArray(LATS[:da.shape[da.dims.index("lat")]], dims=("lat",))
    for name in ("corn_heat_units", "qian_weighted_mean_average", "_chill_portion_one_season"):   # not replaced by this unit
        fn = lambda *a, _n=name, **k: "original " + _n  # noqa: E731
        setattr(mod, name, fn)
    pkg.corn_heat_units = mod.corn_heat_units
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


def _fields(T=731, start="2000-01-01", ny=3, nx=2, tunits="K"):
    rng = np.random.default_rng(11)
    t = TimeAxis.daily(start, T)
    doy = t.doy[:, None, None]
    phase = np.where(LATS[:ny] >= 0, 105.0, 287.0)[None, :, None]
    tas = 284 + 11 * np.sin(2 * np.pi * (doy - phase) / 365) + rng.normal(0, 3, (T, ny, nx)) - (273.15 if tunits == "degC" else 0)
    f = {"tas": tas, "tasmin": tas - rng.uniform(2, 9, (T, ny, nx)), "tasmax": tas + rng.uniform(2, 9, (T, ny, nx)),
         "pr": np.maximum(rng.normal(2.5, 4, (T, ny, nx)), 0) / DAY, "evspsblpot": np.maximum(rng.normal(2.5, 1, (T, ny, nx)), 0) / DAY}
    f = {k: v.astype(np.float32) for k, v in f.items()}
    f["tas"][5, 0, 0] = np.nan
    attrs = {k: {"units": "kg m-2 s-1"} if k in ("pr", "evspsblpot") else {"units": tunits, "standard_name": "air_temperature"} for k in f}
    return t, f, {k: fakexr.field(v, t, attrs=attrs[k]) for k, v in f.items()}


def test_install_replaces_the_six_where_defined_and_where_re_exported(wired):
    mods, names, _, originals = wired
    for modname, m in mods.items():
        for n, fn in originals.items():
            assert f"{modname}.{n}" in names
            assert getattr(m, n) is not fn and getattr(m, n).__wrapped__ is fn and getattr(m, n).__name__ == n
    assert set(originals) == set(agro.ADAPTED)
    assert not any(n.endswith(".corn_heat_units") or n.endswith(".qian_weighted_mean_average") for n in names)
    assert mods["xclim.indices"].corn_heat_units() == "original corn_heat_units"


@pytest.mark.parametrize("tunits", ["K", "degC"])
def test_served_calls_are_one_launch_each_with_the_reference_s_units(dev, wired, tunits):
    mods, _, reached, _ = wired
    m, pkg = mods["xclim.indices._agro"], mods["xclim.indices"]
    t, f, da = _fields(tunits=tunits)
    lat3 = LATS[:, None]
    lat_da = fakexr.DataArray(LATS, dims=("lat",))
    kw = dict(time=t, units=tunits, device=dev)
    both = ["xh_agro_degree_sum"]
    calls = [
        # (the call through the patched module, the mirror's value, units, the entry points it may reach, keeps the field's attributes)
        (lambda: m.huglin_index(da["tas"], da["tasmax"], lat_da, method="huglin"),
         agro.huglin_index(f["tas"], f["tasmax"], lat3, method="huglin", **kw), "", both, False),
        (lambda: pkg.huglin_index(da["tas"], da["tasmax"], method="interpolated", thresh="12 degC", end_date="11-01"),      # lat gathered
         agro.huglin_index(f["tas"], f["tasmax"], lat3, 12.0, method="interpolated", end_date="11-01", **kw), "", both, False),
        (lambda: m.biologically_effective_degree_days(da["tasmin"], da["tasmax"], method="gladstones"),                     # lat gathered
         agro.biologically_effective_degree_days(f["tasmin"], f["tasmax"], lat3, **kw), "K days", ["xh_solar_table"] + both, False),
        (lambda: pkg.biologically_effective_degree_days(da["tasmin"], da["tasmax"], lat_da, method="jones", freq="YS-JAN"),
         agro.biologically_effective_degree_days(f["tasmin"], f["tasmax"], lat3, method="jones", freq="YS-JAN", **kw), "K days",
         ["xh_solar_table"] + both, False),
        (lambda: m.cool_night_index(da["tasmin"]), agro.cool_night_index(f["tasmin"], lat3, **kw), "degC", ["xh_agro_monthly"], True),
        (lambda: m.cool_night_index(da["tasmin"], "south"), agro.cool_night_index(f["tasmin"], "south", **kw), "degC", ["xh_agro_monthly"], True),
        (lambda: pkg.dryness_index(da["pr"], da["evspsblpot"], lat_da, wo="30 cm"),
         agro.dryness_index(f["pr"], f["evspsblpot"], lat3, 300.0, time=t, device=dev), "mm", ["xh_agro_monthly"], False),
        (lambda: m.latitude_temperature_index(da["tas"], lat_factor=60), agro.latitude_temperature_index(f["tas"], lat3, 60, **kw), "",
         ["xh_agro_monthly"], False),
        (lambda: m.effective_growing_degree_days(da["tasmax"], da["tasmin"], method="qian", thresh="6 degC"),
         agro.effective_growing_degree_days(f["tasmax"], f["tasmin"], method="qian", thresh=6.0, **kw), "degC days", ["xh_egdd"], False),
    ]
    for call, want, units, entry_points, keeps in calls:
        trace = dev.start_trace()
        try:
            out = call()
        finally:
            dev.stop_trace()
        assert [n for n, _ in trace if n.startswith("xh_")] == entry_points
        assert out.dims == ("time", "lat", "lon") and out.attrs["units"] == units, (out.dims, out.attrs)
        assert (out.attrs.get("standard_name") == "air_temperature") == keeps
        np.testing.assert_array_equal(out.values, want)
        np.testing.assert_array_equal(out["time"].dt.year.values, [2000, 2001])
        assert set(out.coords) >= {"lat", "lon"}
    assert not reached


@pytest.mark.parametrize("name", ["huglin_index", "biologically_effective_degree_days"])
def test_the_season_sums_keep_every_period_of_the_series(dev, wired, name):
    """select_time of the reference keeps the whole axis (drop=False), so resample(time="MS").sum() gives every month of the series:
    0 where no day of the season falls."""
    mods, _, reached, _ = wired
    t, f, da = _fields(T=400, start="2001-02-10")          # February 2001 .. mid-March 2002: 14 months
    if name == "huglin_index":
        out = mods["xclim.indices._agro"].huglin_index(da["tas"], da["tasmax"], method="huglin", freq="MS")
        full = agro.huglin_index(f["tas"], f["tasmax"], LATS[:, None], method="huglin", freq="MS", time=t, device=dev)
        end = "10-01"
    else:
        out = mods["xclim.indices"].biologically_effective_degree_days(da["tasmin"], da["tasmax"], method="huglin", freq="MS")
        full = agro.biologically_effective_degree_days(f["tasmin"], f["tasmax"], LATS[:, None], method="huglin", freq="MS", time=t, device=dev)
        end = "11-01"
    sel = select_time_mask(t, date_bounds=("04-01", end), include_bounds=(True, False))
    seg, starts = t.segments("MS")
    has = np.array([sel[a:b].any() for a, b in zip(seg[:-1], seg[1:])])
    assert len(has) == 14 and has.sum() == (6 if end == "10-01" else 7) and not has[0] and not has[-1]
    assert out.values.shape == (14, 3, 2)
    np.testing.assert_array_equal(out.values, full)
    assert (out.values[~has] == 0).all() and (out.values[has] > 0).any()
    np.testing.assert_array_equal(out["time"].dt.month.values, [m for _, m in starts])
    np.testing.assert_array_equal(out["time"].dt.year.values, [y for y, _ in starts])
    assert not reached


def test_warnings_of_the_reference_come_through(wired):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._agro"]
    _, _, da = _fields(T=400)
    lat_da = fakexr.DataArray(LATS, dims=("lat",))
    with pytest.warns(DeprecationWarning, match="icclim"):
        m.huglin_index(da["tas"], da["tasmax"], lat_da, method="icclim")
    with pytest.warns(UserWarning, match="not used for method 'icclim'"):
        m.biologically_effective_degree_days(da["tasmin"], da["tasmax"], lat_da, method="icclim", end_date="10-01")
    with pytest.raises(NotImplementedError):                 # the reference's own default: method="smoothed"
        m.huglin_index(da["tas"], da["tasmax"], lat_da)
    with pytest.raises(NotImplementedError):
        m.biologically_effective_degree_days(da["tasmin"], da["tasmax"], lat_da, method="jones", freq="MS")
    with pytest.raises(ValueError, match="Freq not allowed"):
        m.cool_night_index(da["tasmin"], "north", freq="YS-JUL")
    assert not reached


@pytest.mark.parametrize("form", ["chunked", "gappy", "units", "dims", "array", "notserved", "threshold"])
def test_forwarded_forms_reach_the_original(wired, form):
    mods, _, reached, _ = wired
    m = mods["xclim.indices._agro"]
    t, f, da = _fields(T=400)
    tas, tasmax, kw = da["tas"], da["tasmax"], {}
    if form == "chunked":
        tas = fakexr.field(f["tas"], t, attrs={"units": "K"}, chunks={"lat": 2})
    elif form == "gappy":
        keep = np.r_[0:10, 11:400]
        t2 = t.subset(keep)
        tas, tasmax = (fakexr.field(f[k][keep], t2, attrs={"units": "K"}) for k in ("tas", "tasmax"))
    elif form == "units":
        tasmax = fakexr.field(f["tasmax"], t, attrs={"units": "degF"})
    elif form == "dims":
        tasmax = fakexr.field(f["tasmax"][:, :, :1], t, attrs={"units": "K"})
    elif form == "array":
        tas = f["tas"]
    elif form == "threshold":
        kw = {"thresh": fakexr.DataArray(np.full(3, 283.15), dims=("lat",), attrs={"units": "K"})}
    if form == "notserved":      # an axis that does not run from a 1 January to a 31 December
        assert m.dryness_index(da["pr"], da["evspsblpot"], "north") == "original dryness_index"
        assert reached == ["dryness_index"]
        return
    assert m.huglin_index(tas, tasmax, method="huglin", **kw) == "original huglin_index"
    assert reached == ["huglin_index"]


def test_uninstall_restores_by_identity(wired):
    mods, _, _, originals = wired
    patch.uninstall()
    for m in mods.values():
        for n, fn in originals.items():
            assert getattr(m, n) is fn


def test_install_on_modules_without_the_new_names_replaces_nothing_new(dev):
    """The stand-in modules of the older adapter tests hold _chill_portion_one_season and nothing of this unit."""
    reached = []
    mods, _ = _modules(reached, with_agro=False)
    try:
        names = patch.install(fakexr.make_env(), mods)
        assert not [n for n in names if n.split(".")[-1] in agro.ADAPTED]
        assert "xclim.indices._agro._chill_portion_one_season" in names
        assert not any(hasattr(mods["xclim.indices._agro"], n) for n in agro.ADAPTED)
    finally:
        patch.uninstall()
