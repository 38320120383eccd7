"""The xarray adapter of the thermal-comfort unit, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like the
reference — ``xclim.indices.converters`` defines the three functions, ``xclim.indices`` and ``xclim.indices._conversion`` re-export
them, and the two Converter indicators hold them as a staticmethod ``compute`` — with the DataArray stand-in of tests/fakexr.py.
The stand-in originals only record that they were reached (the forwarded forms)."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fakexr  # noqa: E402

from poisoned import poisoned_outputs  # noqa: E402,F401
from xclim_amd import thermal  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402
from xclim_amd.xr_adapter import Env  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("saturation_vapor_pressure", "mean_radiant_temperature", "universal_thermal_climate_index")
NY, NX = 4, 3
LAT, LON = np.linspace(-60, 60, NY), np.array([-100.0, 10.0, 120.0])


def _env():
    base = fakexr.make_env()

    def convert_units_to(source, target, context=None):
        """Fields into the units named by ``target`` (one multiplication), threshold strings into the units of a DataArray target."""
        if isinstance(source, str):
            v, u = source.split(" ", 1)
            return float(v) + (273.15 if u in ("degC", "°C") else 0.0)
        factor = {("km/h", "m s-1"): 1 / 3.6, ("1", "%"): 100.0}[(source.attrs["units"], target)]
        out = source * source.values.dtype.type(factor)
        out.attrs = dict(source.attrs, units=target)
        return out

    return Env(fakexr.DataArray, convert_units_to, base.to_agg_units)


@pytest.fixture()
def wired(dev):
    from xclim_amd import _capi as capi
    from xclim_amd import patch

    old = capi._default_device
    capi._default_device = dev   # (the adapters take the default device: on the host simulation that is the session's)

    reached = []
    conv = types.ModuleType("xclim.indices.converters")
    for n in NAMES:
        def orig(*a, _n=n, **k):
            reached.append(_n)
            return f"original {_n}"
        setattr(conv, n, orig)
    conv._gather_lat = lambda da: fakexr.DataArray(LAT, dims=("lat",))

    def _gather_lon(da):
        if da.attrs.get("no_lon"):
            raise ValueError("No longitude coordinate")
        return fakexr.DataArray(LON, dims=("lon",))

    conv._gather_lon = _gather_lon
    originals = {n: getattr(conv, n) for n in NAMES}
    pub, conversion = types.ModuleType("xclim.indices"), types.ModuleType("xclim.indices._conversion")
    for m in (pub, conversion):
        for n in NAMES:
            setattr(m, n, originals[n])
    ind = types.ModuleType("xclim.indicators.convert._conversion")
    for n in NAMES[1:]:
        ind.__dict__[n] = type(f"Converter_{n}", (), {"compute": staticmethod(originals[n])})()
    mods = {"xclim.indices.converters": conv, "xclim.indices": pub, "xclim.indices._conversion": conversion,
            "xclim.indicators.convert._conversion": ind}
    names = patch.install(_env(), mods)
    try:
        yield mods, names, reached, originals
    finally:
        patch.uninstall()
        capi._default_device = old


def _coord(t, sub):
    n = sub.steps_per_day if sub else 1
    rep = TimeAxis(np.repeat(t.year, n), np.repeat(t.month, n), np.repeat(t.day, n), t.calendar)
    c = fakexr.time_coord(rep)
    s = np.tile(sub.seconds(), len(t)) if sub else np.zeros(len(t), np.int64)
    c._fields.update(hour=s // 3600, minute=s % 3600 // 60, second=s % 60)
    return c


def _fields(sub, dtype=np.float32, **attrs):
    rng = np.random.default_rng(4)
    t = TimeAxis.daily("2001-06-20", 3, "noleap")
    R = 3 * (sub.steps_per_day if sub else 1)
    tas = rng.uniform(270, 305, (R, NY, NX))
    f = {"tas": tas, "hurs": rng.uniform(10, 90, (R, NY, NX)), "sfcWind": rng.uniform(1, 12, (R, NY, NX)), "rsds": rng.uniform(0, 300, (R, NY, NX)),
         "rlds": 0.8 * 5.67e-8 * tas**4, "rlus": 5.67e-8 * tas**4}
    f["rsus"] = 0.2 * f["rsds"]
    f = {k: v.astype(dtype) for k, v in f.items()}
    units = dict(thermal._CF_UNITS)
    coords = {"lat": np.arange(NY), "lon": np.arange(NX), "time": _coord(t, sub)}
    da = {k: fakexr.DataArray(v, coords=coords, dims=("time", "lat", "lon"), attrs=dict(attrs, units=units[k])) for k, v in f.items()}
    return t, f, da


def test_install_replaces_functions_reexports_and_indicator_computes(wired):
    mods, names, _, originals = wired
    for modname in ("xclim.indices.converters", "xclim.indices", "xclim.indices._conversion"):
        for n in NAMES:
            assert f"{modname}.{n}" in names
            assert getattr(mods[modname], n).__wrapped__ is originals[n]
            assert getattr(mods[modname], n) is getattr(mods["xclim.indices.converters"], n)
    for n in NAMES[1:]:
        assert f"xclim.indicators.convert._conversion.{n}.compute" in names
        assert type(mods["xclim.indicators.convert._conversion"].__dict__[n]).__dict__["compute"].__func__.__wrapped__ is originals[n]


@pytest.mark.parametrize("sub", [None, thermal.SubDaily(8), thermal.SubDaily(24, 1800)], ids=["daily", "3hourly", "hourly0030"])
def test_served_calls_reach_the_kernel(wired, sub):
    mods, _, reached, _ = wired
    conv, ind = mods["xclim.indices.converters"], mods["xclim.indicators.convert._conversion"]
    t, f, da = _fields(sub)
    dev = get_device()
    dev.trace = []
    try:
        utci = mods["xclim.indices"].universal_thermal_climate_index(**da)
        mrt = ind.mean_radiant_temperature.compute(da["rsds"], da["rsus"], da["rlds"], da["rlus"], stat="instant")
        given = ind.universal_thermal_climate_index.compute(da["tas"], da["hurs"], da["sfcWind"], mrt=mrt, wind_cap_min=True)
        es = conv.saturation_vapor_pressure(da["tas"], ice_thresh="0 degC", method="SO90")
        launched = [n for n, _ in dev.trace]
    finally:
        dev.trace = None
    assert not reached
    assert launched.count("xh_thermal_comfort") == 3 and launched.count("xh_esat") == 1
    kw = dict(lat=LAT[:, None], lon=LON[None, :], time=t, subdaily=sub)
    assert utci.dims == ("time", "lat", "lon") and utci.attrs["units"] == "degC" and utci.values.dtype == np.float32
    np.testing.assert_array_equal(utci.values, thermal.universal_thermal_climate_index(**f, **kw))
    assert mrt.attrs["units"] == "K" and mrt.values.dtype == np.float64
    exp_mrt = thermal.mean_radiant_temperature(f["rsds"], f["rsus"], f["rlds"], f["rlus"], stat="instant", **kw)
    np.testing.assert_array_equal(mrt.values, exp_mrt)
    np.testing.assert_array_equal(given.values, thermal.universal_thermal_climate_index(f["tas"].astype(np.float64), f["hurs"].astype(np.float64),
                                                                                        f["sfcWind"].astype(np.float64), mrt=exp_mrt, wind_cap_min=True))
    assert es.attrs["units"] == "Pa"
    np.testing.assert_array_equal(es.values, thermal.saturation_vapor_pressure(f["tas"], 273.15, "sonntag90"))
    assert utci["time"] is da["tas"]["time"] or np.array_equal(utci["time"].values, da["tas"]["time"].values)


def test_units_are_converted(wired):
    mods, _, reached, _ = wired
    t, f, da = _fields(None, np.float64)
    kmh = da["sfcWind"] * 3.6
    kmh.attrs = {"units": "km/h"}
    frac = da["hurs"] * 0.01
    frac.attrs = {"units": "1"}
    got = mods["xclim.indices.converters"].universal_thermal_climate_index(da["tas"], frac, kmh, mrt=da["tas"])
    exp = thermal.universal_thermal_climate_index(f["tas"], (f["hurs"] * 0.01) * 100.0, (f["sfcWind"] * 3.6) * (1 / 3.6), mrt=f["tas"])
    np.testing.assert_array_equal(got.values, exp)
    assert not reached


@pytest.mark.parametrize("form", ["chunked", "no_lon", "gappy", "ragged_hours"])
def test_forwarded_forms_reach_the_original(wired, form):
    mods, _, reached, _ = wired
    conv = mods["xclim.indices.converters"]
    sub = thermal.SubDaily(8)
    t, f, da = _fields(sub, no_lon=True) if form == "no_lon" else _fields(sub)
    args = [da[k] for k in ("rsds", "rsus", "rlds", "rlus")]
    kw = {}
    if form == "chunked":
        args[0] = fakexr.DataArray(fakexr.field(f["rsds"], TimeAxis.daily("2001-06-20", 24, "noleap"), chunks={"lat": 2}).data, coords=dict(da["rsds"].coords),
                                   dims=("time", "lat", "lon"), attrs={"units": "W m-2"})
    elif form == "gappy":
        keep = np.r_[0:8, 16:24]
        c = fakexr.time_coord_like(da["rsds"]["time"], keep)
        args = [fakexr.DataArray(f[k][keep], coords={"lat": np.arange(NY), "lon": np.arange(NX), "time": c}, dims=("time", "lat", "lon"),
                                 attrs={"units": "W m-2"}) for k in ("rsds", "rsus", "rlds", "rlus")]
    elif form == "ragged_hours":
        da["rsds"]["time"]._fields["hour"][3] += 1
    assert conv.mean_radiant_temperature(*args, **kw) == "original mean_radiant_temperature"
    assert reached == ["mean_radiant_temperature"]


def test_another_stat_is_the_reference_s_error(wired):
    mods, _, reached, _ = wired
    t, f, da = _fields(None)
    with pytest.raises(NotImplementedError, match="'instant' or 'sunlit'"):
        mods["xclim.indices.converters"].mean_radiant_temperature(da["rsds"], da["rsus"], da["rlds"], da["rlus"], stat="average")
    assert not reached


def test_uninstall_restores(wired):
    from xclim_amd import patch

    mods, _, _, originals = wired
    patch.uninstall()
    for modname in ("xclim.indices.converters", "xclim.indices", "xclim.indices._conversion"):
        for n in NAMES:
            assert getattr(mods[modname], n) is originals[n]
    for n in NAMES[1:]:
        assert type(mods["xclim.indicators.convert._conversion"].__dict__[n]).__dict__["compute"].__func__ is originals[n]
