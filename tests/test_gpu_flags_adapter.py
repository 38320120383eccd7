"""The xarray adapter of data_flags, EXECUTED: ``patch.install(env, modules)`` on a stand-in ``xclim.core.dataflags`` that holds
``data_flags`` (with the reference's signature; it only records that it was reached), ``ecad_compliant`` (which calls ``data_flags``
through the module global, as the reference's does), ``_REGISTRY`` with the thirteen checks under the reference's signatures,
``VARIABLES`` from tests/golden/flags_defaults.json, ``DataQualityException``, ``update_xclim_history`` and an ``xarray`` whose
``Dataset`` is the minimal one below — with the DataArray stand-in of tests/fakexr.py and the units of tests/fakeunits.py."""
import functools
import inspect
import types
from collections import OrderedDict

import numpy as np
import pytest

import fakexr
import flagscpu as R
from stridedabi import FLAGS_TABLE
from test_flags_cpu import DEFAULTS
from xclim_amd import dataflags, patch
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
MODULE = "xclim.core.dataflags"
T = 1096
TIME = TimeAxis.daily("1971-01-01", T)
# the reference's signatures (core/dataflags.py): the history entries bind against them
SIGS = {
    "tasmax_below_tasmin": "tasmax, tasmin", "tas_exceeds_tasmax": "tas, tasmax", "tas_below_tasmin": "tas, tasmin",
    "temperature_extremely_low": "da, *, thresh='-90 degC'", "temperature_extremely_high": "da, *, thresh='60 degC'",
    "negative_accumulation_values": "da", "very_large_precipitation_events": "da, *, thresh='300 mm d-1'",
    "values_op_thresh_repeating_for_n_or_more_days": "da, *, n, thresh, op='=='",
    "wind_values_outside_of_bounds": "da, *, lower='0 m s-1', upper='46 m s-1'",
    "outside_n_standard_deviations_of_climatology": "da, *, n, window=5", "values_repeating_for_n_or_more_days": "da, *, n",
    "percentage_values_outside_of_bounds": "da", "specific_discharge_extremely_high": "da, *, thresh='100 mm d-1'",
}


class Dataset:
    """As much of xarray.Dataset as data_flags and DataQualityException touch."""

    def __init__(self, data_vars=None):
        self.data_vars = OrderedDict(data_vars or {})

    def __getitem__(self, key):
        return self.data_vars[key]

    def __contains__(self, key):
        return key in self.data_vars


def update_xclim_history(func):
    """A stand-in for core/formatting.py's decorator: the call, bound against the function's signature, as the result's history."""

    @functools.wraps(func)
    def wrapper(*args, **kwargs):
        out = func(*args, **kwargs)
        bound = inspect.signature(func).bind(*args, **kwargs)
        shown = ", ".join(f"{k}={v.name if isinstance(v, fakexr.DataArray) else repr(v)}" for k, v in bound.arguments.items())
        out.attrs["history"] = f"{func.__name__}({shown})"
        return out

    return wrapper


def _module(reached):
    mod = types.ModuleType(MODULE)
    mod.reached = reached
    mod.xarray = types.SimpleNamespace(Dataset=Dataset)
    mod.VARIABLES = DEFAULTS
    mod.DataQualityException = dataflags.DataQualityException
    mod.update_xclim_history = update_xclim_history
    mod._REGISTRY = {}
    for name, sig in SIGS.items():
        exec(f"def {name}({sig}):\n    reached.append({name!r})\n    return 'original {name}'\n", mod.__dict__)
        if name != "specific_discharge_extremely_high":          # (the reference does not register it)
            mod._REGISTRY[name] = mod.__dict__[name]
    exec("def data_flags(da, ds=None, flags=None, dims='all', freq=None, raise_flags=False):\n"
         "    reached.append('data_flags')\n    return 'original data_flags'\n"
         "def ecad_compliant(ds, dims='all', raise_flags=False, append=True):\n"
         "    return {var: data_flags(ds[var], ds, dims=dims) for var in ds.data_vars}\n", mod.__dict__)
    return mod


@pytest.fixture()
def wired(dev):
    import xclim_amd._capi as capi

    reached = []
    mod = _module(reached)
    original = mod.data_flags
    old = capi._default_device
    capi._default_device = dev
    names = patch.install(fakexr.make_env(), {MODULE: mod})
    try:
        yield mod, names, reached, original
    finally:
        patch.uninstall()
        capi._default_device = old


def fields(dtype=np.float32, chunks=None):
    rng = np.random.default_rng(4)
    shape = (T, 3, 4)
    tas = (283.0 + 10.0 * np.sin(2 * np.pi * (TIME.doy[:, None, None] - 110) / 365.25) + rng.normal(0, 2.0, shape)).astype(dtype)
    raw = {"tas": tas, "tasmax": (tas + dtype(4.0)).astype(dtype), "tasmin": (tas - dtype(4.0)).astype(dtype)}
    tas[800, 2, 3] = 340.0
    tas[30, 0, 0] = 150.0
    tas[500:506, 1, 2] = 285.0
    tas[901, 1, 1] = np.nan
    attrs = {"units": "K", "standard_name": "air_temperature"}
    das = {k: fakexr.field(v, TIME, attrs=attrs, name=k, chunks=chunks if k == "tas" else None) for k, v in raw.items()}
    return raw, das, Dataset(das)


def test_install_replaces_data_flags_and_uninstall_restores_it(wired):
    mod, names, reached, original = wired
    assert f"{MODULE}.data_flags" in names
    assert mod.data_flags is not original and mod.data_flags.__wrapped__ is original and mod.data_flags.__name__ == "data_flags"
    assert dataflags.ADAPTED == ("data_flags",)
    patch.uninstall()
    assert mod.data_flags is original and not reached


def test_the_six_checks_of_tas_are_one_launch(wired, dev):
    mod, _, reached, _ = wired
    raw, das, ds = fields()
    trace = dev.start_trace()
    try:
        got = mod.data_flags(das["tas"], ds)
    finally:
        dev.stop_trace()
    assert [n for n, _ in trace if n in FLAGS_TABLE] == ["xh_doy_bounds", "xh_data_flags"] and not reached
    assert isinstance(got, Dataset)
    want = R.data_flags(raw["tas"], raw, None, name="tas", time=TIME, units="K", variables=DEFAULTS)
    assert list(got.data_vars) == list(want) and len(want) == 6
    for k, v in got.data_vars.items():
        assert isinstance(v, fakexr.DataArray) and v.dims == () and v.values.dtype == bool and v.name == k
        assert bool(v.values) is bool(want[k]) is True, k
        assert v.attrs["units"] == ""
    d = {k: v.attrs["description"] for k, v in got.data_vars.items()}
    assert d["temperature_extremely_high"] == "Temperatures found in excess of 60 degC in tas."
    assert d["tas_below_tasmin"] == "Mean temperature values found below minimum temperatures."
    assert d["outside_5_standard_deviations_of_climatology"] == ("Values outside of 5 standard deviations from climatology found for tas with "
                                                                 "moving window of 5 days.")
    h = {k: v.attrs["history"] for k, v in got.data_vars.items()}
    assert h["temperature_extremely_low"] == "temperature_extremely_low(da=tas, thresh='-90 degC')"
    assert h["tas_exceeds_tasmax"] == "tas_exceeds_tasmax(tas=tas, tasmax=tasmax)"
    assert h["values_repeating_for_5_or_more_days"] == "values_repeating_for_n_or_more_days(da=tas, n=5)"


@pytest.mark.parametrize("dims,freq,out_dims", [(None, None, ("time", "lat", "lon")), ("time", None, ("lat", "lon")), (("lat", "lon"), None, ("time",)),
                                                (None, "YS", ("time", "lat", "lon")), ("all", "YS", ("time",)), (["lon", "lat", "time"], None, ())])
def test_dims_and_freq(wired, dims, freq, out_dims):
    mod, _, reached, _ = wired
    raw, das, ds = fields(np.float64)
    got = mod.data_flags(das["tas"].transpose("lat", "time", "lon"), ds, dims=dims, freq=freq)
    mirror_dims = {(): "all", ("time",): "cells", ("lat", "lon"): "time", ("time", "lat", "lon"): None}[out_dims]
    want = R.data_flags(raw["tas"], raw, None, mirror_dims, freq, name="tas", time=TIME, units="K", variables=DEFAULTS)
    assert not reached and list(got.data_vars) == list(want)
    for k, v in got.data_vars.items():
        assert v.dims == out_dims and v.attrs["description"] and "history" in v.attrs
        np.testing.assert_array_equal(v.values, want[k], err_msg=k)
        if "time" in out_dims:
            assert len(v["time"].values) == (3 if freq else T) and v["time"].values[0] == das["tas"]["time"].values[0]
        if "lat" in out_dims:
            np.testing.assert_array_equal(v["lat"].values, np.arange(3))


def test_flags_given_by_the_caller_and_absent_companions(wired):
    mod, _, reached, _ = wired
    raw, das, _ = fields()
    flags = {"temperature_extremely_high": {"thresh": "330 K"}, "tas_exceeds_tasmax": None,
             "values_op_thresh_repeating_for_n_or_more_days": {"op": "==", "n": 6, "thresh": "11.85 degC"}}
    got = mod.data_flags(das["tas"], Dataset({"tas": das["tas"]}), flags=flags, dims=None)
    assert list(got.data_vars) == ["temperature_extremely_high", "tas_exceeds_tasmax", "values_eq_11point85_repeating_for_6_or_more_days"]
    assert got["tas_exceeds_tasmax"] is None and not reached
    np.testing.assert_array_equal(got["temperature_extremely_high"].values, raw["tas"].astype(np.float64) > 330.0)
    rep = got["values_eq_11point85_repeating_for_6_or_more_days"]
    assert rep.values.sum() == 6 and rep.values[500:506, 1, 2].all()
    assert rep.attrs["description"] == f"Repetitive values at {11.85 + 273.15} for at least 6 days found for tas."
    assert got["temperature_extremely_high"].attrs["description"] == "Temperatures found in excess of 330 K in tas."


def test_raise_flags(wired):
    mod, _, _, _ = wired
    _, das, ds = fields()
    with pytest.raises(mod.DataQualityException, match="Temperatures found below -90 degC in tas.") as err:
        mod.data_flags(das["tas"], ds, raise_flags=True)
    assert str(err.value).startswith("Data quality flags indicate suspicious values. Flags raised are:\n  - Temperatures found in excess of")
    assert len(err.value.flags) == 6 and isinstance(err.value.flag_array, Dataset)


def test_ecad_compliant_is_served_through_the_module_global(wired, dev):
    mod, _, reached, _ = wired
    _, das, ds = fields()
    trace = dev.start_trace()
    try:
        got = mod.ecad_compliant(ds)
    finally:
        dev.stop_trace()
    assert not reached and set(got) == {"tas", "tasmax", "tasmin"} and all(isinstance(v, Dataset) for v in got.values())
    assert [n for n, _ in trace if n in FLAGS_TABLE] == ["xh_doy_bounds", "xh_data_flags"] * 3


def test_forwarded_forms_reach_the_original(wired):
    mod, _, reached, _ = wired
    _, das, ds = fields()
    _, chunked, _ = fields(chunks={"lat": 2})
    assert mod.data_flags(chunked["tas"], ds) == "original data_flags"                           # a chunked field
    assert mod.data_flags(das["tas"], ds, dims="lat") == "original data_flags"                   # some of the non-time dimensions
    assert mod.data_flags(das["tas"], ds, dims=("time", "lon")) == "original data_flags"
    mod._REGISTRY["my_check"] = lambda da: da                                                    # a user-registered check
    assert mod.data_flags(das["tas"], ds, flags={"my_check": None}) == "original data_flags"
    mod._REGISTRY["negative_accumulation_values"] = lambda da: da                                # ... and one that replaces a check of the reference
    assert mod.data_flags(das["tas"], ds, flags={"negative_accumulation_values": None}) == "original data_flags"
    ints = fakexr.field(np.ones((T, 3, 4), np.int32), TIME, attrs={"units": "K"}, name="tas")     # NotServed: an integer field
    assert mod.data_flags(ints, ds, flags={"temperature_extremely_high": None}) == "original data_flags"
    other = fakexr.field(np.ones((T, 3, 4), np.float32), TIME, attrs={"units": "K"}, name="rls")  # a variable without checks
    assert mod.data_flags(other, ds) == "original data_flags"
    assert reached == ["data_flags"] * 7
    assert mod.data_flags(das["tas"], ds, flags={"temperature_extremely_high": None})["temperature_extremely_high"].values   # still served
