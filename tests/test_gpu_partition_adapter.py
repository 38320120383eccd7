"""The xarray adapter of the uncertainty-partitioning unit, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like
the reference — ``xclim.ensembles._partitioning`` defines the three partition functions next to its ``xr``,
``xclim.ensembles._base`` defines ``ensemble_mean_std_max_min`` next to ``xr`` and ``update_history``, and ``xclim.ensembles``
re-exports all four — with the DataArray stand-in of tests/fakexr.py and a Dataset that is a dict with ``attrs``.  The stand-in
originals only record that they were reached."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fakexr  # noqa: E402
import partitioncpu as P  # noqa: E402

from poisoned import poisoned_outputs  # noqa: E402,F401
from xclim_amd import partitioning  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

pytestmark = pytest.mark.gpu

PARTITIONS = ("hawkins_sutton", "lafferty_sriver", "general_partition")
DA = fakexr.DataArray


class Dataset(dict):
    def __init__(self, data_vars, attrs=None):
        super().__init__(data_vars)
        self.attrs = dict(attrs or {})

    data_vars = property(lambda self: self)


@pytest.fixture()
def wired(dev):
    from xclim_amd import _capi as capi
    from xclim_amd import patch

    old = capi._default_device
    capi._default_device = dev
    reached = []
    part, base, pub = (types.ModuleType(n) for n in ("xclim.ensembles._partitioning", "xclim.ensembles._base", "xclim.ensembles"))

    def hawkins_sutton(da, sm=None, weights=None, baseline=("1971", "2000"), kind="+"):
        reached.append("hawkins_sutton")
        return "original hawkins_sutton"

    def lafferty_sriver(da, sm=None, bb13=False):
        reached.append("lafferty_sriver")
        return "original lafferty_sriver"

    def general_partition(da, sm="poly", var_first=None, mean_first=None, weights=None):
        reached.append("general_partition")
        return "original general_partition"

    def ensemble_mean_std_max_min(ens, min_members=1, weights=None):
        reached.append("ensemble_mean_std_max_min")
        return "original ensemble_mean_std_max_min"

    for f in (hawkins_sutton, lafferty_sriver, general_partition):
        setattr(part, f.__name__, f)
        setattr(pub, f.__name__, f)
    base.ensemble_mean_std_max_min = pub.ensemble_mean_std_max_min = ensemble_mean_std_max_min
    part.xr = base.xr = types.SimpleNamespace(Dataset=Dataset, DataArray=DA)
    base.update_history = lambda text, ds: f"[stamp] {text}"
    mods = {part.__name__: part, base.__name__: base, pub.__name__: pub}
    originals = {f.__name__: f for f in (hawkins_sutton, lafferty_sriver, general_partition, ensemble_mean_std_max_min)}
    names = patch.install(fakexr.make_env(), mods)
    try:
        yield mods, names, reached, originals
    finally:
        patch.uninstall()
        capi._default_device = old


def annual(years):
    return TimeAxis(np.asarray(years), np.full(len(years), 12), np.full(len(years), 31), "standard")


def _da(name, dims_out, cells=6, attrs=None):
    """A family as a DataArray (time, members ..., lon) rearranged into ``dims_out``."""
    fam = P.family(name)
    a = np.ascontiguousarray(fam["da"][..., :cells])
    dims = {"hs": ("time", "scenario", "model", "lon"), "ls": ("time", "scenario", "model", "downscaling", "lon"),
            "gp": ("time", "scenario", "model", "reference", "adjustment", "lon")}[fam["func"]]
    coords = {"time": fakexr.time_coord(annual(fam["years"])), "lon": DA(np.arange(float(cells)), dims=("lon",), attrs={"axis": "X"})}
    for d, n in zip(dims[1:-1], a.shape[1:-1]):
        coords[d] = DA(np.array([f"{d[:3]}{k}" for k in range(n)]), dims=(d,))
    return fam, a, DA(a, dims=dims, coords=coords, name="tas", attrs=attrs or {}).transpose(*dims_out)


def test_the_four_functions_are_replaced_where_defined_and_where_re_exported(wired):
    mods, names, _, _ = wired
    for n in PARTITIONS:
        assert f"xclim.ensembles._partitioning.{n}" in names and f"xclim.ensembles.{n}" in names
        assert mods["xclim.ensembles"].__dict__[n] is mods["xclim.ensembles._partitioning"].__dict__[n]
    assert "xclim.ensembles._base.ensemble_mean_std_max_min" in names and "xclim.ensembles.ensemble_mean_std_max_min" in names


def test_hawkins_sutton_on_dataarrays_in_any_dimension_order(wired, dev):
    mods, _, reached, _ = wired
    fn = mods["xclim.ensembles"].hawkins_sutton
    fam, a, da = _da("hs_nan", ("lon", "scenario", "model", "time"))
    g_want, u_want = partitioning.hawkins_sutton(a, time=annual(fam["years"]), device=dev)
    g, u = fn(da)
    assert g.dims == ("lon", "time") and u.dims == ("uncertainty", "lon", "time") and not reached
    assert np.array_equal(g.values, g_want.T, equal_nan=True) and np.array_equal(u.values, np.swapaxes(u_want, 1, 2), equal_nan=True)
    assert u.coords["uncertainty"].values.tolist() == ["variability", "model", "scenario", "total"]
    assert u.attrs["model"].tolist() == ["mod0", "mod1", "mod2"] and u.attrs["scenario"].tolist() == ["sce0", "sce1"]
    assert sorted(u.attrs) == ["model", "scenario"] and g.coords["lon"].attrs == {"axis": "X"}
    # the members the other way round, weights, kind and baseline handed through
    fam, a, da = _da("hs_main", ("model", "time", "scenario", "lon"))
    w = DA(np.array([1.0, 0.0, 2.5]), dims=("model",))
    g, u = fn(da, None, w, ("1975", "1990"), "*")
    g_want, u_want = partitioning.hawkins_sutton(a, None, [1.0, 0.0, 2.5], ("1975", "1990"), "*", time=annual(fam["years"]), device=dev)
    assert g.dims == ("time", "lon") and np.array_equal(g.values, g_want, equal_nan=True) and np.array_equal(u.values, u_want, equal_nan=True)
    sm = DA(P.fit(a, P.stamps_ns(fam["years"]), 2)[0], dims=("time", "scenario", "model", "lon"))
    before = sm.values.copy()
    fn(_da("hs_main", ("time", "scenario", "model", "lon"))[2], sm)
    assert np.array_equal(sm.values, before) and not reached   # (the reference shifts the caller's sm in place; this does not)
    with pytest.raises(ValueError, match="This algorithm expects annual time series."):
        fn(da.isel(time=slice(0, 60, 2)))
    with pytest.raises(ValueError, match="Some models are missing data for some scenarios"):
        fn(_da("hs_missing", ("time", "scenario", "model", "lon"), cells=9)[2])
    with pytest.raises(ValueError, match=r"^\^$"):
        fn(da, kind="^")


def test_lafferty_sriver_and_general_partition_on_dataarrays(wired, dev):
    mods, _, reached, _ = wired
    fam, a, da = _da("ls_nan", ("downscaling", "lon", "time", "scenario", "model"))
    g_want, u_want = partitioning.lafferty_sriver(np.ascontiguousarray(np.moveaxis(a, 3, 1)), time=annual(fam["years"]),
                                                  dims=("downscaling", "scenario", "model"), device=dev)
    g, u = mods["xclim.ensembles"].lafferty_sriver(da)
    assert g.dims == ("lon", "time") and u.dims == ("uncertainty", "lon", "time")
    assert np.array_equal(g.values, g_want.T, equal_nan=True) and np.array_equal(u.values, np.swapaxes(u_want, 1, 2), equal_nan=True)
    assert u.coords["uncertainty"].values.tolist() == list(partitioning.LS_COMPONENTS)
    assert sorted(u.attrs) == ["downscaling", "model", "scenario"] and u.attrs["downscaling"].tolist() == ["dow0", "dow1"]
    g2, u2 = mods["xclim.ensembles._partitioning"].lafferty_sriver(da, bb13=True)
    assert not np.array_equal(u2.values[1], u.values[1], equal_nan=True) and np.array_equal(u2.values[0], u.values[0], equal_nan=True)
    attrs = {"long_name": "Mean temperature", "units": "K"}
    fam, a, da = _da("gp_nan", ("time", "scenario", "model", "reference", "adjustment", "lon"), attrs=attrs)
    g, u = mods["xclim.ensembles"].general_partition(da)
    g_want, u_want = partitioning.general_partition(a, time=annual(fam["years"]), dims=P.GP_DIMS, device=dev)
    assert np.array_equal(g.values, g_want, equal_nan=True) and np.array_equal(u.values, u_want, equal_nan=True)
    assert u.coords["uncertainty"].values.tolist() == ["scenario", "model", "reference", "adjustment", "variability", "total"]
    assert u.attrs["indicator_long_name"] == "Mean temperature" and u.attrs["indicator_units"] == "K"
    assert u.attrs["indicator_description"] == "unknown" and u.attrs["partition_fit"] == "poly"
    assert all(u.attrs[d].tolist() == [f"{d[:3]}0", f"{d[:3]}1"] for d in P.GP_DIMS)
    sm = DA(P.fit(a, P.stamps_ns(fam["years"]), 2)[0], dims=da.dims)
    _, u = mods["xclim.ensembles"].general_partition(da, sm)
    assert u.attrs["partition_fit"] == "unknown"
    with pytest.raises(ValueError, match="sm should be 'poly' or a DataArray."):
        mods["xclim.ensembles"].general_partition(da, "loess")
    with pytest.raises(ValueError, match="DataArray dimensions should include"):
        mods["xclim.ensembles"].general_partition(da, var_first=["model", "method"])
    assert not reached


def test_what_is_not_served_goes_to_the_original(wired):
    mods, _, reached, _ = wired
    pub = mods["xclim.ensembles"]
    fam, a, da = _da("ls_main", ("time", "scenario", "model", "downscaling", "lon"))
    ints = DA(a.astype(np.int32), dims=da.dims, coords=da.coords)
    assert pub.lafferty_sriver(ints) == "original lafferty_sriver"
    assert pub.lafferty_sriver(da, DA(a.astype(np.float32), dims=da.dims)) == "original lafferty_sriver"   # da float64, sm float32
    chunked = fakexr.field(a, annual(fam["years"]), dims=da.dims, chunks={"lon": 2})
    assert pub.lafferty_sriver(chunked) == "original lafferty_sriver"
    assert pub.general_partition(da, var_first=["model", "downscaling"], mean_first=["scenario"], weights=["scenario"]) == "original general_partition"
    _, _, ill = _da("ls_illposed", ("time", "scenario", "model", "downscaling", "lon"))
    assert pub.lafferty_sriver(ill) == "original lafferty_sriver"   # the ill-posed flag of the launch
    long = DA(np.zeros((513, 2, 2, 1)), dims=("time", "scenario", "model", "lon"), coords={"time": fakexr.time_coord(annual(np.arange(1500, 2013)))})
    assert pub.hawkins_sutton(long) == "original hawkins_sutton"
    wide = DA(np.zeros((60, 2, 65, 1)), dims=("time", "scenario", "model", "lon"), coords={"time": fakexr.time_coord(annual(P.Y60))})
    assert pub.hawkins_sutton(wide) == "original hawkins_sutton"
    five = DA(np.zeros((60, 2, 2, 2, 2, 2)), dims=("time", "a", "b", "c", "d", "e"), coords={"time": fakexr.time_coord(annual(P.Y60))})
    assert pub.general_partition(five, var_first=["a", "b", "c", "d"], mean_first=["e"], weights=["a"]) == "original general_partition"
    assert pub.hawkins_sutton(a) == "original hawkins_sutton"   # not a DataArray
    assert pub.ensemble_mean_std_max_min(Dataset({"tas": DA(np.zeros((3, 4), np.int16), dims=("realization", "lon"))})) == "original ensemble_mean_std_max_min"
    assert reached == ["lafferty_sriver"] * 3 + ["general_partition", "lafferty_sriver", "hawkins_sutton", "hawkins_sutton", "general_partition",
                                                "hawkins_sutton", "ensemble_mean_std_max_min"]


def test_ensemble_mean_std_max_min_on_a_dataset(wired, rng):
    mods, _, reached, _ = wired
    x = rng.normal(280, 5, (4, 3, 5))
    x[0, :, 2] = np.nan
    x[1:, 0, 4] = np.nan
    ens = Dataset({"tg_mean": DA(np.moveaxis(x, 0, 1), dims=("time", "realization", "lon"), attrs={"units": "K", "description": "Mean of tas"},
                                 coords={"lon": DA(np.arange(5.0), dims=("lon",))}),
                   "pr": DA(x[:, 0].astype(np.float32), dims=("realization", "lon"))}, attrs={"title": "ens"})
    fn = mods["xclim.ensembles"].ensemble_mean_std_max_min
    out = fn(ens)
    assert list(out) == [f"{v}_{s}" for v in ("tg_mean", "pr") for s in ("mean", "stdev", "max", "min")] and not reached
    want = P.ensemble_stats(x)
    for s in ("mean", "stdev", "max", "min"):
        got = out[f"tg_mean_{s}"]
        assert got.dims == ("time", "lon") and np.allclose(got.values, want[s], rtol=1e-13, atol=0, equal_nan=True)
        assert got.attrs == {"units": "K", "description": f"Mean of tas : mean_{s} of ensemble"}   # (the reference's own suffix)
        assert out[f"pr_{s}"].attrs == {} and out[f"pr_{s}"].values.dtype == np.float64
    assert out.attrs == {"title": "ens", "history": "[stamp] Computation of statistics on 4 ensemble members."}
    w = DA(np.array([1.0, 0.1, 3.5, 5.0]), dims=("realization",))
    for mm in (None, 2):
        out = fn(ens, mm, w)
        want = P.ensemble_stats(x, mm, w.values)
        for s in ("mean", "stdev", "max", "min"):
            assert np.allclose(out[f"tg_mean_{s}"].values, want[s], rtol=1e-13, atol=0, equal_nan=True), (mm, s)
    assert np.isnan(fn(ens, None)["tg_mean_mean"].values[:, 2]).all()


def test_uninstall_restores_identity(wired):
    from xclim_amd import patch

    mods, _, _, originals = wired
    patch.uninstall()
    for n in PARTITIONS:
        assert mods["xclim.ensembles"].__dict__[n] is originals[n] and mods["xclim.ensembles._partitioning"].__dict__[n] is originals[n]
    assert mods["xclim.ensembles._base"].ensemble_mean_std_max_min is originals["ensemble_mean_std_max_min"]
    assert mods["xclim.ensembles"].ensemble_mean_std_max_min is originals["ensemble_mean_std_max_min"]
