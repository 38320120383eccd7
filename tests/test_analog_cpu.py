"""The spatial-analogue unit without a GPU: the restatement of tests/analogcpu.py against the reference's known answers and
recorded results, the refusals and messages of xclim_amd/analog.py, the xarray adapter on a stand-in Dataset (its launch replaced
by the restatement), and the build files.  The device side is tests/test_gpu_analog.py."""
import json
import os
import re
import types

import numpy as np
import pytest

import analogcpu as R
import fakexr
from xclim_amd import _capi as capi
from xclim_amd import analog as A
from xclim_amd.fields import NotServed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VECTORS = np.load(os.path.join(GOLDEN, "analog_vectors.npz"))
KNOWN = json.load(open(os.path.join(GOLDEN, "analog_known_answers.json")))
SIGNATURE = "target, candidates, dist_dim='time', method='kldiv', **kwargs"   # analog.py:21-29


class Dataset:
    """Stand-in for xr.Dataset as far as spatial_analogs reads it: ``data_vars``, name -> DataArray, in order."""

    def __init__(self, variables):
        self.data_vars = dict(variables)


def datasets(x, y, dims=("time", "lat", "lon"), dist_dim="time", names=None, chunks=None):
    """(target, candidates) of a target (n, d) and fields (d, m, ny, nx) laid out on `dims`."""
    names = names or [f"index{j}" for j in range(x.shape[1])]
    target = Dataset({n: fakexr.DataArray(x[:, j], dims=(dist_dim,), coords={dist_dim: np.arange(len(x))}) for j, n in enumerate(names)})
    cand = {}
    for j, n in enumerate(names):
        f = np.moveaxis(y[j], 0, dims.index(dist_dim))
        coords = {dm: np.arange(s) * (10 if dm != dist_dim else 1) for dm, s in zip(dims, f.shape)}
        data = f
        if chunks:
            data = fakexr.ChunkedArray(f, [tuple([c] * (s // c) + ([s % c] if s % c else [])) for c, s in ((chunks.get(dm, s), s) for dm, s in zip(dims, f.shape))])
        cand[n] = fakexr.DataArray(data, dims=dims, coords=coords)
    return target, Dataset(cand)


def standin_module(reached):
    ns = {"reached": reached}
    exec(f"def spatial_analogs({SIGNATURE}):\n    reached.append((method, kwargs))\n    return 'original spatial_analogs'\n", ns)
    mod = types.ModuleType("xclim.analog")
    mod.spatial_analogs = ns["spatial_analogs"]
    mod.metrics = {}
    return mod


def restated_launch(dev, method, x, fields, *, par=None, k=None, **_):
    """What kernels.analog returns, from the restatement: an object whose get() is (rows, C)."""
    y = np.stack([np.asarray(f, np.float64) for f in fields])
    kw = {}
    if method == "zech_aslan":
        kw["dmin"] = par[0]
    elif method == "szekely_rizzo":
        kw["standardize"] = bool(par[0])
    elif method == "mahalanobis":
        kw["VI"] = np.asarray(par).reshape(x.shape[1], x.shape[1])
    elif method == "kldiv":
        kw["k"] = list(k)
    value = R.cells(method, x, y, **kw)[0]
    return types.SimpleNamespace(get=lambda: value.T.reshape(-1, y.shape[2]))


@pytest.fixture()
def on_restatement(monkeypatch):
    monkeypatch.setattr(A.K, "analog", restated_launch)
    return types.SimpleNamespace(to_device=lambda a: a)


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_the_restatement_reproduces_the_known_answers_to_the_reference_s_decimals():
    assert [k["name"] for k in KNOWN][:5] == [f"matlab/{m}" for m in ("seuclidean", "nearest_neighbor", "zech_aslan", "friedman_rafsky", "kolmogorov_smirnov")]
    assert len(KNOWN) == 9
    for ka in KNOWN:
        value, scale, terms = R.metric(ka["method"], np.array(ka["x"]), np.array(ka["y"]), **ka["kwargs"])
        assert abs(value - ka["expected"]) < 1.5 * 10.0 ** -ka["decimals"], ka["name"]
        assert abs(value - ka["reference"]) <= (0.0 if ka["method"] in R.EXACT else R.tolerance(scale, terms)), ka["name"]


@pytest.mark.parametrize("case", sorted({k.split("/")[0] for k in VECTORS.files}))
def test_the_restatement_reproduces_the_goldens(case):
    x, y = VECTORS[f"{case}/x"], VECTORS[f"{case}/y"].astype(np.float64)
    variants = [k.split("/")[1] for k in VECTORS.files if k.startswith(case + "/") and k.split("/")[1] in R.VARIANTS]
    assert variants
    for variant in variants:
        method, kw = R.VARIANTS[variant]
        kw = {k: (VECTORS[f"{case}/VI"] if isinstance(v, str) else v) for k, v in kw.items()}
        value, scale, terms = R.cells(method, x, y, **kw)
        exp = VECTORS[f"{case}/{variant}"]
        np.testing.assert_array_equal(np.isnan(value), np.isnan(exp), err_msg=f"{case}/{variant}")
        np.testing.assert_array_equal(np.isinf(value), np.isinf(exp), err_msg=f"{case}/{variant}")
        ok = np.isfinite(exp)
        if method in R.EXACT:
            np.testing.assert_array_equal(value, exp, err_msg=f"{case}/{variant}")
        else:
            assert (np.abs(value[ok] - exp[ok]) <= np.broadcast_to(R.tolerance(scale, terms), exp.shape)[ok]).all(), f"{case}/{variant}"


def test_the_fixtures_hold_every_family():
    assert VECTORS["main64/y"].shape == (3, 33, 130) and VECTORS["main32/y"].dtype == np.float32 and VECTORS["main64/x"].shape == (21, 3)
    assert np.isnan(VECTORS["edges/y"][2, 7, 0]) and np.ptp(VECTORS["edges/y"][1, :, 1]) == 0
    for v in R.VARIANTS:
        assert np.isnan(VECTORS[f"nan_target/{v}"]).all() and np.isnan(VECTORS[f"edges/{v}"][0]).all(), v
    assert np.isnan(VECTORS["edges/zech_aslan"][1]) and np.isnan(VECTORS["edges/szekely_rizzo"][1]) and np.isnan(VECTORS["edges/nearest_neighbor"][1])
    assert np.isfinite(VECTORS["edges/szekely_rizzo_raw"][1]) and np.isfinite(VECTORS["edges/kolmogorov_smirnov"][1])
    np.testing.assert_array_equal(VECTORS["same/y"][:, :, 0].T, VECTORS["same/x"])
    assert np.isinf(VECTORS["same/kldiv"][0]) and VECTORS["same/zech_aslan_dmin"][0] != VECTORS["same/zech_aslan"][0]
    assert VECTORS["short/y"].shape[1] == 4 and np.isnan(VECTORS["short/kldiv_k"]).all() and np.isfinite(VECTORS["short/seuclidean"]).all()
    assert VECTORS["main64/kldiv_k"].shape == (130, 3) and VECTORS["long/x"].shape[0] > VECTORS["long/y"].shape[1]
    assert VECTORS["ks1/x"].shape[1] == 1 and VECTORS["ks6/x"].shape[1] == 6
    for case in ("ks1", "ks6"):   # exact ties between the samples
        assert np.isin(VECTORS[f"{case}/y"][0], VECTORS[f"{case}/x"][:, 0]).any()


# ---- refusals and messages -------------------------------------------------------------------------------------------
def test_refusals_and_messages(on_restatement):
    dev = on_restatement
    x, y = VECTORS["main64/x"], list(VECTORS["main64/y"][:, :, :4])
    with pytest.raises(ValueError, match=re.escape("Method `KonMari` is not implemented. Available methods are: seuclidean,nearest_neighbor,"
                                                   "zech_aslan,szekely_rizzo,friedman_rafsky,kolmogorov_smirnov,kldiv,mahalanobis.")):
        A.spatial_analogs(x, y, method="KonMari", device=dev)
    assert list(A.metrics) == list(capi.ANALOG_METHODS) == list(R.METHODS)
    with pytest.raises(NotServed, match="integer"):
        A.spatial_analogs(x, [f.astype(np.int32) for f in y], method="seuclidean", device=dev)
    with pytest.raises(NotServed, match="mixed dtype"):
        A.spatial_analogs(x, [y[0].astype(np.float32), y[1], y[2]], method="seuclidean", device=dev)
    with pytest.raises(NotServed, match="chunked"):
        A.spatial_analogs(x, [fakexr.ChunkedArray(f, [(33,), (2, 2)]) for f in y], method="seuclidean", device=dev)
    big = capi.ANALOG_MAX_SAMPLE + 1
    with pytest.raises(NotServed, match="points"):
        A.spatial_analogs(np.zeros((big, 3)), y, method="seuclidean", device=dev)
    with pytest.raises(NotServed, match="points"):
        A.spatial_analogs(x, [np.zeros((big, 2))] * 3, method="seuclidean", device=dev)
    with pytest.raises(NotServed, match="indices"):
        A.spatial_analogs(np.zeros((9, 11)), [np.zeros((9, 2))] * 11, method="seuclidean", device=dev)
    with pytest.raises(NotServed, match="indices"):
        A.spatial_analogs(np.zeros((9, 7)), [np.zeros((9, 2))] * 7, method="kolmogorov_smirnov", device=dev)
    with pytest.raises(ValueError, match="Too many dimensions: 11."):
        A.spatial_analogs(np.zeros((9, 11)), [np.zeros((9, 2))] * 11, method="kldiv", device=dev)
    for k in (capi.ANALOG_MAX_K + 1, list(range(1, capi.ANALOG_MAX_NK + 2)), 0, 1.5):
        with pytest.raises(NotServed, match="kldiv"):
            A.spatial_analogs(x, y, method="kldiv", k=k, device=dev)
    with pytest.raises(NotServed, match="VI"):
        A.spatial_analogs(x, y, method="mahalanobis", VI=np.eye(2), device=dev)
    with pytest.raises(AttributeError, match="VI not a matrix"):
        A.spatial_analogs(x, y, method="mahalanobis", VI=[[1.0]], device=dev)
    with pytest.raises(AttributeError, match="Shape mismatch"):
        A.spatial_analogs(x, y[:2], method="seuclidean", device=dev)
    with pytest.raises(TypeError, match="unexpected keyword argument 'dmin'"):
        A.spatial_analogs(x, y, method="seuclidean", dmin=1.0, device=dev)
    # what is served comes back on the cells, a list of k last
    assert A.spatial_analogs(x, VECTORS["main64/y"][:, :, :6].reshape(3, 33, 2, 3), method="kldiv", k=[1, 2], device=dev).shape == (2, 3, 2)
    assert A.spatial_analogs(x, y, device=dev).shape == (4,)                       # the reference's default method
    assert A.spatial_analogs(x, [f[:, :0] for f in y], method="zech_aslan", device=dev).shape == (0,)


def test_the_ctypes_arguments_are_converted_by_the_wrapper():
    """kernels._ext_call hands every argument over as the ctypes type of EXT_SIGNATURES: a handle without argtypes is called right."""
    from xclim_amd import kernels as K

    seen = {}
    dev = types.SimpleNamespace(call=lambda name, *args: seen.update(name=name, args=args), empty=lambda shape, dtype: types.SimpleNamespace(ptr=64, shape=shape))
    f = capi.DeviceArray(None, 128, (5, 3), np.float32, owner=False)
    K.analog(dev, "kldiv", np.zeros((6, 2)), [f, f], k=[1, 3])
    assert seen["name"] == "xh_analog" and [type(a) for a in seen["args"]] == capi.EXT_SIGNATURES["xh_analog"][1:]
    values = [a.value for a in seen["args"]]
    assert values[:4] == [capi.ANALOG_METHODS["kldiv"], 6, 5, 2] and values[5:8] == [3, 3, 0] and values[10] == 0 and values[12] == 2 and values[14] == 3


# ---- the adapter -----------------------------------------------------------------------------------------------------
def test_the_adapter_on_a_stand_in_dataset(on_restatement):
    reached = []
    mod = standin_module(reached)
    env = fakexr.make_env()
    fn = A.make_adapters(env, {"spatial_analogs": mod.spatial_analogs}, on_restatement)["spatial_analogs"]
    x, y = VECTORS["main64/x"], VECTORS["main64/y"][:, :, :6].reshape(3, 33, 2, 3)
    names = ["tg_mean", "prcptot", "gdd"]
    for dims in (("time", "lat", "lon"), ("lat", "time", "lon"), ("lat", "lon", "time")):
        target, cand = datasets(x, y, dims, names=names)
        out = fn(target, cand, method="zech_aslan")
        assert isinstance(out, fakexr.DataArray) and out.dims == ("lat", "lon") and out.name == "dissimilarity"
        assert out.attrs == {"long_name": "Dissimilarity between target and candidates, using metric zech_aslan.",
                             "indices": "tg_mean,prcptot,gdd", "metric": "zech_aslan"}
        np.testing.assert_array_equal(out.coords["lat"].values, [0, 10])
        np.testing.assert_array_equal(out.coords["lon"].values, [0, 10, 20])
        np.testing.assert_array_equal(out.values, R.cells("zech_aslan", x, y.reshape(3, 33, 6))[0].reshape(2, 3))
    assert not reached
    # another sample dimension (a stacked MultiIndex is just a sample axis), keyword arguments passed on, the default method
    target, cand = datasets(x, y, ("sample", "lat", "lon"), dist_dim="sample", names=names)
    out = fn(target, cand, dist_dim="sample", method="szekely_rizzo", standardize=False)
    np.testing.assert_array_equal(out.values, R.cells("szekely_rizzo", x, y.reshape(3, 33, 6), standardize=False)[0].reshape(2, 3))
    assert fn(target, cand, "sample").attrs["metric"] == "kldiv" and not reached
    with pytest.raises(ValueError, match="Method `KonMari` is not implemented"):
        fn(target, cand, "sample", "KonMari")
    # forwarded: chunked candidates, integer fields, a target that shares more than dist_dim, other variables, a list of k
    target, cand = datasets(x, y, names=names)
    chunked = datasets(x, y, names=names, chunks={"lat": 1})[1]
    ints = Dataset({n: fakexr.DataArray(v.values.astype(np.int64), dims=v.dims, coords=v.coords) for n, v in cand.data_vars.items()})
    wide = Dataset({n: fakexr.DataArray(np.zeros((21, 2)), dims=("time", "lat")) for n in names})
    other = datasets(x, y, names=["a", "b", "c"])[1]
    forwarded = [((target, chunked), {}), ((target, ints), {}), ((wide, cand), {}), ((target, other), {}), ((target, cand), {"k": [1, 2]}),
                 ((target, cand, ["time"]), {})]
    for args, kw in forwarded:
        assert fn(*args, **kw) == "original spatial_analogs"
    assert len(reached) == len(forwarded) and reached[4] == ("kldiv", {"k": [1, 2]})


def test_patch_install_replaces_spatial_analogs_where_it_is_defined(on_restatement, monkeypatch):
    from xclim_amd import patch

    reached = []
    mod = standin_module(reached)
    original = mod.spatial_analogs
    monkeypatch.setattr(capi, "_default_device", None)
    monkeypatch.setattr(A, "get_device", lambda: on_restatement)
    done = patch.install(fakexr.make_env(), {"xclim.analog": mod})
    try:
        assert done == ["xclim.analog.spatial_analogs"] and mod.spatial_analogs is not original and mod.spatial_analogs.__wrapped__ is original
        target, cand = datasets(VECTORS["main64/x"], VECTORS["main64/y"][:, :, :6].reshape(3, 33, 2, 3))
        assert mod.spatial_analogs(target, cand, method="seuclidean").dims == ("lat", "lon")
    finally:
        patch.uninstall()
    assert mod.spatial_analogs is original


# ---- the build files -------------------------------------------------------------------------------------------------
def test_the_makefile_names_the_unit_and_its_header():
    text = open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", text, flags=re.M).group(1).split()
    assert "analog.hip" in srcs and len(srcs) == len(set(srcs))
    rule = re.search(r"^build/%\.o: (.*)$", text, flags=re.M).group(1).split()
    assert "../../include/ext/xclim_hip_analog.h" in rule
    assert os.path.exists(os.path.join(ROOT, "include", "ext", "xclim_hip_analog.h"))
    assert "-ffp-contract=off" in text
