"""The xarray adapter of the spatial-analogue unit, EXECUTED on the device: ``patch.install(env, modules)`` on a stand-in
``xclim.analog`` whose ``spatial_analogs`` has the reference's signature and only records that it was reached, with the Dataset
and DataArray stand-ins of tests/test_analog_cpu.py and tests/fakexr.py."""
import numpy as np
import pytest

import fakexr
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module run on poisoned output buffers)
from test_analog_cpu import VECTORS, Dataset, datasets, standin_module
from xclim_amd import patch

pytestmark = pytest.mark.gpu
NAMES = ["tg_mean", "prcptot", "gdd"]


@pytest.fixture()
def wired(dev):
    import xclim_amd._capi as capi

    reached = []
    mod = standin_module(reached)
    original = mod.spatial_analogs
    old = capi._default_device
    capi._default_device = dev
    done = patch.install(fakexr.make_env(), {"xclim.analog": mod})
    try:
        yield mod, done, reached, original
    finally:
        patch.uninstall()
        capi._default_device = old
    assert mod.spatial_analogs is original


@pytest.mark.parametrize("case", ["main64", "main32"])
def test_every_method_through_the_installed_adapter(dev, wired, case):
    mod, done, reached, original = wired
    assert done == ["xclim.analog.spatial_analogs"] and mod.spatial_analogs.__wrapped__ is original
    x, y = VECTORS[f"{case}/x"], VECTORS[f"{case}/y"][:, :, :12].reshape(3, 33, 3, 4)
    target, cand = datasets(x, y, ("lat", "time", "lon"), names=NAMES)
    trace = dev.start_trace()
    try:
        for variant, kw in (("seuclidean", {}), ("nearest_neighbor", {}), ("zech_aslan", {}), ("szekely_rizzo_raw", {"standardize": False}),
                            ("friedman_rafsky", {}), ("kolmogorov_smirnov", {}), ("kldiv", {}), ("mahalanobis_VI", {"VI": VECTORS[f"{case}/VI"]})):
            method = variant.split("_raw")[0].split("_VI")[0]
            out = mod.spatial_analogs(target, cand, method=method, **kw)
            assert out.dims == ("lat", "lon") and out.name == "dissimilarity" and out.values.dtype == np.float64
            assert out.attrs == {"long_name": f"Dissimilarity between target and candidates, using metric {method}.",
                                 "indices": ",".join(NAMES), "metric": method}
            exp = VECTORS[f"{case}/{variant}"][:12].reshape(3, 4)
            if method in ("nearest_neighbor", "friedman_rafsky", "kolmogorov_smirnov"):
                np.testing.assert_array_equal(out.values, exp)
            else:   # (the bound of tests/test_gpu_analog.py holds there; here: the same numbers arrive on the right cells)
                np.testing.assert_allclose(out.values, exp, rtol=1e-9, atol=1e-9)
    finally:
        dev.stop_trace()
    assert [name for name, _ in trace if name.startswith("xh_analog")] == ["xh_analog"] * 8 and not reached


def test_what_is_not_served_reaches_the_original(wired):
    mod, _, reached, _ = wired
    x, y = VECTORS["main64/x"], VECTORS["main64/y"][:, :, :6].reshape(3, 33, 2, 3)
    target, cand = datasets(x, y, names=NAMES)
    chunked = datasets(x, y, names=NAMES, chunks={"lon": 2})[1]
    ints = Dataset({n: fakexr.DataArray(v.values.astype(np.int32), dims=v.dims, coords=v.coords) for n, v in cand.data_vars.items()})
    for args, kw in (((target, chunked), {}), ((target, ints), {"method": "seuclidean"}), ((target, cand), {"k": [1, 2]})):
        assert mod.spatial_analogs(*args, **kw) == "original spatial_analogs"
    assert [r[0] for r in reached] == ["kldiv", "seuclidean", "kldiv"]
    with pytest.raises(ValueError, match="Method `KonMari` is not implemented"):
        mod.spatial_analogs(target, cand, method="KonMari")
