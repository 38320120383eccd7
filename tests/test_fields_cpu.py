"""The contract of xclim_amd/fields.py, the front end the multi-field units share: dtypes, shapes, per-cell inputs, the
time-last transposition and the empty result.  No device and no library: a DeviceArray without a device stands in for the
device-array branches."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import fields as F  # noqa: E402
from xclim_amd._capi import DeviceArray  # noqa: E402


def _device(shape, dtype):
    return DeviceArray(None, 0, shape, dtype, owner=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_float_fields_come_back_as_the_same_object(dtype):
    a, d = np.ones((5, 2), dtype), _device((5, 2), dtype)
    assert F.native(a, "tas") is a and F.native(d, "tas") is d
    got = F.native_set({"tas": a, "pr": a})
    assert got["tas"] is a and got["pr"] is a


@pytest.mark.parametrize("dtype", [np.int32, np.float16, bool])
def test_other_dtypes_are_widened_to_float64(dtype):
    a = np.array([[0, 1], [1, 0], [1, 1]], dtype)
    got = F.native(a, "tas")
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, a)


def test_a_mixed_host_set_is_widened_and_none_is_dropped():
    a32, a64 = np.full((5, 2), 1.5, np.float32), np.full((5, 2), 2.5, np.float64)
    got = F.native_set({"tasmin": a32, "tas": None, "tasmax": a64})
    assert list(got) == ["tasmin", "tasmax"]
    assert got["tasmin"].dtype == np.float64 and got["tasmax"].dtype == np.float64
    np.testing.assert_array_equal(got["tasmin"], a32)
    np.testing.assert_array_equal(got["tasmax"], a64)


def test_device_arrays_must_be_float_and_share_one_dtype():
    with pytest.raises(TypeError):
        F.native_set({"tasmin": _device((5, 2), np.float32), "tasmax": _device((5, 2), np.float64)})
    with pytest.raises(TypeError, match="^hurs"):
        F.native(_device((5, 2), np.int32), "hurs")
    with pytest.raises(TypeError, match="^hurs"):
        F.native_set({"tas": _device((5, 2), np.float32), "hurs": _device((5, 2), np.int32)})


def test_shape_of():
    a = np.zeros((5, 2, 3))
    assert F.shape_of({"tas": a, "pr": a}) == (5, (2, 3), 6)
    assert F.shape_of({"tas": np.zeros(5)}) == (5, (), 1)
    with pytest.raises(ValueError, match="time axis"):
        F.shape_of({"tas": np.float64(1.0)})
    with pytest.raises(ValueError, match="^pr"):
        F.shape_of({"tas": np.zeros((5, 2)), "pr": np.zeros((5, 3))})


def test_per_cell_inputs():
    got = F.per_cell(np.array([1, 2, 3]), (2, 3), "lat")
    assert got.dtype == np.float64 and got.flags.c_contiguous
    np.testing.assert_array_equal(got, [1, 2, 3, 1, 2, 3])
    assert F.per_cell(None, (2, 3), "kbdi0") is None
    with pytest.raises(ValueError, match=r"^pr_annual: shape \(4,\) .* \(2, 3\)"):
        F.per_cell(np.ones(4), (2, 3), "pr_annual")


def test_time_last_to_time_first_and_back():
    a = np.arange(30, dtype=np.float32).reshape(2, 3, 5)[::-1]
    assert not a.flags.c_contiguous
    tf = F.time_first(a)
    assert tf.shape == (5, 6) and tf.dtype == np.float32 and tf.flags.c_contiguous
    assert not np.shares_memory(tf, a)
    np.testing.assert_array_equal(tf[:, 4], a[1, 1, :])
    back = F.time_last(tf, (2, 3))
    assert back.shape == a.shape and back.dtype == a.dtype
    np.testing.assert_array_equal(back, a)
    # the loop broadcast of a gufunc: leading axes stretched to the loop shape first
    np.testing.assert_array_equal(F.time_first(a[:1], (2, 3)), F.time_first(np.broadcast_to(a[:1], (2, 3, 5))))
    assert F.time_first(np.zeros((4, 0))).shape == (0, 4)


@pytest.mark.parametrize("rows, cells", [(0, (2, 3)), (7, (0, 4))])
def test_empty_result(rows, cells):
    got = F.empty_result({"bio1": np.float64, "wettest": np.int32}, rows, cells)
    assert list(got) == ["bio1", "wettest"]
    assert got["bio1"].shape == (rows,) + cells and got["bio1"].dtype == np.float64
    assert got["wettest"].shape == (rows,) + cells and got["wettest"].dtype == np.int32


def test_forward_and_not_served_are_defined_once():
    from xclim_amd import anuclim, chill, converters, ffdi, fire, stats

    assert ffdi._Forward is chill._Forward is fire._Forward is F.Forward
    assert converters.NotServed is stats.NotServed is chill.NotServed is anuclim.NotServed is F.NotServed
    assert issubclass(F.NotServed, NotImplementedError) and not issubclass(F.Forward, NotImplementedError)
