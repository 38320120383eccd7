"""The float64 twins of the period reductions (xclim_amd/csrc/f64red.hip) without a GPU: they are declared and exported with
the argument types of _capi.SIGNATURES, and they validate their arguments before touching a device.  The float64 policy
names them in its message under XCLIM_AMD_FLOAT64=native."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from xclim_amd import _capi

NEW = ("xh_thresholded_reduce_f64", "xh_range_reduce_f64", "xh_domain_count_f64", "xh_bivariate_count_f64",
       "xh_rolling_reduce_f64")


def test_the_reduction_twins_are_declared_and_exported():
    lib = _capi.load_library()
    header = (Path(_capi.__file__).resolve().parents[1] / "include" / "xclim_hip.h").read_text()
    for name in NEW:
        assert name in _capi.SIGNATURES
        assert f"int {name}(" in header
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name]


def _bufs():
    buf = (ctypes.c_double * 64)()
    seg = (ctypes.c_int64 * 2)(0, 4)
    return buf, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(seg, ctypes.c_void_p), seg


def test_a_null_context_or_field_is_refused():
    lib = _capi.load_library()
    _, p, segp, _ = _bufs()
    null = None
    ARG = _capi.XH_ERR_ARG
    for ctx, x in ((null, p), (null, null), (p, null)):
        assert lib.xh_thresholded_reduce_f64(ctx, x, 4, 2, 2, 1, 0, 0.5, 2, 0, segp, 1, p, null) == ARG
        assert lib.xh_range_reduce_f64(ctx, x, p, 4, 2, 2, 2, 0, 0, 0, segp, 1, p, null) == ARG
        assert lib.xh_range_reduce_f64(ctx, p, x, 4, 2, 2, 2, 0, 0, 0, segp, 1, p, null) == ARG
        assert lib.xh_domain_count_f64(ctx, x, 4, 2, 2, 1, 0, 0.5, 3, 1.5, 1, segp, 1, p, null) == ARG
        assert lib.xh_bivariate_count_f64(ctx, x, p, 4, 2, 2, 2, 0, 0, 0.5, 0, 0.5, 1, segp, 1, p, null) == ARG
        assert lib.xh_rolling_reduce_f64(ctx, x, 4, 2, 2, 1, 3, 1, 0, p, 2) == ARG
        assert b"NULL" in lib.xh_last_error()


def test_bad_dtypes_mode_or_window_are_refused_before_the_device():
    """A non-NULL stand-in context: every check below fails before the context is read."""
    lib = _capi.load_library()
    _, p, segp, _ = _bufs()
    ctx = p
    null = None
    ARG = _capi.XH_ERR_ARG
    assert lib.xh_thresholded_reduce_f64(ctx, p, 4, 2, 2, 1, 0, 0.5, 3, 0, segp, 1, p, null) == ARG
    assert b"mode" in lib.xh_last_error()
    assert lib.xh_range_reduce_f64(ctx, p, p, 4, 2, 2, 2, 3, 0, 0, segp, 1, p, null) == ARG
    assert b"dtypes" in lib.xh_last_error()
    assert lib.xh_range_reduce_f64(ctx, p, p, 4, 2, 2, 2, 0, 5, 0, segp, 1, p, null) == ARG
    assert b"mode" in lib.xh_last_error()
    assert lib.xh_bivariate_count_f64(ctx, p, p, 4, 2, 2, 2, -1, 0, 0.5, 0, 0.5, 1, segp, 1, p, null) == ARG
    assert b"dtypes" in lib.xh_last_error()
    assert lib.xh_bivariate_count_f64(ctx, p, p, 4, 2, 2, 2, 0, 0, 0.5, 0, 0.5, 3, segp, 1, p, null) == ARG
    assert b"combine" in lib.xh_last_error()
    assert lib.xh_domain_count_f64(ctx, p, 4, 2, 2, 1, 0, 0.5, 3, 1.5, 0, segp, 1, p, null) == ARG
    assert b"combine" in lib.xh_last_error()
    assert lib.xh_rolling_reduce_f64(ctx, p, 4, 2, 2, 1, 0, 1, 0, p, 2) == ARG
    assert b"window" in lib.xh_last_error()
    # segments outside [0, T), an unknown operator or reducer, a column-major view
    bad = (ctypes.c_int64 * 2)(0, 9)
    assert lib.xh_thresholded_reduce_f64(ctx, p, 4, 2, 2, 1, 0, 0.5, 2, 0, ctypes.cast(bad, ctypes.c_void_p), 1, p, null) == ARG
    assert lib.xh_thresholded_reduce_f64(ctx, p, 4, 2, 2, 1, 9, 0.5, 0, 0, segp, 1, p, null) == _capi.XH_ERR_OP
    assert lib.xh_rolling_reduce_f64(ctx, p, 4, 2, 2, 1, 3, 1, 42, p, 2) == _capi.XH_ERR_OP
    assert lib.xh_domain_count_f64(ctx, p, 4, 2, 1, 1, 0, 0.5, 3, 1.5, 1, segp, 1, p, null) == _capi.XH_ERR_LAYOUT


def test_native_names_the_new_reductions_and_the_default_message_stays(monkeypatch):
    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "native")
    with pytest.raises(_capi.Float64FieldError, match="float64 fields are only served by") as e:
        _capi.handle_float64(np.zeros((3, 2)), "quantile")
    msg = str(e.value)
    for name in ("percentile_doy", "spell_length_statistics", "cumulative_difference", "temperature_sum", "thresholded_statistics",
                 "season", "first_day_threshold_reached", "domain_count", "bivariate_count_occurrences",
                 "diurnal / interday_diurnal / extreme_temperature_range", "select_rolling_resample_op", "doymax"):
        assert name in msg
    monkeypatch.delenv("XCLIM_AMD_FLOAT64", raising=False)
    with pytest.raises(_capi.Float64FieldError) as e:
        _capi.handle_float64(np.zeros((3, 2)), "field")
    assert "cumulative_difference" not in str(e.value)
