"""The XCLIM_AMD_FLOAT64=native entry points without a GPU: the float64 twins of compare / run statistics / spells /
percentile_doy (xclim_amd/csrc/f64run.hip) validate their arguments before touching a device, and the policy predicate
parses the three policies."""
import ctypes

import numpy as np
import pytest

from xclim_amd import _capi

NEW = ("xh_compare_map_f64", "xh_run_stats_f64", "xh_spell_mask_f64", "xh_spell_run_stats_f64", "xh_run_stats_doy_f64",
       "xh_percentile_doy_f64")


def test_the_float64_twins_are_declared_and_exported():
    lib = _capi.load_library()
    for name in NEW:
        assert name in _capi.SIGNATURES
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name]


def test_the_float64_twins_refuse_a_null_context_or_argument():
    lib = _capi.load_library()
    null = None
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    seg = (ctypes.c_int64 * 2)(0, 4)
    segp = ctypes.cast(seg, ctypes.c_void_p)
    tidx = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    tidxp = ctypes.cast(tidx, ctypes.c_void_p)
    tb = (ctypes.c_int32 * 1)(0)
    tbp = ctypes.cast(tb, ctypes.c_void_p)
    per = (ctypes.c_double * 1)(90.0)
    perp = ctypes.cast(per, ctypes.c_void_p)
    ARG = _capi.XH_ERR_ARG
    for ctx, x in ((null, p), (null, null)):
        assert lib.xh_compare_map_f64(ctx, x, 4, 2, 2, 0, 0.5, null, 0, 0, 0, p, 2) == ARG
        assert lib.xh_run_stats_f64(ctx, x, 4, 2, 2, 1, 0, 0.5, 1, 0, 1, segp, 1, 1, p, null) == ARG
        assert lib.xh_spell_mask_f64(ctx, x, 4, 2, 2, 1, 3, 0, 0, 0.5, null, p, 2) == ARG
        assert lib.xh_spell_run_stats_f64(ctx, x, 4, 2, 2, 1, 3, 0, 0, 0.5, null, 0, segp, 1, p, null) == ARG
        assert lib.xh_run_stats_doy_f64(ctx, x, 4, 2, 2, 1, 0, p, 1, tidxp, 1, 0, segp, 1, p, null) == ARG
        assert lib.xh_percentile_doy_f64(ctx, x, 4, 2, 2, 1, tbp, 1, 1, 5, perp, 1, 1.0 / 3, 1.0 / 3, p) == ARG
    assert b"NULL" in lib.xh_last_error()


@pytest.mark.parametrize("value, policy", [(None, "raise"), ("raise", "raise"), ("round", "round"), ("native", "native"),
                                           ("NATIVE", "native"), (" native ", "native"), ("bogus", "raise")])
def test_the_float64_policy_is_parsed(monkeypatch, value, policy):
    if value is None:
        monkeypatch.delenv("XCLIM_AMD_FLOAT64", raising=False)
    else:
        monkeypatch.setenv("XCLIM_AMD_FLOAT64", value)
    assert _capi.float64_policy() == policy
    assert _capi.float64_native() == (policy == "native")


def test_native_refuses_a_field_without_a_twin_and_names_the_served_set(monkeypatch):
    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "native")
    with pytest.raises(_capi.Float64FieldError, match="float64 fields are only served by") as e:
        _capi.handle_float64(np.zeros((3, 2)), "quantile")
    assert "percentile_doy" in str(e.value) and "spell_length_statistics" in str(e.value)
    _capi.handle_float64(np.zeros((3, 2), np.float32), "quantile")  # float32 passes


def test_the_default_message_is_unchanged(monkeypatch):
    monkeypatch.delenv("XCLIM_AMD_FLOAT64", raising=False)
    with pytest.raises(_capi.Float64FieldError, match=r"float64 fields are only served by threshold_count, count_occurrences, "
                                                       r"select_resample_op and calc_perc \(xh_\*_f64\)"):
        _capi.handle_float64(np.zeros((3, 2)), "field")
