"""ctypes binding of libxclimhip.so (include/xclim_hip.h) — the thin C-ABI layer named by the north star.

No torch, no cffi (not installed offline).  The library is looked up in-tree (xclim_amd/lib/libxclimhip.so, built by
``__graft_entry__.build()`` / ``make -C xclim_amd/csrc``).  Every compute call goes to the HIP kernels; there is NO CPU
fallback: if the library or a GPU is missing the call raises :class:`BackendUnavailable`.
"""

from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libxclimhip.so")

XH_OK = 0
XH_ERR_HIP, XH_ERR_ARG, XH_ERR_LAYOUT, XH_ERR_OP, XH_ERR_NOTIMPL, XH_ERR_NODEVICE, XH_ERR_LIMIT = -1, -2, -3, -4, -5, -6, -7

OPS = {">": 0, "gt": 0, "<": 1, "lt": 1, ">=": 2, "ge": 2, "<=": 3, "le": 3, "==": 4, "eq": 4, "!=": 5, "ne": 5}
THR_SCALAR_F32, THR_SCALAR_F64, THR_DOY_F64, THR_DOY_F32, THR_FULL_F64, THR_FULL_F32 = range(6)
REDUCERS = {"sum": 0, "integral": 0, "mean": 1, "min": 2, "max": 3, "std": 4, "var": 5, "count": 6, "argmin": 7, "argmax": 8}
RUN_STATS = {"max": 0, "min": 1, "sum": 2, "count": 3, "mean": 4, "std": 5, "first": 6, "last": 7, "plainsum": 8}


class PrecisionWarning(UserWarning):
    """A float64 input was rounded to float32: the kernels compute on float32 fields (xclim keeps the input dtype, so
    values differ at ~1e-7 relative and comparisons of values that close to a threshold can flip)."""


def warn_downcast(a, what: str) -> None:
    """One PrecisionWarning per call site when `a` is a float64 array (python floats and float32 pass silently)."""
    import warnings

    if getattr(a, "dtype", None) == np.float64 and getattr(a, "ndim", 0) > 0:
        warnings.warn(f"{what}: float64 input is rounded to float32 (the HIP kernels compute on float32 fields)",
                      PrecisionWarning, stacklevel=3)


class Float64FieldError(TypeError):
    """A float64 FIELD reached an entry point that only exists for float32 fields.  The reference computes in the input
    dtype; rounding the field first can flip a count next to a threshold, so it is refused unless asked for."""


FLOAT64_POLICIES = ("raise", "round", "native")

# what XCLIM_AMD_FLOAT64=native serves with float64 kernels (xh_*_f64), on top of the four entry points that always do
NATIVE_SERVED = ("compare, get_daily_events, spell_length_statistics, spell_mask, spell_length, the run-length indices "
                 "(maximum_consecutive_*_days, hot / cold / dry / wet spells), warm / cold_spell_duration_index, percentile_doy, "
                 "cumulative_difference, temperature_sum, thresholded_statistics (growing / heating / cooling degree days), season "
                 "(growing / frost season start / end / length), first_day_threshold_reached, first / last_occurrence, domain_count, "
                 "bivariate_count_occurrences, diurnal / interday_diurnal / extreme_temperature_range, "
                 "select_rolling_resample_op (without an indexer), doymax / doymin and the standardized indices "
                 "(standardized_index, standardized_index_fit_params: SPI / SPEI / SSI / SGI)")


def float64_policy() -> str:
    """``XCLIM_AMD_FLOAT64``: "raise" (default, also for an unknown value), "round" or "native"."""
    p = os.environ.get("XCLIM_AMD_FLOAT64", "raise").strip().lower()
    return p if p in FLOAT64_POLICIES else "raise"


def float64_native() -> bool:
    """True under ``XCLIM_AMD_FLOAT64=native``: entry points with a float64 twin upload a float64 field as it is."""
    return float64_policy() == "native"


def handle_float64(a, what: str) -> None:
    """Policy for float64 fields on float32-only kernels (``XCLIM_AMD_FLOAT64``): "raise" (default) -> Float64FieldError;
    "round" -> PrecisionWarning and the field is rounded to float32; "native" -> the entry points with a float64 twin
    (NATIVE_SERVED) never come here, every other one raises Float64FieldError (never rounds).  threshold_count /
    count_occurrences / select_resample_op / calc_perc have native float64 kernels (xh_*_f64) and never come here."""
    if getattr(a, "dtype", None) != np.float64 or getattr(a, "ndim", 0) == 0:
        return
    policy = float64_policy()
    if policy == "round":
        warn_downcast(a, what)
        return
    if policy == "native":
        refuse_float64(what)
    raise Float64FieldError(f"{what}: float64 fields are only served by threshold_count, count_occurrences, select_resample_op and "
                            "calc_perc (xh_*_f64); cast to float32 yourself, or set XCLIM_AMD_FLOAT64=round to have it "
                            "rounded with a PrecisionWarning")


def refuse_float64(what: str) -> None:
    """Float64FieldError for a float64 field on a step without a float64 kernel under ``native`` (an entry point without a
    twin, or a form its twin does not cover: weighted or multi-variable spells, bootstrap, per-cell thresholds ...)."""
    raise Float64FieldError(f"{what}: float64 fields are only served by threshold_count, count_occurrences, select_resample_op, "
                            f"calc_perc and, under XCLIM_AMD_FLOAT64=native, {NATIVE_SERVED}; this call has no float64 "
                            "kernel: cast to float32 yourself, or set XCLIM_AMD_FLOAT64=round to have it rounded with a "
                            "PrecisionWarning")


class BackendUnavailable(RuntimeError):
    """libxclimhip.so is not built/loadable or no MI355X device is visible."""


class XclimHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[xclimhip {code}] {msg}")
        self.code = code
        self.msg = msg


_i32, _i64, _u32, _u64 = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
_vp, _dbl, _flt, _int, _sz = C.c_void_p, C.c_double, C.c_float, C.c_int, C.c_size_t

# name -> argtypes (restype is always int unless listed in _RESTYPES); mirrors the six headers under include/ one to one, a group of
# rows per header.  A new unit adds its header, its rows here, its operands in tests/stridedabi.py and the mirrors of its #defines.
SIGNATURES: dict[str, list] = {
    # include/xclim_hip.h (every .hip file of xclim_amd/csrc that no later group names)
    "xh_abi_version": [],
    "xh_last_error": [],
    "xh_device_count": [C.POINTER(_int)],
    "xh_create": [_int, C.POINTER(_vp)],
    "xh_destroy": [_vp],
    "xh_sync": [_vp],
    "xh_device_name": [_vp, C.c_char_p, _sz],
    "xh_mem_info": [_vp, C.POINTER(_sz), C.POINTER(_sz)],
    "xh_malloc": [_vp, _sz, C.POINTER(_vp)],
    "xh_free": [_vp, _vp],
    "xh_memset": [_vp, _vp, _int, _sz],
    "xh_memcpy_h2d": [_vp, _vp, _vp, _sz],
    "xh_memcpy_d2h": [_vp, _vp, _vp, _sz],
    "xh_memcpy_d2d": [_vp, _vp, _vp, _sz],
    "xh_host_alloc": [_vp, _sz, C.POINTER(_vp)],
    "xh_host_free": [_vp, _vp],
    "xh_host_register": [_vp, _vp, _sz],
    "xh_host_unregister": [_vp, _vp],
    "xh_memcpy2d": [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _int, _int, _int],
    "xh_lane_fence": [_vp, _int, _int],
    "xh_lane_sync": [_vp, _int],
    "xh_timer_start": [_vp],
    "xh_timer_stop": [_vp, C.POINTER(_flt)],
    "xh_stream": [_vp, C.POINTER(_vp)],
    "xh_comm_unique_id": [_vp],
    "xh_comm_init": [_vp, _int, _int, _vp, C.POINTER(_vp)],
    "xh_comm_destroy": [_vp],
    "xh_comm_size": [_vp, C.POINTER(_int), C.POINTER(_int)],
    "xh_comm_allgather": [_vp, _vp, _vp, _sz, _int],
    "xh_comm_fence": [_vp, _int],
    "xh_comm_sync": [_vp],
    "xh_comm_allreduce_f64": [_vp, C.POINTER(_dbl), _int, _int],
    "xh_comm_barrier": [_vp],
    "xh_fill_synthetic": [_vp, _vp, _i64, _i64, _i64, _int, _u64, _i64, _vp, _flt, _flt, _u32],
    "xh_transpose_f32": [_vp, _vp, _i64, _i64, _i64, _vp, _i64],
    "xh_threshold_count": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _dbl, _vp, _i64, _vp, _vp, _int, _vp, _vp],
    "xh_domain_count": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _dbl, _int, _vp, _int, _vp, _vp],
    "xh_resample_reduce": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _int, _vp, _vp],
    "xh_apply_missing_mask": [_vp, _vp, _int, _vp, _vp, _int, _i64, _vp],
    "xh_rolling_reduce": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _vp, _i64],
    "xh_cumsum_reset": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64],
    "xh_rle": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64],
    "xh_run_stats": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _int, _int, _vp, _int, _int, _vp, _vp],
    "xh_bivariate_count": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _dbl, _int, _vp, _int, _vp, _vp],
    "xh_range_reduce": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _int, _vp, _vp],
    "xh_compare_map": [_vp, _vp, _i64, _i64, _i64, _int, _dbl, _int, _vp, _i64, _int, _vp, _i64],
    "xh_thresholded_reduce": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _int, _vp, _int, _vp, _vp],
    "xh_mask_rows": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp, _vp, _int, _vp, _i64],
    "xh_doy_mean_std": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _int, _vp, _vp],
    "xh_spell_mask": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _dbl, _vp, _vp, _i64],
    "xh_percentile_doy_count": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _int, _dbl, _dbl, _dbl, _int, _vp, _int, _vp, _vp],
    "xh_doy_broadcast": [_vp, _vp, _int, _i64, _vp, _i64, _vp],
    "xh_within_bnds_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp],
    "xh_compare_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _int, _vp, _vp, _i64],
    "xh_select_rows": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _i64],
    "xh_mask_u8_to_f32": [_vp, _vp, _i64, _vp],
    "xh_run_stats_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _int, _vp, _int, _int, _vp, _int, _vp, _vp],
    "xh_precip_over_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _vp, _int, _vp, _vp, _int, _vp, _vp, _vp],
    "xh_spell_run_stats": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _dbl, _vp, _int, _vp, _int, _vp, _vp],
    "xh_spell_mask_multi": [_vp, _vp, _int, _vp, _int, _i64, _i64, _i64, _i64, _int, _int, _int, _vp, _vp, _i64],
    "xh_runs_with_holes": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _i64],
    "xh_run_events": [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp],
    "xh_suspicious_run": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _dbl, _vp, _i64],
    "xh_keep_longest_run": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp, _i64],
    "xh_season": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _int, _vp, _vp, _vp],
    "xh_max_run_sum": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _int, _int, _vp],
    "xh_nan_quantile": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _dbl, _dbl, _vp],
    "xh_threshold_count_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _int, _vp, _vp, _int, _vp, _vp],
    "xh_threshold_count_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _dbl, _vp, _i64, _vp, _vp, _int, _vp, _vp],
    "xh_resample_reduce_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _int, _vp, _vp],
    "xh_nan_quantile_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _dbl, _dbl, _vp],
    "xh_compare_map_f64": [_vp, _vp, _i64, _i64, _i64, _int, _dbl, _vp, _i64, _int, _int, _vp, _i64],
    "xh_run_stats_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _int, _int, _vp, _int, _int, _vp, _vp],
    "xh_spell_mask_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _dbl, _vp, _vp, _i64],
    "xh_spell_run_stats_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _dbl, _vp, _int, _vp, _int, _vp, _vp],
    "xh_run_stats_doy_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _int, _vp, _int, _int, _vp, _int, _vp, _vp],
    "xh_percentile_doy_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _int, _vp, _int, _dbl, _dbl, _vp],
    "xh_thresholded_reduce_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _int, _vp, _int, _vp, _vp],
    "xh_range_reduce_f64": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _vp, _int, _vp, _vp],
    "xh_domain_count_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _dbl, _int, _dbl, _int, _vp, _int, _vp, _vp],
    "xh_bivariate_count_f64": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _dbl, _int, _dbl, _int, _vp, _int, _vp, _vp],
    "xh_rolling_reduce_f64": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _vp, _i64],
    "xh_weighted_quantile": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _vp],
    "xh_percentile_doy": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _int, _vp, _int, _dbl, _dbl, _vp],
    "xh_percentile_doy_mapped": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _int, _vp, _int, _dbl, _dbl, _vp, _i64, _vp],
    "xh_doy_interp": [_vp, _vp, _int, _i64, _vp, _vp, _vp, _vp, _int, _vp, _vp],
    "xh_quantile_series": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp],
    "xh_eqm_train": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _int, _vp, _vp],
    "xh_eqm_train_window": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _int, _int, _vp, _int, _int, _vp, _vp],
    "xh_dqm_train_window": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _int, _int, _vp, _int, _int, _vp, _vp, _vp, _vp],
    "xh_eqm_train_groups": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _int, _int, _vp, _vp],
    "xh_dqm_train_groups": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _int, _int, _vp, _vp, _vp, _vp],
    "xh_eqm_adjust": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _int, _vp, _i64],
    "xh_eqm_adjust_g2d": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _int, _int, _vp, _i64],
    "xh_apply_factor": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64],
    "xh_plane_nearest": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _vp, _i64],
    "xh_plane_linear": [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _int, _int, _int, _vp, _i64],
    "xh_qdm_adjust": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _int, _vp],
    "xh_qdm_adjust_groups": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp, _int, _int, _int, _int, _vp, _i64],
    "xh_quantile_cells": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp],
    "xh_adapt_freq": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _dbl, _u64, _vp, _i64, _vp],
    "xh_mask_doy_cells": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64],
    "xh_rolling_dot": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _i64],
    "xh_mask_days_cells": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp, _vp, _vp, _i64],
    "xh_poly_trend": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp],
    "xh_trend_apply": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _vp, _i64],
    "xh_poly_trend_u": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp],
    "xh_trend_apply_u": [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _int, _vp, _i64],
    "xh_window_nanmean": [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64],
    "xh_poly_trend_groups": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _int, _vp, _vp],
    "xh_trend_apply_groups": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp, _int, _vp, _i64],
    "xh_fire_weather": [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int,
                        _int, _int, _int, _vp, _vp, _i64, _vp, _vp],
    "xh_overwintering_dc": [_vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, _vp],
    "xh_si_fit": [_vp, _vp, _i64, _i64, _i64, _vp, _int, _int, _int, _int, _dbl, _int, _int, _vp, _vp, _vp, _vp],
    "xh_si_apply": [_vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _vp, _int, _dbl, _dbl, _dbl, _vp, _i64],
    "xh_si_fit_f64": [_vp, _vp, _i64, _i64, _i64, _vp, _int, _int, _int, _int, _dbl, _int, _int, _vp, _vp, _vp, _vp],
    "xh_si_apply_f64": [_vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _vp, _int, _dbl, _dbl, _dbl, _vp, _i64],
    "xh_mcarthur": [_vp, _i64, _i64, _i64, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp,
                    _i64],
    "xh_solar_table": [_vp, _i64, _i64, _vp, _vp, _dbl, _vp, _vp],
    "xh_pet_month_table": [_vp, _i64, _i64, _vp, _i64, _vp, _int, _vp],
    "xh_pet_daily": [_vp, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _dbl,
                     _dbl, _vp, _vp, _i64],
    "xh_pet_monthly": [_vp, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                       _i64],
    "xh_chill_hourly": [_vp, _i64, _i64, _i64, _int, _vp, _int, _i64, _vp, _vp, _dbl, _dbl, _int, _vp, _vp, _vp, _vp, _i64],
    "xh_chill_daily": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _dbl, _dbl, _int, _vp, _vp, _vp, _vp,
                       _i64],
    "xh_bioclim": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _int, _i64, _vp, _vp, _int, _dbl, _dbl, _dbl,
                   _vp, _vp, _vp, _i64],
    # include/xclim_hip_agro.h (xclim_amd/csrc/agro.hip)
    "xh_agro_degree_sum": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _dbl, _dbl, _dbl,
                           _int, _dbl, _dbl, _dbl, _vp, _vp, _vp, _i64],
    "xh_agro_monthly": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _int, _dbl, _dbl, _dbl,
                        _vp, _vp, _vp, _vp, _i64],
    "xh_egdd": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _dbl, _vp, _vp, _vp, _vp,
                _i64],
    "xh_corn_heat_units": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _dbl, _dbl, _vp, _i64],
    "xh_qian_wma": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _i64],
    # include/xclim_hip_hydro.h (xclim_amd/csrc/hydro.hip)
    "xh_flow_period_stats": [_vp, _i64, _i64, _i64, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64],
    "xh_melt_period_max": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _int, _i64, _vp, _vp, _i64],
    "xh_antecedent_precip": [_vp, _i64, _i64, _i64, _int, _vp, _dbl, _int, _vp, _vp, _i64],
    "xh_sen_slope": [_vp, _i64, _i64, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i64],
    # include/xclim_hip_rain.h (xclim_amd/csrc/rainseason.hip)
    "xh_rain_season": [_vp, _i64, _i64, _i64, _int, _vp, _dbl, _i64, _vp, _vp, _vp, _dbl, _int, _int, _dbl, _int, _int, _dbl, _int, _int,
                       _vp, _vp, _vp, _i64],
    "xh_rolling_zones": [_vp, _i64, _i64, _i64, _int, _vp, _int, _i64, _vp, _vp, _i64],
    # include/xclim_hip_flags.h (xclim_amd/csrc/dataflags.hip)
    "xh_data_flags": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _vp, _i64, _int, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _int, _vp,
                      _i64],
    "xh_doy_bounds": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _int, _int, _int, _dbl, _vp, _vp, _i64],
    # include/xclim_hip_phase.h (xclim_amd/csrc/phase.hip)
    "xh_precip_phase_map": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64],
    "xh_precip_phase_period": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _i64, _vp, _vp, _int, _vp, _vp, _i64, _vp, _vp, _vp, _int,
                               _u32, _vp, _i64],
}
# The prototypes of the headers under include/ext/ (units added while the ABI tests over include/*.h are frozen); checked by
# tests/test_abi_ext_cpu.py.  load_library() declares them after SIGNATURES; the wrappers of these units convert every argument
# to its ctypes type themselves (kernels._ext_call), so a call is right on a handle whose argtypes were never set.
EXT_SIGNATURES: dict[str, list] = {
    # include/ext/xclim_hip_analog.h (xclim_amd/csrc/analog.hip)
    "xh_analog": [_vp, _int, _i64, _i64, _int, _vp, _i64, _i64, _int, _vp, _vp, _i64, _vp, _i64, _vp, _i64],
}
# The prototypes of the headers under include/units/ (one header per unit added while both tests above are frozen); checked by
# tests/test_abi_units_cpu.py, which takes the headers from the directory and from the group comments below.  A new unit adds
# its header there, a comment line naming it and its .hip file, its rows, and the mirrors of its #defines; its wrappers call
# through kernels._ext_call like those of EXT_SIGNATURES.
UNIT_SIGNATURES: dict[str, list] = {
    # include/units/xclim_hip_distfit.h (xclim_amd/csrc/distfit.hip)
    "xh_dist_fit": [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, _int, _dbl, _vp, _int, _int, _vp, _i64, _vp, _vp, _vp, _i64],
    "xh_dist_eval": [_vp, _int, _int, _vp, _i64, _i64, _vp, _int, _vp, _i64],
    # include/units/xclim_hip_thermal.h (xclim_amd/csrc/thermal.hip)
    "xh_esat": [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, _dbl, _dbl, _dbl, _vp, _i64],
    "xh_thermal_comfort": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _vp, _vp,
                           _vp, _i64],
    # include/units/xclim_hip_robust.h (xclim_amd/csrc/robust.hip)
    "xh_change_test": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                       _vp, _vp, _i64],
    "xh_robust_fractions": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _int, _int, _dbl, _vp, _i64],
    "xh_robust_coefficient": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp],
    "xh_ar6_gamma": [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _int, _vp, _i64, _dbl, _vp, _i64],
    # include/units/xclim_hip_humidity.h (xclim_amd/csrc/humidity.hip)
    "xh_air_moisture": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _dbl, _dbl, _dbl, _int, _int, _int, _int,
                        _int, _vp, _i64],
    "xh_wind_map": [_vp, _int, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp, _i64],
    # include/units/xclim_hip_partition.h (xclim_amd/csrc/partition.hip)
    "xh_partition_smooth": [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _int, _int, _int, _int, _i64, _i64, _vp, _vp, _i64,
                            _i64, _vp, _vp, _i64, _vp],
    "xh_partition_components": [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _int, _vp, _int, _int, _i64, _vp, _vp, _i64, _vp],
    "xh_ensemble_stats": [_vp, _vp, _i64, _i64, _i64, _int, _vp, _int, _vp, _i64],
    # include/units/xclim_hip_compound.h (xclim_amd/csrc/compound.hip)
    "xh_compound_doy_days": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                             _i64],
    "xh_degree_exceedance_date": [_vp, _i64, _i64, _i64, _int, _vp, _dbl, _int, _dbl, _i64, _vp, _vp, _vp, _vp, _vp, _i64],
    "xh_blowing_snow_days": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _dbl, _int, _i64, _vp, _vp, _vp, _i64],
    "xh_pair_period_sum": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _i64, _vp, _vp, _i64],
    # include/units/xclim_hip_grid.h (xclim_amd/csrc/grid.hip)
    "xh_grid_masked_dot": [_vp, _i64, _i64, _i64, _int, _vp, _vp, _dbl, _vp, _vp],
    "xh_grid_box_mean": [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64],
    "xh_grid_filter_argmax": [_vp, _i64, _i64, _vp, _i64, _int, _vp, _vp, _i64, _vp, _vp],
}
_RESTYPES = {"xh_last_error": C.c_char_p}
# include/units/xclim_hip_distfit.h: the XH_DIST_* distributions, methods and functions, the XH_DISTFIT_* limit and status bytes
DIST_CODES = {"norm": 0, "gumbel_r": 1, "genextreme": 2, "gamma": 3, "fisk": 4, "lognorm": 5}
DIST_NDISTS = 6          # XH_DIST_NDISTS
DIST_METHODS = {"APP": 0, "ML": 1}
DIST_FUNCS = {"ppf": 0, "isf": 1, "cdf": 2, "pdf": 3}
DISTFIT_MAX_Q = 16       # XH_DISTFIT_MAX_Q
DISTFIT_STATUS = {"fitted": 0, "nan": 1, "budget": 2, "support": 3}
# include/units/xclim_hip_thermal.h: the XH_ESAT_* methods and cases, the XH_THERMAL_* table rows, modes, stats and flag bits
ESAT_METHODS = {"sonntag90": 0, "goffgratch46": 1, "its90": 2, "tetens30": 3, "wmo08": 4, "buck81": 5, "aerk96": 6, "ecmwf": 7}
ESAT_NMETHODS = 8        # XH_ESAT_NMETHODS
ESAT_CASES = {"water": 0, "binary": 1, "interp": 2}
THERMAL_ROWS = {"sin_dec": 0, "cos_dec": 1, "tan_dec": 2, "h_utc": 3, "interval": 4, "tcorr": 5, "inv_d2": 6}
THERMAL_NROW = 7         # XH_THERMAL_NROW
THERMAL_MODES = {"daily": 0, "subdaily": 1}
THERMAL_STATS = {"sunlit": 0, "instant": 1}
THERMAL_FLAGS = {"mask_invalid": 1, "wind_cap_min": 2}
# include/units/xclim_hip_robust.h: the XH_CT_* tests, status bytes and limits, the XH_RF_* output rows and threshold kinds
CT_TESTS = {"moments": 0, "ttest": 1, "welch": 2, "mwu": 3, "bf": 4}
CT_NTESTS = 5            # XH_CT_NTESTS
CT_STATUS = {"done": 0, "nan": 1, "exact_pending": 2}
CT_MAX_T = 512           # XH_CT_MAX_T
CT_LDS_SLOTS = 64        # XH_CT_LDS_SLOTS
RF_ROWS = {"changed": 0, "positive": 1, "changed_positive": 2, "negative": 3, "changed_negative": 4, "valid": 5, "agree": 6}
RF_NFRAC = 7             # XH_RF_NFRAC
RF_THRESH = {"none": 0, "abs": 1, "rel": 2}
RC_MAX_POOL = 8192       # XH_RC_MAX_POOL
# include/units/xclim_hip_humidity.h: the XH_AM_* outputs, the XH_RH_* / XH_INVALID_* / XH_DEW_* choices, the XH_WIND_* operations and flags
AM_OUTPUTS = {"esat": 0, "vp": 1, "vpd": 2, "hurs": 3, "huss": 4, "huss_dew": 5, "tdps": 6, "humidex": 7, "heat_index": 8}
AM_NOUT = 9              # XH_AM_NOUT
RH_METHODS = {"esat": 0, "bohren98": 1}
INVALID_RULES = {"none": 0, "clip": 1, "mask": 2}
DEW_METHODS = {"tetens30": 0, "wmo08": 1, "buck81": 2, "aerk96": 3}
WIND_OPS = {"from_uv": 0, "to_uv": 1, "chill": 2, "power": 3}
WIND_NOPS = 4            # XH_WIND_NOPS
WIND_FLAGS = {"celsius": 1, "kmh": 2, "us": 4, "mask_invalid": 8}
WIND_NPAR = 3            # XH_WIND_NPAR
# include/units/xclim_hip_partition.h: the XH_PT_* limits, rolling statistics, status bytes, baselines, rules, weights and
# variability rules, the XH_ES_* output rows
PT_MAX_T = 512           # XH_PT_MAX_T
PT_MAX_DEG = 4           # XH_PT_MAX_DEG
PT_ROLL = {"mean": 0, "var": 1}
PT_STATUS = {"fitted": 0, "allnan": 1, "illposed": 2}
PT_BASE = {"none": 0, "sub": 1, "div": 2}
PT_MAX_AXES = 4          # XH_PT_MAX_AXES
PT_MAX_AXIS = 64         # XH_PT_MAX_AXIS
PT_MAX_MEMBERS = 4096    # XH_PT_MAX_MEMBERS
PT_MAX_COMP = 8          # XH_PT_MAX_COMP
PT_RULES = {"var_then_mean": 0, "mean_then_var": 1}
PT_WEIGHTS = {"none": 0, "count": 1, "user": 2}
PT_VARIAB = {"mean_all": 0, "hs": 1}
ES_ROWS = {"mean": 0, "std": 1, "max": 2, "min": 3}
ES_NSTAT = 4             # XH_ES_NSTAT
# include/units/xclim_hip_compound.h: the XH_CD_* output bits, in the order of the entry point's output pointers, and the window limit
CD_OUTPUTS = {"cold_dry": 1, "warm_dry": 2, "warm_wet": 4, "cold_wet": 8}
CD_NOUT = 4              # XH_CD_NOUT
BS_MAX_WINDOW = 32       # XH_BS_MAX_WINDOW
# include/units/xclim_hip_grid.h: the tile of xh_grid_masked_dot, the XH_GRID_* output bits in the order of the entry point's output
# pointers, and the filter limit
GRID_CHUNK = 2048        # XH_GRID_CHUNK
GRID_ROWS = 8            # XH_GRID_ROWS
GRID_OUTPUTS = {"dot": 1, "msum": 2}
GRID_MAX_WINDOW = 128    # XH_GRID_MAX_WINDOW
# header under include/units/ -> every integer #define of it, spelled from the mirrors above (tests/test_abi_units_cpu.py compares
# each header with its entry, so a #define without a mirror, or a mirror with another value, fails there)
UNIT_DEFINES = {
    "xclim_hip_distfit.h": {
        **{f"XH_DIST_{k.upper()}": v for k, v in DIST_CODES.items()}, "XH_DIST_NDISTS": DIST_NDISTS,
        **{f"XH_DIST_{k}": v for k, v in DIST_METHODS.items()}, **{f"XH_DIST_{k.upper()}": v for k, v in DIST_FUNCS.items()},
        "XH_DISTFIT_MAX_Q": DISTFIT_MAX_Q, **{f"XH_DISTFIT_{k.upper()}": v for k, v in DISTFIT_STATUS.items()}},
    "xclim_hip_thermal.h": {
        **{f"XH_ESAT_{k.upper()}": v for k, v in ESAT_METHODS.items()}, "XH_ESAT_NMETHODS": ESAT_NMETHODS,
        **{f"XH_ESAT_{k.upper()}": v for k, v in ESAT_CASES.items()},
        **{f"XH_THERMAL_{k.upper()}": v for k, v in THERMAL_ROWS.items()}, "XH_THERMAL_NROW": THERMAL_NROW,
        **{f"XH_THERMAL_{k.upper()}": v for k, v in THERMAL_MODES.items()},
        **{f"XH_THERMAL_{k.upper()}": v for k, v in THERMAL_STATS.items()},
        **{f"XH_THERMAL_{k.upper()}": v for k, v in THERMAL_FLAGS.items()}},
    "xclim_hip_robust.h": {
        **{f"XH_CT_{k.upper()}": v for k, v in CT_TESTS.items()}, "XH_CT_NTESTS": CT_NTESTS,
        **{f"XH_CT_{k.upper()}": v for k, v in CT_STATUS.items()}, "XH_CT_MAX_T": CT_MAX_T, "XH_CT_LDS_SLOTS": CT_LDS_SLOTS,
        **{f"XH_RF_{k.upper()}": v for k, v in RF_ROWS.items()}, "XH_RF_NFRAC": RF_NFRAC,
        **{f"XH_RF_THRESH_{k.upper()}": v for k, v in RF_THRESH.items()}, "XH_RC_MAX_POOL": RC_MAX_POOL},
    "xclim_hip_humidity.h": {
        **{f"XH_AM_{k.upper()}": v for k, v in AM_OUTPUTS.items()}, "XH_AM_NOUT": AM_NOUT,
        **{f"XH_RH_{k.upper()}": v for k, v in RH_METHODS.items()}, **{f"XH_INVALID_{k.upper()}": v for k, v in INVALID_RULES.items()},
        **{f"XH_DEW_{k.upper()}": v for k, v in DEW_METHODS.items()},
        **{f"XH_WIND_{k.upper()}": v for k, v in WIND_OPS.items()}, "XH_WIND_NOPS": WIND_NOPS,
        **{f"XH_WIND_{k.upper()}": v for k, v in WIND_FLAGS.items()}, "XH_WIND_NPAR": WIND_NPAR},
    "xclim_hip_partition.h": {
        "XH_PT_MAX_T": PT_MAX_T, "XH_PT_MAX_DEG": PT_MAX_DEG, **{f"XH_PT_ROLL_{k.upper()}": v for k, v in PT_ROLL.items()},
        **{f"XH_PT_{k.upper()}": v for k, v in PT_STATUS.items()}, **{f"XH_PT_BASE_{k.upper()}": v for k, v in PT_BASE.items()},
        "XH_PT_MAX_AXES": PT_MAX_AXES, "XH_PT_MAX_AXIS": PT_MAX_AXIS, "XH_PT_MAX_MEMBERS": PT_MAX_MEMBERS, "XH_PT_MAX_COMP": PT_MAX_COMP,
        **{f"XH_PT_{k.upper()}": v for k, v in PT_RULES.items()}, **{f"XH_PT_W_{k.upper()}": v for k, v in PT_WEIGHTS.items()},
        **{f"XH_PT_VARIAB_{k.upper()}": v for k, v in PT_VARIAB.items()},
        **{f"XH_ES_{k.upper()}": v for k, v in ES_ROWS.items()}, "XH_ES_NSTAT": ES_NSTAT},
    "xclim_hip_compound.h": {
        **{f"XH_CD_{k.upper()}": v for k, v in CD_OUTPUTS.items()}, "XH_CD_NOUT": CD_NOUT, "XH_BS_MAX_WINDOW": BS_MAX_WINDOW},
    "xclim_hip_grid.h": {
        "XH_GRID_CHUNK": GRID_CHUNK, "XH_GRID_ROWS": GRID_ROWS, **{f"XH_GRID_{k.upper()}": v for k, v in GRID_OUTPUTS.items()},
        "XH_GRID_MAX_WINDOW": GRID_MAX_WINDOW},
}
# the XH_ANALOG_* methods, in the order of the reference's registry
ANALOG_METHODS = {"seuclidean": 0, "nearest_neighbor": 1, "zech_aslan": 2, "szekely_rizzo": 3, "friedman_rafsky": 4,
                  "kolmogorov_smirnov": 5, "kldiv": 6, "mahalanobis": 7}
ANALOG_NMETHODS = 8      # XH_ANALOG_NMETHODS
ANALOG_MAX_D = 10        # XH_ANALOG_MAX_D
ANALOG_KS_MAX_D = 6      # XH_ANALOG_KS_MAX_D
ANALOG_MAX_SAMPLE = 512  # XH_ANALOG_MAX_SAMPLE
ANALOG_MAX_K = 32        # XH_ANALOG_MAX_K
ANALOG_MAX_NK = 16       # XH_ANALOG_MAX_NK
HYDRO_MAX_WINDOW = 32   # XH_HYDRO_MAX_WINDOW
SEN_MAX_YEARS = 181     # XH_SEN_MAX_YEARS
RAIN_MAX_WINDOW = 32    # XH_RAIN_MAX_WINDOW
ZONES_MAX_EDGES = 32    # XH_ZONES_MAX_EDGES
RAIN_START_WINDOW, RAIN_START_BOUNDS, RAIN_END_BOUNDS = 1, 2, 4   # the XH_RAIN_* flag bits
FLAGS_MAX_CHECKS = 16   # XH_FLAGS_MAX_CHECKS
FLAG_CMP, FLAG_OUTSIDE, FLAG_PAIR, FLAG_REPEAT, FLAG_CLIM = 0, 1, 2, 3, 4   # the XH_FLAG_* check kinds
# struct xh_flag_check { int32_t kind, op, n, other; double a, b; }
FLAG_CHECK_DTYPE = np.dtype([("kind", np.int32), ("op", np.int32), ("n", np.int32), ("other", np.int32), ("a", np.float64), ("b", np.float64)])
PHASE_METHODS = {"binary": 0, "brown": 1, "auer": 2, "dai_annual": 3, "dai_seasonal": 4, "given": 5}   # the XH_PHASE_* methods
PHASE_NPAR, PHASE_DAI_NTAB, PHASE_NLIM = 6, 96, 7   # XH_PHASE_NPAR, XH_PHASE_DAI_NTAB, XH_PHASE_NLIM
# the outputs of xh_precip_phase_period in the order of their XH_PHASE_* bits
PHASE_OUTPUTS = ("pr_sum", "solid_sum", "liquid_sum", "pr_n", "solid_n", "liquid_n", "tas_n", "snow_days", "snow_sum_over", "snow_n_over",
                 "first_snow", "last_snow", "hplt_days", "rofg_days")


_lib = None
_lib_lock = threading.Lock()


def library_path() -> str:
    return _LIB_PATH


def load_library() -> C.CDLL:
    """Load libxclimhip.so and declare every prototype of SIGNATURES (the six headers under include/), of EXT_SIGNATURES
    (include/ext/) and of UNIT_SIGNATURES (include/units/).  Raises
    BackendUnavailable."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise BackendUnavailable(
                f"{_LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C xclim_amd/csrc` (needs hipcc)"
            )
        try:
            lib = C.CDLL(_LIB_PATH)
        except OSError as err:  # pragma: no cover
            raise BackendUnavailable(f"cannot load {_LIB_PATH}: {err}") from err
        for name, argtypes in (*SIGNATURES.items(), *EXT_SIGNATURES.items(), *UNIT_SIGNATURES.items()):
            fn = getattr(lib, name)  # AttributeError if the header and the library diverge
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, _int)
        _lib = lib
        return lib


def _check(lib, rc: int):
    if rc != XH_OK:
        msg = lib.xh_last_error()
        msg = msg.decode() if msg else ""
        if rc == XH_ERR_NODEVICE:
            raise BackendUnavailable(msg)
        if rc == XH_ERR_OP:
            raise ValueError(msg)
        raise XclimHipError(rc, msg)


def device_count() -> int:
    lib = load_library()
    n = _int(0)
    _check(lib, lib.xh_device_count(C.byref(n)))
    return n.value


class DeviceArray:
    """A typed device buffer owned by a :class:`Device` (hipMalloc'd through xh_malloc)."""

    __slots__ = ("dev", "ptr", "shape", "dtype", "_owner", "_alloc")

    def __init__(self, dev: "Device", ptr: int, shape, dtype, owner=True, alloc: int = 0):
        self.dev = dev
        self.ptr = ptr
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self._owner = owner
        self._alloc = int(alloc)  # bytes obtained from xh_malloc (0: foreign / view); lets free() hand it to the pool

    @property
    def size(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    @property
    def nbytes(self) -> int:
        return self.size * self.dtype.itemsize

    def reshape(self, *shape) -> "DeviceArray":
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        shape = tuple(shape)
        if -1 in shape:
            known = int(np.prod([s for s in shape if s != -1], dtype=np.int64))
            shape = tuple(self.size // max(known, 1) if s == -1 else s for s in shape)
        assert int(np.prod(shape, dtype=np.int64)) == self.size, (shape, self.shape)
        view = DeviceArray(self.dev, self.ptr, shape, self.dtype, owner=False)
        view._owner = self  # keep the parent alive
        return view

    def get(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        if out.size:
            lib = self.dev.lib
            if self.dev.trace is not None:
                self.dev.trace.append(("d2h", (out.nbytes,)))
            _check(lib, lib.xh_memcpy_d2h(self.dev.ctx, out.ctypes.data_as(_vp), _vp(self.ptr), out.nbytes))
        return out

    def free(self):
        if self._owner is True and self.ptr and self.dev is not None and self.dev.ctx:
            self.dev._release(self.ptr, self._alloc)
        self.ptr = 0
        self._owner = False

    def __del__(self):
        try:
            self.free()
        except Exception:  # pragma: no cover
            pass


class Device:
    """One xh_ctx (HIP stream + scratch) on one GPU.  Not re-entrant: calls are serialised by a lock."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        ctx = _vp()
        _check(self.lib, self.lib.xh_create(device, C.byref(ctx)))
        self.ctx = ctx
        self.index = device
        self.lock = threading.RLock()
        self.trace = None  # list of (entry point, args) while start_trace() is active
        # Test instrumentation, off by default: a byte value (0..255) that empty() fills every allocation with before handing it
        # out, so that an output a kernel does not store reads as that pattern instead of whatever the pool's last user left
        self.poison_empty: int | None = None
        # Freed buffers are kept per exact size and handed out again: hipMalloc / hipFree cost ~0.1-0.4 ms each and
        # hipFree synchronises the device, which is as long as a whole kernel of this library.  Re-use is safe because
        # every kernel of a context runs on its one stream (stream order protects a buffer that is still being read).
        self._pool: dict[int, list[tuple[int, int]]] = {}   # size -> [(release number, address)], oldest first
        self._pool_seq = 0
        self._pool_bytes = 0
        # cap: XCLIM_AMD_POOL_BYTES, else a quarter of the device's memory (72 GB of an MI355X's 288; at least 32 GiB) — a grouped
        # DQM adjust of a 30-year 1440 x 90 band turns over four 5.7 GB buffers per call, and giving those back to the driver
        # costs two seconds per call (hipFree + hipMalloc of multi-GB ranges) against 27 ms of kernels.  A failed allocation
        # empties the pool and retries (empty()).
        cap = os.environ.get("XCLIM_AMD_POOL_BYTES")
        self._pool_cap = int(cap) if cap is not None else None  # None: decided at the first release
        self._pinned: dict[int, int] = {}  # page-locked host ranges we own or registered: address -> bytes
        # device copies of large host inputs, recognised again across calls (resident())
        self._inputs: dict = {}
        self._inputs_bytes = 0
        # "scope" (default): only inside `with dev.keep_inputs():` (patch.install() opens one around every Indicator
        # call); "always": across every call of the process (the caller promises not to edit fields in place, or calls
        # forget_inputs() after doing so); "off"
        self._inputs_mode = os.environ.get("XCLIM_AMD_INPUT_CACHE", "scope").lower()
        if self._inputs_mode not in ("scope", "always", "off"):
            raise ValueError(f"XCLIM_AMD_INPUT_CACHE must be scope, always or off, got {self._inputs_mode!r}")
        self._keep_depth = 0
        self._forget_hooks: list = []  # run by forget_inputs(): caches that live and die with the input copies (xr_adapter's tables)
        cap = os.environ.get("XCLIM_AMD_INPUT_CACHE_BYTES")
        self._inputs_cap = int(cap) if cap is not None else None  # None: half of the free device memory at first use
        self._inputs_min = int(os.environ.get("XCLIM_AMD_INPUT_CACHE_MIN", str(32 << 20)))

    # ---- memory ----
    def empty(self, shape, dtype) -> DeviceArray:
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        nbytes = max(int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, 16)
        ptr = None
        with self.lock:
            free = self._pool.get(nbytes)
            if free:
                self._pool_bytes -= nbytes
                _, ptr = free.pop()        # (the most recently released one)
                if not free:
                    del self._pool[nbytes]
        if ptr is None:
            p = _vp()
            rc = self.lib.xh_malloc(self.ctx, nbytes, C.byref(p))
            if rc != XH_OK and self._pool_bytes:
                self.trim()  # out of memory with buffers parked in the pool: give them back and retry once
                rc = self.lib.xh_malloc(self.ctx, nbytes, C.byref(p))
            while rc != XH_OK and self._inputs:
                # ... or with remembered input copies (resident()): the least recently used one goes, its memory passes
                # through the pool back to the driver, and the allocation is tried again
                self._drop_input(next(iter(self._inputs)))
                self.trim()
                rc = self.lib.xh_malloc(self.ctx, nbytes, C.byref(p))
            _check(self.lib, rc)
            ptr = p.value
        a = DeviceArray(self, ptr, shape, dtype, alloc=nbytes)
        if self.poison_empty is not None:
            # pooled or fresh: the whole allocation, on the context's stream — and waited for, since the block adapter's first
            # copy into a new buffer runs on the copy-in lane, which the compute stream's order does not cover
            _check(self.lib, self.lib.xh_memset(self.ctx, _vp(ptr), int(self.poison_empty), nbytes))
            _check(self.lib, self.lib.xh_sync(self.ctx))
        return a

    def _release(self, ptr: int, nbytes: int) -> None:
        """A freed buffer is parked (per exact size).  Over the cap, or with more than 8 of one size, the OLDEST parked buffers go
        back to the driver — of any size: the pool follows the working set (a bench leg on 45 GB fields must not leave the pool
        full of sizes nobody asks for again while the next leg's 5.7 GB buffers go through hipFree / hipMalloc on every call)."""
        victims = []
        with self.lock:
            if self._pool_cap is None:
                try:
                    self._pool_cap = max(32 << 30, self.mem_info()[1] // 4)
                except Exception:
                    self._pool_cap = 32 << 30
            if not nbytes or nbytes > self._pool_cap:
                victims.append(ptr)
            else:
                self._pool_seq = getattr(self, "_pool_seq", 0) + 1
                self._pool.setdefault(nbytes, []).append((self._pool_seq, ptr))
                self._pool_bytes += nbytes
                while True:
                    if len(self._pool.get(nbytes, ())) > 8:
                        size = nbytes
                    elif self._pool_bytes > self._pool_cap:
                        size = min((lst[0][0], sz) for sz, lst in self._pool.items())[1]
                    else:
                        break
                    _, p = self._pool[size].pop(0)
                    if not self._pool[size]:
                        del self._pool[size]
                    self._pool_bytes -= size
                    victims.append(p)
        for p in victims:
            self.lib.xh_free(self.ctx, _vp(p))

    def trim(self) -> None:
        """Return every pooled buffer to the driver."""
        with self.lock:
            pool, self._pool, self._pool_bytes = self._pool, {}, 0
        for ptrs in pool.values():
            for _, ptr in ptrs:
                self.lib.xh_free(self.ctx, _vp(ptr))

    # ---- pinned host memory + copy lanes (block adapter, blocks.py) ----
    def pinned_empty(self, shape, dtype) -> np.ndarray:
        """numpy array over page-locked host memory (xh_host_alloc): strided copies from / to it are asynchronous and run
        at the full PCIe rate.  Freed when the array (and every view of it) is garbage collected."""
        import weakref

        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = _vp()
        _check(self.lib, self.lib.xh_host_alloc(self.ctx, max(nbytes, 16), C.byref(p)))
        buf = (C.c_char * max(nbytes, 16)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        self._pinned[p.value] = max(nbytes, 16)
        lib, ctx, pinned, addr = self.lib, self.ctx, self._pinned, p.value

        def _free():
            pinned.pop(addr, None)
            if ctx:
                lib.xh_host_free(ctx, _vp(addr))

        weakref.finalize(buf, _free)
        return arr

    def register(self, arr: np.ndarray) -> None:
        """Page-lock caller memory (hipHostRegister) for the lifetime of the registration; costs about as much as one
        copy of the array, so it pays for inputs that are streamed more than once."""
        assert arr.flags.c_contiguous
        _check(self.lib, self.lib.xh_host_register(self.ctx, _vp(arr.ctypes.data), arr.nbytes))
        self._pinned[arr.ctypes.data] = arr.nbytes

    def unregister(self, arr: np.ndarray) -> None:
        if self._pinned.pop(arr.ctypes.data, None) is not None:
            _check(self.lib, self.lib.xh_host_unregister(self.ctx, _vp(arr.ctypes.data)))

    def is_pinned(self, arr: np.ndarray) -> bool:
        a0, a1 = arr.ctypes.data, arr.ctypes.data + arr.nbytes
        return any(p <= a0 and a1 <= p + n for p, n in self._pinned.items())

    def copy2d(self, dst: int, dpitch: int, src: int, spitch: int, width: int, height: int, kind: str, lane: int = 0,
               blocking: bool = True) -> None:
        """xh_memcpy2d: `height` rows of `width` bytes; kind "h2d" | "d2h" | "d2d"; lanes 0 compute / 1 copy-in / 2 copy-out."""
        _check(self.lib, self.lib.xh_memcpy2d(self.ctx, _vp(dst), dpitch, _vp(src), spitch, width, height,
                                              {"h2d": 0, "d2h": 1, "d2d": 2}[kind], lane, int(bool(blocking))))

    def lane_fence(self, from_lane: int, to_lane: int) -> None:
        _check(self.lib, self.lib.xh_lane_fence(self.ctx, from_lane, to_lane))

    def lane_sync(self, lane: int) -> None:
        _check(self.lib, self.lib.xh_lane_sync(self.ctx, lane))

    def zeros(self, shape, dtype) -> DeviceArray:
        a = self.empty(shape, dtype)
        if a.nbytes:
            _check(self.lib, self.lib.xh_memset(self.ctx, _vp(a.ptr), 0, a.nbytes))
        return a

    def copy_d2d(self, dst_ptr: int, src_ptr: int, nbytes: int) -> None:
        _check(self.lib, self.lib.xh_memcpy_d2d(self.ctx, _vp(dst_ptr), _vp(src_ptr), int(nbytes)))

    def to_device(self, arr: np.ndarray, dtype=None) -> DeviceArray:
        arr = np.ascontiguousarray(arr, dtype=dtype)
        d = self.empty(arr.shape, arr.dtype)
        if arr.nbytes:
            if self.trace is not None:
                self.trace.append(("h2d", (arr.nbytes,)))
            _check(self.lib, self.lib.xh_memcpy_h2d(self.ctx, _vp(d.ptr), arr.ctypes.data_as(_vp), arr.nbytes))
        return d

    # ---- device-resident inputs across calls (the caller of the wrappers is the Indicator chain,
    # /root/reference/src/xclim/core/indicator.py:865-944: percentile_doy and the index that consumes its table read the
    # SAME field, and so do an index and the missing-value check after it) ----
    @staticmethod
    def _host_fingerprint(flat: np.ndarray):
        """Second guard against a buffer edited in place while it is remembered: the bit patterns of ~2^16 evenly spaced
        samples plus the first and last 4096 elements, summed as integers (every element of arrays up to 2^16 elements;
        ~0.5 ms on a 1.5 GB field against 27 ms for its upload).  An edit that touches none of the samples is NOT seen,
        and a full checksum costs as much as the transfer it would save (host memory bandwidth ~ PCIe bandwidth) — which
        is why the cache is SCOPED (:meth:`keep_inputs`) instead of trusting this."""
        n = flat.size
        step = max(1, n >> 16)
        u = flat.view(np.uint32 if flat.dtype.itemsize == 4 else np.uint64)
        return (n, int(u[::step].sum(dtype=np.uint64)), int(u[:4096].sum(dtype=np.uint64)), int(u[-4096:].sum(dtype=np.uint64)))

    def keep_inputs(self):
        """Context manager: inside it, large host inputs stay on the device from one call to the next
        (:meth:`resident`); at the exit of the outermost scope every copy is dropped.  The contract of a scope: no field
        handed to this library is edited IN PLACE while the scope is open (or :meth:`forget_inputs` is called after the
        edit).  ``patch.install()`` opens one around every ``Indicator.__call__`` — compute, its ``percentile_doy`` /
        ``resample_doy`` helpers and the missing-value check read the same DataArray and no user code runs in between;
        user code chains calls with ``with xclim_amd.keep_inputs(): per = percentile_doy(tasmax); out = tx90p(tasmax, per)``.
        Outside a scope every call uploads its inputs (the behaviour before round 5) unless XCLIM_AMD_INPUT_CACHE=always."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            with self.lock:
                self._keep_depth += 1
            try:
                yield self
            finally:
                with self.lock:
                    self._keep_depth -= 1
                    last = self._keep_depth == 0
                if last and self._inputs_mode != "always":
                    self.forget_inputs()

        return scope()

    def _inputs_active(self) -> bool:
        return self._inputs_mode == "always" or (self._inputs_mode == "scope" and self._keep_depth > 0)

    def resident(self, arr: np.ndarray) -> DeviceArray:
        """Device copy of a C-contiguous float32 / float64 host array.  Inside a :meth:`keep_inputs` scope large arrays
        (>= XCLIM_AMD_INPUT_CACHE_MIN bytes, default 32 MiB) are remembered by (address, shape, dtype) together with a weak
        reference to the object that owns the memory and a content fingerprint; the next call with the same buffer gets
        the SAME device memory (a view: the kernels only read their inputs) instead of another PCIe transfer.  The cache
        holds at most XCLIM_AMD_INPUT_CACHE_BYTES (default: half of the device memory free at first use; 0 = off), least
        recently used first out — also when an allocation fails (:meth:`empty`) —, and an entry dies with its host array
        or with the scope.  Outside a scope: a plain upload."""
        import weakref

        if (not self._inputs_active() or not isinstance(arr, np.ndarray) or not arr.flags.c_contiguous
                or arr.nbytes < self._inputs_min or arr.dtype not in (np.float32, np.float64)):
            return self.to_device(arr)
        if self._inputs_cap is None:
            self._inputs_cap = self.mem_info()[0] // 2
        if arr.nbytes > self._inputs_cap:
            return self.to_device(arr)
        owner = arr
        while isinstance(owner.base, np.ndarray):
            owner = owner.base
        if owner.base is not None:
            owner = owner.base  # (a buffer object under the outermost ndarray: pinned memory of pinned_empty)
        key = (arr.ctypes.data, arr.nbytes, arr.dtype.str)
        fp = self._host_fingerprint(arr.reshape(-1))
        with self.lock:
            hit = self._inputs.get(key)
            if hit is not None and hit[0]() is owner and hit[2] == fp:
                self._inputs[key] = self._inputs.pop(key)  # most recently used last
                if self.trace is not None:
                    self.trace.append(("resident_hit", (arr.nbytes,)))
                view = DeviceArray(self, hit[1].ptr, arr.shape, arr.dtype, owner=False)
                view._owner = hit[1]
                return view
            if hit is not None:
                self._drop_input(key)
        try:
            ref = weakref.ref(owner)
        except TypeError:
            return self.to_device(arr)
        d = self.to_device(arr)
        with self.lock:
            while self._inputs and self._inputs_bytes + arr.nbytes > self._inputs_cap:
                self._drop_input(next(iter(self._inputs)))
            self._inputs[key] = (ref, d, fp)
            self._inputs_bytes += arr.nbytes
        weakref.finalize(owner, self._drop_input, key, id(d))
        view = DeviceArray(self, d.ptr, arr.shape, arr.dtype, owner=False)
        view._owner = d
        return view

    def _drop_input(self, key, only_id=None) -> None:
        with self.lock:
            hit = self._inputs.get(key)
            if hit is None or (only_id is not None and id(hit[1]) != only_id):
                return
            del self._inputs[key]
            self._inputs_bytes -= hit[1].nbytes
        # (the device memory goes back to the pool when the last view of it is gone)

    def forget_inputs(self) -> None:
        """Drop every remembered input copy (after editing a field in place, or to give the memory back)."""
        with self.lock:
            self._inputs.clear()
            self._inputs_bytes = 0
        for hook in list(self._forget_hooks):
            hook()

    def wrap(self, ptr: int, shape, dtype) -> DeviceArray:
        """Wrap foreign device memory (e.g. a torch tensor's data_ptr()) without taking ownership."""
        return DeviceArray(self, int(ptr), shape, dtype, owner=False)

    def sync(self):
        _check(self.lib, self.lib.xh_sync(self.ctx))

    def name(self) -> str:
        buf = C.create_string_buffer(256)
        _check(self.lib, self.lib.xh_device_name(self.ctx, buf, 256))
        return buf.value.decode()

    def mem_info(self) -> tuple[int, int]:
        f, t = _sz(0), _sz(0)
        _check(self.lib, self.lib.xh_mem_info(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def timer_start(self):
        _check(self.lib, self.lib.xh_timer_start(self.ctx))

    def timer_stop(self) -> float:
        ms = _flt(0)
        _check(self.lib, self.lib.xh_timer_stop(self.ctx, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if self.ctx:
            self.forget_inputs()
            self.trim()
            self.lib.xh_destroy(self.ctx)
            self.ctx = None

    def call(self, name: str, *args):
        """Invoke an entry point with this context as first argument and raise on error."""
        if self.trace is not None:  # launch log for the adapter tests: (entry point, arguments as passed)
            self.trace.append((name, args))
        fn = getattr(self.lib, name)
        with self.lock:
            _check(self.lib, fn(self.ctx, *args))

    def start_trace(self) -> list:
        """Record every C-ABI call made through this context from now on: returns the (growing) list of
        ``(entry point, args)``; :meth:`stop_trace` ends it.  Test instrumentation (tests/test_gpu_adapter.py asserts that
        tx90p through the xarray wrappers reaches ``xh_threshold_count`` with the per-doy table, cdd ``xh_run_stats``)."""
        self.trace = []
        return self.trace

    def stop_trace(self) -> None:
        self.trace = None


_default_device: Device | None = None


def get_device(index: int | None = None) -> Device:
    """Process-wide default context (device from XCLIM_AMD_DEVICE / LOCAL_RANK, else 0)."""
    global _default_device
    if index is None:
        index = int(os.environ.get("XCLIM_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if _default_device is None or _default_device.index != index or _default_device.ctx is None:
        _default_device = Device(index)
    return _default_device


def np_ptr(a: np.ndarray) -> _vp:
    return a.ctypes.data_as(_vp)
