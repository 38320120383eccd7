"""Which elements of its outputs did a call of the C ABI store?  (test infrastructure only)

``watch`` replaces ``dev.call`` on one Device the way ``stridedabi.padded`` does: the real entry point runs on the caller's own
buffers, and after it every OUTPUT operand of the call is downloaded and must not hold the poison pattern of
tests/poisoned.py in any element.  Before the call the same operands are looked at once: an operand that is poison in every
element is "armed" — it came from ``Device.empty`` under the fixture and nothing has written it yet — and the log says so, so
that a sweep can tell a checked operand from one that merely happened to hold old values.

The output operands of an entry point come from two tables, by the parameter names of the headers under include/:
  * the strided ones from ``stridedabi.operands`` (mode "w"; "rw" operands keep what the caller held and are listed in EXEMPT);
  * ``DENSE``, below: every output of the main header without a stride parameter of stridedabi's kind — the period reductions
    (P, C), the quantile and percentile tables, factors, node tables, run statistics — and the outputs of its units whose row pitch
    is called ``ld_out`` (an operand listed here is taken from here, not from stridedabi.PITCHED).
``PLUMBING`` names the entry points that compute nothing.  tests/test_unwritten_outputs_cpu.py asserts that every other entry
point of the header has its outputs in one of the tables or is listed in EXEMPT, and that EXEMPT names nothing but
operands whose header comment says the caller's values are kept."""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import stridedabi as S
from poisoned import unwritten

# ptr: parameter name.  rows / width / dtype: expressions over the call's arguments, as in stridedabi.TABLE.  stride: the
# row-pitch parameter, None for a dense operand (row stride = width).  ptrs: the argument is a HOST array of that many device
# pointers (the argument itself or any entry may be NULL).
Out = namedtuple("Out", "ptr rows width dtype stride ptrs")


def D(ptr, rows="P", width="C", dtype="f4", stride=None, ptrs=None):
    return Out(ptr, rows, width, dtype, stride, ptrs)


_COUNTS = [D("count_out", dtype="i4"), D("valid_out", dtype="i4")]
_VALID = D("valid_out", dtype="i4")
_RED = "'i4' if reducer in (6, 7, 8) else 'f4'"
_RED8 = "'i4' if reducer in (6, 7, 8) else 'f8'"
_TRAIN = [D("af", "G * nq"), D("hist_q", "G * nq")]
_DTRAIN = _TRAIN + [D("scaling", "G", dtype="f8"), D("mu_hist", "G", dtype="f8")]
_SI_FIT = [D("params", "G * 3", dtype="f8"), D("nzeros", "G", dtype="f8"), D("nnotnull", "G", dtype="f8"), D("nfev", "G", dtype="i4")]
_PDOY = [D("out", "nper * ndoy", dtype="f8")]
_CHILL = [D("cp_out", dtype="f8", stride="ld_out"), D("cu_out", dtype="f8", stride="ld_out"), D("valid_out", dtype="i4", stride="ld_out")]

DENSE = {
    "xh_threshold_count": _COUNTS, "xh_threshold_count_doy": _COUNTS, "xh_threshold_count_f64": _COUNTS,
    "xh_domain_count": _COUNTS, "xh_domain_count_f64": _COUNTS, "xh_bivariate_count": _COUNTS, "xh_bivariate_count_f64": _COUNTS,
    "xh_percentile_doy_count": _COUNTS,
    "xh_range_reduce": [D("out"), _VALID], "xh_range_reduce_f64": [D("out", dtype="f8"), _VALID],
    "xh_thresholded_reduce": [D("out"), _VALID], "xh_thresholded_reduce_f64": [D("out", dtype="f8"), _VALID],
    "xh_resample_reduce": [D("out", dtype=_RED), _VALID], "xh_resample_reduce_f64": [D("out", dtype=_RED8), _VALID],
    "xh_apply_missing_mask": [D("out64", dtype="f8")],
    "xh_mask_u8_to_f32": [D("out", 1, "n")],
    "xh_doy_mean_std": [D("mean_out", "ndoy"), D("std_out", "ndoy")],
    "xh_run_stats": [D("out"), _VALID], "xh_run_stats_f64": [D("out"), _VALID],
    "xh_spell_run_stats": [D("out"), _VALID], "xh_spell_run_stats_f64": [D("out"), _VALID],
    "xh_run_stats_doy": [D("out"), _VALID], "xh_run_stats_doy_f64": [D("out"), _VALID],
    "xh_season": [D("start_out"), D("end_out"), D("len_out")],
    "xh_max_run_sum": [D("out")],
    "xh_run_events": [D(n, "P * maxev") for n in ("start_out", "end_out", "len_out", "eff_out", "sum_out")],
    "xh_nan_quantile": [D("out", "nq", dtype="f8")], "xh_nan_quantile_f64": [D("out", "nq", dtype="f8")],
    "xh_weighted_quantile": [D("out", "nq", dtype="f8")],
    "xh_percentile_doy": _PDOY, "xh_percentile_doy_f64": _PDOY, "xh_percentile_doy_mapped": _PDOY,
    "xh_doy_interp": [D("out", "D_out", dtype="f8")],
    "xh_doy_broadcast": [D("out", "T", dtype="f8")],
    "xh_within_bnds_doy": [D("out", "T", dtype="u1")],
    "xh_precip_over_doy": [D("frac"), D("n_over", dtype="i4"), _VALID],
    "xh_quantile_series": [D("out", "nq")],
    "xh_eqm_train": [D("af", "nq"), D("hist_q", "nq")],
    "xh_eqm_train_window": _TRAIN, "xh_eqm_train_groups": _TRAIN, "xh_dqm_train_window": _DTRAIN, "xh_dqm_train_groups": _DTRAIN,
    "xh_quantile_cells": [D("out", 1)],
    "xh_poly_trend": [D("p0", 1, dtype="f8"), D("p1", 1, dtype="f8"), D("nvalid", 1, dtype="i4")],
    "xh_poly_trend_u": [D("p0", 1, dtype="f8"), D("p1", 1, dtype="f8"), D("nvalid", 1, dtype="i4")],
    "xh_poly_trend_groups": [D("p0", "G", dtype="f8"), D("p1", "G", dtype="f8")],
    "xh_fire_weather": [D("winter_pr_out", 1)],
    "xh_overwintering_dc": [D("out", 1, "n")],
    "xh_solar_table": [D("ra_out", "R", "L", "f8"), D("dl_out", "R", "L", "f8")],
    "xh_pet_month_table": [D("out", "M", "L", "f8")],
    "xh_si_fit": _SI_FIT, "xh_si_fit_f64": _SI_FIT,
    # the wrappers of these two hand in periods that cover every row (they refuse the per-row outputs otherwise), so the rows the
    # header leaves unwritten — those outside [seg[0], seg[P]) — do not exist in a call that comes through them
    "xh_chill_hourly": _CHILL + [D("delta_out", "H", dtype="f8", stride="ld_out")],
    "xh_chill_daily": _CHILL + [D("hourly_out", "24 * D", dtype="f8", stride="ld_out")],
    "xh_bioclim": [D("outputs", dtype="f8", stride="ld_out", ptrs=19), D("which_out", dtype="i4", stride="ld_out", ptrs=4),
                   D("count_out", dtype="i4", stride="ld_out", ptrs=4)],
}

# (entry point, operand) -> the words of its header comment that leave part of the operand to the caller
EXEMPT = {
    ("xh_qdm_adjust_groups", "scen"): "scen is written at the listed rows only",
    ("xh_trend_apply_groups", "out"): "rows in no group are not written",
}

# entry points that compute nothing: the context, memory, copies, timing, streams, lanes and the RCCL exchange
PLUMBING = {"xh_abi_version", "xh_last_error", "xh_device_count", "xh_create", "xh_destroy", "xh_sync", "xh_device_name", "xh_mem_info",
            "xh_malloc", "xh_free", "xh_memset", "xh_memcpy_h2d", "xh_memcpy_d2h", "xh_memcpy_d2d", "xh_timer_start", "xh_timer_stop",
            "xh_stream", "xh_comm_unique_id", "xh_comm_init", "xh_comm_destroy", "xh_comm_size", "xh_comm_allgather", "xh_comm_fence",
            "xh_comm_sync", "xh_comm_allreduce_f64", "xh_comm_barrier", "xh_host_alloc", "xh_host_free", "xh_host_register",
            "xh_host_unregister", "xh_memcpy2d", "xh_lane_fence", "xh_lane_sync"}


def compute_entry_points():
    return sorted(set(S.PROTOS) - PLUMBING)


def outputs_of(name):
    """The output operands of an entry point as Out records: stridedabi's "w" operands that DENSE does not list, then DENSE's."""
    dense = list(DENSE.get(name, ()))
    listed = {o.ptr for o in dense}
    outs = [Out(op.ptr, op.rows, op.width, op.dtype, (op.stride, op.minor), op.ptrs) for op in S.operands(name)
            if op.mode == "w" and op.ptr not in listed]
    return outs + dense


def _extents(name, env, dev):
    """[(operand label, device address, rows, width, row stride, dtype)] of the non-NULL output operands of one call."""
    found = []
    for out in outputs_of(name):
        if not env[out.ptr]:
            continue
        if isinstance(out.stride, tuple):   # a strided operand of stridedabi.TABLE: its layout rule (time-minor calls included)
            op = S.Op(out.ptr, out.stride[0], out.rows, out.width, out.dtype, "w", out.stride[1], out.ptrs)
            param, rows, width, dtype = S.layout(op, env, dev)
            stride = env[param]
        else:
            rows, width = int(S._ev(out.rows, env, dev)), int(S._ev(out.width, env, dev))
            dtype = np.dtype(S._DTYPES[out.dtype] if out.dtype in S._DTYPES else S._DTYPES[S._ev(out.dtype, env, dev)])
            stride = env[out.stride] if out.stride else width
        if rows * width == 0:
            continue
        if out.ptrs is None:
            ptrs = [env[out.ptr]]
        else:
            ptrs = list((ctypes.c_uint64 * int(S._ev(out.ptrs, env, dev))).from_address(env[out.ptr]))
        for k, ptr in enumerate(ptrs):
            if ptr:
                found.append((out.ptr if out.ptrs is None else f"{out.ptr}[{k}]", ptr, rows, width, stride, dtype))
    return found


def _body(dev, ptr, rows, width, stride, dtype):
    return S._download(dev, ptr, rows, width, stride, dtype)[1]


@contextlib.contextmanager
def watch(dev, monkeypatch):
    """Inside the block every call of a compute entry point is followed by the check of its output operands.  Yields the log:
    one (entry point, {operand: armed}) per call, `armed` True where the operand was poison in every element before the call."""
    log = []
    real = dev.call

    def checked(name, *args):
        if name in PLUMBING or not (name in S.PROTOS or name in S.UNIT_PROTOS):
            return real(name, *args)
        env = S.arguments(name, args)
        extents = _extents(name, env, dev)
        armed = {label: bool(unwritten(_body(dev, *ext)).all()) for label, *ext in extents}
        result = real(name, *args)
        dev.sync()
        for label, ptr, rows, width, stride, dtype in extents:
            left = unwritten(_body(dev, ptr, rows, width, stride, dtype))
            if (name, label.split("[")[0]) in EXEMPT:
                continue
            assert not left.any(), (f"{name}: {int(left.sum())} of {left.size} elements of {label} ({rows} x {width} {dtype.name}) were not "
                                    f"written, first at (row, column) {tuple(int(i) for i in np.argwhere(left)[0])}; "
                                    f"arguments { {k: v for k, v in env.items() if isinstance(v, (int, float)) and abs(v) < 1 << 32} }")
        log.append((name, armed))
        return result

    with monkeypatch.context() as m:
        m.setattr(dev, "call", checked, raising=False)
        yield log


@pytest.fixture(autouse=True)
def watched(request, monkeypatch):
    """Imported by name into a GPU module: every call of an entry point through ``dev.call`` in a test that uses ``dev`` is followed by
    the check that it wrote every element of its outputs.  Yields the log of ``watch`` (None for a test without the device)."""
    if "dev" not in request.fixturenames:
        yield None
        return
    with watch(request.getfixturevalue("dev"), monkeypatch) as log:
        yield log
