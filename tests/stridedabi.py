"""A padded replay of ``Device.call``: every strided operand of an entry point of include/xclim_hip.h is moved into a view
whose rows are longer than the field is wide, with poison in the extra columns, before the real entry point runs.

``TABLE`` maps each entry point to its strided operands (by the parameter names of the header); ``padded`` is the context
manager that replaces ``dev.call`` on one Device.  The shapes of the tests are small, so every operand takes a host round
trip (``wrap`` / ``get`` / ``to_device``): the helper runs on the real device and on the host simulation alike."""
import contextlib
import ctypes
import os
import re
from collections import namedtuple

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xclim_hip.h")
_vp = ctypes.c_void_p

STRIDE_NAME = re.compile(r"^(st\d*|sc|sn|fst|st_\w+|\w+_st|\w+_stride)$")


def prototypes(path=HEADER):
    """{entry point: [parameter names]} of the header, the context first."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    protos = {}
    for name, params in re.findall(r"\b(?:int|const char\*)\s+(xh_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        names = []
        for p in params.split(","):
            p = p.strip()
            if p and p != "void":
                names.append(re.findall(r"\w+", p)[-1])
        protos[name] = names
    return protos


PROTOS = prototypes()

# ptr / stride: parameter names.  rows / width / dtype: an expression over the call's arguments (by parameter name), or a
# function (arguments, device).  mode: r (read), w (written everywhere), rw (written in part: what the caller held is kept).
# minor: the cell-stride parameter of the seven column entry points, which also take the time-minor layout (st == 1,
# sc >= T): the padded axis is then that one.  ptrs: the pointer argument is a HOST array of that many device pointers.
Op = namedtuple("Op", "ptr stride rows width dtype mode minor ptrs")


def R(ptr, stride="st", rows="T", width="C", dtype="f4", minor=None, ptrs=None):
    return Op(ptr, stride, rows, width, dtype, "r", minor, ptrs)


def W(ptr, stride, rows="T", width="C", dtype="f4", mode="w", minor=None, ptrs=None):
    return Op(ptr, stride, rows, width, dtype, mode, minor, ptrs)


def _thr_rows(a, dev):
    """Rows of the threshold table of xh_threshold_count: T for a full field, else the largest row the index reaches."""
    if a["thr_kind"] in (4, 5):
        return a["T"]
    idx = dev.wrap(a["tidx"], (a["T"],), np.int32).get()
    return int(idx.max()) + 1


X, X8 = R("x"), R("x", dtype="f8")
XM = R("x", minor="sc")   # the column entry points also take st == 1, sc >= T
_MIX1, _MIX2 = "'f4' if dtypes == 1 else 'f8'", "'f4' if dtypes == 2 else 'f8'"
_MASK_OR_F4 = "'u1' if out_kind == 0 else 'f4'"
_PET = "'f8' if f64 else 'f4'"
_FIRE_IN = [R(n) for n in ("tas", "pr", "hurs", "sfcwind", "snd")]
_PLANE = [R("xnew"), R("base"), W("scen", "scen_st")]
_TRAIN = [R("ref"), R("hist")]

TABLE = {
    "xh_fill_synthetic": [W("out", "st")],
    "xh_transpose_f32": [R("in", "in_stride", "rows", "cols"), W("out", "out_stride", "cols", "rows")],
    "xh_threshold_count": [X, R("thr_table", "thr_stride", _thr_rows, dtype="'f8' if thr_kind in (2, 4) else 'f4'")],
    "xh_threshold_count_doy": [X, R("thr_table", "thr_stride", "ndoy", dtype="f8")],
    "xh_domain_count": [X],
    "xh_bivariate_count": [R("x1", "st1"), R("x2", "st2")],
    "xh_range_reduce": [R("low", "st_low"), R("high", "st_high")],
    "xh_select_rows": [X, W("out", "st_out", "n")],
    "xh_compare_map": [R("a"), R("b", "st_b"), W("out", "st_out", dtype=_MASK_OR_F4)],
    "xh_thresholded_reduce": [X],
    "xh_mask_rows": [X, W("out", "out_st")],
    "xh_doy_mean_std": [X],
    "xh_resample_reduce": [X],
    "xh_rolling_reduce": [X, W("out", "out_st")],
    "xh_cumsum_reset": [X, W("out", "out_st")],
    "xh_rle": [X, W("out", "out_st")],
    "xh_run_stats": [X],
    "xh_spell_mask": [X, W("out", "out_st")],
    "xh_spell_run_stats": [X],
    "xh_spell_mask_multi": [R("xs", ptrs="nvar"), W("out", "out_st")],
    "xh_runs_with_holes": [R("start"), R("stop"), W("out", "out_st")],
    "xh_keep_longest_run": [X, W("out", "out_st")],
    "xh_season": [X],
    "xh_max_run_sum": [X],
    "xh_run_events": [R("runs"), R("eff"), R("data")],
    "xh_suspicious_run": [X, W("out", "out_st", dtype="u1")],
    "xh_nan_quantile": [R("x", "sn", "N", minor="sc")],
    "xh_threshold_count_f64": [X8, R("thr_table", "thr_stride", _thr_rows, dtype="f8")],
    "xh_resample_reduce_f64": [X8],
    "xh_nan_quantile_f64": [R("x", "sn", "N", dtype="f8", minor="sc")],
    "xh_compare_map_f64": [R("a", dtype=_MIX1), R("b", "st_b", dtype=_MIX2), W("out", "st_out", dtype=_MASK_OR_F4)],
    "xh_run_stats_f64": [X8],
    "xh_spell_mask_f64": [X8, W("out", "out_st")],
    "xh_spell_run_stats_f64": [X8],
    "xh_run_stats_doy_f64": [X8],
    "xh_percentile_doy_f64": [X8],
    "xh_thresholded_reduce_f64": [X8],
    "xh_range_reduce_f64": [R("low", "st_low", dtype=_MIX1), R("high", "st_high", dtype=_MIX2)],
    "xh_domain_count_f64": [X8],
    "xh_bivariate_count_f64": [R("x1", "st1", dtype=_MIX1), R("x2", "st2", dtype=_MIX2)],
    "xh_rolling_reduce_f64": [X8, W("out", "out_st", dtype="f8")],
    "xh_weighted_quantile": [R("x", "sn", "N")],
    "xh_percentile_doy": [X],
    "xh_percentile_doy_mapped": [X],
    "xh_percentile_doy_count": [X],
    "xh_within_bnds_doy": [X],
    "xh_mask_doy_cells": [X, W("out", "out_st")],
    "xh_mask_days_cells": [X, W("out", "out_st")],
    "xh_rolling_dot": [X, W("out", "out_st")],
    "xh_compare_doy": [X, W("out", "st_out")],
    "xh_run_stats_doy": [X],
    "xh_precip_over_doy": [X],
    "xh_quantile_series": [XM],
    "xh_eqm_train": [R("ref", minor="sc"), R("hist", minor="sc")],
    "xh_eqm_train_window": _TRAIN,
    "xh_dqm_train_window": _TRAIN,
    "xh_eqm_train_groups": _TRAIN,
    "xh_dqm_train_groups": _TRAIN,
    "xh_eqm_adjust": [R("sim"), W("scen", "scen_st")],
    "xh_eqm_adjust_g2d": [R("sim", rows="n"), W("scen", "scen_st", "n")],
    "xh_apply_factor": [R("base"), R("fac", "fst"), W("out", "out_st")],
    "xh_plane_linear": _PLANE,
    "xh_plane_nearest": _PLANE,
    "xh_qdm_adjust": [R("sim", minor="sc"), W("scen", "st", minor="sc")],
    "xh_qdm_adjust_groups": [R("sim"), W("scen", "scen_st", mode="rw")],
    "xh_quantile_cells": [XM],
    "xh_adapt_freq": [R("sim", minor="sc"), W("scen", "st", minor="sc")],
    "xh_poly_trend": [X],
    "xh_trend_apply": [X, W("out", "out_st")],
    "xh_poly_trend_u": [X],
    "xh_trend_apply_u": [X, W("out", "out_st")],
    "xh_window_nanmean": [X, W("out", "out_st")],
    "xh_poly_trend_groups": [R("x")],
    "xh_trend_apply_groups": [R("x"), W("out", "out_st", mode="rw")],
    "xh_fire_weather": _FIRE_IN + [R("season_mask", "st_mask", dtype="u1"), W("outputs", "st_out", ptrs="7"),
                                   W("season_mask_out", "st_out", dtype="u1")],
    "xh_pet_daily": [R(n, dtype=_PET) for n in ("tasmin", "tasmax", "tas", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcwind", "pr")]
                    + [W("pet_out", "st_out", dtype="f8"), W("wb_out", "st_out", dtype="f8")],
    "xh_pet_monthly": [R(n, dtype=_PET) for n in ("tasmin", "tasmax", "tas", "pr")]
                      + [W("pet_out", "st_out", "M", dtype="f8"), W("wb_out", "st_out", "M", dtype="f8")],
    "xh_mcarthur": [R("pr", dtype="'f8' if pr_f64 else 'f4'")]
                   + [R(n, dtype="'f8' if tas_f64 else 'f4'") for n in ("tasmax", "hurs", "sfcwind")]
                   + [R(n, dtype="'f8' if smd_f64 else 'f4'") for n in ("smd", "df")]
                   + [W(n, "st_out", dtype="f8") for n in ("kbdi_out", "df_out", "ffdi_out")],
    "xh_si_fit": [R("x")],
    "xh_si_apply": [R("x"), W("out", "st_out", dtype="f8")],
    "xh_si_fit_f64": [R("x", dtype="f8")],
    "xh_si_apply_f64": [R("x", dtype="f8"), W("out", "st_out", dtype="f8")],
}

# entry points with a stride-like parameter that move bytes and compute nothing
EXEMPT = {}

_DTYPES = {"f4": np.float32, "f8": np.float64, "u1": np.uint8, "i4": np.int32}


def _value(arg):
    """An argument of dev.call as a python number (pointers as addresses, None as 0)."""
    if arg is None:
        return 0
    if isinstance(arg, ctypes.Array):
        return ctypes.addressof(arg)
    if hasattr(arg, "value"):
        return arg.value or 0
    return arg


def _ev(expr, env, dev):
    if callable(expr):
        return expr(env, dev)
    if isinstance(expr, str):
        return eval(expr, {}, env)  # noqa: S307 - the expressions of TABLE above
    return expr


def arguments(name, args):
    """{parameter name: value} of one dev.call (the context is not among the arguments)."""
    names = PROTOS[name][1:]
    assert len(names) == len(args), (name, len(names), len(args))
    return {n: _value(a) for n, a in zip(names, args)}


def layout(op, env, dev):
    """(stride parameter, rows, width, dtype) of an operand in this call: time-minor calls pad the cell stride."""
    rows, width = int(_ev(op.rows, env, dev)), int(_ev(op.width, env, dev))
    dtype = np.dtype(_DTYPES[op.dtype] if op.dtype in _DTYPES else _DTYPES[_ev(op.dtype, env, dev)])
    if op.minor and env[op.stride] == 1 and env[op.minor] != 1:
        return op.minor, width, rows, dtype
    return op.stride, rows, width, dtype


def _dense_view(flat, rows, width, stride):
    return np.lib.stride_tricks.as_strided(flat, (rows, width), (stride * flat.itemsize, flat.itemsize))


def _download(dev, ptr, rows, width, stride, dtype):
    """(flat, view): the caller's operand with its own row stride, flat as it lies in memory and as (rows, width)."""
    flat = dev.wrap(ptr, ((rows - 1) * stride + width,), dtype).get()
    return flat, _dense_view(flat, rows, width, stride)


class _Buffer:
    def __init__(self, dev, mode, ptr, rows, width, stride0, dtype, pad, shift, poison):
        self.ptr0, self.rows, self.width, self.stride0, self.dtype, self.mode = ptr, rows, width, stride0, dtype, mode
        self.stride, self.shift = width + pad, shift
        host = np.empty(shift + rows * self.stride, dtype)
        host.view(np.uint8)[:] = 0xA5
        body = host[shift:].reshape(rows, self.stride)
        if mode in ("r", "rw"):
            body[:, :width] = _download(dev, ptr, rows, width, stride0, dtype)[1]
        if mode == "r":
            body[:, width:] = poison
            host[:shift] = poison
        self.dev_array = dev.to_device(host)
        self.ptr = self.dev_array.ptr + shift * dtype.itemsize

    def finish(self, dev, name):
        """After the call: the pads must be untouched, and the caller's buffer receives what was written."""
        if self.mode == "r":
            return
        host = self.dev_array.get()
        body = host[self.shift:].reshape(self.rows, self.stride)
        dirty = (np.ascontiguousarray(body[:, self.width:]).view(np.uint8) != 0xA5).any() or (host[:self.shift].view(np.uint8) != 0xA5).any()
        assert not dirty, f"{name}: wrote into the padding of a row (stride {self.stride}, width {self.width})"
        flat, view = _download(dev, self.ptr0, self.rows, self.width, self.stride0, self.dtype)
        view[...] = body[:, :self.width]
        tmp = dev.to_device(flat)
        dev.copy_d2d(self.ptr0, tmp.ptr, flat.nbytes)
        dev.sync()


@contextlib.contextmanager
def padded(dev, monkeypatch, pads=(1, 3, 5), shift=0):
    """Inside the block every call of an entry point of TABLE runs on padded, poisoned row views (see the module text).
    Yields the log: one (entry point, {stride parameter: (stride used, width of the operand)}) per replayed call."""
    log = []
    real = dev.call

    def replay(name, *args):
        if name not in TABLE:
            return real(name, *args)
        names = PROTOS[name][1:]
        env = arguments(name, args)
        new = list(args)
        buffers, pad_of, used, finish = {}, {}, {}, []
        nread = 0
        # memory that one operand reads and another writes (an in-place call) is one buffer that keeps what the caller held
        single = [op for op in TABLE[name] if op.ptrs is None and env[op.ptr]]
        inplace = {env[op.ptr] for op in single if op.mode == "r"} & {env[op.ptr] for op in single if op.mode != "r"}
        for op in TABLE[name]:
            if not env[op.ptr]:
                continue
            param, rows, width, dtype = layout(op, env, dev)
            if rows * width == 0:
                continue
            stride0 = env[param]
            if op.ptrs is None:
                ptrs = [env[op.ptr]]
            else:
                n = int(_ev(op.ptrs, env, dev))
                ptrs = list((ctypes.c_uint64 * n).from_address(env[op.ptr]))
            out = []
            for ptr in ptrs:
                if not ptr:
                    out.append(0)
                    continue
                buf = buffers.get(ptr)
                if buf is None:
                    if param not in pad_of:
                        pad_of[param] = pads[len(pad_of) % len(pads)]
                    nread += op.mode == "r"
                    if dtype.kind == "f":
                        poison = (1e30, np.nan)[nread % 2]
                    else:
                        poison = 249
                    mode = "rw" if ptr in inplace else op.mode
                    buf = buffers[ptr] = _Buffer(dev, mode, ptr, rows, width, stride0, dtype, pad_of[param], shift, poison)
                    finish.append(buf)
                else:   # the same memory under two names (in place): one buffer, one stride
                    assert (buf.rows, buf.width, buf.dtype) == (rows, width, dtype), f"{name}: {op.ptr} aliases another shape"
                    assert pad_of.setdefault(param, buf.stride - width) == buf.stride - width, f"{name}: {param} cannot serve the alias"
                out.append(buf.ptr)
                used[param] = (buf.stride, width)
            if op.ptrs is None:
                new[names.index(op.ptr)] = _vp(out[0])
            else:
                new[names.index(op.ptr)] = (ctypes.c_uint64 * len(out))(*out)
            new[names.index(param)] = used.get(param, (stride0,))[0]
        result = real(name, *new)
        for buf in finish:
            buf.finish(dev, name)
        dev.sync()   # (the padded copies go back to the pool when this returns)
        log.append((name, used))
        return result

    with monkeypatch.context() as m:
        m.setattr(dev, "call", replay, raising=False)
        yield log
