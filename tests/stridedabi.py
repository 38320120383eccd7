"""A padded replay of ``Device.call``: every strided operand of an entry point is moved into a view whose rows are longer than the
field is wide, with poison in the extra columns, before the real entry point runs.

This module owns the parsing of the six headers under include/ (``header_declarations``; ``prototypes`` is its view of the names) and the
registry of strided operands, by the parameter names of the headers.  The registry is two pairs of dicts, kept apart because the
guards of tests/test_strided_abi_cpu.py and tests/test_unwritten_outputs_cpu.py range over the first pair alone:
  * ``PROTOS`` / ``TABLE``: include/xclim_hip.h and the operands whose stride parameter matches ``STRIDE_NAME``, each reached by a
    case of tests/test_gpu_strided_abi.py;
  * ``UNIT_PROTOS`` / ``PITCHED``: the five unit headers, and the operands of every entry point whose row pitches are called ``ld``
    and ``ld_out`` — those of the unit headers (``AGRO_TABLE`` ... ``PHASE_TABLE``, with ``AGRO_TABLES`` ... ``PHASE_TABLES`` for their
    other pointers, the host tables) and the chill and BIO1-BIO19 entry points of the main header.  The padded cases of these
    live in the GPU module of their unit.
``parameters`` and ``operands`` look a name up in both.  ``padded`` is the context manager that replaces ``dev.call`` on one Device.
The shapes of the tests are small, so every operand takes a host round trip (``wrap`` / ``get`` / ``to_device``): the helper runs
on the real device and on the host simulation alike."""
import contextlib
import ctypes
import glob
import os
import re
from collections import namedtuple

import numpy as np

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "xclim_hip.h")
HEADERS = sorted(glob.glob(os.path.join(INCLUDE, "*.h")))   # the main header first: "xclim_hip.h" sorts before "xclim_hip_*.h"
_vp = ctypes.c_void_p

STRIDE_NAME = re.compile(r"^(st\d*|sc|sn|fst|st_\w+|\w+_st|\w+_stride)$")


def header_declarations(path=HEADER):
    """{entry point: [(declaration text, parameter name), ...]} of a header, the context first."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    found = {}
    for name, params in re.findall(r"\b(?:int|const char\*)\s+(xh_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        params = [" ".join(p.split()) for p in params.split(",")]
        found[name] = [(p, re.findall(r"\w+", p)[-1]) for p in params if p and p != "void"]
    return found


def prototypes(path=HEADER):
    """{entry point: [parameter names]} of the header, the context first."""
    return {name: [n for _, n in decl] for name, decl in header_declarations(path).items()}


_KINDS = {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32,
          "size_t": ctypes.c_size_t, "double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int}


def is_ctypes_kind(decl, argtype):
    """Is `argtype` the ctypes kind of a parameter declared as `decl`?  A pointer is c_void_p, c_char_p or a POINTER(...) type;
    a scalar is the one type of its C type name."""
    if "*" in decl:
        return argtype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(argtype, ctypes._Pointer)
    return argtype is _KINDS[decl.replace("const ", "").split()[0]]


PROTOS = prototypes()
UNIT_PROTOS = {name: names for path in HEADERS[1:] for name, names in prototypes(path).items()}


def parameters(name):
    """The parameter names of an entry point of any of the six headers, the context first."""
    return PROTOS[name] if name in PROTOS else UNIT_PROTOS[name]


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

# ---- the pitched entry points (ld / ld_out): one slice per unit, imported by name by the unit's test modules ----------------
_F = "'f8' if f64 else 'f4'"


def _unit(reads, writes, rows="P", in_rows="T", ints=("valid_out", "n_out")):
    return [R(n, "ld", in_rows, dtype=_F) for n in reads] + [W(n, "ld_out", rows, dtype="i4" if n in ints else "f8") for n in writes]


AGRO_TABLE = {
    "xh_agro_degree_sum": _unit(("tas", "tasmin", "tasmax"), ("hi_out", "bedd_out", "valid_out")),
    "xh_agro_monthly": _unit(("tasmin", "tas", "pr", "evspsblpot"), ("cni_out", "mtwm_out", "di_out", "valid_out")),
    "xh_egdd": _unit(("tasmin", "tasmax"), ("egdd_out", "start_out", "end_out", "valid_out")),
    "xh_corn_heat_units": _unit(("tasmin", "tasmax"), ("out",), "T"),
    "xh_qian_wma": _unit(("tas",), ("out",), "T"),
}
HYDRO_TABLE = {
    "xh_flow_period_stats": _unit(("q",), ("bfi_out", "rbi_out", "mean_out", "sum_out", "valid_out")),
    "xh_melt_period_max": _unit(("snw", "pr"), ("out",)),
    "xh_antecedent_precip": _unit(("pr",), ("out",), "T"),
    "xh_sen_slope": _unit(("x",), ("slope_out", "p_out", "n_out"), "K", in_rows="P"),
}
RAIN_TABLE = {
    "xh_rain_season": _unit(("pr",), ("start_out", "end_out", "length_out")),
    "xh_rolling_zones": _unit(("x",), ("out",), in_rows="P"),
}
# (the reduced form of `out` of xh_data_flags is K * P bytes without a pitch and is not replayed on padded views)
FLAGS_TABLE = {
    "xh_data_flags": [R("x", "ld", "T", dtype=_F), R("y0", "ld_y0", "T", dtype=_F), R("y1", "ld_y1", "T", dtype=_F),
                      R("lo", "ld_tab", "D", dtype=_F), R("hi", "ld_tab", "D", dtype=_F), W("out", "ld_out", "K * P", dtype="u1")],
    "xh_doy_bounds": [R("x", "ld", "T", dtype=_F), W("lo", "ld_out", "ndoy", dtype=_F), W("hi", "ld_out", "ndoy", dtype=_F)],
}
_FO = "'f8' if (f64 or method != 0) else 'f4'"
PHASE_TABLE = {
    "xh_precip_phase_map": [R("pr", "ld", "T", dtype=_F), R("tas", "ld", "T", dtype=_F), W("snow_out", "ld_out", "T", dtype=_FO),
                            W("rain_out", "ld_out", "T", dtype=_FO)],
    "xh_precip_phase_period": [R("pr", "ld", "T", dtype=_F), R("tas", "ld", "T", dtype=_F), W("outs", "ld_out", "P", dtype="f8", ptrs=14)],
}
CHILL_TABLE = {
    "xh_chill_hourly": [R("tas", "ld", "H", dtype=_F), W("cp_out", "ld_out", "P", dtype="f8"), W("cu_out", "ld_out", "P", dtype="f8"),
                        W("valid_out", "ld_out", "P", dtype="i4"), W("delta_out", "ld_out", "H", dtype="f8")],
    "xh_chill_daily": [R("tasmin", "ld", "D", dtype=_F), R("tasmax", "ld", "D", dtype=_F), W("cp_out", "ld_out", "P", dtype="f8"),
                       W("cu_out", "ld_out", "P", dtype="f8"), W("valid_out", "ld_out", "P", dtype="i4"),
                       W("hourly_out", "ld_out", "24 * D", dtype="f8")],
}
BIOCLIM_TABLE = {"xh_bioclim": [R(n, "ld", "T", dtype=_F) for n in ("tas", "tasmin", "tasmax", "pr")]
                 + [W("outputs", "ld_out", "P", dtype="f8", ptrs="19"), W("which_out", "ld_out", "P", dtype="i4", ptrs="4"),
                    W("count_out", "ld_out", "P", dtype="i4", ptrs="4")]}
PITCHED = {**AGRO_TABLE, **HYDRO_TABLE, **RAIN_TABLE, **FLAGS_TABLE, **PHASE_TABLE, **CHILL_TABLE, **BIOCLIM_TABLE}

# every other pointer of the unit headers' entry points: the host tables and the dense per-cell / per-latitude inputs (no pitch)
AGRO_TABLES = {
    "xh_agro_degree_sum": ("seg", "day_sel", "k_cell", "k_day", "k_period", "lat_idx"),
    "xh_agro_monthly": ("month_off", "month_cal", "month_days", "seg_months", "lat"),
    "xh_egdd": ("seg", "doy", "start_from", "end_from", "day0", "label_doy", "label_days"),
    "xh_corn_heat_units": (),
    "xh_qian_wma": (),
}
HYDRO_TABLES = {"xh_flow_period_stats": ("seg",), "xh_melt_period_max": ("seg",), "xh_antecedent_precip": ("weights",),
                "xh_sen_slope": ("period_of",)}
RAIN_TABLES = {"xh_rain_season": ("seg", "flags", "doy"), "xh_rolling_zones": ("edges",)}
FLAGS_TABLES = {"xh_data_flags": ("checks", "seg", "tidx"), "xh_doy_bounds": ("tbase",)}
PHASE_TABLES = {"xh_precip_phase_map": ("par", "tab", "season", "land"), "xh_precip_phase_period": ("seg", "doy", "par", "tab", "season", "land", "lim")}
HOST_TABLES = {**AGRO_TABLES, **HYDRO_TABLES, **RAIN_TABLES, **FLAGS_TABLES, **PHASE_TABLES}


def operands(name):
    """The strided operands of an entry point of either table; () for one that has none."""
    return TABLE[name] if name in TABLE else PITCHED.get(name, ())

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
        return eval(expr, {}, env)  # noqa: S307 - the expressions of the tables above
    return expr


def arguments(name, args):
    """{parameter name: value} of one dev.call (the context is not among the arguments)."""
    names = parameters(name)[1:]
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
    """Inside the block every call of an entry point of TABLE or PITCHED runs on padded, poisoned row views (see the module text).
    Yields the log: one (entry point, {stride parameter: (stride used, width of the operand)}) per replayed call."""
    log = []
    real = dev.call

    def replay(name, *args):
        ops = operands(name)
        if not ops:
            return real(name, *args)
        names = parameters(name)[1:]
        env = arguments(name, args)
        new = list(args)
        buffers, pad_of, used, finish = {}, {}, {}, []
        nread = 0
        # memory that one operand reads and another writes (an in-place call) is one buffer that keeps what the caller held
        single = [op for op in ops if op.ptrs is None and env[op.ptr]]
        inplace = {env[op.ptr] for op in single if op.mode == "r"} & {env[op.ptr] for op in single if op.mode != "r"}
        for op in ops:
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
