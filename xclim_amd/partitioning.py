"""Host mirror of ``xclim.ensembles._partitioning`` (reference: src/xclim/ensembles/_partitioning.py) and of
``ensemble_mean_std_max_min`` (src/xclim/ensembles/_base.py:141-211) on the uncertainty-partitioning unit
(include/units/xclim_hip_partition.h).

A field is a numpy or device array ``(time, *member axes in the order of dims, *cells)`` with an annual :class:`TimeAxis`.  One
launch of ``xh_partition_smooth`` fits the polynomial of every series, masks it, subtracts or divides by the baseline mean and
takes the rolling statistic of the residual; one launch of ``xh_partition_components`` folds the member axes.  The partition
functions return ``(g, u)``: ``g`` ``(time, *cells)`` and ``u`` ``(component, time, *cells)`` float64 with the components in the
reference's order (:data:`HS_COMPONENTS`, :data:`LS_COMPONENTS`, :func:`general_components`); with ``keep=True`` the smoothed cube
follows as a third, device-resident ``(time, members, cells)`` array that can be passed back as ``sm``.

:class:`NotServed` (the adapter forwards these to the reference): integer or chunked fields, ``da`` and ``sm`` of different dtypes,
more than 512 years, more than 4 member axes or sizes beyond the unit's limits, member axes beyond those the function partitions,
a ``mean_first`` dimension that is also in ``weights`` (the reference's result then grows extra dimensions by broadcasting), and a
series whose fit is ill-posed (fewer valid years than coefficients, or a pivot below the rcond analogue: the reference's
minimum-norm answer is not reproduced).

ASSUMPTIONS (xarray cannot be executed where this was built): ``polyfit`` fits on nanoseconds since 1970-01-01 as float64 with
``np.vander``, columns scaled by their norms over ALL rows, ``lstsq`` on the rows that are not NaN with ``rcond = T eps``;
``polyval`` is Horner on the same numbers; ``rolling(center=True)`` of window w covers rows i - w // 2 .. i + (w - 1) // 2 with
``min_periods = w``; ``weighted`` gives NaN entries zero weight; ``mean(dim=[...])`` over several dimensions pools them; the fitted
values do not depend on the origin or unit of the abscissa beyond rounding, so every calendar is served through
``TimeAxis.ordinal()``.
"""

from __future__ import annotations

import numpy as np

from . import _capi as capi
from . import kernels as K
from ._capi import DeviceArray, get_device
from .fields import NotServed
from .timeaxis import TimeAxis

HS_COMPONENTS = ("variability", "model", "scenario", "total")
LS_COMPONENTS = ("model", "scenario", "downscaling", "variability", "total")
_GP_DEFAULT = ["model", "reference", "adjustment"]


def general_components(var_first=None, mean_first=None) -> tuple:
    """The ``uncertainty`` coordinate of ``general_partition``: mean_first, var_first, "variability", "total"."""
    return (*(mean_first or ["scenario"]), *(var_first or _GP_DEFAULT), "variability", "total")


def _years(time, T: int) -> np.ndarray:
    """The years of an annual axis: one stamp per consecutive year (the reference asks ``xr.infer_freq`` for "A" / "Y")."""
    if not isinstance(time, TimeAxis):
        raise TypeError("time must be the TimeAxis of da")
    if len(time) != T:
        raise ValueError(f"time has {len(time)} stamps, da {T} rows")
    y = np.asarray(time.year)
    if T < 3 or not np.all(np.diff(y) == 1):   # (infer_freq needs three stamps)
        raise ValueError("This algorithm expects annual time series.")
    return y


def poly_basis(time: TimeAxis, deg: int = 4) -> np.ndarray:
    """float64 (T, deg + 1): the orthonormal factor of the Vandermonde matrix of the time abscissa, centred on its mean and scaled
    by its largest distance from it."""
    x = np.asarray(time.ordinal(), np.float64)
    x = x - x.mean()
    x = x / max(np.abs(x).max(), 1.0)
    q, _ = np.linalg.qr(np.vander(x, deg + 1, increasing=True))
    return np.ascontiguousarray(q)


def _cube(a, nmember: int, dev, what: str):
    """(DeviceArray (T, N, C), member lengths, cells shape) of a numpy or device array (T, *members, *cells) in its own dtype."""
    if not isinstance(a, DeviceArray):
        if getattr(a, "chunks", None) is not None:
            raise NotServed(f"partitioning: {what} is chunked")
        a = np.asarray(a)
    if np.dtype(a.dtype).kind in "iub":
        raise NotServed(f"partitioning: {what} is an integer field")
    if np.dtype(a.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise NotServed(f"partitioning: {what} is {np.dtype(a.dtype).name}; float32 and float64 fields are served")
    if len(a.shape) < 1 + nmember:
        raise ValueError(f"partitioning: {what} {tuple(a.shape)} has no room for time and {nmember} member axes")
    T, members, cells = int(a.shape[0]), [int(v) for v in a.shape[1:1 + nmember]], tuple(int(v) for v in a.shape[1 + nmember:])
    N, C = int(np.prod(members, dtype=np.int64)), int(np.prod(cells, dtype=np.int64))
    if nmember > capi.PT_MAX_AXES:
        raise NotServed(f"partitioning: {nmember} member axes; up to {capi.PT_MAX_AXES} are served")
    if T > capi.PT_MAX_T:
        raise NotServed(f"partitioning: {T} years; up to {capi.PT_MAX_T} are served")
    if any(m > capi.PT_MAX_AXIS for m in members) or N > capi.PT_MAX_MEMBERS or N < 1:
        raise NotServed(f"partitioning: member axes {members}; up to {capi.PT_MAX_AXIS} entries each and {capi.PT_MAX_MEMBERS} members are served")
    if isinstance(a, DeviceArray):
        return a.reshape(T, N, C), members, cells
    return dev.to_device(np.ascontiguousarray(a.reshape(T, N, C))), members, cells


def _same_dtype(da, sm) -> None:
    """``da`` and a given ``sm`` of one dtype (asked before anything is uploaded)."""
    if sm is not None and np.dtype(sm.dtype) != np.dtype(da.dtype):
        raise NotServed(f"partitioning: da is {np.dtype(da.dtype).name} and sm {np.dtype(sm.dtype).name}")


def _given_sm(sm, y: DeviceArray, nmember: int, dev):
    if not isinstance(sm, DeviceArray):
        sm = np.asarray(sm)
    _same_dtype(y, sm)
    s = sm if isinstance(sm, DeviceArray) and len(sm.shape) == 3 else _cube(sm, nmember, dev, "sm")[0]
    if tuple(s.shape) != tuple(y.shape):
        raise ValueError(f"partitioning: sm {tuple(sm.shape)} does not have the shape of da")
    return s


def _smooth(dev, y, sm, nmember, time, T, deg, **kw):
    """One launch of xh_partition_smooth; NotServed when the launch raises the ill-posed flag."""
    if sm is None:
        res = K.partition_smooth(dev, y, poly_basis(time, deg), **kw)
    else:
        res = K.partition_smooth(dev, y, sm_in=_given_sm(sm, y, nmember, dev), **kw)
    if res["flag"].get()[0]:
        raise NotServed("partitioning: a series has fewer valid years than coefficients, or an ill-conditioned fit")
    return res


def _finish(out, g, planes, cells, res, keep):
    o = out.get()
    T = o.shape[1]
    u = np.stack([o[k] for k in planes]).reshape((len(planes), T) + cells)
    gg = g.get().reshape((T,) + cells)
    return (gg, u, res["sm"]) if keep else (gg, u)


def poly_smooth(da, time, deg: int = 4, *, device=None, keep: bool = False):
    """The masked polynomial fit of every series of ``da`` ``(time, ...)``: the reference's
    ``xr.polyval(da.time, da.polyfit("time", deg, skipna=True).polyfit_coefficients).where(da.notnull())``, float64."""
    dev = device or get_device()
    if not 0 <= int(deg) <= capi.PT_MAX_DEG:
        raise NotServed(f"poly_smooth: degree {deg}; 0 .. {capi.PT_MAX_DEG} are served")
    shape = tuple(da.shape)
    y, _, _ = _cube(da, 0, dev, "da")
    _years(time, shape[0])
    res = _smooth(dev, y, None, 0, time, shape[0], int(deg), outputs=("sm", "flag"))
    return res["sm"] if keep else res["sm"].get().reshape(shape)


def _axes(dims, needed, message):
    dims = tuple(dims)
    if not set(needed).issubset(dims):
        raise ValueError(message)
    if set(dims) != set(needed) or len(dims) != len(set(dims)):
        raise NotServed(f"partitioning: member axes {dims} beyond {tuple(needed)}: put them among the cells")
    return dims


def hawkins_sutton(da, sm=None, weights=None, baseline=("1971", "2000"), kind: str = "+", *, time, dims=("scenario", "model"),
                   device=None, keep: bool = False):
    """_partitioning.py:57-162.  ``weights``: a vector over the models.  Components: :data:`HS_COMPONENTS`."""
    dev = device or get_device()
    years = _years(time, int(da.shape[0]))
    dims = _axes(dims, ("scenario", "model"), "DataArray dimensions should include 'time', 'scenario' and 'model'.")
    _same_dtype(da, sm)
    y, members, cells = _cube(da, 2, dev, "da")
    T = y.shape[0]
    m_ax, s_ax = dims.index("model"), dims.index("scenario")
    rows = np.flatnonzero((years >= int(baseline[0])) & (years <= int(baseline[1])))
    b = (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)
    after = np.flatnonzero(years >= 2000)
    t0 = int(after[0]) if after.size else T
    if sm is not None:   # n_valid then counts sm: the members without data are found on the host
        missing = bool(np.isnan(y.get()).all(axis=0).any())
    res = _smooth(dev, y, sm, 2, time, T, 4, window=10, stat="mean", baseline=b, kind="+" if kind not in ("+", "*") else kind)
    if sm is None:
        missing = bool((res["n_valid"].get() == 0).any())
    if missing:
        raise ValueError("Some models are missing data for some scenarios")
    if kind not in ("+", "*"):
        raise ValueError(kind)
    w = np.ones(members[m_ax]) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w.size != members[m_ax]:
        raise ValueError(f"hawkins_sutton: {members[m_ax]} model weights needed, got {w.size}")
    comps = [(s_ax, "mean_then_var", "user"), (m_ax, "var_then_mean", "user")]   # total = variability + scenario + model
    out, g = K.partition_components(dev, res["sm"], res["roll"], members, comps, weights=w, w_axis=m_ax, variab="hs", t0=t0,
                                    g_order=(m_ax, s_ax))
    return _finish(out, g, (0, 2, 1, 3), cells, res, keep)


def lafferty_sriver(da, sm=None, bb13: bool = False, *, time, dims=("scenario", "model", "downscaling"), device=None, keep: bool = False):
    """_partitioning.py:192-281.  Components: :data:`LS_COMPONENTS`."""
    dev = device or get_device()
    _years(time, int(da.shape[0]))
    dims = _axes(dims, ("scenario", "model", "downscaling"), "DataArray dimensions should include 'time', 'scenario', 'downscaling' and 'model'.")
    _same_dtype(da, sm)
    y, members, cells = _cube(da, 3, dev, "da")
    res = _smooth(dev, y, sm, 3, time, y.shape[0], 4, window=11, stat="var")
    s_ax, m_ax, d_ax = dims.index("scenario"), dims.index("model"), dims.index("downscaling")
    comps = [(s_ax, "var_then_mean" if bb13 else "mean_then_var", "none"), (m_ax, "var_then_mean", "count"), (d_ax, "var_then_mean", "count")]
    out, g = K.partition_components(dev, res["sm"], res["roll"], members, comps, g_order=(m_ax, s_ax, d_ax))
    return _finish(out, g, (2, 1, 3, 0, 4), cells, res, keep)


def general_partition(da, sm="poly", var_first=None, mean_first=None, weights=None, *, time, dims, device=None, keep: bool = False):
    """_partitioning.py:284-401.  Components: :func:`general_components`."""
    dev = device or get_device()
    var_first = list(var_first or _GP_DEFAULT)
    mean_first = list(mean_first or ["scenario"])
    weights = list(weights or _GP_DEFAULT)
    all_types = mean_first + var_first
    _years(time, int(da.shape[0]))
    dims = _axes(dims, all_types, f"DataArray dimensions should include {all_types} and time.")
    if isinstance(sm, str):
        if sm != "poly":
            raise ValueError("sm should be 'poly' or a DataArray.")
        sm = None
    elif sm is None or not hasattr(sm, "shape"):
        raise ValueError("sm should be 'poly' or a DataArray.")
    if any(t in weights for t in mean_first):
        raise NotServed("general_partition: a mean_first dimension that is weighted (the reference's result grows dimensions)")
    _same_dtype(da, sm)
    y, members, cells = _cube(da, len(dims), dev, "da")
    res = _smooth(dev, y, sm, len(dims), time, y.shape[0], 4, window=11, stat="var")
    comps = [(dims.index(t), "mean_then_var", "none") for t in mean_first]
    comps += [(dims.index(t), "var_then_mean", "count" if t in weights else "none") for t in var_first]
    k = len(comps)
    out, g = K.partition_components(dev, res["sm"], res["roll"], members, comps, g_order=tuple(dims.index(t) for t in all_types))
    return _finish(out, g, (*range(1, k + 1), 0, k + 1), cells, res, keep)


def _host(a):
    return a.get() if isinstance(a, DeviceArray) else np.asarray(a)


def fractional_uncertainty(u, components) -> np.ndarray:
    """_partitioning.py:404-423: ``u / u[total] * 100`` along the leading component axis named by ``components``."""
    u = _host(u)
    return u / u[list(components).index("total")] * 100


def hawkins_sutton_09_weighting(da, obs, baseline=("1971", "2000"), *, time) -> np.ndarray:
    """_partitioning.py:165-189: 1 / (obs + |x_m - obs|) with x_m the value of the baseline's last year minus the baseline mean;
    ``da`` is (time, model, ...)."""
    a = _host(da)
    years = np.asarray(time.year)
    sel = (years >= int(baseline[0])) & (years <= int(baseline[1]))
    with np.errstate(all="ignore"):
        mm = np.nanmean(a[sel], axis=0)
    xm = np.squeeze(a[years == int(baseline[1])], axis=0) - mm
    return 1 / (obs + np.abs(xm - obs))


def ensemble_mean_std_max_min(ens, min_members: int | None = 1, weights=None, *, device=None, keep: bool = False):
    """_base.py:141-211 for one variable ``(realization, ...)``: {"mean", "stdev", "max", "min"}, float64.  ``keep=True``: the
    device array (4, E) under "stats" instead."""
    dev = device or get_device()
    if not isinstance(ens, DeviceArray):
        if getattr(ens, "chunks", None) is not None:
            raise NotServed("ensemble_mean_std_max_min: a chunked field")
        ens = np.asarray(ens)
    if np.dtype(ens.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise NotServed(f"ensemble_mean_std_max_min: {np.dtype(ens.dtype).name} fields; float32 and float64 are served")
    R, rest = int(ens.shape[0]), tuple(int(v) for v in ens.shape[1:])
    if not 1 <= R <= 65535:
        raise NotServed(f"ensemble_mean_std_max_min: {R} realizations")
    x = ens.reshape(R, -1) if isinstance(ens, DeviceArray) else dev.to_device(np.ascontiguousarray(ens.reshape(R, -1)))
    out = K.ensemble_stats(dev, x, weights, R if min_members is None else int(min_members))
    if keep:
        return {"stats": out}
    o = out.get()
    return {name: o[capi.ES_ROWS[row]].reshape(rest) for name, row in (("mean", "mean"), ("stdev", "std"), ("max", "max"), ("min", "min"))}


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------------
ADAPTED = ("hawkins_sutton", "lafferty_sriver", "general_partition")


def make_adapters(env, originals: dict, xr=None) -> dict:
    """``hawkins_sutton``, ``lafferty_sriver`` and ``general_partition`` of ``xclim.ensembles._partitioning`` on DataArrays with
    their dimensions in any order: ``g`` keeps the dimensions of ``da`` without the member dimensions, in their order, the
    components the same behind a leading ``uncertainty`` dimension with its coordinate; the attributes are those of
    _partitioning.py:155-157, :273-275 and :386-392.  Whatever raises :class:`NotServed` goes to the original."""
    from .xr_adapter import forwarding_adapter, time_axis_of

    DA = env.DataArray

    def cube(da, needed, what):
        if not isinstance(da, DA):
            raise NotServed(f"partitioning: {what} is not a DataArray")
        if getattr(da.data, "chunks", None) is not None:
            raise NotServed(f"partitioning: {what} is chunked")
        if "time" not in da.dims:
            raise NotServed(f"partitioning: {what} has no time dimension")
        members = tuple(d for d in da.dims if d in needed)
        rest = tuple(d for d in da.dims if d != "time" and d not in members)
        return np.asarray(da.transpose("time", *members, *rest).values), members, rest

    def axis(da):
        try:
            return time_axis_of(da)
        except Exception:
            raise NotServed("partitioning: a time coordinate without calendar fields") from None

    def given(sm, da, members, rest):
        if sm is None:
            return None
        if not isinstance(sm, DA) or set(sm.dims) != set(da.dims):
            raise NotServed("partitioning: sm is not a DataArray on the dimensions of da")
        return np.ascontiguousarray(sm.transpose("time", *members, *rest).values)   # (a copy: the caller's sm stays as it is)

    def wrap(da, g, u, names, members, rest, attrs):
        keep = tuple(d for d in da.dims if d not in members)
        perm = [("time", *rest).index(d) for d in keep]
        coords = {k: c for k, c in da.coords.items() if k in keep}
        g_da = DA(np.transpose(g, perm), dims=keep, coords=coords, name=da.name)
        ucoords = dict(coords, uncertainty=DA(np.array(names), dims=("uncertainty",)))
        u_attrs = dict(attrs)
        for d in members:
            u_attrs[d] = np.asarray(da.coords[d].values) if d in da.coords else np.arange(da.shape[da.dims.index(d)])
        u_da = DA(np.transpose(u, [0] + [p + 1 for p in perm]), dims=("uncertainty",) + keep, coords=ucoords, attrs=u_attrs)
        return g_da, u_da

    def hs(p):
        da, sm, weights = p["da"], p["sm"], p["weights"]
        a, members, rest = cube(da, ("scenario", "model"), "da")
        w = None
        if weights is not None:
            if not isinstance(weights, DA) or tuple(weights.dims) != ("model",):
                raise NotServed("hawkins_sutton: weights along more than model")
            w = np.asarray(weights.values, np.float64)
        g, u = hawkins_sutton(a, given(sm, da, members, rest), w, tuple(p["baseline"]), p["kind"], time=axis(da), dims=members)
        return wrap(da, g, u, HS_COMPONENTS, ("model", "scenario"), rest, {})

    def ls(p):
        da = p["da"]
        a, members, rest = cube(da, ("scenario", "model", "downscaling"), "da")
        g, u = lafferty_sriver(a, given(p["sm"], da, members, rest), bool(p["bb13"]), time=axis(da), dims=members)
        return wrap(da, g, u, LS_COMPONENTS, ("model", "scenario", "downscaling"), rest, {})

    def gp(p):
        da, sm = p["da"], p["sm"]
        var_first, mean_first = list(p["var_first"] or _GP_DEFAULT), list(p["mean_first"] or ["scenario"])
        all_types = mean_first + var_first
        a, members, rest = cube(da, all_types, "da")
        if isinstance(sm, str) or not isinstance(sm, DA):
            given_sm = sm if isinstance(sm, str) else None   # (None: the mirror raises the reference's ValueError)
        else:
            given_sm = given(sm, da, members, rest)
        g, u = general_partition(a, given_sm, var_first, mean_first, p["weights"], time=axis(da), dims=members)
        attrs = {"indicator_long_name": da.attrs.get("long_name", "unknown"), "indicator_description": da.attrs.get("description", "unknown"),
                 "indicator_units": da.attrs.get("units", "unknown"), "partition_fit": sm if isinstance(sm, str) else "unknown"}
        return wrap(da, g, u, general_components(var_first, mean_first), tuple(all_types), rest, attrs)

    return {"hawkins_sutton": forwarding_adapter("hawkins_sutton", originals["hawkins_sutton"], hs),
            "lafferty_sriver": forwarding_adapter("lafferty_sriver", originals["lafferty_sriver"], ls),
            "general_partition": forwarding_adapter("general_partition", originals["general_partition"], gp)}


class _BaseMirror:
    """``ensemble_mean_std_max_min`` of ``xclim.ensembles._base`` for ``patch.install``: the names ``<v>_mean`` / ``_stdev`` /
    ``_max`` / ``_min``, the variable's attributes with the reference's description suffix, and the history line."""
    ADAPTED = ("ensemble_mean_std_max_min",)

    @staticmethod
    def make_adapters(env, originals: dict, xr=None, update_history=None) -> dict:
        from .xr_adapter import forwarding_adapter

        DA = env.DataArray
        Dataset = getattr(xr, "Dataset", None)

        def stats(p):
            ens, min_members, weights = p["ens"], p["min_members"], p["weights"]
            if Dataset is None or not hasattr(ens, "data_vars"):
                raise NotServed("ensemble_mean_std_max_min: no Dataset")
            w = None
            if weights is not None:
                if not isinstance(weights, DA) or tuple(weights.dims) != ("realization",):
                    raise NotServed("ensemble_mean_std_max_min: weights along more than realization")
                w = np.asarray(weights.values, np.float64)
            out, size = {}, None
            for v, da in dict(ens.data_vars).items():
                if not isinstance(da, DA) or "realization" not in da.dims or getattr(da.data, "chunks", None) is not None:
                    raise NotServed("ensemble_mean_std_max_min: a variable that is chunked or has no realization dimension")
                rest = tuple(d for d in da.dims if d != "realization")
                size = da.shape[da.dims.index("realization")]
                res = ensemble_mean_std_max_min(np.asarray(da.transpose("realization", *rest).values), min_members, w)
                coords = {k: c for k, c in da.coords.items() if k in rest}
                for stat in ("mean", "stdev", "max", "min"):
                    vv = f"{v}_{stat}"
                    attrs = dict(da.attrs)
                    if "description" in attrs:
                        attrs["description"] = attrs["description"] + " : " + vv.split("_", maxsplit=1)[-1] + " of ensemble"
                    out[vv] = DA(res[stat], dims=rest, coords=coords, attrs=attrs)
            ds = Dataset(out, attrs=dict(getattr(ens, "attrs", {})))
            if update_history is not None and size is not None:
                ds.attrs["history"] = update_history(f"Computation of statistics on {size} ensemble members.", ds)
            return ds

        return {"ensemble_mean_std_max_min": forwarding_adapter("ensemble_mean_std_max_min", originals["ensemble_mean_std_max_min"], stats)}


base_mirror = _BaseMirror
