"""Host mirror of the spatial-analogue dissimilarity metrics (reference: ``spatial_analogs`` and the ``metrics`` registry of
src/xclim/analog.py:21-628).  The kernels are in xclim_amd/csrc/analog.hip, their C ABI in include/ext/xclim_hip_analog.h.

:func:`spatial_analogs` works on arrays: one target sample ``(n, d)`` against the candidate sample of every cell of ``d`` fields
``(m, *cells)``, ONE launch of ``xh_analog`` with a lane per cell, where the reference calls a Python function per cell through
``xr.apply_ufunc(..., vectorize=True)``.  The eight metric functions carry the reference's names, parameters and defaults and
work on a single pair ``(x, y)`` with the reference's 1-D handling, through the same kernel with one cell.

ASSUMPTIONS (xarray is neither needed nor used here).  All arithmetic is float64 on the widened values: the reference takes
``std`` of a float32 field in float32 before ``astype(double)``, which this unit does not reproduce.  Sums run in row order
where numpy sums pairwise; the results agree within a few rounding errors of the terms added.  ``nearest_neighbor`` on a cell
whose standardized values are not finite (a cell constant in one index) is NaN for that cell, where the reference's KD-tree
raises ``ValueError`` for the whole call.  ``nearest_neighbor``, ``friedman_rafsky`` and ``kldiv`` take the first of two exactly
equal distances in pooled order; the reference's trees take whichever their traversal meets first.

:class:`NotServed` (the adapter forwards these to the reference): integer fields, chunked fields, fields of mixed dtype, more
than ``ANALOG_MAX_SAMPLE`` points in a sample, more than ``ANALOG_MAX_D`` indices (``ANALOG_KS_MAX_D`` for
``kolmogorov_smirnov``), ``k`` above ``ANALOG_MAX_K`` or more than ``ANALOG_MAX_NK`` of them, ``mahalanobis`` with a ``VI`` that is
not ``(d, d)``.
"""

from __future__ import annotations

import numpy as np

from . import kernels as K
from ._capi import (ANALOG_KS_MAX_D, ANALOG_MAX_D, ANALOG_MAX_K, ANALOG_MAX_NK, ANALOG_MAX_SAMPLE, ANALOG_METHODS, DeviceArray,
                    get_device)
from .fields import SERVED, NotServed

__all__ = ["spatial_analogs", "dissimilarity", "metrics", "seuclidean", "nearest_neighbor", "zech_aslan", "szekely_rizzo",
           "friedman_rafsky", "kolmogorov_smirnov", "kldiv", "mahalanobis", "NotServed", "ADAPTED", "make_adapters"]

# the keyword arguments of every metric with the reference's defaults (analog.py:182, :217, :255, :323, :389, :434, :499, :591)
_KEYWORDS = {"seuclidean": {}, "nearest_neighbor": {}, "zech_aslan": {"dmin": 1e-12}, "szekely_rizzo": {"standardize": True},
             "friedman_rafsky": {}, "kolmogorov_smirnov": {}, "kldiv": {"k": 1}, "mahalanobis": {"VI": None}}


def _unknown(method):
    return ValueError(f"Method `{method}` is not implemented. Available methods are: {','.join(ANALOG_METHODS)}.")


def _keywords(method, kwargs):
    extra = set(kwargs) - set(_KEYWORDS[method])
    if extra:
        raise TypeError(f"{method}() got an unexpected keyword argument {sorted(extra)[0]!r}")
    return {**_KEYWORDS[method], **kwargs}


def _target(target):
    """The target as float64 (n, d): a 2-D array, a 1-D series (one index) or a sequence of d series."""
    if isinstance(target, (list, tuple)):
        target = np.stack([np.asarray(t, np.float64).reshape(-1) for t in target], axis=1)
    x = np.asarray(target, np.float64)
    x = x[:, None] if x.ndim == 1 else x
    if x.ndim != 2:
        raise ValueError(f"target must be (n, d), got shape {x.shape}")
    return np.ascontiguousarray(x)


def _candidates(candidates, d):
    """The d candidate fields as they came, each ``(m, *cells)``, and their common shape and dtype."""
    if isinstance(candidates, DeviceArray):
        raise TypeError("candidates: a sequence of d fields; a device array is ONE field")
    fields = list(candidates)
    if len(fields) != d:
        raise AttributeError("Shape mismatch")
    out = []
    for f in fields:
        if getattr(f, "chunks", None) is not None or hasattr(f, "dask"):
            raise NotServed("chunked candidate fields")
        f = f if isinstance(f, DeviceArray) else np.asarray(f)
        if np.dtype(f.dtype).kind in "iub":
            raise NotServed("integer fields are not served")
        if np.dtype(f.dtype) not in SERVED:
            raise NotServed(f"fields of dtype {np.dtype(f.dtype).name}")
        out.append(f)
    if len({np.dtype(f.dtype) for f in out}) > 1:
        raise NotServed("fields of mixed dtype")
    shapes = {tuple(f.shape) for f in out}
    if len(shapes) > 1 or len(out[0].shape) < 1:
        raise ValueError(f"candidates: every field must have one (m, *cells) shape, got {sorted(shapes)}")
    return out


def _parameters(method, kw, x):
    """(par, k, is k a list) of the kernel for the keyword arguments of a metric."""
    d = x.shape[1]
    if method == "zech_aslan":
        return [float(kw["dmin"])], None, False
    if method == "szekely_rizzo":
        return [1.0 if kw["standardize"] else 0.0], None, False
    if method == "mahalanobis":
        VI = kw["VI"]
        if not isinstance(VI, np.ndarray):
            if VI is not None:
                raise AttributeError("VI not a matrix")
            with np.errstate(all="ignore"):
                v = np.atleast_2d(np.cov(x, rowvar=False))
                try:
                    VI = np.linalg.inv(v)
                except np.linalg.LinAlgError:
                    VI = np.linalg.pinv(v)
        if VI.shape != (d, d):
            raise NotServed(f"mahalanobis: VI must be ({d}, {d}), got {VI.shape}")
        return np.asarray(VI, np.float64), None, False
    if method == "kldiv":
        k = kw["k"]
        many = np.iterable(k)
        ka = np.atleast_1d(k)
        if d > 10:
            raise ValueError(f"Too many dimensions: {d}.")
        if ka.dtype.kind not in "iu" or ka.ndim != 1 or ka.size < 1 or ka.min() < 1:
            raise NotServed("kldiv: k must be a positive integer or a list of them")
        if ka.max() > ANALOG_MAX_K or ka.size > ANALOG_MAX_NK:
            raise NotServed(f"kldiv: k of up to {ANALOG_MAX_K} and at most {ANALOG_MAX_NK} of them are served")
        return None, ka.astype(np.int32), many
    return None, None, False


def dissimilarity(method: str, target, candidates, *, device=None, keep: bool = False, **kwargs):
    """The metric ``method`` between ``target`` and the candidate sample of every cell; see :func:`spatial_analogs`."""
    if method not in ANALOG_METHODS:
        raise _unknown(method)
    kw = _keywords(method, kwargs)
    x = _target(target)
    n, d = x.shape
    if not isinstance(candidates, (list, tuple)) and not isinstance(candidates, DeviceArray):
        c = candidates
        if getattr(c, "chunks", None) is not None or hasattr(c, "dask"):
            raise NotServed("chunked candidate fields")
        c = np.asarray(c)
        candidates = [c] if c.ndim == 1 and d == 1 else list(c)
    fields = _candidates(candidates, d)
    m, cell_shape = int(fields[0].shape[0]), tuple(fields[0].shape[1:])
    C_ = int(np.prod(cell_shape, dtype=np.int64))
    par, k, many = _parameters(method, kw, x)
    if n < 1 or m < 1:
        raise ValueError("the samples must hold at least one point")
    if n > ANALOG_MAX_SAMPLE or m > ANALOG_MAX_SAMPLE:
        raise NotServed(f"samples of up to {ANALOG_MAX_SAMPLE} points are served, got {n} and {m}")
    if d > (ANALOG_KS_MAX_D if method == "kolmogorov_smirnov" else ANALOG_MAX_D):
        raise NotServed(f"{method}: {d} indices")
    rows = len(k) if k is not None else 1
    dev = device or get_device()
    if C_ == 0:
        out = dev.empty((rows, 0), np.float64) if keep else np.empty((rows, 0))
    else:
        on_dev = [f.reshape(m, C_) if isinstance(f, DeviceArray) else dev.to_device(np.ascontiguousarray(f).reshape(m, C_)) for f in fields]
        out = K.analog(dev, method, x, on_dev, par=par, k=k)
    if keep:
        return out
    res = np.asarray(out if C_ == 0 else out.get())
    if many:
        return np.moveaxis(res.reshape((rows,) + cell_shape), 0, -1)
    return res[0].reshape(cell_shape)


def spatial_analogs(target, candidates, dist_dim=0, method: str = "kldiv", *, device=None, keep: bool = False, **kwargs):
    """analog.py:21-105 on arrays.  ``target``: ``(n, d)``, or a sequence of ``d`` series; ``candidates``: a sequence of ``d``
    fields ``(m, *cells)`` or an array ``(d, m, *cells)``, float32 or float64 (numpy arrays, or ``(m, C)`` device arrays), with the
    sample axis ``dist_dim`` of every field (default: axis 0).  Returns the dissimilarity of every cell, float64 ``(*cells)`` —
    ``(*cells, nk)`` for ``kldiv`` with a list of ``k`` — or the ``(1 | nk, C)`` device array with ``keep``.  ``kwargs`` go to
    the metric."""
    if method not in ANALOG_METHODS:
        raise _unknown(method)
    if isinstance(dist_dim, bool) or not isinstance(dist_dim, (int, np.integer)):
        raise TypeError("dist_dim: on arrays, the sample axis of the candidate fields as an integer")
    if dist_dim != 0:
        if isinstance(candidates, DeviceArray) or any(isinstance(f, DeviceArray) for f in candidates):
            raise ValueError("dist_dim: device arrays are (m, C), the sample axis first")
        candidates = [np.moveaxis(np.asarray(f), int(dist_dim), 0) for f in candidates]
    return dissimilarity(method, target, candidates, device=device, keep=keep, **kwargs)


def _single(method):
    def fn(x, y, *, device=None, **kwargs):
        kw = _keywords(method, kwargs)
        many = method == "kldiv" and np.iterable(kw["k"])
        x, y = np.asarray(x), np.asarray(y)
        if np.any(np.isnan(x)) or np.any(np.isnan(y)):
            return np.nan
        x, y = np.atleast_2d(x), np.atleast_2d(y)
        x = x.T if x.shape[0] == 1 else x
        y = y.T if y.shape[0] == 1 else y
        if x.shape[1] != y.shape[1]:
            raise AttributeError("Shape mismatch")
        y = y if y.dtype in SERVED else y.astype(np.float64)
        out = dissimilarity(method, x, [y[:, j] for j in range(y.shape[1])], device=device, **kwargs)
        return [np.float64(v) for v in out] if many else np.float64(out)

    fn.__name__ = fn.__qualname__ = method
    fn.__doc__ = (f"``{method}(x, y)`` of analog.py on one pair, ``x`` (n, d) and ``y`` (m, d) (1-D samples are columns), through "
                  "``xh_analog`` with one cell; the reference's keyword arguments and defaults.")
    return fn


seuclidean, nearest_neighbor, zech_aslan, szekely_rizzo = (_single(m) for m in ("seuclidean", "nearest_neighbor", "zech_aslan", "szekely_rizzo"))
friedman_rafsky, kolmogorov_smirnov, kldiv, mahalanobis = (_single(m) for m in ("friedman_rafsky", "kolmogorov_smirnov", "kldiv", "mahalanobis"))
# the reference's registry, in its order
metrics = {m: globals()[m] for m in ANALOG_METHODS}


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------
ADAPTED = ("spatial_analogs",)


def make_adapters(env, originals: dict, device=None) -> dict:
    """``spatial_analogs`` of ``xclim.analog`` on Datasets: the variables of ``data_vars`` in order are the indices (analog.py:60-72),
    target and candidates share ``dist_dim`` only, and the result is the DataArray the reference returns: the candidates' other
    dimensions and coordinates, the name "dissimilarity" and the three attributes of :99-103.  Chunked inputs and everything
    :class:`NotServed` go to the original."""
    from .xr_adapter import forwarding_adapter

    DA = env.DataArray

    def run(p):
        method, dist_dim, kwargs = p["method"], p["dist_dim"], dict(p.get("kwargs") or {})
        target, candidates = p["target"], p["candidates"]
        if not isinstance(dist_dim, str):
            raise NotServed("dist_dim: a sequence of dimensions")
        try:
            tvars, cvars = dict(target.data_vars), dict(candidates.data_vars)
        except AttributeError:
            raise NotServed("target and candidates must be Datasets") from None
        names = [str(n) for n in tvars]
        if not names or names != [str(n) for n in cvars]:
            raise NotServed("target and candidates must hold the same variables in the same order")
        if method not in ANALOG_METHODS:
            raise _unknown(method)
        if method == "kldiv" and np.iterable(kwargs.get("k", 1)):
            raise NotServed("kldiv with a list of k has no scalar result per cell")
        first = next(iter(cvars.values()))
        for v in list(tvars.values()) + list(cvars.values()):
            if not isinstance(v, DA):
                raise NotServed("a variable that is not a DataArray")
            if getattr(v.data, "chunks", None) is not None:
                raise NotServed("chunked fields")
        if any(tuple(v.dims) != (dist_dim,) for v in tvars.values()):
            raise NotServed("a target with more dimensions than dist_dim")
        if any(dist_dim not in v.dims or tuple(v.dims) != tuple(first.dims) for v in cvars.values()):
            raise NotServed("candidates on different dimensions")
        cell_dims = tuple(dm for dm in first.dims if dm != dist_dim)   # (the target's only dimension is dist_dim: nothing else is shared)
        x = np.stack([np.asarray(v.values, np.float64) for v in tvars.values()], axis=1)
        fields = [np.asarray(v.transpose(dist_dim, *cell_dims).values) for v in cvars.values()]
        out = dissimilarity(method, x, fields, device=device, **kwargs)
        coords = {k: c for k, c in first.coords.items() if k in cell_dims}
        attrs = {"long_name": f"Dissimilarity between target and candidates, using metric {method}.", "indices": ",".join(names),
                 "metric": method}
        return DA(out, dims=cell_dims, coords=coords, name="dissimilarity", attrs=attrs)

    return {"spatial_analogs": forwarding_adapter("spatial_analogs", originals["spatial_analogs"], run)}
