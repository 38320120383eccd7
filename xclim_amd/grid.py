"""Host mirror of what reduces ACROSS the grid: ``sea_ice_area`` and ``sea_ice_extent`` (reference:
src/xclim/indices/_threshold.py:3057-3131) and ``jetstream_metric_woollings`` (src/xclim/indices/_synoptic.py:23-116).  The kernels
are in xclim_amd/csrc/grid.hip, their C ABI and every order of summation in include/units/xclim_hip_grid.h.

The three functions carry the reference's names, parameters and defaults on arrays (thresholds as plain numbers in the units of the
data), plus ``device`` and ``keep``.  :func:`sea_ice` is the fused form: users ask for the area and the extent of the same field,
and there both are ONE launch of ``xh_grid_masked_dot``, which reads the field once.  Nothing here needs a time axis: a leading
dimension of the field that ``areacello`` lacks (time, member) is a row.

ASSUMPTIONS (xarray is neither needed nor used here).  All arithmetic is float64 on the widened fields, where the reference's
einsum and ``mean`` stay in float32 for float32 fields; a sea-ice sum is rounded once, to numpy's promotion of the operands.  The
zonal mean of the jet is not rounded to float32 before the filter.  The filter adds its 61 products in row order from the first,
where ``dot`` leaves the order to BLAS: that order is what makes the known answer of the reference's test (0.999276877412766)
exact.

:class:`NotServed` (the adapters forward these to the reference): integer or chunked fields, an ``areacello`` with a dimension
the field lacks or one on ``time``, 2-D (curvilinear) latitudes or longitudes, ``ua`` with dimensions beyond time and the three
axes, coordinates that cannot be identified, pressure units other than Pa / hPa / mbar.
"""

from __future__ import annotations

import types

import numpy as np

from . import kernels as K
from ._capi import GRID_MAX_WINDOW, DeviceArray, get_device
from .fields import SERVED, NotServed

__all__ = ["sea_ice_area", "sea_ice_extent", "sea_ice", "jetstream_metric_woollings", "lanczos_weights", "jet_box", "find_coordinate", "SEA_ICE_OUTPUTS",
           "SEA_ICE_FACTORS", "PRESSURE_UNITS", "JET_WINDOW", "JET_CUTOFF", "NotServed", "threshold", "synoptic", "ADAPTED", "make_adapters"]

# the results of sea_ice -> the outputs of xh_grid_masked_dot
SEA_ICE_OUTPUTS = {"area": "dot", "extent": "msum"}
# convert_units_to("100 %", siconc) for the units of a concentration
SEA_ICE_FACTORS = {"%": 100.0, "percent": 100.0, "": 1.0, "1": 1.0}
# hPa per unit of a pressure coordinate
PRESSURE_UNITS = {"Pa": 100.0, "pascal": 100.0, "hPa": 1.0, "mbar": 1.0, "millibar": 1.0}
JET_WINDOW, JET_CUTOFF = 61, 0.1   # _synoptic.py:82-84, following Woollings (2010)
_TOO_SHORT = "Time series is too short to apply 61-day Lanczos filter (got a length of  {})"
_NO_LON = "Make sure the grid includes longitude values in a range between -60 and 0°E."
_NO_LAT = "Make sure the grid includes latitude values in a range between 15 and 75°N."
_NO_PLEV = "Make sure the grid includes pressure values in a range between 750 and 950 hPa."


# ---- sea_ice_area, sea_ice_extent --------------------------------------------------------------------------------------------
def _float_field(a, name):
    if isinstance(a, DeviceArray):
        if np.dtype(a.dtype) not in SERVED:
            raise NotServed(f"{name}: device arrays must be float32 or float64")
        return a
    a = np.asarray(a)
    if a.dtype not in SERVED:
        raise NotServed(f"{name}: integer fields (dtype {a.dtype.name}) are not served")
    return a


def _sea_ice(siconc, areacello, thresh, factor, outputs, device, keep):
    who = "sea_ice"
    outputs = tuple(outputs)
    if not outputs or set(outputs) - set(SEA_ICE_OUTPUTS):
        raise ValueError(f"{who}: outputs must be a non-empty subset of {', '.join(SEA_ICE_OUTPUTS)}")
    outputs = tuple(o for o in SEA_ICE_OUTPUTS if o in outputs)
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.integer, np.floating)):
        raise NotServed("a threshold that is not a number")
    x = _float_field(siconc, "siconc")
    w = areacello if isinstance(areacello, DeviceArray) else np.asarray(areacello)
    wdtype = np.dtype(w.dtype)
    if wdtype.kind not in "fiub":
        raise TypeError(f"{who}: areacello must be numeric, got {wdtype.name}")
    cells = tuple(int(s) for s in w.shape)
    shape = tuple(int(s) for s in x.shape)
    if len(cells) > len(shape) or shape[len(shape) - len(cells):] != cells:
        raise ValueError(f"{who}: areacello {cells} is not on the trailing dimensions of siconc {shape}")
    rows = shape[:len(shape) - len(cells)]
    T, C_ = int(np.prod(rows, dtype=np.int64)), int(np.prod(cells, dtype=np.int64))
    if np.dtype(x.dtype) == np.float32:
        thresh = np.float32(thresh)   # numpy >= 2: a Python scalar next to a float32 field is a float32 (the rule of humidity.py)
    dtypes = {"area": np.result_type(x.dtype, wdtype), "extent": np.result_type(np.bool_, wdtype)}
    dev = device or get_device()
    if T == 0 or C_ == 0:   # no row, or rows without a cell (a sum of nothing): no launch
        if keep:
            return {o: dev.zeros((T,), np.float64) for o in outputs}
        return {o: np.zeros(rows, dtypes[o]) for o in outputs}
    xd = x.reshape(T, C_) if isinstance(x, DeviceArray) else dev.to_device(np.ascontiguousarray(x).reshape(T, C_))
    if isinstance(w, DeviceArray):
        if wdtype != np.float64:
            raise TypeError(f"{who}: device weights must be float64")
        wd = w.reshape(C_)
    else:
        wd = dev.to_device(np.ascontiguousarray(w, dtype=np.float64).reshape(C_))
    outs = K.grid_masked_dot(dev, xd, wd, float(thresh), [SEA_ICE_OUTPUTS[o] for o in outputs])
    outs = {o: outs[SEA_ICE_OUTPUTS[o]] for o in outputs}
    if keep:
        return outs
    res = {}
    for o in outputs:
        s = outs[o].get().reshape(rows)
        res[o] = (s / factor if o == "area" else s).astype(dtypes[o])
    return res


def _factor(units):
    try:
        return SEA_ICE_FACTORS[str(units).strip()]
    except KeyError:
        raise ValueError(f"units must be one of {list(SEA_ICE_FACTORS)}, got {units!r}") from None


def sea_ice(siconc, areacello, thresh: float = 15.0, outputs=tuple(SEA_ICE_OUTPUTS), *, units: str = "%", device=None,
            keep: bool = False) -> dict:
    """Any subset of ``{"area", "extent"}`` from ONE launch of ``xh_grid_masked_dot``, which reads ``siconc`` once.  ``siconc``
    ``(*rows, *cells)`` float32 or float64, ``areacello`` ``(*cells)``: every leading dimension ``areacello`` lacks is a row.
    ``thresh`` is a number in the ``units`` of the field ("%", or "" / "1" for a fraction), rounded to float32 first next to a
    float32 field.  Results ``(*rows)`` in numpy's promotion of the operands (the extent: the dtype of ``areacello``); the float64
    sum is divided by the factor of ``units`` (the area) and rounded once.  A NaN concentration adds ``0 * areacello``; a NaN or
    infinite cell area makes every row NaN, as ``xarray.dot`` does.  ``keep=True``: the float64 ``(rows)`` device sums as the
    kernel leaves them, the area BEFORE the division by the factor."""
    return _sea_ice(siconc, areacello, thresh, _factor(units), outputs, device, keep)


def sea_ice_area(siconc, areacello, thresh: float = 15.0, *, units: str = "%", device=None, keep: bool = False):
    """_threshold.py:3057-3093: the sum of ``siconc * areacello / factor`` over the cells with ``siconc >= thresh``
    (``xarray.dot(siconc.where(siconc >= t, 0), areacello) / factor``).  See :func:`sea_ice`."""
    return _sea_ice(siconc, areacello, thresh, _factor(units), ("area",), device, keep)["area"]


def sea_ice_extent(siconc, areacello, thresh: float = 15.0, *, units: str = "%", device=None, keep: bool = False):
    """_threshold.py:3096-3131: the sum of ``areacello`` over the cells with ``siconc >= thresh`` (``xarray.dot(siconc >= t,
    areacello)``).  See :func:`sea_ice`."""
    return _sea_ice(siconc, areacello, thresh, _factor(units), ("extent",), device, keep)["extent"]


# ---- jetstream_metric_woollings ----------------------------------------------------------------------------------------------
def lanczos_weights(window_size: int = JET_WINDOW, cutoff: float = JET_CUTOFF) -> np.ndarray:
    """``_compute_low_pass_filter_weights`` (_synoptic.py:103-116), restated: the ``window_size`` weights of the low-pass Lanczos
    filter, float64, bit for bit the reference's."""
    order = ((window_size - 1) // 2) + 1
    nwts = 2 * order + 1
    w = np.zeros([nwts])
    n = nwts // 2
    w[n] = 2 * cutoff
    k = np.arange(1.0, n)
    sigma = np.sin(np.pi * k / n) * n / (np.pi * k)
    firstfactor = np.sin(2.0 * np.pi * cutoff * k) / (np.pi * k)
    w[n - 1:0:-1] = firstfactor * sigma
    w[n + 1:-1] = firstfactor * sigma
    return w[0 + (window_size % 2):-1]


def _coordinate(a, name):
    a = np.asarray(a)
    if a.ndim != 1:
        raise NotServed(f"{name}: a {a.ndim}-D coordinate (a curvilinear grid) is not served")
    return a


def jet_box(lat, lon, plev, pmin: float, pmax: float):
    """The three coordinate masks of _synoptic.py:53-71 as index lists ``(iz, iy, ix)``: longitudes in [300, 360] or [-60, 0],
    latitudes in [15, 75], levels in ``[pmin, pmax]`` (750 and 950 hPa in the units of the coordinate).  The reference's three
    ``ValueError``s, in its order."""
    lon, lat, plev = _coordinate(lon, "lon"), _coordinate(lat, "lat"), _coordinate(plev, "plev")
    ilon = ((lon >= 300) & (lon <= 360)) | ((lon >= -60) & (lon <= 0))
    if not ilon.any():
        raise ValueError(_NO_LON)
    ilat = (lat >= 15) & (lat <= 75)
    if not ilat.any():
        raise ValueError(_NO_LAT)
    ip = (plev >= pmin) & (plev <= pmax)
    if not ip.any():
        raise ValueError(_NO_PLEV)
    return np.flatnonzero(ip), np.flatnonzero(ilat), np.flatnonzero(ilon)


def _jet(ua, lat, lon, plev, pmin, pmax, order, device, keep):
    who = "jetstream_metric_woollings"
    order = str(order).lower()
    if sorted(order) != ["x", "y", "z"]:
        raise ValueError(f"{who}: order must be a permutation of 'zyx', got {order!r}")
    u = _float_field(ua, "ua")
    if len(u.shape) != 4:
        raise NotServed(f"{who}: ua must be (time, three axes), got {len(u.shape)} dimensions")
    iz, iy, ix = jet_box(lat, lon, plev, pmin, pmax)
    T = int(u.shape[0])
    ext = dict(zip(order, (int(s) for s in u.shape[1:])))
    for k, c in (("z", plev), ("y", lat), ("x", lon)):
        if ext[k] != np.asarray(c).shape[0]:
            raise ValueError(f"{who}: axis {k} of ua has {ext[k]} entries, its coordinate {np.asarray(c).shape[0]}")
    if T <= JET_WINDOW:   # (T <= filter_freq = 10 is implied)
        raise ValueError(_TOO_SHORT.format(T))
    stride = dict(zip(order, (ext[order[1]] * ext[order[2]], ext[order[2]], 1)))
    ld = ext["z"] * ext["y"] * ext["x"]
    dev = device or get_device()
    ud = u if isinstance(u, DeviceArray) else dev.to_device(np.ascontiguousarray(u))
    zm = K.grid_box_mean(dev, ud, T, ld, (ext["z"], ext["y"], ext["x"]), (stride["z"], stride["y"], stride["x"]), iz, iy, ix)
    out = K.grid_filter_argmax(dev, zm, lanczos_weights(), ("smax", "jmax"))
    if keep:
        return out
    jmax, smax = out["jmax"].get(), out["smax"].get()
    lats = np.asarray(lat)[iy].astype(np.float64)
    jetlat = np.where(jmax >= 0, lats[np.maximum(jmax, 0)], np.nan)
    return jetlat, smax


def jetstream_metric_woollings(ua, lat, lon, plev, *, plev_units: str = "Pa", order: str = "zyx", device=None, keep: bool = False):
    """_synoptic.py:23-116: ``(jetlat, jetstr)``, float64 ``(T)`` — the latitude and the strength of the maximum of the zonal
    wind between 750 and 950 hPa, averaged over the longitudes -60 .. 0 °E and the selected levels (NaN samples skipped), low-pass
    filtered with the 61 Lanczos weights (cutoff 0.1) in a centred window, over the latitudes 15 .. 75 °N.  The first and the last
    30 rows, and every row whose window holds a NaN mean, are NaN at that latitude; ``jetlat`` is the FIRST latitude, in the order
    of ``lat``, that holds the maximum.
    ``ua`` ``(T, *three axes)`` float32 or float64, read in place; ``order``: which of the levels (z), latitudes (y) and
    longitudes (x) each of the three axes is — "zyx", or "zxy" for the layout of the reference's own test.  ``lat``, ``lon``,
    ``plev``: the 1-D coordinates; ``plev_units``: "Pa", "hPa" or "mbar".  The reference's ``ValueError``s are raised: no longitude,
    latitude or level in the box, and ``T <= 61``.  One launch of ``xh_grid_box_mean`` and one of ``xh_grid_filter_argmax``.
    ``keep=True``: ``{"smax": (T) float64, "jmax": (T) int32}`` on the device, ``jmax`` an index into the selected latitudes."""
    try:
        per_hpa = PRESSURE_UNITS[str(plev_units).strip()]
    except KeyError:
        raise NotServed(f"plev_units {plev_units!r}") from None
    return _jet(ua, lat, lon, plev, 750.0 * per_hpa, 950.0 * per_hpa, order, device, keep)


# ---- the xarray adapters (patch.install) -------------------------------------------------------------------------------------
# The replaced functions are defined in two modules of the reference and patch.install_mirror wants one defining module per mirror:
# two namespaces, each with its own ADAPTED and make_adapters.
def _in_memory(DA, da, name):
    from .xr_adapter import is_chunked

    if not isinstance(da, DA) or is_chunked(da):
        raise NotServed(f"{name}: not an in-memory DataArray")
    return da


def _row_result(DA, a, rows, values, name, attrs):
    coords = {d: a.coords[d] for d in rows if d in a.coords}
    return DA(np.asarray(values), coords=coords, dims=tuple(rows), name=name, attrs=attrs)


def _threshold_adapters(env, originals: dict, device=None) -> dict:
    """``sea_ice_area`` and ``sea_ice_extent`` of ``xclim.indices._threshold``: one launch of ``xh_grid_masked_dot`` each.  The
    threshold passes ``convert_units_to(thresh, siconc)``, the factor ``convert_units_to("100 %", siconc)``; the result is on the
    dimensions ``areacello`` lacks, with ``units = areacello.units`` and no other attribute (``xarray.dot`` keeps none)."""
    from .xr_adapter import forwarding_adapter

    DA = env.DataArray

    def runner(output):
        def run(p):
            sic, area = _in_memory(DA, p["siconc"], "siconc"), _in_memory(DA, p["areacello"], "areacello")
            cells = tuple(area.dims)
            if set(cells) - set(sic.dims):
                raise NotServed("areacello has a dimension the field lacks")
            if "time" in cells:
                raise NotServed("areacello varies along a row dimension")
            if np.dtype(sic.dtype) not in SERVED:
                raise NotServed("integer fields")
            t = env.convert_units_to(p["thresh"], sic)
            factor = float(env.convert_units_to("100 %", sic))
            rows = tuple(d for d in sic.dims if d not in cells)
            field_cells = tuple(d for d in sic.dims if d in cells)
            if tuple(sic.dims) != rows + field_cells:   # cells in front of a row dimension: the field itself is re-ordered
                sic = sic.transpose(*rows, *field_cells)
            w = area.transpose(*field_cells).values    # the weights are small: they follow the field's order
            out = _sea_ice(np.asarray(sic.values), w, t, factor, (output,), device, False)[output]
            return _row_result(DA, sic, rows, out, None, {"units": area.attrs["units"]})
        return run

    return {"sea_ice_area": forwarding_adapter("sea_ice_area", originals["sea_ice_area"], runner("area")),
            "sea_ice_extent": forwarding_adapter("sea_ice_extent", originals["sea_ice_extent"], runner("extent"))}


_CF_AXES = {"latitude": ("latitude", "Y", ("lat", "latitude", "rlat", "y", "Y")),
            "longitude": ("longitude", "X", ("lon", "longitude", "rlon", "x", "X")),
            "vertical": (("air_pressure", "atmosphere_sigma_coordinate", "altitude", "height"), "Z",
                         ("plev", "lev", "level", "pressure", "vertical", "z", "Z"))}


def find_coordinate(da, key):
    """The name of the latitude, longitude or vertical coordinate of a DataArray: by ``standard_name``, then by ``axis``, then by
    the usual names (no ``cf`` accessor is needed); :class:`NotServed` without exactly one."""
    standard, axis, usual = _CF_AXES[key]
    standard = (standard,) if isinstance(standard, str) else standard
    names = list(da.coords)
    for pick in (lambda c: c.attrs.get("standard_name") in standard, lambda c: c.attrs.get("axis") == axis):
        found = [n for n in names if pick(da.coords[n])]
        if len(found) == 1:
            return found[0]
        if found:
            raise NotServed(f"several {key} coordinates: {found}")
    found = [n for n in usual if n in names]
    if not found:
        raise NotServed(f"no {key} coordinate")
    return found[0]


def _synoptic_adapters(env, originals: dict, device=None) -> dict:
    """``jetstream_metric_woollings`` of ``xclim.indices._synoptic``: the coordinates are found by :func:`find_coordinate`, the
    bounds of the levels pass ``convert_units_to("750 hPa", vertical)``; ``jetlat`` and ``jetstr`` are on ``time`` with the
    reference's names and units (the units of the latitude and of ``ua``)."""
    from .xr_adapter import forwarding_adapter

    DA = env.DataArray

    def run(p):
        ua = _in_memory(DA, p["ua"], "ua")
        if np.dtype(ua.dtype) not in SERVED:
            raise NotServed("integer fields")
        names = {k: find_coordinate(ua, k) for k in ("vertical", "latitude", "longitude")}
        coords = {k: ua.coords[n] for k, n in names.items()}
        if any(tuple(c.dims) != (names[k],) for k, c in coords.items()):
            raise NotServed("2-D (curvilinear) coordinates")
        if "time" not in ua.dims or set(ua.dims) != {"time", *names.values()} or len(ua.dims) != 4:
            raise NotServed("ua with dimensions beyond time and the three axes")
        a = ua.transpose("time", ...)
        letter = {names["vertical"]: "z", names["latitude"]: "y", names["longitude"]: "x"}
        order = "".join(letter[d] for d in a.dims[1:])
        pmin = float(env.convert_units_to("750 hPa", coords["vertical"]))
        pmax = float(env.convert_units_to("950 hPa", coords["vertical"]))
        jetlat, jetstr = _jet(np.asarray(a.values), coords["latitude"].values, coords["longitude"].values, coords["vertical"].values, pmin,
                              pmax, order, device, False)
        tc = {"time": a.coords["time"]}
        return (DA(jetlat, coords=tc, dims=("time",), name="jetlat", attrs={"units": coords["latitude"].attrs["units"]}),
                DA(jetstr, coords=tc, dims=("time",), name="jetstr", attrs={"units": ua.attrs["units"]}))

    return {"jetstream_metric_woollings": forwarding_adapter("jetstream_metric_woollings", originals["jetstream_metric_woollings"], run)}


threshold = types.SimpleNamespace(ADAPTED=("sea_ice_area", "sea_ice_extent"), make_adapters=_threshold_adapters)
synoptic = types.SimpleNamespace(ADAPTED=("jetstream_metric_woollings",), make_adapters=_synoptic_adapters)
ADAPTED = threshold.ADAPTED + synoptic.ADAPTED


def make_adapters(env, originals: dict, device=None) -> dict:
    """Same-signature replacements of the three functions (``ADAPTED``) on DataArrays: the adapters of both namespaces.  Whatever
    :class:`NotServed` refuses goes to the saved originals; no other exception is caught."""
    return {**_threshold_adapters(env, originals, device), **_synoptic_adapters(env, originals, device)}


assert JET_WINDOW <= GRID_MAX_WINDOW
