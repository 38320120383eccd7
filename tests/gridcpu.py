"""numpy restatement of the three bodies of the grid-reduction unit, written from reading them — ``sea_ice_area`` and
``sea_ice_extent`` (reference: src/xclim/indices/_threshold.py:3057-3131) and ``jetstream_metric_woollings``
(src/xclim/indices/_synoptic.py:23-116) — the oracle of tests/test_grid_cpu.py and tests/test_gpu_grid.py (test infrastructure
only; the reference's own code needs xarray and cf_xarray, which the tests do not).

It follows the reference step by step, whole arrays at a time, in float64 on the widened fields: ``where(siconc >= t, siconc, 0)``
times the areas, summed over the cells (``xarray.dot``: every product is taken, so a NaN area or an infinite one next to a masked
cell makes the sum NaN); the three coordinate masks; the mean over levels and longitudes that skips NaN; the 61 Lanczos weights;
the centred window (``rolling(center=True).construct``: NaN outside the series) times the weights, ADDED IN ROW ORDER FROM THE FIRST
TERM (the order the device states; ``dot`` leaves it to BLAS); ``idxmax`` / ``max`` over the latitudes, which skip NaN.

``*_terms`` give, next to a sum, the sum of the absolute values of its terms: the scale of the 1e-12 bounds of the GPU tests."""
import numpy as np

NO_LON = "Make sure the grid includes longitude values in a range between -60 and 0°E."
NO_LAT = "Make sure the grid includes latitude values in a range between 15 and 75°N."
NO_PLEV = "Make sure the grid includes pressure values in a range between 750 and 950 hPa."


def _threshold(siconc, thresh):
    # numpy >= 2: the Python scalar of `siconc >= t` is a float32 next to a float32 field
    return np.float64(np.float32(thresh)) if np.asarray(siconc).dtype == np.float32 else np.float64(thresh)


def masked_dot_terms(siconc, areacello, thresh):
    """``(dot, msum, |dot| terms, |msum| terms)`` over the trailing (cell) dimensions of ``areacello``, float64."""
    x, w = np.asarray(siconc).astype(np.float64), np.asarray(areacello).astype(np.float64)
    axes = tuple(range(x.ndim - w.ndim, x.ndim))
    t = _threshold(siconc, thresh)
    with np.errstate(invalid="ignore"):
        inside = x >= t
        a, m = np.where(inside, x, 0.0) * w, np.where(inside, 1.0, 0.0) * w
    return a.sum(axes), m.sum(axes), np.abs(a).sum(axes), np.abs(m).sum(axes)


def sea_ice_area(siconc, areacello, thresh=15.0, factor=100.0):
    """_threshold.py:3089-3091: ``xarray.dot(siconc.where(siconc >= t, 0), areacello) / factor``."""
    return masked_dot_terms(siconc, areacello, thresh)[0] / factor


def sea_ice_extent(siconc, areacello, thresh=15.0):
    """_threshold.py:3128-3129: ``xarray.dot(siconc >= t, areacello)``."""
    return masked_dot_terms(siconc, areacello, thresh)[1]


def lanczos_weights(window_size=61, cutoff=0.1):
    """_synoptic.py:103-116."""
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


def jet_masks(lat, lon, plev, pmin, pmax):
    """_synoptic.py:53-71, with its three errors in its order."""
    lon, lat, plev = np.asarray(lon), np.asarray(lat), np.asarray(plev)
    ilon = ((lon >= 300) & (lon <= 360)) | ((lon >= -60) & (lon <= 0))
    if not ilon.any():
        raise ValueError(NO_LON)
    ilat = (lat >= 15) & (lat <= 75)
    if not ilat.any():
        raise ValueError(NO_LAT)
    ip = (plev >= pmin) & (plev <= pmax)
    if not ip.any():
        raise ValueError(NO_PLEV)
    return ip, ilat, ilon


def box_mean_terms(u_tzyx, iz, iy, ix):
    """``(mean, sum of |samples| / their number)`` over the selected levels and longitudes of ``u`` (T, Z, Y, X), NaN skipped, NaN
    without a sample; float64 (T, ny)."""
    u = np.asarray(u_tzyx).astype(np.float64)[:, np.asarray(iz, int)][:, :, np.asarray(iy, int)][:, :, :, np.asarray(ix, int)]
    ok = ~np.isnan(u)
    n = ok.sum((1, 3)).astype(np.float64)
    s, sa = np.where(ok, u, 0.0).sum((1, 3)), np.where(ok, np.abs(u), 0.0).sum((1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, np.nan), np.where(n > 0, sa / n, np.nan)


def box_mean(u_tzyx, iz, iy, ix):
    return box_mean_terms(u_tzyx, iz, iy, ix)[0]


def filter_terms(zm, wts):
    """``(f, sum of |terms|)``: f[t] = zm[t - W // 2] * wts[0] + zm[t - W // 2 + 1] * wts[1] + ..., in that order; NaN where the
    window leaves the rows."""
    zm, wts = np.asarray(zm, np.float64), np.asarray(wts, np.float64)
    T, W = zm.shape[0], len(wts)
    f, fa = np.full(zm.shape, np.nan), np.full(zm.shape, np.nan)
    lo, hi = W // 2, T - W + W // 2   # the rows t with 0 <= t - W // 2 and t - W // 2 + W <= T
    if hi >= lo:
        rows = np.arange(lo, hi + 1) - W // 2
        s = zm[rows] * wts[0]
        a = np.abs(s)
        for k in range(1, W):
            term = zm[rows + k] * wts[k]
            s, a = s + term, a + np.abs(term)
        f[lo:hi + 1], fa[lo:hi + 1] = s, a
    return f, fa


def first_max(f):
    """``(smax, jmax)`` of every row: the largest value that is not NaN and the first index that holds it; NaN / -1 without one."""
    f = np.asarray(f, np.float64)
    smax, jmax = np.full(f.shape[0], np.nan), np.full(f.shape[0], -1, np.int32)
    for t in range(f.shape[0]):
        ok = ~np.isnan(f[t])
        if ok.any():
            smax[t] = f[t][ok].max()
            jmax[t] = int(np.flatnonzero(ok & (f[t] == smax[t]))[0])
    return smax, jmax


def to_tzyx(ua, order):
    """``ua`` (T, three axes in ``order``, a permutation of "zyx") as (T, Z, Y, X)."""
    return np.transpose(np.asarray(ua), (0,) + tuple(1 + order.index(k) for k in "zyx"))


def jetstream_metric_woollings(ua, lat, lon, plev, pmin=75000.0, pmax=95000.0, order="zyx"):
    """_synoptic.py:52-100 on arrays: ``(jetlat, jetstr)``, float64 (T)."""
    ip, ilat, ilon = jet_masks(lat, lon, plev, pmin, pmax)
    u = to_tzyx(ua, order)
    zonal_mean = box_mean(u, np.flatnonzero(ip), np.flatnonzero(ilat), np.flatnonzero(ilon))
    if u.shape[0] <= 10 or u.shape[0] <= 61:
        raise ValueError(f"Time series is too short to apply 61-day Lanczos filter (got a length of  {u.shape[0]})")
    ua_lf, _ = filter_terms(zonal_mean, lanczos_weights(61, 1 / 10))
    smax, jmax = first_max(ua_lf)
    lats = np.asarray(lat, np.float64)[ilat]
    return np.where(jmax >= 0, lats[np.maximum(jmax, 0)], np.nan), smax
