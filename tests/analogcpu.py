"""A numpy / scipy restatement of the eight dissimilarity metrics of xclim.analog (reference: src/xclim/analog.py:181-628), the
CPU side of tests/test_analog_cpu.py and tests/test_gpu_analog.py.  Test infrastructure only.

Every metric is a function of ONE pair ``(x, y)``, ``x`` (n, d) and ``y`` (m, d) float64, written with whole-array numpy and
scipy calls (``pdist`` / ``cdist``, a KD-tree, ``csgraph.minimum_spanning_tree``), not with the loops of the kernel.  ``cells``
runs one over the cells of a candidate array ``(d, m, C)``.

A float-valued metric returns ``(value, scale, terms)``: ``scale`` bounds, in units of one rounding error, what a different
but equally valid order of operations can change, and ``terms`` counts the additions behind the value.  The GPU tests allow
``max(1e-12, (2 * terms + 8) * 2**-53) * scale``.  How ``scale`` is put together, metric by metric (u = 2**-53):

* ``seuclidean`` = sqrt(sum_k delta_k^2 / var_k), delta_k = mean x_k - mean y_k.  A mean of n values carries an error of about
  n u mean|x_k|; d(value) / d(delta_k) = delta_k / (var_k value), at most 1 / sqrt(var_k) in size.  scale = sum_k (mean|x_k| +
  mean|y_k|) / sqrt(var_k) + value; terms = n + m + d.
* ``mahalanobis`` = sqrt(delta VI delta): d(value) = (VI_sym delta) . d(delta) / value.  scale = sum_k |(VI_sym delta)_k| (mean|x_k| +
  mean|y_k|) / value + sum_ij |delta_i VI_ij delta_j| / value + value; terms = n + m + d * d.
* ``zech_aslan`` adds logarithms of distances, divided by the number of pairs of their group.  A relative error e of a distance is
  an ABSOLUTE error e of its logarithm whatever the logarithm's size (it may be zero), so every group contributes its mean
  |log| plus one: scale = mean|log xx| + mean|log yy| + mean|log xy| + 3; terms = the pairs + n + m (the deviations).
* ``szekely_rizzo`` adds distances: scale = w (2 sXY + sXX + sYY); terms as above.
* ``kldiv``: the logarithms again: scale = (sum_i |log(r_i / s_i)| + n) d / n + |log(m / (n - 1))|; terms = n + 2 d.

``nearest_neighbor``, ``friedman_rafsky`` and ``kolmogorov_smirnov`` are quotients of integer counts and are compared bit for
bit: they return ``(value, 0.0, 0)``.
"""
import numpy as np
from scipy import spatial
from scipy.sparse.csgraph import minimum_spanning_tree
from scipy.spatial import cKDTree

METHODS = ("seuclidean", "nearest_neighbor", "zech_aslan", "szekely_rizzo", "friedman_rafsky", "kolmogorov_smirnov", "kldiv",
           "mahalanobis")
EXACT = ("nearest_neighbor", "friedman_rafsky", "kolmogorov_smirnov")

# the runs of the fixtures: name -> (metric, keyword arguments); "VI" stands for the matrix stored with the case
VARIANTS = {
    "seuclidean": ("seuclidean", {}),
    "nearest_neighbor": ("nearest_neighbor", {}),
    "zech_aslan": ("zech_aslan", {}),
    "zech_aslan_dmin": ("zech_aslan", {"dmin": 0.75}),
    "szekely_rizzo": ("szekely_rizzo", {}),
    "szekely_rizzo_raw": ("szekely_rizzo", {"standardize": False}),
    "friedman_rafsky": ("friedman_rafsky", {}),
    "kolmogorov_smirnov": ("kolmogorov_smirnov", {}),
    "kldiv": ("kldiv", {}),
    "kldiv_k": ("kldiv", {"k": [1, 2, 15]}),
    "mahalanobis": ("mahalanobis", {}),
    "mahalanobis_VI": ("mahalanobis", {"VI": "VI"}),
}


def tolerance(scale, terms):
    """The bound of tests/test_gpu_analog.py on |device - reference| for a float-valued metric."""
    return np.maximum(1e-12, (2.0 * np.asarray(terms, np.float64) + 8.0) * 2.0 ** -53) * np.asarray(scale, np.float64)


def _two_d(x, y):
    x, y = np.atleast_2d(np.asarray(x, np.float64)), np.atleast_2d(np.asarray(y, np.float64))
    x = x.T if x.shape[0] == 1 else x
    y = y.T if y.shape[0] == 1 else y
    if x.shape[1] != y.shape[1]:
        raise AttributeError("Shape mismatch")
    return x, y


def seuclidean(x, y):
    n, d = x.shape
    var = x.var(axis=0, ddof=1)
    delta = x.mean(axis=0) - y.mean(axis=0)
    value = np.sqrt((delta * delta / var).sum())
    scale = ((np.abs(x).mean(axis=0) + np.abs(y).mean(axis=0)) / np.sqrt(var)).sum() + value
    return value, scale, n + len(y) + d


def mahalanobis(x, y, *, VI=None):
    n, d = x.shape
    if not isinstance(VI, np.ndarray):
        if VI is not None:
            raise AttributeError("VI not a matrix")
        v = np.atleast_2d(np.cov(x, rowvar=False))
        try:
            VI = np.linalg.inv(v)
        except np.linalg.LinAlgError:
            VI = np.linalg.pinv(v)
    delta = x.mean(axis=0) - y.mean(axis=0)
    value = np.sqrt(delta @ VI @ delta)
    spread = np.abs(x).mean(axis=0) + np.abs(y).mean(axis=0)
    sym = 0.5 * (VI + VI.T)
    scale = ((np.abs(sym @ delta) * spread).sum() + np.abs(delta[:, None] * VI * delta[None, :]).sum()) / value + value
    return value, scale, n + len(y) + d * d


def _v(x, y):
    return x.std(axis=0, ddof=1) * y.std(axis=0, ddof=1)


def zech_aslan(x, y, *, dmin=1e-12):
    n, m = len(x), len(y)
    v = _v(x, y)
    logs = [np.log(np.maximum(dd, dmin)) for dd in (spatial.distance.pdist(x, "seuclidean", V=v), spatial.distance.pdist(y, "seuclidean", V=v),
                                                   spatial.distance.cdist(x, y, "seuclidean", V=v).ravel())]
    counts = (n * (n - 1), m * (m - 1), n * m)
    phi = [-lg.sum() / c for lg, c in zip(logs, counts)]
    scale = sum(np.abs(lg).sum() / c for lg, c in zip(logs, counts)) + 3.0
    return phi[0] + phi[1] - phi[2], scale, sum(len(lg) for lg in logs) + n + m


def szekely_rizzo(x, y, *, standardize=True):
    n, m = len(x), len(y)
    kw = {"metric": "seuclidean", "V": _v(x, y)} if standardize else {"metric": "euclidean"}
    dxy, dxx, dyy = spatial.distance.cdist(x, y, **kw), spatial.distance.pdist(x, **kw), spatial.distance.pdist(y, **kw)
    sxy, sxx, syy = dxy.sum() / (n * m), dxx.sum() * 2 / n ** 2, dyy.sum() * 2 / m ** 2
    w = n * m / (n + m)
    return w * (sxy + sxy - sxx - syy), w * (sxy + sxy + sxx + syy), dxy.size + dxx.size + dyy.size + n + m


def nearest_neighbor(x, y):
    s = np.sqrt(_v(x, y))
    with np.errstate(all="ignore"):
        xy = np.vstack([x / s, y / s])
    if not np.isfinite(xy).all():   # (the reference's KD-tree raises for the whole call; the device writes NaN into the cell)
        return np.nan, 0.0, 0
    _, ind = cKDTree(xy).query(xy, k=2)
    same = (ind[:, 0] < len(x)) == (ind[:, 1] < len(x))
    return same.mean(), 0.0, 0


def friedman_rafsky(x, y):
    n = len(x) + len(y)
    xy = np.vstack([x, y])
    mst = minimum_spanning_tree(spatial.distance.squareform(spatial.distance.pdist(xy, "euclidean")))
    edges = np.array(mst.nonzero()).T
    diff = np.logical_xor(*(edges < len(x)).T).sum()
    return 1.0 - (1.0 + diff) / n, 0.0, 0


def kolmogorov_smirnov(x, y):
    def pivot(a, b):
        d = a.shape[1]
        weights = 2 ** np.arange(d)
        best = 0.0
        for p in a:   # one pivot: the orthant codes of both samples, counted
            ca = np.bincount(((p <= a) * weights).sum(axis=1), minlength=2 ** d)
            cb = np.bincount(((p <= b) * weights).sum(axis=1), minlength=2 ** d)
            best = max(best, float(np.max(np.abs(1.0 * ca / len(a) - 1.0 * cb / len(b)))))
        return best

    return max(pivot(x, y), pivot(y, x)), 0.0, 0


def kldiv(x, y, *, k=1):
    many = np.iterable(k)
    ka = np.atleast_1d(k)
    n, d = x.shape
    m = len(y)
    if d > 10:
        raise ValueError(f"Too many dimensions: {d}.")
    if n < 5 or m < 5:
        nan = np.full(len(ka), np.nan)
        return (nan, np.zeros(len(ka)), 0) if many else (np.nan, 0.0, 0)
    kmax = int(max(ka)) + 1
    r, _ = cKDTree(x).query(x, k=kmax)
    s, _ = cKDTree(y).query(x, k=kmax)
    r, s = r.reshape(n, -1), s.reshape(n, -1)
    with np.errstate(all="ignore"):
        logs = np.stack([np.log(r[:, ki] / s[:, ki - 1]) for ki in ka])   # (nk, n)
        const = np.log(m / (n - 1.0))
        value = -logs.sum(axis=1) * d / n + const
        scale = (np.abs(logs).sum(axis=1) + n) * d / n + abs(const)
    return (value, scale, n + 2 * d) if many else (value[0], scale[0], n + 2 * d)


FUNCTIONS = {"seuclidean": seuclidean, "nearest_neighbor": nearest_neighbor, "zech_aslan": zech_aslan, "szekely_rizzo": szekely_rizzo,
             "friedman_rafsky": friedman_rafsky, "kolmogorov_smirnov": kolmogorov_smirnov, "kldiv": kldiv, "mahalanobis": mahalanobis}


def metric(method, x, y, **kwargs):
    """``(value, scale, terms)`` of one pair with the reference's overhead: NaN anywhere gives NaN, 1-D samples are columns."""
    nk = len(kwargs["k"]) if method == "kldiv" and np.iterable(kwargs.get("k", 1)) else None
    if np.any(np.isnan(x)) or np.any(np.isnan(y)):
        return (np.nan, 0.0, 0) if nk is None else (np.full(nk, np.nan), np.zeros(nk), 0)
    x, y = _two_d(x, y)
    with np.errstate(all="ignore"):
        return FUNCTIONS[method](x, y, **kwargs)


def cells(method, x, fields, **kwargs):
    """``(value, scale, terms)`` over the cells of ``fields`` (d, m, C): arrays (C,), or (C, nk) for kldiv with a list of k."""
    fields = np.asarray(fields, np.float64)
    out = [metric(method, x, fields[:, :, c].T, **kwargs) for c in range(fields.shape[2])]
    value, scale = np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.float64)
    return value, scale, max((o[2] for o in out), default=0)
