"""Generate tests/golden/analog_vectors.npz and tests/golden/analog_known_answers.json by EXECUTING the reference's spatial
analogue metrics.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_analog_golden.py

src/xclim/analog.py imports xarray and boltons, which are not installed here.  Its source is compiled as it stands with two
stand-ins in ``sys.modules``: an empty ``xarray`` (the metrics never touch it; the annotations are strings) and a
``boltons.funcutils`` whose ``wraps`` is ``functools.wraps``.  Nothing of the reference is copied into this repository: the
fixtures hold inputs and the outputs of the reference's own ``metrics`` registry, cell by cell — what ``xr.apply_ufunc(...,
vectorize=True)`` does.  The names of the runs and their keyword arguments are ``VARIANTS`` of tests/analogcpu.py.

analog_vectors.npz, one group of arrays per case ``<case>/...``: ``x`` (n, d) the target, ``y`` (d, m, C) the candidate fields,
``VI`` the matrix of the "mahalanobis_VI" run and ``<variant>`` (C,) or (C, nk) the reference's results.  A float32 case stores
float32 fields; its results are the reference's on the widened values.  Where the reference's KD-tree raises for a cell that
is constant in one index (nearest_neighbor) the fixture holds NaN: the device writes NaN into that cell.

  main64 / main32   n = 21, m = 33, d = 3, 130 cells: a normal target, candidates N(0.3, 1.2^2).  Every cell is asserted to have
                    pooled pairwise distances, raw (friedman_rafsky) and standardized (nearest_neighbor), that differ by at
                    least 1e-10 relative when sorted: neighbours and spanning trees are unique far beyond rounding.
  edges             the same target on 6 cells: a NaN in one index of cell 0, cell 1 constant in index 1, cells 2-5 ordinary.
  nan_target        a target with one NaN on 4 cells.
  same              n = m = 21: cell 0 IS the target (distances below dmin, r / s with s = 0), cell 1 is the target moved by
                    1e-13, cell 2 ordinary.  Run for the metrics that do not depend on the order of equal neighbours.
  short             m = 4 (kldiv answers NaN), 5 cells.
  long              n = 40, m = 17, d = 2, 9 cells (n > m).
  ks1 / ks6         d = 1 and d = 6 for kolmogorov_smirnov, values on a coarse grid so that exact ties abound, 12 cells.

analog_known_answers.json: the known answers of the reference's tests/test_analog.py with their inputs (the Matlab sample, the
7-point Friedman-Rafsky case, the iris rows of the Szekely-Rizzo case, a 1-D KS sample with scipy.stats.ks_2samp's statistic)
and the reference's result for each.
"""
import functools
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference/src/xclim/analog.py"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from analogcpu import VARIANTS  # noqa: E402

SEED = 2024


def reference_metrics():
    stubs = {"xarray": types.ModuleType("xarray"), "boltons": types.ModuleType("boltons"), "boltons.funcutils": types.ModuleType("boltons.funcutils")}
    stubs["xarray"].Dataset = stubs["xarray"].DataArray = object
    stubs["boltons.funcutils"].wraps = functools.wraps
    stubs["boltons"].funcutils = stubs["boltons.funcutils"]
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        ns = {"__name__": "reference_analog"}
        exec(compile(open(REF).read(), REF, "exec"), ns)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert list(ns["metrics"]) == ["seuclidean", "nearest_neighbor", "zech_aslan", "szekely_rizzo", "friedman_rafsky",
                                   "kolmogorov_smirnov", "kldiv", "mahalanobis"], list(ns["metrics"])
    return ns["metrics"]


def run(metrics, variant, x, y, VI):
    """The reference over the cells of y (d, m, C) -> (C,) or (C, nk)."""
    name, kw = VARIANTS[variant]
    kw = {k: (VI if isinstance(v, str) else v) for k, v in kw.items()}
    out = []
    for c in range(y.shape[2]):
        yc = np.ascontiguousarray(y[:, :, c].T.astype(np.float64))
        with np.errstate(all="ignore"):
            try:
                out.append(np.asarray(metrics[name](x, yc, **kw), np.float64))
            except ValueError as e:   # nearest_neighbor's KD-tree on a cell whose standardized values are not finite
                assert name == "nearest_neighbor", (variant, c, e)
                out.append(np.float64(np.nan))
    nk = len(kw["k"]) if np.iterable(kw.get("k", 1)) else None
    if nk is not None:   # (the reference's NaN test answers one NaN for the whole list)
        out = [np.broadcast_to(o, (nk,)) for o in out]
    return np.array(out, np.float64)


def min_relative_gap(points):
    from scipy.spatial.distance import pdist

    dd = np.sort(pdist(points))
    return float(np.min(np.diff(dd) / dd[1:]))


def assert_no_ties(x, y):
    worst = np.inf
    for c in range(y.shape[2]):
        yc = y[:, :, c].T.astype(np.float64)
        s = np.sqrt(x.std(0, ddof=1) * yc.std(0, ddof=1))
        worst = min(worst, min_relative_gap(np.vstack([x, yc])), min_relative_gap(np.vstack([x / s, yc / s])))
    assert worst >= 1e-10, f"a cell has two pooled distances {worst:.2e} apart (relative): another seed"
    return worst


def main():
    metrics = reference_metrics()
    rng = np.random.default_rng(SEED)
    n, m, d, C = 21, 33, 3, 130
    x = rng.normal(0.0, 1.0, (n, d))
    y = rng.normal(0.3, 1.2, (d, m, C))
    VI = np.linalg.inv(np.cov(rng.normal(0.0, 1.5, (50, d)), rowvar=False))
    everything = list(VARIANTS)
    cases = {"main64": (x, y, everything), "main32": (x, y.astype(np.float32), everything)}
    print("minimum relative gap of the sorted pooled distances:", assert_no_ties(x, y), assert_no_ties(x, y.astype(np.float32)))

    e = rng.normal(0.3, 1.2, (d, m, 6))
    e[2, 7, 0] = np.nan
    e[1, :, 1] = 0.625
    cases["edges"] = (x, e, everything)
    xn = x.copy()
    xn[5, 1] = np.nan
    cases["nan_target"] = (xn, y[:, :, :4].copy(), everything)
    s = rng.normal(0.3, 1.2, (d, n, 3))
    s[:, :, 0] = x.T
    s[:, :, 1] = x.T + 1e-13
    cases["same"] = (x, s, ["seuclidean", "zech_aslan", "zech_aslan_dmin", "szekely_rizzo", "szekely_rizzo_raw", "kolmogorov_smirnov",
                            "kldiv", "kldiv_k", "mahalanobis", "mahalanobis_VI"])
    cases["short"] = (x, rng.normal(0.3, 1.2, (d, 4, 5)), everything)
    x2 = rng.normal(0.0, 1.0, (40, 2))
    VI2 = np.linalg.inv(np.cov(rng.normal(0.0, 1.5, (50, 2)), rowvar=False))
    y2 = rng.normal(0.3, 1.2, (2, 17, 9))
    assert_no_ties(x2, y2)
    cases["long"] = (x2, y2, everything)
    cases["ks1"] = (np.round(rng.normal(0.0, 1.0, (25, 1)), 1), np.round(rng.normal(0.3, 1.2, (1, 30, 12)), 1), ["kolmogorov_smirnov"])
    cases["ks6"] = (np.round(rng.normal(0.0, 1.0, (12, 6))), np.round(rng.normal(0.3, 1.2, (6, 15, 12))), ["kolmogorov_smirnov"])

    store = {}
    for case, (cx, cy, variants) in cases.items():
        cvi = VI2 if cx.shape[1] == 2 else VI
        store[f"{case}/x"], store[f"{case}/y"] = cx, cy
        if "mahalanobis_VI" in variants:
            store[f"{case}/VI"] = cvi
        for v in variants:
            store[f"{case}/{v}"] = run(metrics, v, cx, cy, cvi)
    assert np.isnan(store["edges/zech_aslan"][:2]).all() and np.isnan(store["edges/szekely_rizzo"][:2]).all()
    assert np.isnan(store["edges/nearest_neighbor"][:2]).all() and np.isfinite(store["edges/friedman_rafsky"][1])
    assert np.isnan(store["short/kldiv"]).all() and np.isnan(store["nan_target/seuclidean"]).all()
    np.savez_compressed(os.path.join(HERE, "analog_vectors.npz"), **store)

    # ---- the known answers of the reference's tests/test_analog.py ----
    from scipy import stats
    from sklearn import datasets

    z = 1.0 * (np.arange(30) + 1) / 30 - 0.5
    mx, my = np.vstack([z * 2 + 30, z * 3 + 40, z]).T, np.vstack([z * 2.2 + 31, z[::-1] * 2.8 + 38, z * 1.1]).T
    known = []

    def answer(name, method, ax, ay, expected, decimals, **kw):
        got = float(metrics[method](ax, ay, **kw))
        assert abs(got - expected) < 1.5 * 10.0 ** -decimals, (name, got, expected)
        known.append({"name": name, "method": method, "kwargs": kw, "x": np.asarray(ax, np.float64).tolist(),
                      "y": np.asarray(ay, np.float64).tolist(), "expected": expected, "decimals": decimals, "reference": got})

    for method, expected in (("seuclidean", 2.8463), ("nearest_neighbor", 1.0), ("zech_aslan", 0.77802), ("friedman_rafsky", 0.96667),
                             ("kolmogorov_smirnov", 0.96667)):
        answer(f"matlab/{method}", method, mx, my, expected, 4)
    answer("friedman_rafsky/7 points", "friedman_rafsky", [[1, 2], [2, 2], [3, 1]], [[1, 1], [2, 4], [3, 2], [4, 2]], 2.0 / 7, 3)
    iris = np.asarray(datasets.load_iris().data, np.float64)
    answer("szekely_rizzo/iris 80-70", "szekely_rizzo", iris[:80], iris[80:], 116.1987, 4, standardize=False)
    answer("szekely_rizzo/iris 50-100", "szekely_rizzo", iris[:50], iris[50:], 199.6205, 4, standardize=False)
    kx, ky = rng.standard_normal(50) + 1, rng.standard_normal(50)
    answer("kolmogorov_smirnov/ks_2samp", "kolmogorov_smirnov", kx, ky, float(stats.ks_2samp(kx, ky)[0]), 3)
    with open(os.path.join(HERE, "analog_known_answers.json"), "w") as f:
        json.dump(known, f, indent=0)
    print(f"{len(store)} arrays, {len(known)} known answers")


if __name__ == "__main__":
    main()
