"""The spatial-analogue unit on the device (xclim_amd/analog.py, xclim_amd/csrc/analog.hip) against the reference's recorded
results (tests/golden/analog_vectors.npz, analog_known_answers.json; made by tests/golden/make_analog_golden.py).

nearest_neighbor, friedman_rafsky and kolmogorov_smirnov are quotients of integer counts: bit for bit.  The NaN and inf pattern is
the reference's everywhere.  The float-valued metrics agree within ``max(1e-12, (2 terms + 8) 2^-53) * scale`` with ``scale`` and
``terms`` from the restatement of tests/analogcpu.py (its module text derives them).  The kernel has ONE path — a lane's arrays
always live in the work buffer — so there is no switch point between an LDS and a scratch form to stand on; what changes with
the shape is the launch (lanes striding over the cells) and the size of the per-lane arrays, and both are run at their ends."""
import functools
import json
import os

import numpy as np
import pytest

import analogcpu as R
from poisoned import POISON, pattern, poisoned_outputs, unwritten  # noqa: F401  (autouse: every test runs on poisoned output buffers)
from xclim_amd import _capi as capi
from xclim_amd import analog as A
from xclim_amd import kernels as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = np.load(os.path.join(GOLDEN, "analog_vectors.npz"))
KNOWN = json.load(open(os.path.join(GOLDEN, "analog_known_answers.json")))
CASES = sorted({k.split("/")[0] for k in VECTORS.files})


def variants_of(case):
    return [k.split("/")[1] for k in VECTORS.files if k.startswith(case + "/") and k.split("/")[1] in R.VARIANTS]


def keywords(case, variant):
    method, kw = R.VARIANTS[variant]
    return method, {k: (VECTORS[f"{case}/VI"] if isinstance(v, str) else v) for k, v in kw.items()}


@functools.lru_cache(maxsize=None)
def restated(case, variant):
    """(value, scale, terms) of the restatement over all cells of a case: computed once, shared, never changed."""
    method, kw = keywords(case, variant)
    out = R.cells(method, VECTORS[f"{case}/x"], VECTORS[f"{case}/y"].astype(np.float64), **kw)
    for a in out[:2]:
        a.setflags(write=False)
    return out


def compare(case, variant, got, cells):
    """`got` (C,) or (C, nk) for the first `cells` cells of a case against the reference's recorded result."""
    method, _ = keywords(case, variant)
    exp = VECTORS[f"{case}/{variant}"][:cells]
    assert got.shape == exp.shape and got.dtype == np.float64
    assert not unwritten(got).any(), "an output element was not written"
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{case}/{variant}: NaN pattern")
    inf = np.isinf(exp)
    np.testing.assert_array_equal(np.isinf(got), inf, err_msg=f"{case}/{variant}: inf pattern")
    np.testing.assert_array_equal(got[inf], exp[inf])
    if method in R.EXACT:
        np.testing.assert_array_equal(got, exp, err_msg=f"{case}/{variant}")
        return
    _, scale, terms = restated(case, variant)
    tol = R.tolerance(scale[:cells], terms)
    ok = np.isfinite(exp)
    err = np.abs(got[ok] - exp[ok])
    worst = float((err / tol[ok]).max()) if ok.any() else 0.0
    print(f"{case}/{variant} C={cells}: max |got - ref| / tolerance = {worst:.3g}")
    assert (err <= tol[ok]).all(), f"{case}/{variant}: {worst:.3g} times the tolerance"


def device_run(dev, case, variant, cells, **extra):
    method, kw = keywords(case, variant)
    y = VECTORS[f"{case}/y"]
    return A.dissimilarity(method, VECTORS[f"{case}/x"], [np.ascontiguousarray(f[:, :cells]) for f in y], device=dev, **kw, **extra)


@pytest.mark.parametrize("cells", [1, 65, 130])
@pytest.mark.parametrize("case", ["main64", "main32"])
def test_the_goldens_in_both_dtypes(dev, case, cells):
    assert VECTORS[f"{case}/y"].dtype == (np.float64 if case == "main64" else np.float32)
    for variant in variants_of(case):
        compare(case, variant, device_run(dev, case, variant, cells), cells)


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("main")])
def test_one_family_per_decision(dev, case):
    """A NaN in a cell, a NaN in the target, a constant index, a cell equal to the target, m = 4, n > m, KS with exact ties in one and
    in six indices."""
    cells = VECTORS[f"{case}/y"].shape[2]
    assert variants_of(case)
    for variant in variants_of(case):
        compare(case, variant, device_run(dev, case, variant, cells), cells)


def test_the_restatement_agrees_with_the_goldens():
    """(no device: the tolerance's scale comes from a restatement that reproduces the reference)"""
    for variant in variants_of("main64"):
        value, scale, terms = restated("main64", variant)
        exp = VECTORS[f"main64/{variant}"]
        if R.VARIANTS[variant][0] in R.EXACT:
            np.testing.assert_array_equal(value, exp)
        else:
            assert (np.abs(value - exp) <= R.tolerance(scale, terms)).all(), variant


def _padded(dev, a, ld, poison):
    host = np.full((a.shape[0], ld), poison, a.dtype)
    host[:, :a.shape[1]] = a
    return dev.to_device(host)


@pytest.mark.parametrize("case", ["main64", "main32"])
def test_padded_row_views_give_the_same_bits_and_keep_their_padding(dev, case):
    """ld > C and ld_out > C: the fields' padding holds poison (1e30 and NaN by turns) that must not be read into a result, the
    output's padding a byte pattern that must come back untouched."""
    x, y = VECTORS[f"{case}/x"], VECTORS[f"{case}/y"]
    cells, ld, ld_out = 67, 67 + 5, 67 + 3
    for variant in variants_of(case):
        method, kw = keywords(case, variant)
        dense = device_run(dev, case, variant, cells)
        fields = [_padded(dev, f[:, :cells], ld, (1e30, np.nan)[j % 2]) for j, f in enumerate(y)]
        par, k, many = A._parameters(method, {**A._KEYWORDS[method], **kw}, np.asarray(x, np.float64))
        rows = len(k) if k is not None else 1
        out = dev.to_device(np.full((rows, ld_out), pattern(np.float64)))
        K.analog(dev, method, x, fields, par=par, k=k, C_=cells, ld=ld, out=out, ld_out=ld_out)
        got = out.get()
        assert unwritten(got[:, cells:]).all(), f"{variant}: wrote into the padding of an output row"
        got = got[:, :cells].T if many else got[0, :cells]
        np.testing.assert_array_equal(got, dense, err_msg=variant)
        compare(case, variant, np.ascontiguousarray(got), cells)


def test_lanes_striding_over_the_cells_give_the_same_bits(dev, monkeypatch):
    """One workgroup of 256 lanes for 130 cells repeated to 650: every lane takes two or three cells, and its arrays in the work
    buffer are used again."""
    case, reps = "main64", 5
    y = np.tile(VECTORS[f"{case}/y"], (1, 1, reps))
    once = {v: device_run(dev, case, v, 130) for v in variants_of(case)}
    monkeypatch.setenv("XH_DIAGNOSTICS", "1")
    monkeypatch.setenv("XH_ANALOG_MAX_BLOCKS", "1")
    for variant in variants_of(case):
        method, kw = keywords(case, variant)
        got = A.dissimilarity(method, VECTORS[f"{case}/x"], list(y), device=dev, **kw)
        np.testing.assert_array_equal(got, np.concatenate([once[variant]] * reps, axis=0), err_msg=variant)


def _unique_sample(rng, n, m, d, cells):
    from scipy.spatial.distance import pdist

    x, y = rng.normal(0, 1, (n, d)), rng.normal(0.3, 1.2, (d, m, cells))
    # neighbours and the spanning tree are unique beyond rounding: two float64 evaluations of one distance differ by at most
    # (d + 2) * 2^-53 < 1e-15 relative, and no two of the up to 523 776 sorted distances are closer than a hundred times that
    for c in range(cells):
        dd = np.sort(pdist(np.vstack([x, y[:, :, c].T])))
        assert np.min(np.diff(dd) / dd[1:]) >= 1e-13
    return x, y


@pytest.mark.parametrize("n, m, d", [(183, 183, 2), (366, 366, 1), (512, 512, 2)])
def test_a_year_of_daily_samples_and_the_largest_samples(dev, n, m, d):
    """n + m = 366, a year against a year, and the limit of the header: the per-lane arrays at their largest (2 * 1024 keys and
    sides, k = 32), against the restatement."""
    rng = np.random.default_rng(n + m + d)
    cells = 3
    x, y = _unique_sample(rng, n, m, d, cells)
    runs = [("friedman_rafsky", {}), ("kldiv", {"k": [1, capi.ANALOG_MAX_K]}), ("kolmogorov_smirnov", {}), ("seuclidean", {})]
    if n < 512:
        runs += [("zech_aslan", {}), ("szekely_rizzo", {}), ("nearest_neighbor", {})]
    for method, kw in runs:
        got = A.dissimilarity(method, x, list(y), device=dev, **kw)
        value, scale, terms = R.cells(method, x, y, **kw)
        if method in R.EXACT:
            np.testing.assert_array_equal(got, value, err_msg=method)
        else:
            assert (np.abs(got - value) <= R.tolerance(scale, terms)).all(), (method, got, value)


def test_single_pairs_reproduce_the_known_answers(dev):
    """C = 1 through the single-pair functions: the known answers of the reference's own tests, to their decimals, and the
    reference's result within the tolerance."""
    assert len(KNOWN) == 9
    for ka in KNOWN:
        x, y, kw = np.array(ka["x"]), np.array(ka["y"]), ka["kwargs"]
        got = A.metrics[ka["method"]](x, y, device=dev, **kw)
        assert isinstance(got, np.float64)
        assert abs(got - ka["expected"]) < 1.5 * 10.0 ** -ka["decimals"], (ka["name"], got)
        if ka["method"] in R.EXACT:
            assert got == ka["reference"], ka["name"]
        else:
            _, scale, terms = R.metric(ka["method"], x, y, **kw)
            assert abs(got - ka["reference"]) <= R.tolerance(scale, terms), (ka["name"], got, ka["reference"])
    x, y = VECTORS["main64/x"], VECTORS["main64/y"][:, :, 3].T
    many = A.kldiv(x, y, k=[1, 2, 15], device=dev)
    assert isinstance(many, list) and len(many) == 3
    np.testing.assert_array_equal(many, device_run(dev, "main64", "kldiv_k", 4)[3])
    assert np.isnan(A.seuclidean(np.array([1.0, np.nan, 2.0]), np.arange(4.0), device=dev))
    with pytest.raises(AttributeError, match="Shape mismatch"):
        A.seuclidean(np.zeros((5, 2)), np.zeros((5, 3)), device=dev)


def test_one_past_each_limit_answers_limit_and_leaves_the_output_untouched(dev):
    S, D = capi.ANALOG_MAX_SAMPLE, capi.ANALOG_MAX_D
    cells = 3

    def call(method, n, m, d, k=None):
        fields = [dev.to_device(np.ones((m, cells))) for _ in range(d)]
        out = dev.empty((len(k) if k is not None else 1, cells), np.float64)
        par = {"zech_aslan": [1e-12], "szekely_rizzo": [1.0], "mahalanobis": np.eye(d)}.get(method)
        try:
            K.analog(dev, method, np.ones((n, d)), fields, par=par, k=k, out=out, ld_out=cells)
        finally:
            assert unwritten(out.get()).all(), (method, n, m, d, k)

    for method in capi.ANALOG_METHODS:
        k = [1] if method == "kldiv" else None
        for n, m, d in ((S + 1, 5, 1), (5, S + 1, 1), (5, 5, D + 1)):
            with pytest.raises(capi.XclimHipError) as e:
                call(method, n, m, d, k)
            assert e.value.code == capi.XH_ERR_LIMIT, (method, n, m, d)
    for d, k in ((capi.ANALOG_KS_MAX_D + 1, None),):
        with pytest.raises(capi.XclimHipError) as e:
            call("kolmogorov_smirnov", 5, 5, d, k)
        assert e.value.code == capi.XH_ERR_LIMIT
    for k in ([capi.ANALOG_MAX_K + 1], [1] * (capi.ANALOG_MAX_NK + 1)):
        with pytest.raises(capi.XclimHipError) as e:
            call("kldiv", 5, 5, 1, k)
        assert e.value.code == capi.XH_ERR_LIMIT
    # ... and AT each limit the call is served (the sizes of the largest per-lane arrays are run in the test above)
    rng = np.random.default_rng(5)
    x, y = rng.normal(0, 1, (7, D)), rng.normal(0, 1, (D, 9, cells))
    for method, kw in (("seuclidean", {}), ("kldiv", {"k": list(range(1, capi.ANALOG_MAX_NK + 1))}), ("zech_aslan", {})):
        got = A.dissimilarity(method, x, list(y), device=dev, **kw)
        value, scale, terms = R.cells(method, x, y, **kw)
        np.testing.assert_array_equal(np.isinf(got), np.isinf(value))
        ok = np.isfinite(value)
        assert (np.abs(got[ok] - value[ok]) <= np.broadcast_to(R.tolerance(scale, terms), value.shape)[ok]).all(), method
    x6, y6 = np.round(rng.normal(0, 1, (9, 6))), np.round(rng.normal(0, 1, (6, 8, cells)))
    np.testing.assert_array_equal(A.dissimilarity("kolmogorov_smirnov", x6, list(y6), device=dev), R.cells("kolmogorov_smirnov", x6, y6)[0])


def test_keep_returns_the_device_array_and_device_fields_are_taken_as_they_are(dev):
    x, y = VECTORS["main64/x"], VECTORS["main64/y"]
    fields = [dev.to_device(np.ascontiguousarray(f[:, :65])) for f in y]
    kept = A.spatial_analogs(x, fields, method="kldiv", k=[1, 2, 15], device=dev, keep=True)
    assert isinstance(kept, capi.DeviceArray) and kept.shape == (3, 65) and kept.dtype == np.float64
    np.testing.assert_array_equal(kept.get().T, device_run(dev, "main64", "kldiv_k", 65))
    # the sample axis elsewhere, cells on a grid, the target as a sequence of series, candidates as one array
    grid = np.moveaxis(y[:, :, :12].reshape(3, 33, 3, 4), 1, -1)   # (d, 3, 4, m)
    got = A.spatial_analogs(list(x.T), list(grid), dist_dim=-1, method="zech_aslan", device=dev)
    np.testing.assert_array_equal(got, device_run(dev, "main64", "zech_aslan", 12).reshape(3, 4))
    np.testing.assert_array_equal(A.spatial_analogs(x, y[:, :, :12], method="seuclidean", device=dev), device_run(dev, "main64", "seuclidean", 12))
