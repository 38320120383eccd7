"""The grid-reduction unit on the device (xclim_amd/csrc/grid.hip, xclim_amd.grid) against the numpy restatement tests/gridcpu.py on
tests/golden/grid_vectors.npz.  EXACT comparison where every sum is exact in float64 in any order (concentrations on a 1/4 % grid,
areas that are integers below 2^20, winds on a 1/64 grid, filters with dyadic weights); on one random family per kernel within 1e-12
x the sum of a value's absolute terms, the bound the hydrology, humidity and partition units assert (the measured share of the bound
is printed before it is asserted).  Shapes: 1, 63, 64, 65, XH_GRID_CHUNK - 1, XH_GRID_CHUNK, XH_GRID_CHUNK + 1 and 2 * XH_GRID_CHUNK
+ 3 cells on 1, XH_GRID_ROWS - 1 and XH_GRID_ROWS + 1 rows; 1 .. 3 levels, 1, 63, 65 and 130 longitudes, 1, 3 and 65 latitudes in
both layouts; 62, 66 and 130 rows.  Every test runs on poisoned output buffers (tests/poisoned.py)."""
import numpy as np
import pytest

import gridcpu as G
from poisoned import poisoned_outputs, unwritten  # noqa: F401  (autouse: the tests of this module run on poisoned output buffers)
from test_grid_cpu import CHUNK, MOVED_THRESH, ROWS, WEIGHTS, check_known_answers, decode, jet_block, mirror_api
from xclim_amd import _capi as capi
from xclim_amd import grid
from xclim_amd import kernels as K
from xclim_amd._capi import DeviceArray

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
IDS = ["float32", "float64"]
CELLS = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
TROWS = (1, ROWS - 1, ROWS + 1)
BOUND = 1e-12
THRESH = 15.0


def bits(a, b, what=""):
    """Equal bit for bit, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    assert not unwritten(a).any(), f"{what}: unwritten elements"
    np.testing.assert_array_equal(a, b, err_msg=what)


def within(got, want, terms, what):
    """|got - want| <= 1e-12 x the sum of the value's absolute terms, the same NaN pattern; prints the measured share."""
    got, want, terms = np.asarray(got), np.asarray(want), np.asarray(terms)
    assert got.shape == want.shape and not unwritten(got).any(), what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    ok = ~np.isnan(want)
    share = (np.abs(got[ok] - want[ok]) / (BOUND * terms[ok])).max() if ok.any() else 0.0
    print(f"{what}: {100 * share:.3g} % of the bound")
    assert share <= 1.0, f"{what}: {share:.3g} x the bound"


def _view(dev, flat, off, shape):
    v = DeviceArray(dev, flat.ptr + off * flat.dtype.itemsize, shape, flat.dtype, owner=False)
    v._owner = flat
    return v


def _dot(dev, x, w, thr=THRESH, outputs=("dot", "msum")):
    out = K.grid_masked_dot(dev, dev.to_device(np.ascontiguousarray(x)), dev.to_device(np.asarray(w, np.float64)), thr, outputs)
    return {k: v.get() for k, v in out.items()}


# ---- xh_grid_masked_dot -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", CELLS)
def test_masked_dot_exact(dev, C, dtype):
    x, w = decode("dot/exact/q", dtype), decode("dot/exact/area")
    for T in TROWS:
        got = _dot(dev, x[:T, :C], w[:C])
        dot, msum, _, _ = G.masked_dot_terms(x[:T, :C], w[:C], THRESH)
        bits(got["dot"], dot, f"dot T={T} C={C}")
        bits(got["msum"], msum, f"msum T={T} C={C}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_dot_random_within_the_bound(dev, dtype):
    x, w = decode("dot/random/x", dtype), decode("dot/random/area")
    got = _dot(dev, x, w)
    dot, msum, adot, amsum = G.masked_dot_terms(x, w, THRESH)
    within(got["dot"], dot, adot, f"masked dot {np.dtype(dtype).name}")
    within(got["msum"], msum, amsum, f"masked sum {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("off,pad", [(0, 4), (4, 8), (1, 5), (2, 3)], ids=["aligned-padded", "aligned-offset", "offset-1", "offset-2"])
def test_masked_dot_on_padded_and_offset_views(dev, dtype, off, pad):
    """A (T, C) block with row pitch C + pad that begins ``off`` elements into its buffer; everything outside the block is NaN, which
    a read past a row would carry into its sum.  (0, 4) and (4, 8) keep the 16-byte path with a partial last group, the others take
    the cell-by-cell path."""
    C, T = CHUNK + 67, ROWS + 1
    x, w = decode("dot/exact/q", dtype)[:T, :C], decode("dot/exact/area")[:C]
    ld = C + pad
    host = np.full(T * ld + off + 4, np.nan, dtype)
    host[off:off + T * ld].reshape(T, ld)[:, :C] = x
    flat = dev.to_device(host)
    out = K.grid_masked_dot(dev, _view(dev, flat, off, (T, ld)), dev.to_device(w), THRESH, C_=C, ld=ld)
    dot, msum, _, _ = G.masked_dot_terms(x, w, THRESH)
    bits(out["dot"].get(), dot, "dot")
    bits(out["msum"].get(), msum, "msum")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_masked_dot_decisions(dev, dtype):
    """A sample equal to the threshold counts; a NaN sample adds 0 * w; a NaN weight, and an infinite one next to a masked cell,
    make the row NaN; a threshold that float32 rounding moves across a sample."""
    C = 70
    x, w = decode("dot/exact/q", dtype)[:3, :C].copy(), decode("dot/exact/area")[:C].copy()
    x[0, 5], x[1, 64], x[2, 69] = THRESH, np.nan, 14.75
    for tag, ww in (("finite", w), ("nan weight", np.where(np.arange(C) == 63, np.nan, w)), ("inf weight", np.where(np.arange(C) == 69, np.inf, w))):
        got = _dot(dev, x, ww)
        dot, msum, _, _ = G.masked_dot_terms(x, ww, THRESH)
        bits(got["dot"], dot, tag)
        bits(got["msum"], msum, tag)
        if tag == "nan weight":
            assert np.isnan(got["dot"]).all() and np.isnan(got["msum"]).all()
        if tag == "inf weight":
            assert np.isnan(got["msum"][2]) and np.isnan(got["dot"][2])      # 0 * inf of the masked cell 69 of row 2
    below = np.float32(MOVED_THRESH)            # the float32 neighbour below the threshold
    x[0, 7] = below
    ext = grid.sea_ice_extent(x, w, MOVED_THRESH, device=dev)
    bits(ext, G.sea_ice_extent(x, w, MOVED_THRESH), "moved threshold")
    x7 = x.copy()
    x7[0, 7] = 0.0
    counted = ext[0] - grid.sea_ice_extent(x7, w, MOVED_THRESH, device=dev)[0]
    assert counted == (w[7] if dtype == np.float32 else 0.0)     # next to a float32 field the threshold is rounded onto the sample


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_each_output_alone_equals_the_fused_launch_and_rows_alone_the_whole_field(dev, dtype):
    x, w = decode("dot/random/x", dtype), decode("dot/random/area")
    xd, wd = dev.to_device(x), dev.to_device(w)
    trace = dev.start_trace()
    try:
        full = K.grid_masked_dot(dev, xd, wd, THRESH)
    finally:
        dev.stop_trace()
    assert [n for n, _ in trace if n.startswith("xh_grid")] == ["xh_grid_masked_dot"]      # both outputs: ONE launch
    full = {k: v.get() for k, v in full.items()}
    for o in ("dot", "msum"):
        alone = K.grid_masked_dot(dev, xd, wd, THRESH, (o,))
        assert list(alone) == [o]
        bits(alone[o].get(), full[o], f"{o} alone")
    for t in range(x.shape[0]):
        row = _dot(dev, x[t:t + 1], w)
        bits(row["dot"], full["dot"][t:t + 1], f"row {t} alone")
        bits(row["msum"], full["msum"][t:t + 1], f"row {t} alone")


def test_the_mirror_s_rows_dtypes_and_fused_form(dev):
    x64, w64 = decode("dot/exact/q")[:6, :130].reshape(2, 3, 10, 13), decode("dot/exact/area")[:130].reshape(10, 13)
    dot, msum, _, _ = G.masked_dot_terms(x64, w64, THRESH)
    for xt, wt, ta, te in ((np.float32, np.float32, np.float32, np.float32), (np.float32, np.float64, np.float64, np.float64),
                           (np.float64, np.float32, np.float64, np.float32), (np.float64, np.int32, np.float64, np.int32)):
        out = grid.sea_ice(x64.astype(xt), w64.astype(wt), THRESH, device=dev)
        assert list(out) == ["area", "extent"] and out["area"].dtype == ta and out["extent"].dtype == te
        bits(out["area"], (dot / 100.0).astype(ta), "area")
        bits(out["extent"], msum.astype(te), "extent")
    frac = x64 / 128.0                                       # fractions on a dyadic grid: still exact in any order
    bits(grid.sea_ice_area(frac, w64, 0.15, units="", device=dev), G.sea_ice_area(frac, w64, 0.15, 1.0), "fraction")
    kept = grid.sea_ice(x64, w64, THRESH, device=dev, keep=True)
    bits(kept["area"].get().reshape(2, 3), dot, "kept: the sum before the division")


def test_the_known_answers_on_the_device(dev):
    check_known_answers(mirror_api(dev))


# ---- xh_grid_box_mean -------------------------------------------------------------------------------------------------------------
def _lists(nz, ny, nx, Z, Y, X):
    """Index lists that are not contiguous and not sorted."""
    rng = np.random.default_rng(nz * 1000 + ny * 10 + nx)
    return tuple(rng.permutation(n)[:k] for n, k in ((Z, nz), (Y, ny), (X, nx)))


def _box(dev, u_tzyx, layout, lists):
    """The device's box mean of a (T, Z, Y, X) block stored in ``layout`` ("zyx" or "zxy"), read in place."""
    T, Z, Y, X = u_tzyx.shape
    stored = np.ascontiguousarray(u_tzyx if layout == "zyx" else np.transpose(u_tzyx, (0, 1, 3, 2)))
    strides = (Y * X, X, 1) if layout == "zyx" else (Y * X, 1, Y)
    return K.grid_box_mean(dev, dev.to_device(stored), T, Z * Y * X, (Z, Y, X), strides, *lists).get()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["zyx", "zxy"])
@pytest.mark.parametrize("nz", [1, 2, 3])
def test_box_mean_exact(dev, nz, layout, dtype):
    Z, Y, X = 4, 67, 132
    u = jet_block(3, Z, Y, X, dtype)
    for nx in (1, 63, 65, 130):
        for ny in (1, 3, 65):
            lists = _lists(nz, ny, nx, Z, Y, X)
            want = G.box_mean(u, *lists)
            # the mean of n samples on the 1/64 grid: an exact sum and one division, the same on both sides
            bits(_box(dev, u, layout, lists), want, f"nz={nz} ny={ny} nx={nx}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("layout", ["zyx", "zxy"])
def test_box_mean_random_nan_samples_and_views(dev, layout, dtype):
    u = decode("jet/random/u", dtype).copy()               # (66, 3, 5, 67)
    u[5, 2, 2, 33] = np.nan                                  # one NaN sample (level 2, latitude 2: both selected): skipped by the mean
    u[7, :, 3, :] = np.nan                                   # a (t, latitude) without a sample: NaN
    lists = (np.array([2, 0]), np.array([4, 2, 3, 0]), np.arange(66, 0, -1))
    want, terms = G.box_mean_terms(u, *lists)
    got = _box(dev, u, layout, lists)
    assert np.isnan(got[7, 2]) and np.isnan(got).sum() == 1
    within(got, want, terms, f"box mean {layout} {np.dtype(dtype).name}")
    sel = u[5][[2, 0]][:, 2, 1:].astype(np.float64)
    assert np.isnan(sel).sum() == 1 and abs(got[5, 1] - np.nansum(sel) / (sel.size - 1)) <= BOUND * np.nansum(np.abs(sel))
    # a padded output: ld_zm beyond ny, nothing outside the block written
    T, Z, Y, X = u.shape
    stored = np.ascontiguousarray(u if layout == "zyx" else np.transpose(u, (0, 1, 3, 2)))
    flat = dev.empty((T * 7 + 3,), np.float64)
    K.grid_box_mean(dev, dev.to_device(stored), T, Z * Y * X, (Z, Y, X), (Y * X, X, 1) if layout == "zyx" else (Y * X, 1, Y), *lists,
                    out=_view(dev, flat, 3, (T, 7)), ld_out=7)
    host = flat.get()
    block = host[3:].reshape(T, 7)
    bits(block[:, :4].copy(), got, "padded output")
    assert unwritten(block[:, 4:]).all() and unwritten(host[:3]).all()


# ---- xh_grid_filter_argmax --------------------------------------------------------------------------------------------------------
def _filter(dev, zm, wts, outputs=("f", "smax", "jmax")):
    out = K.grid_filter_argmax(dev, dev.to_device(np.ascontiguousarray(zm, dtype=np.float64)), wts, outputs)
    return {k: v.get() for k, v in out.items()}


def _check_filter(dev, zm, wts, what):
    got = _filter(dev, zm, wts)
    f, _ = G.filter_terms(zm, wts)
    smax, jmax = G.first_max(f)
    bits(got["f"], f, what + " f")
    bits(got["smax"], smax, what + " smax")
    bits(got["jmax"], jmax, what + " jmax")
    return got


@pytest.mark.parametrize("T", [62, 66, 130])
@pytest.mark.parametrize("W", [1, 2, 61, 128])
def test_filter_argmax_exact(dev, T, W):
    """Zonal means on the 1/64 grid and dyadic weights (multiples of 1/8 up to 2): every product and every sum is exact."""
    wts = ((np.arange(W) * 5) % 17) / 8.0
    for ny in (1, 3, 65):
        zm = jet_block(T, 1, ny, 1)[:, 0, :, 0]
        got = _check_filter(dev, zm, wts, f"T={T} W={W} ny={ny}")
        inside = max(T - W + 1, 0)
        assert (~np.isnan(got["f"][:, 0])).sum() == inside and (got["jmax"] >= 0).sum() == inside


def test_filter_argmax_lanczos_random_within_the_bound(dev):
    zm = decode("filter/random/zm")
    got = _filter(dev, zm, WEIGHTS)
    f, terms = G.filter_terms(zm, WEIGHTS)
    within(got["f"], f, terms, "Lanczos filter")
    smax, jmax = G.first_max(got["f"])                       # the maximum is a selection: exact on the device's own f
    bits(got["smax"], smax, "smax")
    bits(got["jmax"], jmax, "jmax")
    alone = _filter(dev, zm, WEIGHTS, ("smax", "jmax"))      # f is optional
    assert list(alone) == ["smax", "jmax"]
    bits(alone["smax"], got["smax"], "smax without f")
    bits(alone["jmax"], got["jmax"], "jmax without f")


def test_filter_argmax_nan_latitudes_ties_and_the_limit(dev):
    T, ny, W = 130, 65, 61
    wts = ((np.arange(W) * 5) % 17 + 1) / 8.0
    zm = jet_block(T, 1, ny, 1)[:, 0, :, 0]
    clean = _check_filter(dev, zm, wts, "clean")
    # a (t, latitude) that is NaN: that latitude is NaN in the 61 rows whose window holds it, skipped by the maximum, nothing else moves
    hole = zm.copy()
    hole[64, 40] = np.nan
    got = _check_filter(dev, hole, wts, "hole")
    rows = np.flatnonzero(np.isnan(got["f"][:, 40]) & ~np.isnan(clean["f"][:, 40]))
    assert rows.tolist() == list(range(64 - 30, 64 + 31)) and len(rows) == 61
    others = np.delete(np.arange(ny), 40)
    bits(got["f"][:, others], clean["f"][:, others], "the other latitudes")
    assert not (got["jmax"][rows] == 40).any()
    # every latitude NaN on one row of the input: -1 / NaN on the rows whose window holds it
    gone = zm.copy()
    gone[64, :] = np.nan
    got = _check_filter(dev, gone, wts, "row of NaN")
    assert (got["jmax"][34:95] == -1).all() and np.isnan(got["smax"][34:95]).all() and (got["jmax"][95:100] >= 0).all()
    # a tie between two latitudes: the first in field order, also across the lanes of the wave (0 and 64) and within one (3 and 5)
    for a, b in ((3, 5), (0, 64), (10, 9)):
        tie = zm - 100.0
        tie[:, a] = tie[:, b] = zm[:, 7] + 50.0
        got = _check_filter(dev, tie, wts, f"tie {a} {b}")
        assert (got["jmax"][30:100] == min(a, b)).all()
    # 129 weights: XH_ERR_LIMIT, before anything is launched, the outputs untouched
    zd, smax = dev.to_device(zm), dev.empty((T,), np.float64)
    w129 = np.ones(capi.GRID_MAX_WINDOW + 1)
    with pytest.raises(capi.XclimHipError) as e:
        K._ext_call(dev, "xh_grid_filter_argmax", T, ny, K._vp(zd.ptr), ny, len(w129), capi.np_ptr(w129), K._vp(0), ny, K._vp(smax.ptr), K._vp(0))
    assert e.value.code == capi.XH_ERR_LIMIT and unwritten(smax.get()).all()
    with pytest.raises(ValueError, match="up to 128 weights"):
        K.grid_filter_argmax(dev, zd, w129)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("order", ["zyx", "zxy"])
def test_the_jet_mirror_end_to_end(dev, order, dtype):
    """66 rows of the exact family on a grid with latitudes and longitudes inside and outside the box, levels in hPa; the mirror
    against the restatement: the means are exact, the filter adds in the same order, so everything is equal bit for bit."""
    lat, lon, plev = np.linspace(10.0, 80.0, 15), np.linspace(-70.0, 10.0, 33), np.array([1000.0, 925.0, 850.0, 700.0])
    u = jet_block(66, 4, 15, 33, dtype)
    u[40, 2, 6, 9] = np.nan
    stored = np.ascontiguousarray(u if order == "zyx" else np.transpose(u, (0, 1, 3, 2)))
    jetlat, jetstr = grid.jetstream_metric_woollings(stored, lat, lon, plev, plev_units="hPa", order=order, device=dev)
    wlat, wstr = G.jetstream_metric_woollings(stored, lat, lon, plev, 750.0, 950.0, order)
    bits(jetlat, wlat, "jetlat")
    bits(jetstr, wstr, "jetstr")
    assert (~np.isnan(jetstr)).sum() == 6 and set(jetlat[30:36]) <= set(lat[(lat >= 15) & (lat <= 75)])
