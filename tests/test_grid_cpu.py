"""The grid-reduction unit without a GPU (xclim_amd.grid, include/units/xclim_hip_grid.h): the numpy restatement tests/gridcpu.py
reproduces the known answers of the reference's own tests (tests/golden/grid_known_answers.json), the mirror's Lanczos weights equal
the recorded ones of the reference bit for bit, the exact families of tests/golden/grid_vectors.npz are exact (every partial sum is
an integer multiple of their grid below 2^53), the mirrors of the header's ``#define``s, and every ``NotServed`` / ``ValueError``
path of the mirror, which is taken before a device is asked for.  Also the helpers that tests/test_gpu_grid*.py import."""
import json
import os
import re

import numpy as np
import pytest

import gridcpu as G
from xclim_amd import _capi as capi
from xclim_amd import grid

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "units", "xclim_hip_grid.h")
KNOWN = json.load(open(os.path.join(HERE, "golden", "grid_known_answers.json")))
_Z = np.load(os.path.join(HERE, "golden", "grid_vectors.npz"))
META = json.loads(str(_Z["meta"]))
CHUNK, ROWS = capi.GRID_CHUNK, capi.GRID_ROWS
WEIGHTS = np.array(KNOWN["lanczos_weights_61_0.1"])
MOVED_THRESH = next(t for t in (15.1, 15.2, 15.3, 15.4, 15.6) if float(np.float32(t)) < t)   # a threshold that float32 rounds DOWN


class NoDevice:
    """Handed in as ``device=``: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


def decode(name, dtype=np.float64):
    """A family of grid_vectors.npz as the tests use it: quarter percents -> %, integer areas, 1/64 m s-1 -> m s-1 (all exact in
    float32 too); the random families as stored."""
    a = _Z[name]
    if name == "dot/exact/q":
        return (a.astype(np.float64) / 4.0).astype(dtype)
    if name == "jet/exact/q":
        return (a.astype(np.float64) / 64.0).astype(dtype)
    if name == "dot/exact/area":
        return a.astype(np.float64)
    return a.astype(dtype) if a.dtype.kind == "f" and name.endswith(("/x", "/u")) else a


def jet_block(T, Z, Y, X, dtype=np.float64):
    """The exact jet family at (T, Z, Y, X): the stored (130, 4, 8, 16) block tiled along Y and X, every tile shifted by a multiple of
    1/64 m s-1 of its own, so that no two latitudes and no two longitudes hold the same series."""
    base = decode("jet/exact/q")
    y, x = np.arange(Y), np.arange(X)
    u = base[:T, :Z][:, :, y % base.shape[2]][:, :, :, x % base.shape[3]]
    u = u + ((y // base.shape[2]) * 5)[None, None, :, None] / 64.0 + ((x // base.shape[3]) * 3)[None, None, None, :] / 64.0
    return u.astype(dtype)


def sea_ice_geometry(k=KNOWN["sea_ice"]):
    """conftest.py:233-251 and test_seaice.py:11-19: ``(areacello (180, 360) in m2, siconc (rows, 180, 360) in %)``."""
    r = k["r"]
    lon_bnds, lat_bnds = np.arange(-180, 181, 1), np.arange(-90, 91, 1)
    lat = np.convolve(lat_bnds, [0.5, 0.5], "valid")
    area = r * np.radians(np.diff(lat_bnds))[:, np.newaxis] * r * np.cos(np.radians(lat)[:, np.newaxis]) * np.radians(np.diff(lon_bnds))
    s = np.where(lat > 0, float(k["north"]), float(k["south"]))[:, None] * np.ones_like(area)
    return area, np.stack([s] * k["rows"])


def jet_case(k=KNOWN["jet"]):
    """test_indices.py:2283-2308: ``(ua (66, 3, 3, 3) in the order (time, Z, X, Y), coordinates)``."""
    ua = np.zeros((k["T"], len(k["Z"]), len(k["X"]), len(k["Y"])))
    ua[...] = np.array(k["value_by_Y"])
    return ua, {n: np.array(k[n], float) for n in "ZXY"}


def check_known_answers(api):
    """``api``: ``sea_ice_area`` / ``sea_ice_extent`` as ``f(siconc, areacello, thresh, units)`` and ``jet`` as ``f(ua, lat, lon,
    plev, order)``; the restatement here, the mirror on the device in tests/test_gpu_grid.py."""
    k = KNOWN["sea_ice"]
    area, sic = sea_ice_geometry(k)
    thresh = float(k["thresh"].split()[0])
    for case in k["cases"]:
        a, s = area * case["area_scale"], sic * case["siconc_scale"]
        t = thresh * case["siconc_scale"]
        r2 = np.pi * k["r"] ** 2 * case["area_scale"]
        ext, sia = api["sea_ice_extent"](s, a, t, case["siconc_units"]), api["sea_ice_area"](s, a, t, case["siconc_units"])
        assert ext.shape == sia.shape == (k["rows"],)
        np.testing.assert_array_almost_equal(ext / (2 * r2), 1, k["decimals"])
        np.testing.assert_array_almost_equal(sia / r2, 1, k["decimals"])
        np.testing.assert_allclose(ext / (2 * r2), k["numpy_ratio"], atol=1e-7)
        np.testing.assert_allclose(sia / r2, k["numpy_ratio"], atol=1e-7)
    k = KNOWN["jet"]
    ua, c = jet_case(k)
    with pytest.raises(ValueError, match="longitude values in a range between -60 and 0"):
        api["jet"](ua, c["Y"], c["X"], c["Z"], "zxy")
    jetlat, jetstr = api["jet"](ua, c["Y"], c["X"] + k["shift_X"], c["Z"], "zxy")
    assert jetlat.shape == jetstr.shape == (k["T"],) and jetlat.dtype == jetstr.dtype == np.float64
    assert np.sum(~np.isnan(jetlat)) == np.sum(~np.isnan(jetstr)) == k["not_nan"]
    assert np.nanmax(jetlat) == k["jetlat_max"]
    assert np.nanmax(jetstr) == k["jetstr_max"]          # equality: the 61 weights added in row order from the first


def restatement_api():
    factor = {"%": 100.0, "": 1.0}
    return {"sea_ice_area": lambda s, a, t, units: G.sea_ice_area(s, a, t, factor[units]),
            "sea_ice_extent": lambda s, a, t, units: G.sea_ice_extent(s, a, t),
            "jet": lambda ua, lat, lon, plev, order: G.jetstream_metric_woollings(ua, lat, lon, plev, order=order)}


def mirror_api(dev):
    return {"sea_ice_area": lambda s, a, t, units: grid.sea_ice_area(s, a, t, units=units, device=dev),
            "sea_ice_extent": lambda s, a, t, units: grid.sea_ice_extent(s, a, t, units=units, device=dev),
            "jet": lambda ua, lat, lon, plev, order: grid.jetstream_metric_woollings(ua, lat, lon, plev, order=order, device=dev)}


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def test_the_restatement_reproduces_the_reference_s_known_answers():
    check_known_answers(restatement_api())


def test_the_weights_are_the_reference_s_bit_for_bit():
    assert WEIGHTS.shape == (grid.JET_WINDOW,) == (61,)
    assert grid.lanczos_weights().tobytes() == WEIGHTS.tobytes()
    assert G.lanczos_weights().tobytes() == WEIGHTS.tobytes()
    s = WEIGHTS[0] * 1.0
    for v in WEIGHTS[1:]:
        s = s + v * 1.0
    assert s == KNOWN["jet"]["jetstr_max"]               # row order from the first term gives the literal of the reference's test ...
    assert float(np.sum(WEIGHTS)) != s or float(np.dot(WEIGHTS, np.ones(61))) != s   # ... which numpy's own orders do not (both) give


def test_the_header_s_defines_are_mirrored():
    text = open(HEADER).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(XH_GRID_\w+)\s+(\d+)", text, re.M)}
    assert defines == capi.UNIT_DEFINES["xclim_hip_grid.h"]
    assert (META["chunk"], META["rows"]) == (CHUNK, ROWS) == (defines["XH_GRID_CHUNK"], defines["XH_GRID_ROWS"])
    assert set(grid.SEA_ICE_OUTPUTS.values()) == set(capi.GRID_OUTPUTS)
    for name in ("xh_grid_masked_dot", "xh_grid_box_mean", "xh_grid_filter_argmax"):
        assert name in capi.UNIT_SIGNATURES and re.search(rf"\bint {name}\(", text)


def test_the_exact_families_are_exact():
    """Every term is a multiple of the family's grid and the sum of the absolute terms stays below 2^53 grid steps: the sum is
    the same in any order."""
    x, w = decode("dot/exact/q"), decode("dot/exact/area")
    assert np.all(x * 4 == np.round(x * 4)) and np.all(w == np.round(w)) and w.max() < 2 ** 20 and x.shape == (ROWS + 1, 2 * CHUNK + 3)
    assert np.array_equal(decode("dot/exact/q", np.float32).astype(np.float64), x)
    assert (np.abs(x) * 4 * w).sum(1).max() < 2.0 ** 53
    u = jet_block(130, 4, 67, 132)
    assert np.all(u * 64 == np.round(u * 64)) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.abs(u * 64).sum((1, 3)).max() < 2.0 ** 53
    assert len({u[:, 0, y, 0].tobytes() for y in range(67)}) == 67 and len({u[:, 0, 0, x].tobytes() for x in range(132)}) == 132


def test_restatement_decisions():
    w = np.array([2.0, 3.0, 5.0])
    below = float(np.float32(MOVED_THRESH))        # the float32 neighbour BELOW the threshold: float32 rounding moves the threshold onto it
    assert below < MOVED_THRESH
    x = np.array([[15.0, np.nan, 14.75], [below, 100.0, 0.0]])
    assert G.sea_ice_extent(x, w, 15.0).tolist() == [2.0, 5.0]                   # equal to the threshold counts; NaN adds 0
    assert G.sea_ice_area(x, w, 15.0, 1.0).tolist() == [30.0, 2 * below + 300.0]
    # a threshold that float32 rounding moves across a sample: next to a float32 field the sample counts, next to a float64 one not
    assert G.sea_ice_extent(x.astype(np.float32), w, MOVED_THRESH).tolist() == [0.0, 5.0]
    assert G.sea_ice_extent(x, w, MOVED_THRESH).tolist() == [0.0, 3.0]
    assert np.isnan(G.sea_ice_extent(x, np.array([2.0, np.nan, 5.0]), 15.0)).all()
    assert np.isnan(G.sea_ice_extent(x, np.array([2.0, 3.0, np.inf]), 15.0)).all()     # 0 * inf: the masked cell of both rows
    assert G.sea_ice_extent(x, np.array([2.0, np.inf, 5.0]), 15.0)[1] == np.inf          # 1 * inf where the cell counts
    f, _ = G.filter_terms(np.arange(10.0)[:, None], [1.0, 1.0])
    assert np.isnan(f[0, 0]) and f[1:, 0].tolist() == [1.0, 3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0, 17.0]   # W = 2: rows t - 1 and t
    smax, jmax = G.first_max(np.array([[np.nan, 2.0, 2.0], [np.nan, np.nan, np.nan]]))
    assert jmax.tolist() == [1, -1] and smax[0] == 2.0 and np.isnan(smax[1])


def test_mirror_checks_come_before_the_device():
    nd = NoDevice()
    area, sic = np.ones((3, 4)), np.ones((2, 3, 4))
    with pytest.raises(grid.NotServed, match="integer"):
        grid.sea_ice_area(sic.astype(np.int32), area, device=nd)
    with pytest.raises(ValueError, match="trailing dimensions"):
        grid.sea_ice_extent(sic, np.ones((4, 3)), device=nd)
    with pytest.raises(ValueError, match="units must be one of"):
        grid.sea_ice_area(sic, area, units="permille", device=nd)
    with pytest.raises(ValueError, match="outputs must be"):
        grid.sea_ice(sic, area, outputs=("volume",), device=nd)
    with pytest.raises(grid.NotServed, match="not a number"):
        grid.sea_ice_area(sic, area, thresh=np.ones(2), device=nd)
    ua, c = jet_case()
    lon = c["X"] - 180
    for lat, lo, plev, text in ((c["Y"], c["X"], c["Z"], "longitude values in a range between -60 and 0°E"),
                                (c["Y"] + 70, lon, c["Z"], "latitude values in a range between 15 and 75°N"),
                                (c["Y"], lon, c["Z"] / 1000, "pressure values in a range between 750 and 950 hPa")):
        with pytest.raises(ValueError, match=text):
            grid.jetstream_metric_woollings(ua, lat, lo, plev, order="zxy", device=nd)
    with pytest.raises(ValueError, match=re.escape("too short to apply 61-day Lanczos filter (got a length of  61)")):
        grid.jetstream_metric_woollings(ua[:61], c["Y"], lon, c["Z"], order="zxy", device=nd)
    with pytest.raises(grid.NotServed, match="curvilinear"):
        grid.jetstream_metric_woollings(ua, np.ones((3, 3)), lon, c["Z"], order="zxy", device=nd)
    with pytest.raises(grid.NotServed, match="dimensions"):
        grid.jetstream_metric_woollings(ua[..., None], c["Y"], lon, c["Z"], order="zxy", device=nd)
    with pytest.raises(grid.NotServed, match="integer"):
        grid.jetstream_metric_woollings(ua.astype(np.int64), c["Y"], lon, c["Z"], order="zxy", device=nd)
    with pytest.raises(grid.NotServed, match="plev_units"):
        grid.jetstream_metric_woollings(ua, c["Y"], lon, c["Z"], plev_units="atm", order="zxy", device=nd)
    with pytest.raises(ValueError, match="permutation"):
        grid.jetstream_metric_woollings(ua, c["Y"], lon, c["Z"], order="tzy", device=nd)
    assert grid.jet_box(c["Y"], lon, c["Z"] / 100, 750.0, 950.0)[0].tolist() == [0, 1]     # hPa: 750 and 850 of 750, 850, 1000


def test_patch_install_names_the_three_functions():
    import types

    import fakexr
    from xclim_amd import patch

    mods = {"xclim.indices": types.ModuleType("xclim.indices"), "xclim.indices._threshold": types.ModuleType("xclim.indices._threshold"),
            "xclim.indices._synoptic": types.ModuleType("xclim.indices._synoptic")}
    origs = {"sea_ice_area": lambda siconc, areacello, thresh="15 %": "original", "sea_ice_extent": lambda siconc, areacello, thresh="15 %": "original",
             "jetstream_metric_woollings": lambda ua: "original"}
    for n, fn in origs.items():
        setattr(mods["xclim.indices._synoptic" if n.startswith("jet") else "xclim.indices._threshold"], n, fn)
        setattr(mods["xclim.indices"], n, fn)
    names = patch.install(fakexr.make_env(), mods)
    try:
        for n in grid.ADAPTED:
            assert f"xclim.indices.{n}" in names and getattr(mods["xclim.indices"], n).__wrapped__ is origs[n]
        # what is not a DataArray is forwarded without a device
        assert mods["xclim.indices"].sea_ice_area(np.ones(3), np.ones(3)) == "original"
        assert mods["xclim.indices"].jetstream_metric_woollings(np.ones(3)) == "original"
    finally:
        patch.uninstall()
    assert all(getattr(mods["xclim.indices"], n) is origs[n] for n in grid.ADAPTED)
