"""CPU checks of the winter-chill indices: the numpy restatement (tests/chillcpu.py) against the reference's own outputs
(tests/golden/chill_vectors.npz, tests/golden/make_chill_golden.py) and known answers, the C ABI of the two new entry
points, and the host logic of xclim_amd.chill that runs before any device is touched (indexer -> row_sel, hourly period
offsets and expected counts, argument errors)."""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import chillcpu  # noqa: E402
import stridedabi as S  # noqa: E402

from xclim_amd import _capi  # noqa: E402
from xclim_amd import chill  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "chill_vectors.npz"))
CASES = [str(c) for c in GOLD["cases"]]
KIND = {c: str(GOLD[f"{c}/meta"][4]) for c in CASES}
HOURLY = [c for c in CASES if KIND[c] == "hourly"]
DAILY = [c for c in CASES if KIND[c] == "daily"]
K2C = 273.15
EDGES = (1.4, 2.4, 9.1, 12.4, 15.9, 17.9)
# float64 marches against the reference's float64 run: the project's tolerance for them (KBDI / DF, PET); the reference in
# extended precision differs from its own float64 run by 8e-15 on these cases, so 1e-12 leaves room for a 1-ulp exp
RTOL = 1e-12


def decode(q, dtype):
    """int16 tenths, -32768 = NaN (tests/golden/make_chill_golden.py: decode); float64 members are stored as they are."""
    if q.dtype != np.int16:
        return np.asarray(q, dtype)
    return np.where(q == -32768, np.nan, q.astype(np.float64) / 10).astype(dtype)


class Case:
    def __init__(self, name):
        g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
        self.name, self.g = name, g
        self.dtype = np.dtype(str(g["meta"][0]))
        self.units, self.freq, self.kind = str(g["meta"][1]), str(g["meta"][2]), str(g["meta"][4])
        self.indexer = {k: (tuple(v) if k == "date_bounds" else v) for k, v in json.loads(str(g["meta"][3])).items()}
        y, m, d, n = (int(v) for v in g["start"])
        self.time = TimeAxis.daily(f"{y:04d}-{m:02d}-{d:02d}", n)
        self.seg = g["seg"]                       # DAY offsets of the periods
        self.sel = g["sel"].astype(bool) if "sel" in g else None
        if self.kind == "hourly":
            q = GOLD[f"{g['tas_of']}/tas"] if "tas_of" in g else g["tas"]
            self.tas = decode(q, self.dtype)
            self.cells = g["delta_cells"] if "delta_cells" in g else np.arange(self.tas.shape[1])
        else:
            self.tasmin, self.tasmax = decode(g["tasmin"], self.dtype), decode(g["tasmax"], self.dtype)
            self.lat, self.dl, self.hourly = g["lat"], g["dl"], g["hourly"]
            self.cells = np.arange(self.tasmin.shape[1])
        self.add_K, self.sub_C = (0.0, K2C) if self.units == "K" else (K2C, 0.0)

    def rows_sel(self):
        return None if self.sel is None else np.repeat(self.sel, 24)

    def kelvin(self, tas):
        """The widened field in K, as the device forms it: ``(double) t + add_K``."""
        return np.asarray(tas, np.float64) + self.add_K

    def celsius(self, tas):
        """The field in degC in its own dtype, as the device forms it: ``t - (dtype) sub_C``."""
        tas = np.asarray(tas)
        return tas - tas.dtype.type(self.sub_C)


_CACHE = {}


def golden_case(name) -> Case:
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


def check_delta(got, exp, what="delta"):
    """A float64 march against the reference's float64 run: the same releases, and every value to RTOL."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert not np.isnan(got).any(), f"{what}: NaN in delta"
    np.testing.assert_array_equal(got > 0, exp > 0, err_msg=f"{what}: release pattern")
    np.testing.assert_allclose(got, exp, rtol=RTOL, atol=0, err_msg=what)


def check_sums(got, exp, what="cp"):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_allclose(got, exp, rtol=RTOL, atol=0, equal_nan=True, err_msg=what)


def nan_empty(cp, c: Case):
    """Chill portions with NaN for the periods without a selected day (what the golden file records there)."""
    cp = np.array(cp, np.float64)
    if c.sel is not None:
        for p, (a, b) in enumerate(zip(c.seg[:-1], c.seg[1:])):
            if not c.sel[a:b].any():
                cp[p] = np.nan
    return cp


def test_golden_cover_the_traps():
    assert {"known_linspace", "known_units", "known_equator", "seasonal_f64", "seasonal_f32", "date_bounds_3y", "month_djf_2y",
            "nan_hours", "utah_edges_f64", "utah_edges_f32", "daily_f64", "daily_f32"} <= set(CASES)
    assert float(GOLD["min_margin"]) >= 1e-9
    for name in CASES:
        assert float(GOLD[f"{name}/margin"]) >= 1e-9, name   # no release hangs on the last bit of exp
    c = golden_case("seasonal_f64")
    assert c.tas.shape == (24 * 210, 64) and len(c.seg) == 3
    c = golden_case("date_bounds_3y")
    assert c.freq == "YS-JUL" and len(c.seg) == 4 and c.indexer == {"date_bounds": ("09-01", "03-30")}
    c = golden_case("month_djf_2y")
    assert c.indexer == {"month": [12, 1, 2]} and len(c.seg) == 3
    inner = c.sel[c.seg[0]:c.seg[1]]
    assert inner[0] and inner[-1] and not inner.all()   # the dropped months lie INSIDE the period: the state carries
    c = golden_case("nan_hours")
    t = c.tas
    assert np.isnan(t[:, 5]).all() and np.isnan(t[0, 2]) and np.isnan(t[24 * c.seg[1], 3]) and np.isnan(t[300, 1])
    for name, dt in (("utah_edges_f64", np.float64), ("utah_edges_f32", np.float32)):
        t = golden_case(name).tas
        assert t.dtype == dt
        for e in EDGES:
            assert (t == dt(e)).any() and (t == np.nextafter(dt(e), dt(100))).any() and (t == np.nextafter(dt(e), dt(-100))).any()
    for name in ("daily_f64", "daily_f32"):
        c = golden_case(name)
        assert set(np.abs(c.lat)) == {0.0, 45.0, 67.0, 80.0} and (c.lat < 0).any()
        assert np.isnan(c.dl).any() and np.isnan(c.tasmin[17, 1])
        assert np.isnan(c.hourly[16 * 24 + 20:17 * 24, 1]).all() and not np.isnan(c.hourly[16 * 24, 1])  # the NaN reaches the night before
    c = golden_case("seasonal_f32")
    assert c.g["gap32"].shape == c.g["cp"].shape and c.g["delta32"].dtype == np.float32


def test_known_answers():
    """tests/test_indices.py:375-399 and tests/test_helpers.py:302-338 of the reference, through the restatement."""
    tas = np.linspace(0, 15, 120 * 24)[:, None] + K2C
    cp, _, _ = chillcpu.portions(tas, np.array([0, 2880]))
    np.testing.assert_array_almost_equal(cp[0], [72.2441765], decimal=7)
    v = np.array(10 * [1.1] + 15 * [2.0] + 20 * [5.6] + 10 * [16.0] + 5 * [20.0] + 12 * [np.nan])[:, None] + K2C
    assert chillcpu.units(v - K2C, np.array([0, 72]))[0, 0] == 0.5 * 15 + 20 - 0.5 * 10 - 5
    assert chillcpu.units(v - K2C, np.array([0, 72]), positive_only=True)[0, 0] == 0.5 * 15 + 20 - 0.5 * 3
    c = golden_case("known_equator")
    h = chillcpu.hourly_temperature(c.tasmin, c.tasmax, c.dl)
    exp = [0.0, 3.90180644, 7.65366865, 11.11140466, 14.14213562, 16.62939225, 18.47759065, 19.61570561, 20.0, 19.61570561,
           18.47759065, 16.62939225, 14.14213562, 10.32039099, 8.0848137, 6.49864636, 5.26831939, 4.26306907, 3.41314202,
           2.67690173, 2.02749177, 1.44657476, 0.92107141, 0.44132444]
    np.testing.assert_allclose(h[:, 0], exp)


@pytest.mark.parametrize("name", HOURLY)
def test_restatement_matches_reference_hourly(name):
    c = golden_case(name)
    seg = 24 * c.seg
    cp, delta, valid = chillcpu.portions(c.kelvin(c.tas), seg, c.rows_sel())
    check_delta(delta[:, c.cells], c.g["delta"])
    check_sums(nan_empty(cp, c), c.g["cp"])
    if "cu" in c.g:
        np.testing.assert_array_equal(chillcpu.units(c.celsius(c.tas), seg), c.g["cu"])
        np.testing.assert_array_equal(chillcpu.units(c.celsius(c.tas), seg, positive_only=True), c.g["cu_pos"])


@pytest.mark.parametrize("name", DAILY)
def test_restatement_matches_reference_daily(name):
    c = golden_case(name)
    li = np.arange(len(c.lat))
    h = chillcpu.hourly_temperature(c.tasmin, c.tasmax, c.dl[:, li])
    np.testing.assert_array_equal(np.isnan(h), np.isnan(c.hourly))
    np.testing.assert_allclose(h, c.hourly, rtol=RTOL, atol=0, equal_nan=True)
    seg = 24 * c.seg
    cp, delta, _ = chillcpu.portions(c.kelvin(c.hourly), seg)
    check_delta(delta, c.g["delta"])
    check_sums(cp, c.g["cp"])
    np.testing.assert_array_equal(chillcpu.units(c.celsius(c.hourly), seg), c.g["cu"])
    np.testing.assert_array_equal(chillcpu.units(c.celsius(c.hourly), seg, positive_only=True), c.g["cu_pos"])


def test_nan_rule_of_the_dynamic_model():
    """A NaN hour makes E NaN to the end of the period: delta is 0 from there on (never NaN) and the sum is that of the hours
    before it; a NaN on the period's first hour changes nothing (inter_E starts at 0 whatever the temperature)."""
    c = golden_case("nan_hours")
    d = c.g["delta"]
    assert not np.isnan(d).any()
    assert (d[300:24 * c.seg[1], 1] == 0).all() and (d[:300, 1] > 0).any()
    assert (d[24 * c.seg[1]:, 1] > 0).any()       # the next period starts afresh
    assert (d[:, 5] == 0).all() and (c.g["cp"][:, 5] == 0).all()
    assert (d[:24 * c.seg[1], 2] > 0).any() and (d[24 * c.seg[1]:, 3] > 0).any()


# ---- the C ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nargs", [("xh_chill_hourly", 18), ("xh_chill_daily", 21)])
def test_entry_point_header_ctypes_and_exports(name, nargs):
    lib = _capi.load_library()
    assert hasattr(lib, name)
    decl = S.header_declarations()[name]
    sig = _capi.SIGNATURES[name]
    assert len(decl) == nargs == len(sig)
    for (d, _), s in zip(decl, sig):   # pointers, 64-bit sizes, ints and doubles line up one to one
        assert S.is_ctypes_kind(d, s) and (s is ctypes.c_void_p or "*" not in d), (name, d, s)


def test_entry_points_reject_bad_arguments():
    """Argument errors come back as codes before anything is launched (a NULL context touches no device)."""
    lib = _capi.load_library()
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(64)  # never dereferenced: the checks fail first
    assert lib.xh_chill_hourly(null, 48, 4, 4, 0, some, 24, 1, some, null, 0.0, K2C, 0, some, null, null, null, 4) == _capi.XH_ERR_ARG
    assert lib.xh_chill_daily(null, 2, 4, 4, 0, some, some, some, 1, some, 1, some, null, 0.0, K2C, 0, some, null, null, null,
                              4) == _capi.XH_ERR_ARG


# ---- host logic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["date_bounds_3y", "month_djf_2y", "seasonal_f64", "nan_hours"])
def test_indexer_to_row_sel_and_hourly_periods(name):
    """The host's selection and period offsets against the generator's own restatement of select_time / resample."""
    c = golden_case(name)
    np.testing.assert_array_equal(chill.hourly_segments(c.time, c.freq), 24 * c.seg)
    rs = chill.row_selection(c.time, **c.indexer)
    if c.sel is None:
        assert rs is None
    else:
        assert rs.shape == (24 * len(c.time),) and rs.dtype == bool
        np.testing.assert_array_equal(rs, np.repeat(c.sel, 24))
        np.testing.assert_array_equal(chill.day_selection(c.time, **c.indexer), c.sel)


def test_hourly_expected_counts():
    t = TimeAxis.daily("2001-01-01", 730)
    np.testing.assert_array_equal(chill.hourly_expected_count(t, "YS"), [24 * 365, 24 * 365])
    np.testing.assert_array_equal(chill.hourly_expected_count(t, "YS", month=[12, 1, 2]), [24 * 90, 24 * 90])
    # the reference's indicator test (tests/test_atmos.py:84-103): four calendar years give five July-to-June seasons, and the
    # first and the last hold only a part of the selected winter, so MissingAny makes them NaN
    t = TimeAxis.daily("1990-01-01", 1461)
    idx = {"date_bounds": ("09-01", "03-30")}
    seg, _ = t.segments("YS-JUL")
    sel = chill.day_selection(t, **idx)
    have = 24 * np.array([sel[a:b].sum() for a, b in zip(seg[:-1], seg[1:])])
    expected = chill.hourly_expected_count(t, "YS-JUL", **idx)
    np.testing.assert_array_equal(expected, 24 * np.array([211, 211, 212, 211, 211]))
    np.testing.assert_array_equal(have != expected, [True, False, False, False, True])


def test_host_argument_errors():
    t = TimeAxis.daily("2001-01-01", 3)
    x = np.full((72, 2), 280.0)
    with pytest.raises(ValueError, match="24 \\* 3 days = 72 expected"):
        chill.chill_portions(x[:60], t)
    with pytest.raises(ValueError, match="72 expected"):
        chill.chill_units(np.full((73, 2), 5.0), t)
    with pytest.raises(ValueError, match="units must be one of"):
        chill.chill_portions(x, t, units="degF")
    with pytest.raises(TypeError, match="unknown indexer"):
        chill.chill_portions(x, t, hour=3)
    with pytest.raises(ValueError, match="Only one method of indexing"):
        chill.chill_portions(x, t, month=[1], season="DJF")
    with pytest.raises(TypeError, match="daily TimeAxis"):
        chill.chill_portions(x, None)
    with pytest.raises(ValueError, match="mask_missing=False"):
        chill.chill_portions(x, t, keep=True, mask_missing=True)
    d = np.full((3, 2), 280.0)
    with pytest.raises(chill.NotServed, match="infill_polar_days"):
        chill.make_hourly_temperature(d, d + 5, [10.0, 20.0], t, infill_polar_days=True)
    with pytest.raises(ValueError, match="differs"):
        chill.make_hourly_temperature(d, np.full((3, 3), 285.0), [10.0, 20.0], t)
    with pytest.raises(ValueError, match="time has 3 rows"):
        chill.chill_portions_from_daily(np.full((4, 2), 280.0), np.full((4, 2), 285.0), [10.0, 20.0], t)
    with pytest.raises(ValueError, match="does not broadcast"):
        chill.chill_units_from_daily(d, d + 5, [1.0, 2.0, 3.0], t)
    gappy = TimeAxis([2001, 2001, 2001], [1, 1, 1], [1, 2, 4])
    with pytest.raises(chill.NotServed):
        chill.chill_from_daily(d, d + 5, 10.0, gappy)


def test_adapter_forward_decisions():
    """What the adapter hands to the reference's original, decided before any device work."""
    for bad in (np.ones((3, 30), np.float16), np.ones((3, 30), np.int64), np.ones((0, 30)), np.ones((3, 0), np.float32),
                np.float64(280.0)):
        with pytest.raises(chill._Forward):
            chill.chill_portion_one_season(bad)
    seen = []
    ad = chill.make_adapters(lambda a: seen.append(a.dtype) or "forwarded")["_chill_portion_one_season"]
    assert ad(np.ones((2, 5), np.float16)) == "forwarded" and seen == [np.dtype(np.float16)]
