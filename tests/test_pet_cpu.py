"""CPU checks of potential evapotranspiration and the water budget: the numpy restatement of the kernels (tests/petcpu.py)
against the reference's own outputs (tests/golden/pet_vectors.npz, tests/golden/make_pet_golden.py), known answers of the
decimal-year day angle, the C ABI of the new entry points, and the argument errors of xclim_amd.converters (raised before
any device is touched)."""

import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import petcpu  # noqa: E402
import stridedabi as S  # noqa: E402

from xclim_amd import _capi  # noqa: E402
from xclim_amd import converters as xc  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

CASES = petcpu.golden_cases()
NAMES = [n for n, _ in CASES]
ENTRY = {"xh_solar_table": 8, "xh_pet_month_table": 8, "xh_pet_daily": 24, "xh_pet_monthly": 20}


def test_golden_cover_the_traps():
    by = dict(CASES)
    methods = {xc.METHODS[c["method"]] for c in by.values()}
    assert methods == {"BR65", "HG85", "MB05", "FAO_PM98", "TW48", "DA02"}
    for m in methods:  # every method with float32 and float64 fields
        assert {c["dtype"] for c in by.values() if xc.METHODS[c["method"]] == m} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {c["time"].calendar for c in by.values()} >= {"standard", "noleap", "360_day"}
    assert any(c["time_of_day"] == 12.0 for c in by.values())
    assert all(c["pet_dtype"] == "float64" for c in by.values())  # the reference's result dtype, float32 fields included
    assert any("wb" in c and xc.METHODS[c["method"]] in ("TW48",) for c in by.values())
    assert any("wb" in c and xc.METHODS[c["method"]] in xc.K.PET_DAILY for c in by.values())
    assert sorted(np.abs(by["br65_f32_noon"]["lat"])) == [0, 45, 45, 67, 67, 80, 80]
    assert np.isnan(by["br65_f32_noon"]["dl"]).any()  # polar day and night
    assert (by["br65_f32_noon"]["ra"] == 0).any()  # polar night
    tw = by["tw48_f32_partial"]
    assert tw["time"].day[0] != 1 and np.isnan(tw["pet"][:, 5]).all()  # partial months; a cell whose months are all <= 0 degC
    assert (by["da02_f32_partial"]["pet"][:, 2] == 0).all()  # ab < 0: ab ** 0.76 is NaN -> 0
    assert by["mb05_f32_custom"]["kw"] == {"peta": 0.0147, "petb": 0.07353}
    assert any(np.isnan(f).any() for c in by.values() for f in c["fields"].values())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    c = dict(CASES)[name]
    pet, wb = petcpu.restated(c)
    tw48 = xc.METHODS[c["method"]] == "TW48"
    f32 = c["dtype"] == np.float32
    petcpu.close(pet, c["pet"], f32, tw48)
    if "wb" in c:
        petcpu.close(wb, c["wb"], f32, tw48)
    if "ra" in c:
        ra, dl = petcpu.solar_table(xc.day_angle(c["time"], c["time_of_day"]), c["lat"])
        petcpu.close(ra, c["ra"], False)
        petcpu.close(dl, c["dl"], False)


def test_day_angle_known_answers():
    t = TimeAxis([2001, 2001, 2000, 2001], [1, 7, 12, 12], [1, 1, 31, 30], "standard")
    np.testing.assert_array_equal(xc.day_angle(t), [0.0, (2001 + 181 / 365) % 1 * 2 * np.pi,
                                                    (2000 + 365 / 366) % 1 * 2 * np.pi, (2001 + 363 / 365) % 1 * 2 * np.pi])
    np.testing.assert_allclose(xc.day_angle(t.subset(slice(1, 2)), 12.0), [2 * np.pi * 181.5 / 365], rtol=1e-12)
    t360 = TimeAxis([2001, 2001], [1, 7], [1, 1], "360_day")
    np.testing.assert_allclose(xc.day_angle(t360), [0.0, 2 * np.pi * 180 / 360], rtol=1e-12)
    np.testing.assert_allclose(xc.day_angle(TimeAxis([2000], [3], [1], "noleap")), [2 * np.pi * 59 / 365], rtol=1e-12)
    np.testing.assert_allclose(xc.day_angle(TimeAxis([2000], [3], [1], "all_leap")), [2 * np.pi * 60 / 366], rtol=1e-12)
    np.testing.assert_allclose(xc.day_angle(TimeAxis([1900], [3], [1], "julian")), [2 * np.pi * 60 / 366], rtol=1e-12)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_entry_point_header_ctypes_and_exports(name):
    lib = _capi.load_library()
    assert hasattr(lib, name)
    assert len(S.header_declarations()[name]) == ENTRY[name] == len(_capi.SIGNATURES[name])


def test_entry_points_reject_bad_arguments():
    """Argument errors come back as codes with a NULL context (no device is touched)."""
    lib = _capi.load_library()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(64)  # never dereferenced: the checks fail first
    assert lib.xh_solar_table(null, 10, 3, some, some, 1361.0, some, null) == _capi.XH_ERR_ARG
    assert lib.xh_pet_month_table(null, 10, 3, some, 2, some, 0, some) == _capi.XH_ERR_ARG
    assert lib.xh_pet_daily(null, 10, 4, 4, 0, 0, *([some] * 10), some, 3, some, 0.1, 0.1, some, null, 4) == _capi.XH_ERR_ARG
    assert lib.xh_pet_monthly(null, 10, 4, 4, 4, 0, some, some, some, some, 1, 0, some, some, some, 3, some, some, null,
                              4) == _capi.XH_ERR_ARG


def _f(T=40, C=3, dtype=np.float32, v=280.0):
    return np.full((T, C), v, dtype)


def test_host_argument_errors():
    t = TimeAxis.daily("2001-01-01", 40)
    x = _f()
    lat = np.array([10.0, 20.0, 30.0])
    with pytest.raises(NotImplementedError, match="'bogus' method is not implemented"):
        xc.potential_evapotranspiration(x, x, time=t, lat=lat, method="bogus")
    with pytest.raises(ValueError, match="Wind speed is required for Allen98 method"):
        xc.potential_evapotranspiration(x, x, hurs=x, rsds=x, rsus=x, rlds=x, rlus=x, time=t, method="FAO_PM98")
    with pytest.raises(ValueError, match="needs tasmax"):
        xc.potential_evapotranspiration(x, time=t, lat=lat, method="HG85")
    with pytest.raises(ValueError, match="needs tas, or tasmin and tasmax"):
        xc.potential_evapotranspiration(tasmin=x, time=t, lat=lat, method="TW48")
    with pytest.raises(ValueError, match="needs pr"):
        xc.potential_evapotranspiration(x, x, time=t, lat=lat, method="DA02")
    with pytest.raises(ValueError, match="differs"):
        xc.potential_evapotranspiration(x, _f(C=4), time=t, lat=lat)
    with pytest.raises(ValueError, match="does not broadcast"):
        xc.potential_evapotranspiration(x, x, time=t, lat=np.ones(5), device=object())
    with pytest.raises(ValueError, match="rows"):
        xc.potential_evapotranspiration(x, x, time=t.subset(slice(0, 30)), lat=lat)
    gappy = TimeAxis(np.r_[t.year[:10], t.year[11:]], np.r_[t.month[:10], t.month[11:]], np.r_[t.day[:10], t.day[11:]])
    with pytest.raises(xc.NotServed, match="gap-free"):
        xc.potential_evapotranspiration(x[1:], x[1:], time=gappy, lat=lat, device=object())
    monthly = TimeAxis([2001] * 12, np.arange(1, 13), np.ones(12, int))
    with pytest.raises(xc.NotServed):
        xc.potential_evapotranspiration(x[:12], x[:12], time=monthly, lat=lat, method="TW48", device=object())
    with pytest.raises(xc.NotServed, match="DA02"):
        xc.water_budget(x, x, x, time=t, lat=lat, method="DA02", device=object())
    with pytest.raises(xc.NotServed, match="calendar"):
        xc.potential_evapotranspiration(x, x, time=TimeAxis(t.year, t.month, t.day, "weird"), lat=lat, device=object())


def test_months_cover_whole_calendar_months():
    """The monthly tables are built over whole months even when the data start and end inside one (_get_D_from_M)."""
    t = TimeAxis.daily("2000-02-10", 60)
    seg, months, days, dseg, ndays = xc._months(t)
    assert list(zip(months.year, months.month)) == [(2000, 2), (2000, 3), (2000, 4)]
    np.testing.assert_array_equal(seg, [0, 20, 51, 60])
    np.testing.assert_array_equal(ndays, [29, 31, 30])
    assert len(days) == 90 and days.day[0] == 1 and days.day[-1] == 30
    np.testing.assert_array_equal(dseg, [0, 29, 60, 90])
