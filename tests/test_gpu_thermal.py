"""The thermal-comfort unit on the GPU, stage by stage against the numpy restatement (tests/thermalcpu.py), which
tests/test_thermal_cpu.py holds against the reference's own code.

Tolerances (none taken from what the device gives):
  csza   the same zero / non-zero / NaN pattern and |d| <= 1e-12: the generator of the cases keeps |tan lat tan dec| at least 1e-6
         from 1, where acos amplifies a few 2^-53 by at most 707, so the hour angles are good to about 3e-13.
  mrt    the restatement at the DEVICE's csza: |d| <= 1e-12 mrt sum|terms| / |S|, S the bracket under the fourth root.
  utci   the restatement at the device's mrt: |d| <= 1e-12 scale, scale the polynomial of the absolute values with |dt| replaced
         by |mrt_C| + |tas_C| (any order of 211 terms of at most seven roundings stays below 5e-14 scale); float32 fields: the
         float64 result rounded once, one float32 ulp more.  The NaN pattern is identical.
  e_sat  1e-12 relative; one float32 ulp more for float32 fields.
Measured on the MI355X (worst over the module): csza |d| 9.6e-14; mrt 2.3e-4 of its bound; utci 1.3e-3 of its bound for float64
fields and 0.5 for float32 fields (the one rounding to float32); e_sat inside 1e-12.  End to end: MEASURED below."""
import numpy as np
import pytest

import thermalcpu as TC
from poisoned import poisoned_outputs, unwritten  # noqa: F401
from xclim_amd import _capi, thermal
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

FRAMES = {"daily3": (None, 3), "hourly72": (thermal.SubDaily(24, 1800), 3), "3hourly24": (thermal.SubDaily(8), 3), "hourly24": (thermal.SubDaily(24), 1)}


def _frame(name, cal="standard", start="2001-06-20"):
    sub, days = FRAMES[name]
    t = TimeAxis.daily(start, days, cal)
    return t, sub, days * (sub.steps_per_day if sub else 1)


def _grid(C, rng):
    """Latitudes from pole to pole (polar day and night at the June solstice) and longitudes around the globe.  From 65 cells on,
    twelve cells just equatorward of each polar circle, where the June night (north) is shorter than a three-hour interval, at
    longitudes that put local midnight early, in the middle and late in the interval 21:00-24:00 UTC: the three cases of an
    interval across midnight, among them the one with two sunlit parts."""
    if C < 65:
        return np.concatenate([[66.0], np.linspace(-89, 89, max(C - 1, 0))])[:C], rng.uniform(-180, 360, C)
    band = np.repeat([65.5, 66.0, 66.4], 4)
    lat = np.concatenate([np.linspace(-89, 89, C - 24), band, -band])
    lon = np.concatenate([rng.uniform(-180, 360, C - 24), np.tile([5.0, 16.0, 27.0, 38.0], 6)])
    return lat, lon


def _safe(rows, latr):
    tt = np.abs(np.tan(latr)[None, :] * rows[_capi.THERMAL_ROWS["tan_dec"]][:, None])
    return np.abs(tt - 1) > 1e-6


def _weather(R, C, rng, dtype, nan=True):
    f = {"tas": rng.uniform(225, 325, (R, C)), "hurs": rng.uniform(3, 100, (R, C)), "sfcWind": rng.uniform(0, 18, (R, C)),
         "rsds": np.where(rng.random((R, C)) < 0.15, rng.uniform(-5, 0, (R, C)), rng.uniform(0, 1000, (R, C))),
         "rlds": rng.uniform(150, 450, (R, C))}
    f["rsus"] = 0.2 * np.abs(f["rsds"])
    f["rlus"] = f["rlds"] + rng.uniform(0, 120, (R, C))
    f["sfcWind"].flat[:: 7] = 0.5   # exactly the lower validity bound, which is inside
    if nan:
        for k, n in enumerate(f):
            f[n].flat[k * 3 + 1:: 41] = np.nan
    return {k: v.astype(dtype) for k, v in f.items()}


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _check_csza(got, exp):
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(got == 0, exp == 0)
    d = np.nanmax(np.abs(got - exp), initial=0.0)
    print("csza worst |d|", d)
    assert d <= 1e-12


def _check_mrt(got, cs, rows, f):
    exp, S, mag = TC.mrt(cs, rows[_capi.THERMAL_ROWS["inv_d2"]], f["rsds"], f["rsus"], f["rlds"], f["rlus"])
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    with np.errstate(all="ignore"):
        tol = 1e-12 * exp * mag / np.abs(S)
    print("mrt worst |d| / tol", np.max(np.abs(got - exp)[ok] / tol[ok], initial=0.0))
    assert np.all(np.abs(got - exp)[ok] <= tol[ok])


def _check_utci(got, f, mrt_k, dtype, **kw):
    exp, scale = TC.utci(f["tas"], f["hurs"], f["sfcWind"], mrt_k, **kw)
    assert got.dtype == dtype
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert exp.size < 100 or ok.mean() > 0.2   # (the fields are drawn so that the validity box holds a good part of them)
    tol = 1e-12 * scale + (_ulp32(exp) if dtype == np.float32 else 0.0)
    print("utci worst |d| / tol", np.max(np.abs(got.astype(np.float64) - exp)[ok] / tol[ok], initial=0.0))
    assert np.all(np.abs(got.astype(np.float64) - exp)[ok] <= tol[ok])


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("cal", ["standard", "noleap"])
def test_csza_every_branch(dev, frame, cal):
    t, sub, R = _frame(frame, cal)
    rng = np.random.default_rng(5)
    lat, lon = _grid(130, rng)
    rows = thermal.solar_rows(t, subdaily=sub)
    latr = TC.wrap(lat * (np.pi / 180))
    assert _safe(rows, latr).all()
    for stat, kstat in (("average", "sunlit"), ("instant", "instant")):
        got = thermal.cosine_of_solar_zenith_angle(t, lat, lon, stat=stat, subdaily=sub, device=dev)
        exp, br = TC.csza(rows, latr, lon * (np.pi / 180), "subdaily" if sub else "daily", kstat)
        assert got.shape == (R, 130) and got.dtype == np.float64
        _check_csza(got, exp)
        if frame == "3hourly24" and stat == "average":
            assert set(br.ravel()) == set(range(10)), sorted(set(br.ravel()))


@pytest.mark.parametrize("C", [1, 65, 130])
@pytest.mark.parametrize("frame", ["daily3", "3hourly24", "hourly72"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_utci_from_seven_fields(dev, C, frame, dtype):
    t, sub, R = _frame(frame)
    rng = np.random.default_rng(C + R)
    lat, lon = _grid(C, rng)
    f = _weather(R, C, rng, dtype)
    res = thermal.universal_thermal_climate_index(**f, lat=lat, lon=lon, time=t, subdaily=sub, outputs=("utci", "mrt"), device=dev)
    rows = thermal.solar_rows(t, subdaily=sub)
    cs = thermal.cosine_of_solar_zenith_angle(t, lat, lon, subdaily=sub, device=dev)
    _check_mrt(res["mrt"], cs, rows, f)
    _check_utci(res["utci"], f, res["mrt"], dtype)
    # each output alone is the same numbers
    alone = thermal.universal_thermal_climate_index(**f, lat=lat, lon=lon, time=t, subdaily=sub, device=dev)
    np.testing.assert_array_equal(alone, res["utci"])
    rad = {k: f[k] for k in ("rsds", "rsus", "rlds", "rlus")}
    np.testing.assert_array_equal(thermal.mean_radiant_temperature(**rad, lat=lat, lon=lon, time=t, subdaily=sub, device=dev), res["mrt"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("flags", [dict(mask_invalid=True, wind_cap_min=True), dict(mask_invalid=False, wind_cap_min=False),
                                   dict(mask_invalid=False, wind_cap_min=True)])
def test_utci_with_mrt_given_and_the_flags(dev, dtype, flags):
    rng = np.random.default_rng(11)
    R, C = 24, 130
    f = _weather(R, C, rng, dtype)
    f = {k: f[k] for k in ("tas", "hurs", "sfcWind")}
    f["tas"] = rng.uniform(240, 320, (R, C)).astype(dtype)
    mrt = (f["tas"].astype(np.float64) + rng.uniform(-33, 33, (R, C))).astype(dtype)
    mrt.flat[5::37] = np.nan
    # both sides of each of the six bounds, in the field's dtype
    f["tas"][0, :4] = np.array([223.1, 223.2, 323.1, 323.2], dtype)
    f["sfcWind"][1, :5] = np.array([0.49, 0.5, 0.51, 16.99, 17.01], dtype)
    mrt[2, :4] = f["tas"][2, :4] + np.array([-30.1, -29.9, 29.9, 30.1], dtype)
    f["tas"][1:3, :5], f["sfcWind"][0, :5], f["sfcWind"][2, :5], f["hurs"][:3, :5] = 290, 3, 3, 50
    mrt[:2, :5] = f["tas"][:2, :5] + 1
    mrt[2, :4] = f["tas"][2, :4] + np.array([-30.1, -29.9, 29.9, 30.1], dtype)
    got = thermal.universal_thermal_climate_index(**f, mrt=mrt, device=dev, **flags)
    _check_utci(got, f, mrt, dtype, **flags)
    if flags["mask_invalid"]:
        assert np.isnan(got[0, 0]) and not np.isnan(got[0, 1]) and not np.isnan(got[0, 2]) and np.isnan(got[0, 3])
        assert not np.isnan(got[1, :4]).any() and np.isnan(got[1, 4])   # (the wind floor lifts 0.49 to 0.5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", list(_capi.ESAT_METHODS))
def test_esat(dev, dtype, method):
    rng = np.random.default_rng(3)
    tas = rng.uniform(200, 330, (3, 130)).astype(dtype)
    tas[0, :6] = np.array([250.15, 250.17, 273.14, 273.16, 273.17, np.nan], dtype)
    for kw in ({}, {"ice_thresh": 273.15}, {"ice_thresh": 250.16, "interp_power": 2, "water_thresh": 273.16},
               {"ice_thresh": 258.15, "interp_power": 1.5}):
        got = thermal.saturation_vapor_pressure(tas, method=method, device=dev, **kw)
        exp = TC.esat(tas, method, kw.get("ice_thresh"), kw.get("interp_power"), kw.get("water_thresh", 273.15))
        assert got.dtype == dtype and np.array_equal(np.isnan(got), np.isnan(exp)) and np.isnan(got[0, 5])
        ok = ~np.isnan(exp)
        tol = 1e-12 * np.abs(exp) + (_ulp32(exp) if dtype == np.float32 else 0.0)
        assert np.all(np.abs(got.astype(np.float64) - exp)[ok] <= tol[ok]), (method, kw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_padded_row_views_keep_the_padding(dev, dtype):
    """ld > C and ld_out > C: the padding of the fields holds values that would show (1e30) and the padding of the outputs holds the
    poison of the module's fixture before and after."""
    t, sub, R = _frame("3hourly24")
    C, ld, ldo = 65, 72, 80
    rng = np.random.default_rng(8)
    lat, lon = _grid(C, rng)
    f = _weather(R, C, rng, dtype, nan=False)
    wide = {}
    for k, v in f.items():
        w = np.full((R, ld), 1e30, dtype)
        w[:, :C] = v
        wide[k] = dev.to_device(w)
    outs = {"utci": dev.empty((R, ldo), dtype), "mrt": dev.empty((R, ldo), np.float64), "csza": dev.empty((R, ldo), np.float64)}
    rows = thermal.solar_rows(t, subdaily=sub)
    latr, lonr = TC.wrap(lat * (np.pi / 180)), lon * (np.pi / 180)
    K.thermal_comfort(dev, wide, rows, latr, lonr, mode="subdaily", outputs=("utci", "mrt", "csza"), C_=C, ld=ld, outs=outs, ld_out=ldo)
    dense = K.thermal_comfort(dev, {k: dev.to_device(v) for k, v in f.items()}, rows, latr, lonr, mode="subdaily", outputs=("utci", "mrt", "csza"))
    for k, o in outs.items():
        got = o.get()
        assert unwritten(got[:, C:]).all(), k
        assert not unwritten(got[:, :C]).any(), k
        np.testing.assert_array_equal(got[:, :C], dense[k].get())
    e = dev.empty((R, ldo), dtype)
    K.esat(dev, wide["tas"], "its90", C_=C, ld=ld, out=e, ld_out=ldo)
    got = e.get()
    assert unwritten(got[:, C:]).all() and not unwritten(got[:, :C]).any()
    np.testing.assert_array_equal(got[:, :C], K.esat(dev, dev.to_device(f["tas"]), "its90").get())


def test_argument_errors(dev):
    x = dev.to_device(np.full((3, 4), 290.0, np.float32))
    with pytest.raises(Exception, match="mrt_out with mrt_in"):
        K.thermal_comfort(dev, {"tas": x, "hurs": x, "sfcWind": x, "mrt": x}, outputs=("utci", "mrt"))
    with pytest.raises(Exception, match="rsds, rsus, rlds and rlus"):
        K.thermal_comfort(dev, {"tas": x, "hurs": x, "sfcWind": x}, outputs=("utci",))
    with pytest.raises(Exception, match="solar tables"):
        K.thermal_comfort(dev, {"rsds": x, "rsus": x, "rlds": x, "rlus": x}, outputs=("mrt",))
    with pytest.raises(Exception, match="solar tables"):   # sub-daily rows without lon
        K.thermal_comfort(dev, {}, np.zeros((_capi.THERMAL_NROW, 3)), np.zeros(4), None, mode="subdaily", outputs=("csza",), shape=(3, 4, False))


# ---- end to end against the reference's recorded chain (tests/golden/thermal_chain_*.npz) and its tests' known answers -------------
from test_thermal_cpu import CHAIN, GRID, KNOWN, chain_case  # noqa: E402

# the worst relative difference measured on the MI355X (mrt: |d| / mrt; utci: |d| / scale, the polynomial of magnitudes), by dtype of
# the fields; ten times each is asserted, as for the distribution fits.  float32 fields differ by the reference's float32 route
# (0.5 * rlds in float32, the float32 exp, numba's float32 _utci), which the unit does not reproduce.
MEASURED = {"float64": {"mrt": 1.9e-14, "utci": 4.0e-15}, "float32": {"mrt": 1.5e-8, "utci": 1.55e-6}}


def _worst(kind, dt, got, exp, ref_scale):
    assert np.array_equal(np.isnan(got), np.isnan(exp)) or (kind == "utci" and dt == np.float32)
    ok = ~np.isnan(got) & ~np.isnan(exp)
    w = float(np.max(np.abs(got.astype(np.float64) - exp.astype(np.float64))[ok] / ref_scale[ok]))
    print(f"end to end {kind} {np.dtype(dt).name}: worst relative difference {w:.3e}")
    bound = MEASURED[np.dtype(dt).name][kind]
    assert w <= 10 * bound, (w, bound)


@pytest.mark.parametrize("path", CHAIN, ids=[p.split("thermal_chain_")[1][:-4] for p in CHAIN])
@pytest.mark.parametrize("stat", ["sunlit", "instant"])
def test_end_to_end_against_the_recorded_reference(dev, path, stat):
    """Measured worst relative differences on the MI355X: see MEASURED above and DESIGN.md section 3."""
    z, t, sub, dt = chain_case(path)
    f = {k: z[k] for k in ("tas", "hurs", "sfcWind", "rsds", "rsus", "rlds", "rlus")}
    res = thermal.universal_thermal_climate_index(**f, stat=stat, lat=GRID[0], lon=GRID[1], time=t, subdaily=sub, outputs=("utci", "mrt"), device=dev)
    cs = thermal.cosine_of_solar_zenith_angle(t, GRID[0], GRID[1], stat="average" if stat == "sunlit" else "instant", subdaily=sub, device=dev)
    _check_csza(cs, z[f"csza_{stat}"])
    scale = TC.utci(f["tas"], f["hurs"], f["sfcWind"], z[f"mrt_{stat}"])[1]
    _worst("mrt", dt, res["mrt"], z[f"mrt_{stat}"], np.abs(z[f"mrt_{stat}"]))
    _worst("utci", dt, res["utci"], z[f"utci_{stat}"], scale)
    if stat == "sunlit":
        for tag, kw in (("given", {}), ("given_cap_nomask", dict(mask_invalid=False, wind_cap_min=True))):
            got = thermal.universal_thermal_climate_index(f["tas"], f["hurs"], f["sfcWind"], mrt=z["mrt_in"], device=dev, **kw)
            _worst("utci", dt, got, z[f"utci_{tag}"], TC.utci(f["tas"], f["hurs"], f["sfcWind"], z["mrt_in"], **kw)[1])


def test_known_answers_on_the_device(dev):
    for a in KNOWN["test_universal_thermal_climate_index"]:
        x = lambda v: np.array([[v]])   # noqa: E731
        got = thermal.universal_thermal_climate_index(x(a["tas"]), x(a["hurs"]), x(a["sfcWind_kmh"] * (1 / 3.6)), mrt=x(a["mrt"]),
                                                      wind_cap_min=a["wind_cap_min"], device=dev)[0, 0]
        assert np.isnan(got) if a["expected"] is None else abs(got - a["expected"]) <= a["rtol"] * abs(a["expected"])
    for a in KNOWN["test_mean_radiant_temperature"]:
        got = thermal.mean_radiant_temperature(*(np.array([[a[k]]]) for k in ("rsds", "rsus", "rlds", "rlus")), stat=a["stat"], lat=[a["lat"]],
                                               lon=[a["lon"]], time=TimeAxis.daily(a["start"], 1, "standard"), device=dev)
        np.testing.assert_allclose(got, a["expected"], rtol=a["rtol"])
    for a in KNOWN["test_cosine_of_solar_zenith_angle"]:
        got = thermal.cosine_of_solar_zenith_angle(TimeAxis.daily(a["start"], a["days"], a["calendar"]), a["lat"], a["lon"],
                                                   subdaily=thermal.SubDaily(a["steps_per_day"], a["offset_seconds"]), device=dev)
        np.testing.assert_allclose(got[a["rows"][0]:a["rows"][1]], a["expected"], rtol=a["rtol"])
    for a in KNOWN["test_saturation_vapor_pressure"]:
        for m in a["methods"]:
            got = thermal.saturation_vapor_pressure(np.array(a["tas"])[:, None], a["ice_thresh"], m, a["interp_power"], device=dev)[:, 0]
            k = 1 if m == "tetens30" else 0
            np.testing.assert_allclose(got[k:], a["expected"][k:], atol=a["atol"], rtol=a["rtol"])
