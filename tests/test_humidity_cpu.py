"""The numpy restatement of the humidity, heat-stress and wind unit (tests/humiditycpu.py) against the reference's own code, without a
GPU: the vectors tests/golden/make_humidity_golden.py recorded by executing the reference (tests/golden/humidity_vectors.npz), the
known answers of the reference's tests to those tests' own tolerances (tests/golden/humidity_known_answers.json), and the mirrors of
the unit's ``#define``s.

float64 vectors: the restatement is the reference's expression on the same numpy, so 1e-12 x the sum of the absolute terms holds
with room (it is the bound the device is held to in tests/test_gpu_humidity.py), the heat index and the vapour pressure are equal
bit for bit, and so is every NaN, mask, clip, calm and power-regime decision.  float32 vectors: the reference stays in float32 where
the restatement widens; the generator measured that distance per function (``f32_distance``, in units of the value's scale), and
twice the recorded figure is asserted, which covers numpy's exp / log / pow differing by an ulp between CPUs."""
import numpy as np
import pytest

import humiditycases as HCS
import humiditycpu as HC
from xclim_amd import _capi

KNOWN = HCS.KNOWN
FUNCTION_OF, WIND_FUNCTION_OF = HCS.FUNCTION_OF, HCS.WIND_FUNCTION_OF


def _against_reference(tag, key, fn, val, scale, ref):
    ref = np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(val), np.isnan(ref)), key
    ok = np.isfinite(ref) & np.isfinite(val)
    if tag == "f64":
        assert np.all(np.abs(val - ref)[ok] <= 1e-12 * scale[ok]), key
        for plateau in (0.0, 1.0, 100.0, 360.0):   # clip, calm, north and regime decisions
            assert np.array_equal(val == plateau, ref == plateau), (key, plateau)
    else:
        if "exact/" in key:   # (on a bound the float32 route may decide otherwise: compared where both decide alike)
            return
        worst = HCS.f32_distance(key, val, scale, ref)
        assert worst <= 2 * KNOWN["f32_distance"][fn], (key, worst)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_restatement_reproduces_the_recorded_air_moisture_vectors(tag):
    for key, output, names, kw in HCS.AIR_CASES:
        val, scale = HCS.restated(tag, names, output, kw)
        ref = HCS.VECTORS[f"{tag}/air/{key}"]
        assert ref.shape == (3, 130) or "exact/" in key
        if tag == "f64" and output in HCS.BIT_IDENTICAL:
            np.testing.assert_array_equal(val, ref, err_msg=key)
        _against_reference(tag, key, FUNCTION_OF[output], val, scale, ref)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_the_restatement_reproduces_the_recorded_wind_vectors(tag):
    for key, (val, scale) in HCS.wind_restated(tag).items():
        fn = WIND_FUNCTION_OF[key.replace("exact/", "").split("/")[0]]
        _against_reference(tag, key, fn, val, scale, HCS.VECTORS[f"{tag}/wind/{key}"])


def test_the_fused_composition_is_the_reference_s():
    f = {k: v.astype(np.float64) for k, v in HCS.air_fields("f64", HCS.FUSED_FIELDS).items()}
    res = HC.air_moisture(outputs=HCS.FUSED_OUTPUTS, **f)
    for o in HCS.FUSED_OUTPUTS:
        _against_reference("f64", f"fused/{o}", FUNCTION_OF[o], *res[o], HCS.VECTORS[f"f64/air/fused/{o}"])


def test_the_families_hold_every_decision():
    z = HCS.VECTORS
    for tag in ("f64", "f32"):
        h = z[f"{tag}/air/hurs_tdps_rule/None"]
        assert (h < 0).sum() == 0 and (h > 100).any() and ((h > 0) & (h < 100)).any()   # (a ratio of pressures is never negative)
        hh = z[f"{tag}/air/hurs_huss_rule/None"]
        assert (hh < 0).any() and (hh > 100).any()
        assert np.isnan(z[f"{tag}/air/hurs_tdps_rule/mask"]).sum() > np.isnan(h).sum()
        q = z[f"{tag}/air/huss_rule/None"]
        assert (q < 0).any() and (q != z[f"{tag}/air/huss_rule/clip"])[~np.isnan(q)].any()
        huss = z[f"{tag}/air/huss"]
        assert (huss == 0).any() and (huss < 0).any() and (huss > 0).any()
        assert np.array_equal(np.isnan(z[f"{tag}/air/tdps/buck81/water"]), ~(huss > 0) | np.isnan(z[f"{tag}/air/ps"]))
        hi = z[f"{tag}/air/heat_index"]
        assert np.isnan(hi).any() and np.isfinite(hi).any()
        for k in ("tas", "tdps", "hurs", "huss", "ps"):
            assert np.isnan(z[f"{tag}/air/{k}"]).any(), k
        d = z[f"{tag}/wind/from_uv/dir"]
        assert (d == 0).any() and (d == 360).any() and all(((d > a) & (d < a + 90)).any() for a in (0, 90, 180, 270))
        for m in ("CAN", "US"):
            assert np.isnan(z[f"{tag}/wind/chill/{m}/True"]).sum() > np.isnan(z[f"{tag}/wind/chill/{m}/False"]).sum()
        for name in ("plain", "density"):
            _, _, regime = HC.wind_power_potential(z[f"{tag}/wind/power/wind"].astype(np.float64),
                                                   z[f"{tag}/wind/power/rho"].astype(np.float64) if name == "density" else None)
            assert set(np.unique(regime)) == {0, 1, 2, 3}


def test_every_sample_keeps_its_distance_from_the_decision_bounds():
    z = HCS.VECTORS
    for tag, rel in (("f64", 1e-6), ("f32", 1e-4)):
        for k in ("tas", "tdps"):
            t = z[f"{tag}/air/{k}"].astype(np.float64)
            for b in (250.15, 273.15, 273.16, 293.15):
                assert not np.any(np.abs(t - b) <= rel * b), (tag, k, b)
        for k in ("hurs_tdps_rule/None", "hurs_huss_rule/None", "hurs_bohren_rule/None"):
            h = z[f"{tag}/air/{k}"].astype(np.float64)
            # (huss == 0 gives exactly 0 % on every route: no rounding stands behind that one)
            assert not np.any(np.abs(h - 100) <= rel * 100) and not np.any((h != 0) & (np.abs(h) <= rel)), (tag, k)
        w = z[f"{tag}/wind/power/wind"].astype(np.float64)
        for b in (3.5, 13.0, 25.0, 3.3, 11.7, 24.9):
            assert not np.any(np.abs(w - b) <= rel * b), (tag, b)
        t, s = z[f"{tag}/wind/chill/tas"].astype(np.float64) - 273.15, z[f"{tag}/wind/chill/sfcWind"].astype(np.float64) * 3.6
        assert not np.any(np.abs(t) <= rel * 273.15) and not np.any(np.abs(t - 10) <= rel * 283.15)
        assert not np.any(np.abs(s - 5) <= rel * 5) and not np.any(np.abs(s - 4.828032) <= rel * 5)


# ---- the known answers of the reference's own tests, to those tests' tolerances ------------------------------------------------
def _nan(v):
    return np.array([np.nan if x is None else x for x in v], np.float64)


def test_known_humidex_and_heat_index():
    a = KNOWN["test_humidex"]
    tas, tdps = np.array(a["tas_degC"], float), np.array(a["tdps_degC"], float)
    got = HC.air_moisture(tas=tas, tdps=tdps, outputs=("humidex",), units="degC")["humidex"][0]
    np.testing.assert_array_almost_equal(got, a["expected"], a["decimal"])
    np.testing.assert_allclose(got, a["reference_tdps"], rtol=1e-13)
    got_k = HC.air_moisture(tas=tas + 273.15, tdps=tdps + 273.15, outputs=("humidex",))["humidex"][0]
    np.testing.assert_array_almost_equal(got_k - 273.15, a["expected"], a["decimal"])
    hurs = HC.air_moisture(tas=tas, tdps=tdps, outputs=("hurs",), units="degC", method="bohren98")["hurs"][0]
    np.testing.assert_allclose(hurs, a["hurs_bohren98"], rtol=1e-13)
    got = HC.air_moisture(tas=tas, hurs=hurs, outputs=("humidex",), units="degC")["humidex"][0]
    np.testing.assert_array_almost_equal(got, a["expected"], a["decimal"])
    np.testing.assert_allclose(got, a["reference_hurs"], rtol=1e-13)
    a = KNOWN["test_heat_index"]
    got = HC.heat_index(np.array(a["tas_degC"], float), np.array(a["hurs"], float))[0]
    np.testing.assert_array_almost_equal(got, _nan(a["expected"]), a["decimal"])
    np.testing.assert_array_equal(got, _nan(a["reference"]))
    got = HC.air_moisture(tas=np.array(a["tas_degC"], float) + 273.15, hurs=np.array(a["hurs"], float), outputs=("heat_index",))["heat_index"][0]
    np.testing.assert_allclose(got, _nan(a["reference_K"]), rtol=1e-13)


def test_known_wind_answers():
    a = KNOWN["test_wind_chill"]
    t, v = np.array(a["tas_K"]) - 273.15, np.array(a["sfcWind_kmh"], float)
    np.testing.assert_allclose(HC.wind_chill_index(t, v)[0], _nan(a["expected"]), rtol=a["rtol"])
    assert np.isnan(HC.wind_chill_index(t, v, "US")[0][-1]) and a["reference_US"][-1] is None
    a = KNOWN["TestWindConversion"]
    u, v = np.array(a["uas_kmh"]) * (1 / 3.6), np.array(a["vas_kmh"]) * (1 / 3.6)
    (w, _), (d, _) = HC.uas_vas_to_sfcwind(u, v)
    assert np.all(np.around(w, a["decimals"]) == np.around(a["expected_wind"], a["decimals"]))
    assert np.all(np.around(d, a["decimals"]) == np.around(a["expected_dir"], a["decimals"]))
    (uu, _), (vv, _) = HC.sfcwind_to_uas_vas(np.array(a["wind_kmh"]) * (1 / 3.6), np.array(a["wind_from_dir"], float))
    assert np.all(np.around(uu, a["decimals"]) == np.around(a["expected_uas"], a["decimals"]))
    assert np.all(np.around(vv, a["decimals"]) == np.around(a["expected_vas"], a["decimals"]))


def test_known_humidity_answers():
    a = KNOWN["test_relative_humidity_dewpoint"]
    for m, by_rule in a["reference"].items():
        for rule, ref in by_rule.items():
            got = HC.relative_humidity(a["tas_K"], a["tdps_K"], method=m, invalid_values=None if rule == "None" else rule)[0]
            exp = _nan([a["exp0"][rule]] + a["expected_tail"])
            np.testing.assert_allclose(got, exp, rtol=a["rtol"], atol=a["atol"])
            np.testing.assert_allclose(got, _nan(ref), rtol=1e-13)
    a = KNOWN["test_specific_humidity_from_dewpoint"]
    got = HC.specific_humidity_from_dewpoint(np.array(a["tdps_degC"]) + 273.15, a["ps_Pa"])[0]
    np.testing.assert_array_almost_equal(got, a["expected"], a["decimal"])
    a = KNOWN["test_vapor_pressure"]
    q = HC.specific_humidity_from_dewpoint(a["tas_K"], a["ps_Pa"], "buck81")[0]
    np.testing.assert_allclose(HC.vapor_pressure(q, a["ps_Pa"])[0], HC.esat(a["tas_K"], "buck81")[0], rtol=a["rtol"])
    np.testing.assert_array_equal(HC.vapor_pressure(a["huss"], a["ps_Pa"])[0], a["reference_vp"])
    a = KNOWN["test_vapor_pressure_deficit"]
    for m, ref in a["reference"].items():
        got = HC.vapor_pressure_deficit(a["tas_K"], a["hurs"], m)[0]
        np.testing.assert_allclose(got, a["expected"], atol=a["atol"], rtol=a["rtol"])
        np.testing.assert_allclose(got, ref, rtol=1e-13)
    a = KNOWN["test_relative_humidity"]
    for m, by_rule in a["reference"].items():
        for rule, ref in by_rule.items():
            got = HC.relative_humidity(a["tas_K"], None, a["huss"], a["ps_Pa"], m, None if rule == "None" else rule, ice_thresh=a["ice_thresh_K"])[0]
            np.testing.assert_allclose(got, _nan([a["exp0"][rule]] + a["expected_tail"]), atol=a["atol"], rtol=a["rtol"])
            np.testing.assert_allclose(got, _nan(ref), rtol=1e-13)
    a = KNOWN["test_specific_humidity"]
    for m, by_rule in a["reference"].items():
        for rule, ref in by_rule.items():
            got = HC.specific_humidity(a["tas_K"], a["hurs"], a["ps_Pa"], m, None if rule == "None" else rule, ice_thresh=a["ice_thresh_K"])[0]
            np.testing.assert_allclose(got, _nan([a["exp0"][rule]] + a["expected_tail"]), atol=a["atol"], rtol=a["rtol"])
            np.testing.assert_allclose(got, _nan(ref), rtol=1e-13)
    a = KNOWN["test_dewpoint_from_specific_humidity"]
    for m, ref in a["reference"].items():
        got = HC.dewpoint_from_specific_humidity(a["huss"], a["ps_Pa"], m)[0]
        np.testing.assert_allclose(got, _nan(a["expected"]), atol=a["atol"], rtol=a["rtol"])
        np.testing.assert_allclose(got, _nan(ref), rtol=1e-13)


def test_the_mirrors_of_the_defines():
    d = _capi.UNIT_DEFINES["xclim_hip_humidity.h"]
    assert [d[f"XH_AM_{k.upper()}"] for k in HC.OUTPUTS] == list(range(_capi.AM_NOUT)) and tuple(_capi.AM_OUTPUTS) == HC.OUTPUTS
    assert sorted(_capi.WIND_OPS.values()) == list(range(_capi.WIND_NOPS))
    assert sorted(_capi.WIND_FLAGS.values()) == [1, 2, 4, 8]
    assert set(_capi.DEW_METHODS) == {"tetens30", "wmo08", "buck81", "aerk96"} and _capi.INVALID_RULES == {"none": 0, "clip": 1, "mask": 2}
    assert len(_capi.UNIT_SIGNATURES["xh_air_moisture"]) == 23 and len(_capi.UNIT_SIGNATURES["xh_wind_map"]) == 13


def test_the_mirror_s_errors_are_the_reference_s():
    from xclim_amd import humidity as H

    t = np.full((2, 3), 290.0)
    with pytest.raises(ValueError, match="At least one of `tdps` or `hurs` must be given."):
        H.humidex(t)
    with pytest.raises(ValueError, match=r"To use method 'bohren98' \(BA98\), dewpoint must be given."):
        H.relative_humidity(t, huss=t, ps=t, method="bohren98")
    with pytest.raises(ValueError, match="`huss` and `ps` must be provided if `tdps` is not given."):
        H.relative_humidity(t, huss=t)
    with pytest.raises(ValueError, match="`method` must be one of 'US' and 'CAN'. Got 'EU'."):
        H.wind_chill_index(t, t, method="EU")
    with pytest.raises(ValueError, match="Method magnus is not in"):
        H.relative_humidity(t, tdps=t, method="magnus")
    with pytest.raises(KeyError):
        H.dewpoint_from_specific_humidity(t, t, method="sonntag90")
    with pytest.raises(H.NotServed, match="integer field"):
        H.heat_index(np.full((2, 3), 300), t)
    with pytest.raises(H.NotServed, match="different shapes"):
        H.heat_index(t, t[:1])
    with pytest.raises(H.NotServed, match="not served"):
        H.heat_index(t, t, units="degF")
    assert H.saturation_vapor_pressure.__module__ == "xclim_amd.thermal"
