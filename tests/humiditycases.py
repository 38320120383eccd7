"""The recorded cases of tests/golden/humidity_vectors.npz (tests/golden/make_humidity_golden.py) as calls: each case names the
fields it reads, the output it checks and the keyword arguments, which ``xclim_amd.humidity.air_moisture`` and the restatement
``humiditycpu.air_moisture`` both take.  Shared by tests/test_humidity_cpu.py (restatement against the reference) and
tests/test_gpu_humidity.py (device against both)."""
import json
import os

import numpy as np

import humiditycpu as HC

HERE = os.path.dirname(os.path.abspath(__file__))
VECTORS = np.load(os.path.join(HERE, "golden", "humidity_vectors.npz"))
KNOWN = json.load(open(os.path.join(HERE, "golden", "humidity_known_answers.json")))
METHODS = [str(m) for m in VECTORS["methods"]]
ESAT_CASES = {"water": {}, "binary": dict(ice_thresh=273.15), "interp": dict(ice_thresh=250.15, interp_power=2)}
RULES = ("clip", "mask", None)
DTYPES = {"f64": np.float64, "f32": np.float32}
BIT_IDENTICAL = ("heat_index", "vp")   # float64 fields: equal to the recorded reference bit for bit
FUNCTION_OF = {"hurs": "relative_humidity", "esat": "saturation_vapor_pressure", "vpd": "vapor_pressure_deficit", "huss": "specific_humidity",
               "huss_dew": "specific_humidity_from_dewpoint", "vp": "vapor_pressure", "tdps": "dewpoint_from_specific_humidity",
               "humidex": "humidex", "heat_index": "heat_index"}
WIND_FUNCTION_OF = {"from_uv": "uas_vas_to_sfcwind", "to_uv": "sfcwind_to_uas_vas", "chill": "wind_chill_index", "power": "wind_power_potential"}


def f32_distance(key, val, scale, ref):
    """The largest |restatement rounded once to float32 - the reference's float32 route| / scale; where the scale is 0 (the plateaus
    of the power curve, a calm direction) the two must be equal."""
    ref = np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(val), np.isnan(ref)), key
    ok = np.isfinite(ref) & np.isfinite(val)
    pos = ok & (scale > 0)
    d = np.abs(val.astype(np.float32).astype(np.float64) - ref)
    assert np.all(d[ok & ~pos] == 0), key
    return float(np.max(d[pos] / scale[pos], initial=0.0))


def air_cases():
    """[(key under "<tag>/air/", output, {argument: key of its field}, keyword arguments)]"""
    td, hp = dict(tas="tas", tdps="tdps"), dict(tas="tas", hurs="hurs", ps="ps")
    cases = []
    for m in METHODS:
        for c, kw in ESAT_CASES.items():
            cases.append((f"hurs_tdps/{m}/{c}", "hurs", td, dict(method=m, invalid_values=None, **kw)))
    for r in RULES:
        cases.append((f"hurs_tdps_rule/{r}", "hurs", td, dict(invalid_values=r)))
        cases.append((f"hurs_huss_rule/{r}", "hurs", dict(tas="tas", huss="huss", ps="ps"), dict(invalid_values=r)))
        cases.append((f"hurs_bohren_rule/{r}", "hurs", td, dict(method="bohren98", invalid_values=r)))
        cases.append((f"huss_rule/{r}", "huss", hp, dict(huss_invalid_values=r)))
    for c, kw in ESAT_CASES.items():
        cases.append((f"esat/{c}", "esat", dict(tas="tas"), dict(method="ecmwf", **kw)))
        cases.append((f"vpd/{c}", "vpd", dict(tas="tas", hurs="hurs"), dict(method="wmo08", **kw)))
        cases.append((f"huss/{c}", "huss", hp, dict(method="goffgratch46", **kw)))
        cases.append((f"huss_dew/{c}", "huss_dew", dict(tdps="tdps", ps="ps"), dict(method="its90", **kw)))
        cases.append((f"exact/esat/{c}", "esat", dict(tas="exact/tas"), dict(method="buck81", units="degC", **kw)))
    cases.append(("vp", "vp", dict(huss="huss", ps="ps"), {}))
    for m in ("tetens30", "wmo08", "buck81", "aerk96"):
        for v in ("water", "ice"):
            cases.append((f"tdps/{m}/{v}", "tdps", dict(huss="huss", ps="ps"), dict(dew_method=m, variant=v)))
    cases.append(("humidex_tdps", "humidex", td, {}))
    cases.append(("humidex_hurs", "humidex", dict(tas="tas", hurs="hurs"), {}))
    cases.append(("heat_index", "heat_index", dict(tas="tas", hurs="hurs"), {}))
    tdc = dict(tas="degC/tas", tdps="degC/tdps")
    cases.append(("degC/humidex_tdps", "humidex", tdc, dict(units="degC")))
    cases.append(("degC/humidex_hurs", "humidex", dict(tas="degC/tas", hurs="hurs"), dict(units="degC")))
    cases.append(("degC/heat_index", "heat_index", dict(tas="degC/tas", hurs="hurs"), dict(units="degC")))
    cases.append(("degC/hurs_tdps", "hurs", tdc, dict(units="degC", method="wmo08", ice_thresh=273.15)))
    cases.append(("exact/heat_index", "heat_index", dict(tas="exact/tas", hurs="exact/hurs"), dict(units="degC")))
    return cases


AIR_CASES = air_cases()
FUSED_FIELDS = dict(tas="tas", tdps="tdps", ps="ps")
FUSED_OUTPUTS = ("hurs", "huss", "humidex", "heat_index")


def air_fields(tag, names):
    return {arg: VECTORS[f"{tag}/air/{key}"] for arg, key in names.items()}


def restated(tag, names, output, kw):
    """(value, scale) of the float64 restatement on the recorded fields, widened."""
    f = {k: v.astype(np.float64) for k, v in air_fields(tag, names).items()}
    return HC.air_moisture(outputs=(output,), thr32=tag == "f32", **f, **kw)[output]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def check(got, val, scale, dtype, what, bit_identical_to=None):
    """``got`` against the restatement ``val``: the same NaN pattern, and 1e-12 x scale (float64) with one float32 ulp of the value
    rounded once on top for float32 fields.  Returns the worst |d| / (1e-12 scale) over the finite float64 samples."""
    got = np.asarray(got)
    assert got.dtype == dtype and got.shape == val.shape, (what, got.dtype, got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(val)), what
    if bit_identical_to is not None:
        np.testing.assert_array_equal(got, bit_identical_to, err_msg=what)
    ok = np.isfinite(val)
    ref = val if dtype == np.float64 else val.astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - ref)
        tol = 1e-12 * scale + (ulp32(val) if dtype == np.float32 else 0.0)
        assert np.all(d[ok] <= tol[ok]), (what, float(np.max((d / tol)[ok])))
        pos = ok & (scale > 0)
        return float(np.max(d[pos] / (1e-12 * scale[pos]), initial=0.0)) if dtype == np.float64 else 0.0


# ---- the wind cases: {key under "<tag>/wind/": (value, scale)} of the restatement, and the same keys from the mirror -----------------
def wind_restated(tag):
    dtype = DTYPES[tag]
    g = lambda k: VECTORS[f"{tag}/wind/{k}"].astype(np.float64)   # noqa: E731
    thr32 = tag == "f32"
    res = {}
    res["from_uv/wind"], res["from_uv/dir"] = HC.uas_vas_to_sfcwind(g("uas"), g("vas"), 0.5, dtype)
    res["exact/from_uv/wind"], res["exact/from_uv/dir"] = HC.uas_vas_to_sfcwind(g("exact/uas"), 0 * g("exact/uas"), 0.5, dtype)
    res["to_uv/uas"], res["to_uv/vas"] = HC.sfcwind_to_uas_vas(g("speed"), g("dir"))
    for m in ("CAN", "US"):
        for mask in (True, False):
            res[f"chill/{m}/{mask}"] = HC.wind_chill_index(g("chill/tas") - 273.15, g("chill/sfcWind") * 3.6, m, mask)
        res[f"exact/chill/{m}"] = HC.wind_chill_index(g("exact/chill/tas"), g("exact/chill/sfcWind") * 3.6, m, True)
    for name, kw in (("plain", {}), ("density", dict(air_density=g("power/rho"))), ("custom", dict(cut_in=3.3, rated=11.7, cut_out=24.9))):
        res[f"power/{name}"] = HC.wind_power_potential(g("power/wind"), thr32=thr32, **kw)[:2]
    res["exact/power/plain"] = HC.wind_power_potential(g("exact/power/wind"), thr32=thr32)[:2]
    return res


def wind_mirror(H, tag, **kw):
    """The same keys from the functions of ``H`` (xclim_amd.humidity) on the recorded fields in their own dtype."""
    g = lambda k: VECTORS[f"{tag}/wind/{k}"]   # noqa: E731
    res = {}
    res["from_uv/wind"], res["from_uv/dir"] = H.uas_vas_to_sfcwind(g("uas"), g("vas"), **kw)
    res["exact/from_uv/wind"], res["exact/from_uv/dir"] = H.uas_vas_to_sfcwind(g("exact/uas"), np.zeros_like(g("exact/uas")), "0.5 m/s", **kw)
    res["to_uv/uas"], res["to_uv/vas"] = H.sfcwind_to_uas_vas(g("speed"), g("dir"), **kw)
    for m in ("CAN", "US"):
        for mask in (True, False):
            res[f"chill/{m}/{mask}"] = H.wind_chill_index(g("chill/tas"), g("chill/sfcWind"), m, mask, **kw)
        res[f"exact/chill/{m}"] = H.wind_chill_index(g("exact/chill/tas"), g("exact/chill/sfcWind"), m, units="degC", **kw)
    res["power/plain"] = H.wind_power_potential(g("power/wind"), **kw)
    res["power/density"] = H.wind_power_potential(g("power/wind"), g("power/rho"), **kw)
    res["power/custom"] = H.wind_power_potential(g("power/wind"), cut_in="3.3 m/s", rated=11.7, cut_out=24.9, **kw)
    res["exact/power/plain"] = H.wind_power_potential(g("exact/power/wind"), **kw)
    return res
