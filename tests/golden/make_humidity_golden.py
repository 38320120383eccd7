"""Generate tests/golden/humidity_vectors.npz and tests/golden/humidity_known_answers.json by EXECUTING the reference's humidity,
heat-stress and wind conversions.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_humidity_golden.py

As tests/golden/make_thermal_golden.py and make_pet_golden.py: the functions are AST-extracted from src/xclim/indices/converters.py
(nothing is copied into this repository), their decorators and annotations dropped, and their WHOLE bodies executed on the restated
DataArray (make_pet_golden.Arr: an ndarray with units).  Extracted: ``humidex``, ``heat_index``, ``uas_vas_to_sfcwind``,
``sfcwind_to_uas_vas``, ``vapor_pressure``, ``vapor_pressure_deficit``, ``relative_humidity``, ``specific_humidity``,
``specific_humidity_from_dewpoint``, ``dewpoint_from_specific_humidity``, ``wind_chill_index``, ``wind_power_potential`` and
``_wind_power_factor`` (through np.vectorize where the reference uses numba), with ``saturation_vapor_pressure`` and its two
helpers under them.  Restated: unit conversion as ONE multiplication or offset, ``units2pint`` (the delta of K and of degC is the
same number), ``xr.where`` and ``xr.apply_ufunc``.

humidity_vectors.npz holds 3 rows by 130 cells per family, as ``<f64|f32>/<family>/<name>``: one family per decision of the kernels
(``air_families`` and ``wind_families`` below).  Every sample stays at least 1e-6 relative (float64) or 1e-4 (float32) away from a decision bound (``nudge``),
except in the family ``exact``, whose samples sit ON the bounds and are given in degC (and in values float32 holds), so that float32
and float64 fields hold the same value.  humidity_known_answers.json holds the inputs and expectations of the reference's own tests
(tests/test_indices.py: test_humidex, test_heat_index, test_wind_chill, TestWindConversion, test_relative_humidity*,
test_specific_humidity*, test_vapor_pressure*, test_dewpoint_from_specific_humidity; tests/test_converters.py: the two
test_relative_humidity_dewpoint* and test_humidex, the ones that need no data file and are not the same call again) next to what the
executed reference gives for them, and ``f32_distance``: per function, the largest distance, in units of the value's scale
(tests/humiditycpu.py), from the float64 restatement rounded once to float32 to the reference's float32 route, measured here.
"""

import ast
import json
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_pet_golden as P  # noqa: E402

REF = "/root/reference/src/xclim/indices/converters.py"
NAMES = ["humidex", "heat_index", "uas_vas_to_sfcwind", "sfcwind_to_uas_vas", "vapor_pressure", "vapor_pressure_deficit",
         "relative_humidity", "specific_humidity", "specific_humidity_from_dewpoint", "dewpoint_from_specific_humidity",
         "wind_chill_index", "wind_power_potential", "_wind_power_factor", "saturation_vapor_pressure",
         "_saturation_vapor_pressure_over_water", "_saturation_vapor_pressure_over_ice"]
METHODS = ["sonntag90", "goffgratch46", "its90", "tetens30", "wmo08", "buck81", "aerk96", "ecmwf"]
CASES = {"water": {}, "binary": dict(ice_thresh="0 degC"), "interp": dict(ice_thresh="-23 degC", interp_power=2)}
_SAME = {"kelvin": "K", "degK": "K", "celsius": "degC", "°C": "degC", "C": "degC", "": "1", "m/s": "m s-1", "km h-1": "km/h", "degree": "deg"}
_FACTOR = {("%", "1"): 1e-2, ("1", "%"): 100.0, ("m s-1", "km/h"): 3.6, ("km/h", "m s-1"): 1 / 3.6}


def arr(a, units):
    return P.Arr(a, units)


def convert_units_to(x, target, context=None):
    if isinstance(target, np.ndarray):   # a threshold to the unit of a field
        target = target.units
    target = _SAME.get(target, target)
    if isinstance(x, str):
        v, _, u = x.partition(" ")
        v, u = float(v), _SAME.get(u.strip(), u.strip())
        if u == target or u == "kg/m^3":
            return v
        if (u, target) == ("degC", "K"):
            return v + 273.15
        return v * _FACTOR[(u, target)]
    if not hasattr(x, "units") or x.units is None:
        return x
    src = _SAME.get(x.units, x.units)
    if src == target or target == "delta":
        return x
    if (src, target) == ("K", "degC"):
        out = x - 273.15
    elif (src, target) == ("degC", "K"):
        out = x + 273.15
    else:
        out = x * _FACTOR[(src, target)]
    return out.assign_attrs(units=target)


class _Delta:
    units = "delta"

    def __rmul__(self, k):
        return self

    def __sub__(self, o):
        return self


def extract():
    import types

    def where(c, a, b):
        ref = next((v for v in (b, a, c) if isinstance(v, P.Arr)), None)
        return arr(np.where(np.asarray(c), np.asarray(a), np.asarray(b)), getattr(ref, "units", None))

    def apply_ufunc(f, *args):
        return arr(np.vectorize(f, otypes=[float])(*[np.asarray(a) if isinstance(a, np.ndarray) else a for a in args]), None)

    ns = {"np": np, "xr": types.SimpleNamespace(where=where, apply_ufunc=apply_ufunc, DataArray=P.Arr), "cast": lambda t, v: v, "namedtuple": namedtuple,
          "convert_units_to": convert_units_to, "units2pint": lambda a: _Delta()}
    tree = ast.parse(open(REF).read())
    body = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in NAMES:
            node.decorator_list = []
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            body.append(node)
        elif isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "ESAT_FORMULAS_COEFFICIENTS":
            body.append(node)
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    missing = set(NAMES) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")
    return ns


def nudge(x, bounds, rel=1e-3):
    """Move every sample that lies within ``rel`` (relative, at least absolute on a bound of 0) of a bound to ``3 rel`` above it."""
    x = np.array(x, np.float64)
    for b in bounds:
        w = rel * max(abs(b), 1.0)
        x = np.where(np.abs(x - b) <= w, b + 3 * w, x)
    return x


R, C = 3, 130
T_BOUNDS = [250.15, 273.15, 273.16, 293.15, 283.15]   # the e_sat thresholds of CASES, 20 degC, 10 degC


def fields(rng):
    """The (3, 130) fields of the air-moisture families, float64, rounded to values float32 keeps apart from the bounds."""
    tas = nudge(np.round(rng.uniform(235, 320, (R, C)), 2), T_BOUNDS)
    tdps = nudge(np.round(tas - rng.uniform(-1.5, 18, (R, C)), 2), T_BOUNDS)   # (a dewpoint above tas: more than 100 %)
    hurs = np.round(rng.uniform(-8, 115, (R, C)), 2)        # below 0, inside, above the cap
    hurs = nudge(hurs, [0.0, 100.0])
    huss = np.round(rng.uniform(2e-4, 0.03, (R, C)), 6)
    huss.flat[::9] = 0.0                                     # dewpoint: huss at 0, negative and positive
    huss.flat[4::17] = -np.round(rng.uniform(1e-4, 1e-3, huss.flat[4::17].shape), 6)
    ps = np.round(rng.uniform(60000, 105000, (R, C)), 0)
    return dict(tas=tas, tdps=tdps, hurs=hurs, huss=huss, ps=ps)


def with_nan(f):
    """A NaN in each input in turn (and two at once on the last stripe)."""
    g = {k: v.copy() for k, v in f.items()}
    for k, n in enumerate(g):
        g[n].flat[k * 5 + 2::43] = np.nan
    return g


UNITS = dict(tas="K", tdps="K", hurs="%", huss="1", ps="Pa")


def A(f, dtype, units=None):
    u = dict(UNITS, **(units or {}))
    return {k: arr(v.astype(dtype), u[k]) for k, v in f.items()}


def air_families(ns, rng, dtype, out, tag):
    f = with_nan(fields(rng))
    a = A(f, dtype)
    for k, v in a.items():
        out[f"{tag}/air/{k}"] = np.asarray(v)
    put = lambda name, v: out.__setitem__(f"{tag}/air/{name}", np.asarray(v))   # noqa: E731
    with np.errstate(all="ignore"):
        for m in METHODS:   # each e_sat method crossed with the three cases
            for c, kw in CASES.items():
                put(f"hurs_tdps/{m}/{c}", ns["relative_humidity"](a["tas"], tdps=a["tdps"], method=m, invalid_values=None, **kw))
        for rule in ("clip", "mask", None):   # each invalid_values rule
            put(f"hurs_tdps_rule/{rule}", ns["relative_humidity"](a["tas"], tdps=a["tdps"], invalid_values=rule))
            put(f"hurs_huss_rule/{rule}", ns["relative_humidity"](a["tas"], huss=a["huss"], ps=a["ps"], invalid_values=rule))
            put(f"hurs_bohren_rule/{rule}", ns["relative_humidity"](a["tas"], tdps=a["tdps"], method="bohren98", invalid_values=rule))
            put(f"huss_rule/{rule}", ns["specific_humidity"](a["tas"], a["hurs"], a["ps"], invalid_values=rule))
        for c, kw in CASES.items():
            put(f"esat/{c}", ns["saturation_vapor_pressure"](a["tas"], method="ecmwf", **kw))
            put(f"vpd/{c}", ns["vapor_pressure_deficit"](a["tas"], a["hurs"], method="wmo08", **kw))
            put(f"huss/{c}", ns["specific_humidity"](a["tas"], a["hurs"], a["ps"], method="goffgratch46", **kw))
            put(f"huss_dew/{c}", ns["specific_humidity_from_dewpoint"](a["tdps"], a["ps"], method="its90", **kw))
        put("vp", ns["vapor_pressure"](a["huss"], a["ps"]))
        for m in ("tetens30", "wmo08", "buck81", "aerk96"):
            for variant in ("water", "ice"):
                put(f"tdps/{m}/{variant}", ns["dewpoint_from_specific_humidity"](a["huss"], a["ps"], method=m, variant=variant))
        put("humidex_tdps", ns["humidex"](a["tas"], tdps=a["tdps"]))
        put("humidex_hurs", ns["humidex"](a["tas"], hurs=a["hurs"]))
        put("heat_index", ns["heat_index"](a["tas"], a["hurs"]))
        # the same fields in degC
        fc = dict(f, tas=np.round(f["tas"] - 273.15, 2), tdps=np.round(f["tdps"] - 273.15, 2))
        ac = A(fc, dtype, dict(tas="degC", tdps="degC"))
        put("degC/tas", ac["tas"]), put("degC/tdps", ac["tdps"])
        put("degC/humidex_tdps", ns["humidex"](ac["tas"], tdps=ac["tdps"]))
        put("degC/humidex_hurs", ns["humidex"](ac["tas"], hurs=ac["hurs"]))
        put("degC/heat_index", ns["heat_index"](ac["tas"], ac["hurs"]))
        put("degC/hurs_tdps", ns["relative_humidity"](ac["tas"], tdps=ac["tdps"], method="wmo08", ice_thresh="0 degC"))
        # the reference's composition of the fused launch (tas, tdps, ps) -> (hurs, huss, humidex, heat_index)
        h = ns["relative_humidity"](a["tas"], tdps=a["tdps"])
        put("fused/hurs", h)
        put("fused/huss", ns["specific_humidity"](a["tas"], h, a["ps"]))
        put("fused/humidex", ns["humidex"](a["tas"], tdps=a["tdps"]))
        put("fused/heat_index", ns["heat_index"](a["tas"], h))
        # a family on the decision bounds, in degC: the ice / water thresholds of the three cases, 20 degC
        te = np.tile(np.array([-23.0, 0.0, 20.0, -23.5, 0.5, 20.5, -22.5, -0.5, 19.5, 30.0]), (R, 1))
        he = np.tile(np.array([0.0, 100.0, 50.0, 0.0, 100.0, 100.0, 0.0, 50.0, 100.0, 0.0]), (R, 1))
        ae = dict(tas=arr(te.astype(dtype), "degC"), hurs=arr(he.astype(dtype), "%"))
        put("exact/tas", ae["tas"]), put("exact/hurs", ae["hurs"])
        for c, kw in CASES.items():
            put(f"exact/esat/{c}", ns["saturation_vapor_pressure"](ae["tas"], method="buck81", **kw))
        put("exact/heat_index", ns["heat_index"](ae["tas"], ae["hurs"]))


def wind_families(ns, rng, dtype, out, tag):
    put = lambda name, v: out.__setitem__(f"{tag}/wind/{name}", np.asarray(v))   # noqa: E731
    # direction: the four quadrants, due north (and the other three axes), calm; a NaN in each input
    ang = nudge(np.round(rng.uniform(0, 360, (R, C)), 1), [0.0, 90.0, 180.0, 270.0, 360.0], 1e-2)   # mathematical angle, off the axes
    spd = np.round(rng.uniform(0.6, 25, (R, C)), 2)
    spd.flat[::8] = np.round(rng.uniform(0.01, 0.4, spd.flat[::8].shape), 2)   # calm
    u, v = np.round(spd * np.cos(np.radians(ang)), 3), np.round(spd * np.sin(np.radians(ang)), 3)
    u[0, :4], v[0, :4] = [0.0, 0.0, 3.0, -3.0], [-5.0, 5.0, 0.0, 0.0]          # due north, south, west, east
    u.flat[7::41], v.flat[11::41] = np.nan, np.nan
    uas, vas = arr(u.astype(dtype), "m s-1"), arr(v.astype(dtype), "m s-1")
    w, d = ns["uas_vas_to_sfcwind"](uas, vas)
    assert not np.any(np.abs(np.asarray(w, np.float64) - 0.5) < 1e-3)
    dd = np.asarray(d, np.float64)
    assert not np.any(np.abs(dd - 0.5) < 1e-3)   # (the one bound of ``round() == 0``: the remainder is never negative)
    put("uas", uas), put("vas", vas), put("from_uv/wind", w), put("from_uv/dir", d)
    direction = np.round(rng.uniform(0, 360, (R, C)), 1)
    direction[0, :5] = [0.0, 90.0, 180.0, 270.0, 360.0]
    direction.flat[5::37] = np.nan
    sp2 = spd.copy()
    sp2.flat[9::37] = np.nan
    sw, sd = arr(sp2.astype(dtype), "m s-1"), arr(direction.astype(dtype), "degree")
    uu, vv = ns["sfcwind_to_uas_vas"](sw, sd)
    put("speed", sw), put("dir", sd), put("to_uv/uas", uu), put("to_uv/vas", vv)
    # wind chill: both methods on both sides of each bound (0 and 10 degC; 5 and 4.828032 km/h = 1.3889 and 1.34112 m s-1)
    tk = nudge(np.round(rng.uniform(243, 290, (R, C)), 2), [273.15, 283.15])
    ws = nudge(np.round(rng.uniform(0.2, 20, (R, C)), 3), [5 / 3.6, 4.828032 / 3.6], 2e-3)
    ws.flat[::6] = nudge(np.round(rng.uniform(1.2, 1.5, ws.flat[::6].shape), 3), [5 / 3.6, 4.828032 / 3.6], 2e-3)
    tk.flat[3::39], ws.flat[8::39] = np.nan, np.nan
    t, s = arr(tk.astype(dtype), "K"), arr(ws.astype(dtype), "m s-1")
    put("chill/tas", t), put("chill/sfcWind", s)
    with np.errstate(all="ignore"):
        for m in ("CAN", "US"):
            for mask in (True, False):
                put(f"chill/{m}/{mask}", ns["wind_chill_index"](t, s, method=m, mask_invalid=mask))
        # on the temperature bounds, in degC
        te = np.tile(np.array([0.0, 10.0, -0.5, 0.5, 9.5, 10.5]), (R, 1))
        se = np.tile(np.array([3.0, 3.0, 1.0, 1.0, 3.0, 3.0]), (R, 1))
        t2, s2 = arr(te.astype(dtype), "degC"), arr(se.astype(dtype), "m s-1")
        put("exact/chill/tas", t2), put("exact/chill/sfcWind", s2)
        for m in ("CAN", "US"):
            put(f"exact/chill/{m}", ns["wind_chill_index"](t2, s2, method=m))
    # wind power: the four regimes, with and without density
    ws = nudge(np.round(rng.uniform(0, 32, (R, C)), 2), [3.5, 13.0, 25.0])
    ws.flat[6::31] = np.nan
    rho = np.round(rng.uniform(0.9, 1.4, (R, C)), 3)
    rho.flat[2::47] = np.nan
    with np.errstate(invalid="ignore"):   # a scaled speed next to a bound: standard density there (the speed itself is nudged)
        near = np.any([np.abs(ws * (rho / 1.225) ** (1 / 3) - b) < 2e-3 * b for b in (3.5, 13.0, 25.0)], axis=0)
    rho[near] = 1.225
    s, r =arr(ws.astype(dtype), "m s-1"), arr(rho.astype(dtype), "kg m-3")
    scaled = np.asarray(s, np.float64) * (np.asarray(r, np.float64) / 1.225) ** (1 / 3)
    for b in (3.5, 13.0, 25.0):
        assert not np.any(np.abs(scaled - b) < 1e-3 * b)
    put("power/wind", s), put("power/rho", r)
    put("power/plain", ns["wind_power_potential"](s))
    put("power/density", ns["wind_power_potential"](s, air_density=r))
    put("power/custom", ns["wind_power_potential"](s, cut_in="3.3 m/s", rated="11.7 m/s", cut_out="24.9 m/s"))
    we = np.tile(np.array([3.5, 13.0, 25.0, 3.25, 12.5, 24.5, 25.5]), (R, 1))   # on the bounds
    se = arr(we.astype(dtype), "m s-1")
    ce = np.tile(np.array([0.5, 0.0, 0.25, 0.75]), (R, 1))
    put("exact/power/wind", se), put("exact/power/plain", ns["wind_power_potential"](se))
    ue, ve = arr(ce.astype(dtype), "m s-1"), arr(np.zeros_like(ce).astype(dtype), "m s-1")
    we_, de_ = ns["uas_vas_to_sfcwind"](ue, ve)
    put("exact/uas", ue), put("exact/from_uv/wind", we_), put("exact/from_uv/dir", de_)


def f32_distance():
    """Per function: the largest |restatement rounded once to float32 - the reference's float32 route| / scale over the float32
    vectors just written (the cases of tests/humiditycases.py, the family on the bounds left out); the restatement is evaluated
    on the float32 fields widened."""
    import humiditycases as HCS

    dist = {}
    for key, output, names, kw in HCS.AIR_CASES:
        if "exact/" not in key:
            val, scale = HCS.restated("f32", names, output, kw)
            fn = HCS.FUNCTION_OF[output]
            dist[fn] = max(dist.get(fn, 0.0), HCS.f32_distance(key, val, scale, HCS.VECTORS[f"f32/air/{key}"]))
    for key, (val, scale) in HCS.wind_restated("f32").items():
        if "exact/" not in key:
            fn = HCS.WIND_FUNCTION_OF[key.split("/")[0]]
            dist[fn] = max(dist.get(fn, 0.0), HCS.f32_distance(key, val, scale, HCS.VECTORS[f"f32/wind/{key}"]))
    return dist


def known_answers(ns):
    K2C = 273.15
    col = lambda v, u: arr(np.asarray(v, np.float64)[:, None], u)   # noqa: E731
    lst = lambda a: [None if np.isnan(x) else float(x) for x in np.asarray(a, np.float64).ravel()]   # noqa: E731
    ka = {}
    with np.errstate(all="ignore"):
        tas, tdps = [15, 25, 35, 40], [10, 15, 25, 25]
        hurs = ns["relative_humidity"](col(tas, "degC"), col(tdps, "degC"), method="bohren98")
        ka["test_humidex"] = dict(tas_degC=tas, tdps_degC=tdps, expected=[16, 29, 47, 52], decimal=0,
                                  reference_tdps=lst(ns["humidex"](col(tas, "degC"), col(tdps, "degC"))),
                                  reference_tdps_K=lst(ns["humidex"](col(np.array(tas) + K2C, "K"), col(tdps, "degC"))),
                                  reference_hurs=lst(ns["humidex"](col(tas, "degC"), hurs=hurs)), hurs_bohren98=lst(hurs))
        tas = [15, 20, 25, 25, 30, 30, 35, 35, 40, 40, 45, 45]
        hurs = [5, 5, 0, 25, 25, 50, 25, 50, 25, 50, 25, 50]
        ka["test_heat_index"] = dict(tas_degC=tas, hurs=hurs, expected=[None, None, 24, 25, 28, 31, 34, 41, 41, 55, 50, 73], decimal=0,
                                     reference=lst(ns["heat_index"](col(tas, "degC"), col(hurs, "%"))),
                                     reference_K=lst(ns["heat_index"](col(np.array(tas) + K2C, "K"), col(hurs, "%"))))
        tas, wind = (np.array([-1, -10, -20, 10, -15]) + K2C).tolist(), [10, 60, 20, 6, 2]
        ka["test_wind_chill"] = dict(tas_K=tas, sfcWind_kmh=wind, rtol=1e-7,
                                     expected=[-4.509267062481955, -22.619869069856854, -30.478945408950928, None, -16.443],
                                     reference=lst(ns["wind_chill_index"](col(tas, "K"), col(wind, "km/h"))),
                                     reference_US=lst(ns["wind_chill_index"](col(tas, "K"), col(wind, "km/h"), method="US")))
        uas, vas = [3.6, -3.6, -1, 0], [3.6, 3.6, -1, -18]
        w, d = ns["uas_vas_to_sfcwind"](col(uas, "km/h"), col(vas, "km/h"))
        wind, wdir = [float(np.hypot(3.6, 3.6)), float(np.hypot(3.6, 3.6)), float(np.hypot(1, 1)), 18.0], [225, 135, 0, 360]
        uu, vv = ns["sfcwind_to_uas_vas"](col(wind, "km/h"), col(wdir, "degree"))
        ka["TestWindConversion"] = dict(uas_kmh=uas, vas_kmh=vas, wind_kmh=wind, wind_from_dir=wdir, decimals=10,
                                        expected_wind=[x / 3.6 for x in wind], expected_dir=wdir, reference_wind=lst(w), reference_dir=lst(d),
                                        expected_uas=[1, -1, 0, 0], expected_vas=[1, 1, -float(np.hypot(1, 1)) / 3.6, -5],
                                        reference_uas=lst(uu), reference_vas=lst(vv))
        tas = (np.array([-20, -10, -1, 10, 20, 25, 30, 40, 60]) + K2C).tolist()
        tdps = (np.array([-15, -10, -2, 5, 10, 20, 29, 20, 30]) + K2C).tolist()
        ka["test_relative_humidity_dewpoint"] = dict(
            tas_K=tas, tdps_K=tdps, expected_tail=[100, 93, 71, 52, 73, 94, 31, 20], exp0={"clip": 100, "mask": None, "None": 151}, rtol=0.02,
            atol=1, also_in_test_converters=["test_relative_humidity_dewpoint", "test_relative_humidity_dewpoint_clip"],
            reference={m: {str(r): lst(ns["relative_humidity"](col(tas, "K"), tdps=col(tdps, "K"), method=m, invalid_values=r))
                           for r in ("clip", "mask", None)} for m in ("bohren98", "tetens30", "sonntag90", "goffgratch46", "wmo08")})
        ka["test_specific_humidity_from_dewpoint"] = dict(
            tdps_degC=[16.973], ps_Pa=[101325.0], expected=[0.012], decimal=3,
            reference=lst(ns["specific_humidity_from_dewpoint"](col([16.973], "degC"), col([101325.0], "Pa"))))
        tas = (np.array([-1, 10, 20, 25, 30, 40, 60]) + K2C).tolist()
        ps = [101325.0] * 7
        q = ns["specific_humidity_from_dewpoint"](tdps=col(tas, "K"), ps=col(ps, "Pa"), method="buck81")
        ka["test_vapor_pressure"] = dict(tas_K=tas, ps_Pa=ps, rtol=1e-6, huss=lst(q), reference_vp=lst(ns["vapor_pressure"](huss=q, ps=col(ps, "Pa"))),
                                         reference_esat=lst(ns["saturation_vapor_pressure"](col(tas, "K"), method="buck81")))
        hurs = [0, 0.5, 0.8, 0.9, 0.95, 0.99, 1]
        ka["test_vapor_pressure_deficit"] = dict(
            tas_K=tas, hurs=hurs, expected=[567, 1220, 2317, 3136, 4200, 7300, 19717], atol=0.5, rtol=0.005,
            reference={m: lst(ns["vapor_pressure_deficit"](col(tas, "K"), col(hurs, "%"), method=m))
                       for m in ("tetens30", "sonntag90", "goffgratch46", "wmo08", "its90")})
        tas = (np.array([-10, -10, 10, 20, 35, 50, 75, 95]) + K2C).tolist()
        huss, ps = [0.003, 0.001] + [0.005] * 6, [101325.0] * 8
        ka["test_relative_humidity"] = dict(
            tas_K=tas, huss=huss, ps_Pa=ps, ice_thresh_K=273.15, expected_tail=[62.5, 66.0, 35.0, 14.5, 6.5, 2.0, 1.0],
            exp0={"clip": 100, "mask": None, "None": 188}, atol=0.5, rtol=0.005,
            reference={m: {str(r): lst(ns["relative_humidity"](col(tas, "K"), huss=col(huss, "1"), ps=col(ps, "Pa"), method=m, invalid_values=r,
                                                               ice_thresh="0 degC")) for r in ("clip", "mask", None)}
                       for m in ("tetens30", "sonntag90", "goffgratch46", "wmo08")})
        tas = (np.array([20, -10, 10, 20, 35, 50, 75, 95]) + K2C).tolist()
        hurs, ps = [150, 10, 90, 20, 80, 50, 70, 40], (1000 * np.array([100] * 4 + [101] * 4, float)).tolist()
        ka["test_specific_humidity"] = dict(
            tas_K=tas, hurs=hurs, ps_Pa=ps, ice_thresh_K=273.15, expected_tail=[1.6e-4, 6.9e-3, 3.0e-3, 2.9e-2, 4.1e-2, 2.1e-1, 5.7e-1],
            exp0={"clip": 1.4e-2, "mask": None, "None": 2.2e-2}, atol=1e-4, rtol=0.05,
            reference={m: {str(r): lst(ns["specific_humidity"](col(tas, "K"), col(hurs, "%"), col(ps, "Pa"), method=m, invalid_values=r,
                                                               ice_thresh="0 degC")) for r in ("clip", "mask", None)}
                       for m in ("tetens30", "sonntag90", "goffgratch46", "wmo08")})
        huss = np.linspace(0, 0.01, 8).tolist()
        ka["test_dewpoint_from_specific_humidity"] = dict(
            huss=huss, ps_Pa=ps, expected=[None, 260.3, 269.3, 274.8, 279.0, 282.3, 285.0, 287.3], atol=0.1, rtol=0.05,
            reference={m: lst(ns["dewpoint_from_specific_humidity"](col(huss, "1"), col(ps, "Pa"), method=m))
                       for m in ("tetens30", "wmo08", "aerk96", "buck81")})
    return ka


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the humidity vectors can only be regenerated in the build container")
    ns = extract()
    out = {"methods": np.array(METHODS)}
    for tag, dtype in (("f64", np.float64), ("f32", np.float32)):
        rng = np.random.default_rng(20261101)   # (the same fields in both dtypes)
        air_families(ns, rng, dtype, out, tag)
        wind_families(ns, rng, dtype, out, tag)
    known = known_answers(ns)
    path = os.path.join(HERE, "humidity_vectors.npz")
    np.savez_compressed(path, **out)
    for final in (False, True):   # (tests/humiditycases.py reads both files: the distances come from what was written)
        if final:
            known["f32_distance"] = f32_distance()
        with open(os.path.join(HERE, "humidity_known_answers.json"), "w") as fh:
            json.dump(known, fh, indent=1)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")
    for k, v in known["f32_distance"].items():
        print(f"  f32 distance {k}: {v:.3e}")


if __name__ == "__main__":
    main()
