"""Generate tests/golden/thermal_vectors.npz by EXECUTING the reference's thermal-comfort code.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_thermal_golden.py

As tests/golden/make_pet_golden.py: the functions are AST-extracted from src/xclim/indices/converters.py and helpers.py (nothing
is copied into this repository), their decorators and annotations dropped, and their WHOLE bodies executed on numpy arrays,
through np.vectorize where the reference uses numba: ``_utci``, ``_saturation_vapor_pressure_over_water``,
``_saturation_vapor_pressure_over_ice``, ``_wrap_radians`` and ``_sunlit_integral_of_cosine_of_solar_zenith_angle``.

The whole chain is executed too (see "the whole chain" below): ``universal_thermal_climate_index``, ``mean_radiant_temperature``,
``_fdir_ratio``, ``saturation_vapor_pressure``, ``cosine_of_solar_zenith_angle``, ``solar_declination``,
``time_correction_for_solar_angle``, ``distance_from_sun`` and ``day_angle``, on 130 cells and 3 days of daily, hourly (from 00:30)
and 3-hourly rows in the standard and noleap calendars, float64 and float32: one tests/golden/thermal_chain_<case>.npz each (inputs,
``csza``, ``mrt``, ``utci`` for both stats, UTCI with ``mrt`` given).  tests/golden/thermal_known_answers.json records the inputs and
expectations of the reference's own tests next to what the executed reference gives for them.  thermal_vectors.npz holds the leaf
functions (the polynomial over and beyond its validity box, every e_sat method over water and ice and in the three cases, every
branch of the sunlit integral: each of the ten is hit, every pair of compared hour angles lies at least 1e-9 apart).
"""

import ast
import os
import sys

import numpy as np

REF = "/root/reference/src/xclim/indices"
HERE = os.path.dirname(os.path.abspath(__file__))
HELPERS = ["_wrap_radians", "_sunlit_integral_of_cosine_of_solar_zenith_angle"]
CONVERTERS = ["_utci", "_saturation_vapor_pressure_over_water", "_saturation_vapor_pressure_over_ice"]
METHODS = ["sonntag90", "goffgratch46", "its90", "tetens30", "wmo08", "buck81", "aerk96", "ecmwf"]


class _NoOptions:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def extract():
    ns = {"np": np, "xr": type("XR", (), {"set_options": staticmethod(lambda **kw: _NoOptions())})}
    for fname, names in (("helpers.py", HELPERS), ("converters.py", CONVERTERS)):
        path = os.path.join(REF, fname)
        tree = ast.parse(open(path).read())
        body = []
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                node.decorator_list = []
                node.returns = None
                for a in node.args.args + node.args.kwonlyargs:
                    a.annotation = None
                body.append(node)
            elif isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "ESAT_FORMULAS_COEFFICIENTS":
                body.append(node)
        mod = ast.Module(body=body, type_ignores=[])
        ast.fix_missing_locations(mod)
        exec(compile(mod, path, "exec"), ns)
    missing = set(HELPERS + CONVERTERS) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")
    return ns


def branch_of(hss, hs, he, dl):
    """Which of the ten branches the reference's tests select (the order of helpers.py:359-393)."""
    hsr = -hss
    if np.isnan(hss) and dl > 0:
        return 1 if he < hs else 0
    if np.isnan(hss) and dl < 0:
        return 2
    if hs > hss and he < hsr:
        return 3
    if hs < hsr and he < hsr:
        return 4
    if hs > hss and he > hss:
        return 5
    if hs > he >= hsr and hs >= hss:
        return 6
    if he < hs and hs >= hsr >= he:
        return 7
    if hss >= hs > he >= hsr:
        return 8
    return 9


# ---- the whole chain: the public functions on a restated DataArray ---------------------------------------------------------------
# The bodies of universal_thermal_climate_index, mean_radiant_temperature, _fdir_ratio, saturation_vapor_pressure,
# cosine_of_solar_zenith_angle, solar_declination, time_correction_for_solar_angle, distance_from_sun and day_angle are executed
# whole.  Restated: the DataArray (make_pet_golden.Arr: an ndarray with units and a time axis, time on axis 0, row quantities as
# (R, 1) columns), the time coordinate (STime), unit conversion as ONE multiplication (or the temperature offset), cftime.date2num
# (integer microseconds since 2000-01-01 12:00 in the axis's own calendar, divided once), xr.where / apply_ufunc / infer_freq.
# ASSUMPTIONS as make_pet_golden.py: the decimal year is year + (dayofyear - 1 + hours / 24) / days_in_year.
CHAIN_HELPERS = ["_wrap_radians", "distance_from_sun", "day_angle", "solar_declination", "time_correction_for_solar_angle",
                 "cosine_of_solar_zenith_angle", "_sunlit_integral_of_cosine_of_solar_zenith_angle"]
CHAIN_CONVERTERS = ["_utci", "universal_thermal_climate_index", "_fdir_ratio", "mean_radiant_temperature", "saturation_vapor_pressure",
                    "_saturation_vapor_pressure_over_water", "_saturation_vapor_pressure_over_ice"]
CELLS = {}   # the lat / lon the reference gathers from the field's coordinates


def _pet():
    import make_pet_golden as P   # (this directory is sys.path[0] when the generator runs)
    return P


def _ordinal(y, m, d, cal):
    P = _pet()
    y, m, d = (np.asarray(v, np.int64) for v in (y, m, d))
    if cal == "360_day":
        return y * 360 + (m - 1) * 30 + d
    cum = np.concatenate([[0], np.cumsum(P.MLEN)])[:-1]
    doy = cum[m - 1] + d + ((m > 2) & P.leap(y, cal))
    if cal == "noleap":
        return y * 365 + doy
    y1 = y - 1
    return y1 * 365 + y1 // 4 - y1 // 100 + y1 // 400 + doy


class STime:
    """A time coordinate: the days (year, month, day) repeated ``steps`` times, row r at ``offset + (r % steps) * 86400 / steps``
    seconds of its day."""

    dtype = "datetime64[ns]"
    coords, dims = (), ("time",)

    def __init__(self, y, m, d, cal, steps=1, offset=0, hour=0.0):
        P = _pet()
        self.days = P.Time(y, m, d, cal)
        self.calendar, self.steps = cal, steps
        n = len(self.days)
        self.year, self.month, self.day = (np.repeat(v, steps) for v in (self.days.year, self.days.month, self.days.day))
        self.sec = (np.tile(offset + np.arange(steps) * (86400 // steps), n) if steps > 1 else np.full(n, int(hour * 3600))).astype(np.int64)
        self.interval = 86400 // steps
        self.freq = "D" if steps == 1 else "h"
        self.time = self.dt = self

    def __len__(self):
        return len(self.year)

    @property
    def decimal_year(self):
        P = _pet()
        t = P.Time(self.year, self.month, self.day, self.calendar)
        t.hour = self.sec / 3600
        return _arr(np.asarray(t.decimal_year), time=self)

    def epoch_ns(self):
        return (_ordinal(self.year, self.month, self.day, self.calendar) - _ordinal(1970, 1, 1, self.calendar)) * 86400 * 10**9 + self.sec * 10**9

    def astype(self, kind):
        return _arr(self.epoch_ns().astype(np.float64)[:, None], time=self)

    def copy(self, data):
        return _arr(np.asarray(data), time=self)

    def diff(self, dim):
        s = self

        class _D:
            dt = property(lambda d: d)
            seconds = property(lambda d: d)

            def reindex(d, time, method):
                return _arr(np.full((len(s), 1), float(s.interval)), time=s)
        return _D()


def _arr(a, units=None, time=None):
    return _pet().Arr(a, units, time)


def _units(x, target, context=None):
    if isinstance(x, str):
        v, u = x.split(" ", 1)
        v = float(v)
        if u in ("°", "deg") and target == "rad":
            return v * (np.pi / 180)
        if target == "K":
            return {"degC": v + 273.15, "°C": v + 273.15, "K": v}[u]
        raise KeyError((x, target))
    if not hasattr(x, "units"):
        return x
    src = x.units["units"] if isinstance(x.units, dict) else x.units   # (assign_attrs({"units": ...}) hands Arr a dict)
    same = {"degrees_north": "deg", "degrees_east": "deg", "degree_north": "deg", "degree_east": "deg", "degrees": "deg", "m/s": "m s-1"}
    s, t = same.get(src, src), same.get(target, target)
    if s == t:
        return x
    if (s, t) == ("K", "degC"):
        out = x - 273.15
    elif (s, t) == ("degC", "K"):
        out = x + 273.15
    else:
        out = x * {("deg", "rad"): np.pi / 180, ("Pa", "kPa"): 1e-3, ("%", "1"): 1e-2, ("km/h", "m s-1"): 1 / 3.6}[(s, t)]
    return out.assign_attrs(units=target)


def _date2num(time, units, calendar):
    assert units == "days since 2000-01-01 12:00:00"
    us = (_ordinal(time.year, time.month, time.day, time.calendar) - _ordinal(2000, 1, 1, time.calendar)) * 86400 * 10**6 \
        + time.sec * 10**6 - 43200 * 10**6
    return (us / (86400 * 10**6))[:, None]


def extract_chain():
    import types

    P = _pet()

    def apply_ufunc(f, *args, input_core_dims=None, dask=None, output_dtypes=None):
        t = next((a.time for a in args if getattr(a, "time", None) is not None), None)
        bare = [np.asarray(a) if isinstance(a, np.ndarray) else a for a in args]
        out = np.vectorize(f, otypes=[float])(*bare)
        if output_dtypes:
            out = out.astype(output_dtypes[0])
        return _arr(out, time=t)

    def where(c, a, b):
        ref = next((v for v in (b, a, c) if isinstance(v, P.Arr)), None)
        return _arr(np.where(np.asarray(c), np.asarray(a), np.asarray(b)), getattr(ref, "units", None), getattr(ref, "time", None))

    xr = types.SimpleNamespace(DataArray=lambda a, coords=None, dims=None: _arr(a), set_options=lambda **kw: _NoOptions(),
                               apply_ufunc=apply_ufunc, where=where, infer_freq=lambda t: t.freq,
                               CFTimeIndex=None)
    ns = {"np": np, "xr": xr, "nb": None, "cast": lambda t, v: v, "XR2409": True, "_chunk_like": lambda *a, chunks=None: a,
          "convert_units_to": _units, "get_calendar": lambda d: d.calendar, "ensure_cftime_array": lambda d: d,
          "cftime": types.SimpleNamespace(date2num=_date2num), "CFTimeIndex": None,
          "_gather_lat": lambda da: CELLS["lat"], "_gather_lon": lambda da: CELLS["lon"]}
    for fname, names in (("helpers.py", CHAIN_HELPERS), ("converters.py", CHAIN_CONVERTERS)):
        path = os.path.join(REF, fname)
        tree = ast.parse(open(path).read())
        body = []
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                node.decorator_list = []
                node.returns = None
                for a in node.args.args + node.args.kwonlyargs:
                    a.annotation = None
                body.append(node)
            elif isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "ESAT_FORMULAS_COEFFICIENTS":
                body.append(node)
        mod = ast.Module(body=body, type_ignores=[])
        ast.fix_missing_locations(mod)
        exec(compile(mod, path, "exec"), ns)
    missing = set(CHAIN_HELPERS + CHAIN_CONVERTERS) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")
    return ns


def grid(C):
    """The cells of the chain cases: pole to pole, and twelve cells just equatorward of each polar circle at longitudes that put local
    midnight early, in the middle and late in a three-hour interval (the three midnight-crossing branches)."""
    rng = np.random.default_rng(7)
    band = np.repeat([65.5, 66.0, 66.4], 4)
    lat = np.concatenate([np.linspace(-89, 89, C - 24), band, -band])
    lon = np.concatenate([np.round(rng.uniform(-180, 360, C - 24), 2), np.tile([5.0, 16.0, 27.0, 38.0], 6)])
    return lat, lon


def weather(R, C, rng, dtype):
    """Fields with a good half of the samples inside the validity box, and every family of the kernel's decisions: rsds <= 0, winds
    below 0.5, exactly 0.5 and above 17, temperatures and radiant temperatures beyond the box, a NaN stripe in every field."""
    tas = rng.uniform(252, 318, (R, C))
    sig = 5.67e-8
    f = {"tas": tas, "hurs": rng.uniform(3, 100, (R, C)), "sfcWind": rng.uniform(0.6, 16, (R, C)),
         "rsds": np.where(rng.random((R, C)) < 0.1, rng.uniform(-5, 0, (R, C)), np.where(rng.random((R, C)) < 0.1, rng.uniform(250, 1000, (R, C)), rng.uniform(0, 250, (R, C)))),
         "rlds": 0.8 * sig * tas**4 + rng.uniform(-30, 30, (R, C)), "rlus": sig * tas**4 + rng.uniform(-20, 40, (R, C))}
    f["rsus"] = 0.2 * np.abs(f["rsds"])
    f["sfcWind"].flat[::7] = 0.5
    f["sfcWind"].flat[3::23] = rng.uniform(0.0, 0.49, f["sfcWind"].flat[3::23].shape)
    f["sfcWind"].flat[5::29] = rng.uniform(17.01, 20, f["sfcWind"].flat[5::29].shape)
    f["tas"].flat[2::31] = rng.choice([221.0, 223.0, 323.3, 325.0], f["tas"].flat[2::31].shape)
    f["rlds"].flat[4::37] += rng.choice([-250.0, 350.0], f["rlds"].flat[4::37].shape)
    for k, n in enumerate(sorted(f)):
        f[n].flat[k * 3 + 1::41] = np.nan
    return {k: np.round(v, 3).astype(dtype) for k, v in f.items()}


UNITS = {"tas": "K", "hurs": "%", "sfcWind": "m s-1", "rsds": "W m-2", "rsus": "W m-2", "rlds": "W m-2", "rlus": "W m-2", "mrt": "K"}
CHAIN = [  # name, calendar, steps per day, offset seconds, dtype
    ("daily_std_f64", "standard", 1, 0, np.float64), ("hourly_std_f64", "standard", 24, 1800, np.float64),
    ("hourly_noleap_f32", "noleap", 24, 1800, np.float32), ("3hourly_noleap_f64", "noleap", 8, 0, np.float64),
    ("3hourly_std_f32", "standard", 8, 0, np.float32), ("daily_noleap_f32", "noleap", 1, 0, np.float32)]


def chain(out, known):
    ns = extract_chain()
    P = _pet()
    C = 130
    lat, lon = grid(C)
    CELLS.update(lat=_arr(lat, "degrees_north"), lon=_arr(lon, "degrees_east"))
    out.update(chain_names=np.array([c[0] for c in CHAIN]), chain_lat=lat, chain_lon=lon)
    rng = np.random.default_rng(20261021)
    branches = set()
    for name, cal, steps, offset, dtype in CHAIN:
        days = P.Time.daily(2001, 6, 20, 3, cal)
        t = STime(days.year, days.month, days.day, cal, steps, offset)
        R = len(t)
        f = weather(R, C, rng, dtype)
        a = {k: _arr(v, UNITS[k], t) for k, v in f.items()}
        with np.errstate(all="ignore"):
            dec = ns["solar_declination"](t)
            cs = {"sunlit": ns["cosine_of_solar_zenith_angle"](t, dec, CELLS["lat"], lon=CELLS["lon"], stat="average", sunlit=True),
                  "instant": ns["cosine_of_solar_zenith_angle"](t, dec, CELLS["lat"], lon=CELLS["lon"], stat="instant",
                                                               time_correction=ns["time_correction_for_solar_angle"](t))}
            tt = np.abs(np.tan(np.asarray(ns["_wrap_radians"](lat * (np.pi / 180))))[None, :] * np.tan(np.asarray(dec)))
            assert np.all(np.abs(tt - 1) > 1e-6), name
            p = f"chain/{name}/"
            for k, v in f.items():
                out[p + k] = v
            out[p + "meta"] = np.array([cal, str(steps), str(offset), np.dtype(dtype).name])
            for stat in ("sunlit", "instant"):
                mrt = ns["mean_radiant_temperature"](a["rsds"], a["rsus"], a["rlds"], a["rlus"], stat=stat)
                utci = ns["universal_thermal_climate_index"](a["tas"], a["hurs"], a["sfcWind"], rsds=a["rsds"], rsus=a["rsus"],
                                                             rlds=a["rlds"], rlus=a["rlus"], stat=stat)
                out[p + f"csza_{stat}"], out[p + f"mrt_{stat}"], out[p + f"utci_{stat}"] = (np.asarray(v) for v in (cs[stat], mrt, utci))
                assert np.asarray(cs[stat]).shape == (R, C) and np.asarray(utci).dtype == dtype, (name, np.asarray(utci).dtype)
                assert np.isfinite(np.asarray(utci)).mean() >= 0.5, (name, np.isfinite(np.asarray(utci)).mean())
            mrt_in = _arr((f["tas"].astype(np.float64) + rng.uniform(-33, 33, (R, C))).round(2).astype(dtype), "K", t)
            out[p + "mrt_in"] = np.asarray(mrt_in)
            for tag, kw in (("given", {}), ("given_cap_nomask", dict(mask_invalid=False, wind_cap_min=True))):
                out[p + f"utci_{tag}"] = np.asarray(ns["universal_thermal_climate_index"](a["tas"], a["hurs"], a["sfcWind"], mrt=mrt_in, **kw))
        case = {k[len(p):]: out.pop(k) for k in [k for k in out if k.startswith(p)]}   # one file per case: each stays below 1 MiB
        np.savez_compressed(os.path.join(HERE, f"thermal_chain_{name}.npz"), **case)
        if steps > 1:   # which branches the sunlit averages of this case took
            h0 = ((t.sec % 86400) / 86400) * 2 * np.pi + np.pi
            hs = h0[:, None] + (lon * (np.pi / 180))[None, :]
            he = hs + 2 * np.pi * t.interval / 86400
            w = lambda x: np.asarray(ns["_wrap_radians"](x))   # noqa: E731
            latr = w(lat * (np.pi / 180))
            with np.errstate(invalid="ignore"):
                tn = -np.tan(latr)[None, :] * np.tan(np.asarray(dec))
                hss = w(np.arccos(np.where(np.abs(tn) <= 1, tn, np.nan)))
            hs, he = w(hs), w(he)
            for x, y in ((hs, hss), (hs, -hss), (he, hss), (he, -hss), (hs, he)):
                with np.errstate(invalid="ignore"):
                    assert not np.any(np.abs(x - y) < 1e-9), name
            dl = np.asarray(dec) * latr[None, :]
            branches |= {branch_of(*v) for v in zip(hss.ravel(), hs.ravel(), he.ravel(), dl.ravel())}
    assert branches == set(range(10)), sorted(branches)
    # e_sat of the chain: every method in the three cases, both sides of both thresholds
    tas = np.concatenate([rng.uniform(200, 330, 60).round(2), [250.15, 250.17, 273.14, 273.16, 273.17]])
    out["esat_case_tas"] = tas
    cases = {"water": {}, "binary": dict(ice_thresh="0 degC"), "interp": dict(ice_thresh="-23 degC", interp_power=2)}
    for cname, kw in cases.items():
        out[f"esat_case_{cname}"] = np.stack([np.asarray(ns["saturation_vapor_pressure"](_arr(tas, "K"), method=m, **kw)) for m in METHODS])
    # ---- the known answers of the reference's own tests: inputs, what the executed reference gives, what its tests expect -------
    K2C = 273.15
    one = STime([2000], [7], [1], "standard")
    ka = []
    for cap, wind, exp in ((False, 2, 17.70), (False, 1, None), (True, 1, 17.76)):
        v = ns["universal_thermal_climate_index"](_arr(np.array([[16 + K2C]]), "K", one), _arr(np.array([[36.0]]), "%", one),
                                                  _arr(np.array([[float(wind)]]), "km/h", one), mrt=_arr(np.array([[22 + K2C]]), "K", one),
                                                  wind_cap_min=cap)
        ka.append(dict(tas=16 + K2C, hurs=36.0, sfcWind_kmh=wind, mrt=22 + K2C, wind_cap_min=cap, expected=exp, rtol=1e-3,
                       reference=None if np.isnan(float(np.asarray(v)[0, 0])) else float(np.asarray(v)[0, 0])))
    known["test_universal_thermal_climate_index"] = ka
    CELLS.update(lat=_arr(np.array([-21.45]), "degrees_north"), lon=_arr(np.array([133.125]), "degrees_east"))
    rad = [_arr(np.array([[v]]), "W m-2", one) for v in (195.08, 36.686, 294.91, 396.19)]
    known["test_mean_radiant_temperature"] = [
        dict(rsds=195.08, rsus=36.686, rlds=294.91, rlus=396.19, lat=-21.45, lon=133.125, start="2000-07-01", stat=s, expected=e, rtol=1e-3,
             reference=float(np.asarray(ns["mean_radiant_temperature"](*rad, stat=s))[0, 0])) for s, e in (("sunlit", 295.0), ("instant", 294.9))]
    exp_czda = [[0.0, 0.0610457, 0.0], [0.09999178, 0.18221077, 0.0], [0.31387116, 0.285383, 0.0], [0.52638271, 0.35026199, 0.0],
                [0.70303168, 0.37242693, 0.0]]
    sites = dict(lat=[0.0, 45.0, 70.0], lon=[-40.0, 0.0, 80.0])
    known["test_cosine_of_solar_zenith_angle"] = []
    for cal in ("standard", "noleap"):
        t2 = STime([1900, 1900], [1, 1], [1, 2], cal, 24, 1800)
        got = ns["cosine_of_solar_zenith_angle"](t2, ns["solar_declination"](t2), _arr(np.array(sites["lat"]), "degree_north"),
                                                 _arr(np.array(sites["lon"]), "degree_east"), stat="average", sunlit=True)
        known["test_cosine_of_solar_zenith_angle"].append(dict(calendar=cal, start="1900-01-01", days=2, steps_per_day=24, offset_seconds=1800,
                                                               rows=[7, 12], expected=exp_czda, rtol=1e-3, reference=np.asarray(got)[7:12].tolist(), **sites))
    tas10 = (np.array([-30, -20, -10, -1, 10, 20, 25, 30, 40, 60]) + K2C)
    tail = [1228, 2339, 3169, 4247, 7385, 19947]
    known["test_saturation_vapor_pressure"] = [
        dict(tas=tas10.tolist(), methods=["tetens30", "sonntag90", "goffgratch46", "wmo08", "its90", "buck81", "aerk96", "ecmwf"], ice_thresh=it,
             interp_power=pw, expected=e0 + tail, atol=0.5, rtol=0.005, tetens30_skips_first=True)
        for it, pw, e0 in ((None, None, [51, 125, 286, 568]), (273.15, None, [38, 103, 260, 563]), (250.15, 2, [38, 103, 268, 568]))]
    known["test_saturation_vapor_pressure_converters"] = dict(tas=tas10[1:].tolist(), method="sonntag90", ice_thresh=273.15,
                                                              expected=[103, 260, 563] + tail, atol=0.5, rtol=0.005)


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the thermal vectors can only be regenerated in the build container")
    ns = extract()
    rng = np.random.default_rng(20261020)
    out = {"methods": np.array(METHODS)}
    # the polynomial: inside the validity box and a margin around it
    n = 400
    ta, va = rng.uniform(-55, 55, n), rng.uniform(0.0, 20, n)
    dt, pa = rng.uniform(-35, 35, n), rng.uniform(0, 5, n)
    out.update(poly_ta=ta, poly_va=va, poly_dt=dt, poly_pa=pa, poly_utci=np.vectorize(ns["_utci"], otypes=[float])(ta, va, dt, pa))
    # e_sat of every method over water and over ice
    t = np.concatenate([rng.uniform(180, 330, 120), [250.16, 273.15, 273.16, 273.17]])
    out["esat_tas"] = t
    out["esat_water"] = np.stack([np.asarray(ns["_saturation_vapor_pressure_over_water"](t, m)) for m in METHODS])
    out["esat_ice"] = np.stack([np.asarray(ns["_saturation_vapor_pressure_over_ice"](t, m)) for m in METHODS])
    # the sunlit average: latitudes up to the poles, declinations of the year, intervals of 1, 3, 8 and 24 hours from any start
    m = 6000
    lat = ns["_wrap_radians"](np.deg2rad(np.concatenate([rng.uniform(-89.9, 89.9, m - 2000), rng.uniform(60, 89.9, 1000), rng.uniform(-89.9, -60, 1000)])))
    dec = rng.uniform(-0.409, 0.409, m)
    with np.errstate(invalid="ignore"):
        tt = -np.tan(lat) * np.tan(dec)
        hss = ns["_wrap_radians"](np.arccos(np.where(np.abs(tt) <= 1, tt, np.nan)))
    start = rng.uniform(0, 2 * np.pi, m) + np.pi
    hs = ns["_wrap_radians"](start)
    he = ns["_wrap_radians"](start + 2 * np.pi * rng.choice([1, 3, 8, 23.9], m) / 24)
    keep = np.abs(np.abs(tt) - 1) > 1e-6
    for a, b in ((hs, hss), (hs, -hss), (he, hss), (he, -hss), (hs, he)):
        with np.errstate(invalid="ignore"):
            keep &= ~(np.abs(a - b) < 1e-9)
    lat, dec, hss, hs, he = (v[keep] for v in (lat, dec, hss, hs, he))
    br = np.array([branch_of(*v) for v in zip(hss, hs, he, dec * lat)])
    assert set(br) == set(range(10)), f"branches hit: {sorted(set(br))}"
    f = np.vectorize(ns["_sunlit_integral_of_cosine_of_solar_zenith_angle"], otypes=[float])
    with np.errstate(invalid="ignore"):
        out.update(sun_lat=lat, sun_dec=dec, sun_hss=hss, sun_hs=hs, sun_he=he, sun_branch=br, sun_avg=f(dec, lat, hss, hs, he, True))
    known = {}
    chain(out, known)
    import json

    with open(os.path.join(HERE, "thermal_known_answers.json"), "w") as fh:
        json.dump(known, fh, indent=1)
    path = os.path.join(HERE, "thermal_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; branches", np.bincount(br))


if __name__ == "__main__":
    main()
