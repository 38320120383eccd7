"""Generate tests/golden/pet_vectors.npz by EXECUTING the reference's potential evapotranspiration code.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_pet_golden.py

src/xclim/indices/converters.py and helpers.py cannot be imported here (xarray, pint, numba, cftime).  The functions below
are AST-extracted (nothing is copied into this repository) with their decorators and annotations dropped, and their
WHOLE bodies are executed on numpy arrays: ``potential_evapotranspiration`` (every method branch), ``water_budget``,
``fao_allen98``, ``_saturation_vapor_pressure_over_water`` (sonntag90), and from helpers.py ``day_angle``,
``solar_declination``, ``eccentricity_correction_factor``, ``cosine_of_solar_zenith_angle``,
``_sunlit_integral_of_cosine_of_solar_zenith_angle`` (through np.vectorize, as numba's vectorize), ``_wrap_radians``,
``extraterrestrial_solar_radiation``, ``day_lengths`` and ``wind_speed_height_conversion``.

Only the xarray / pint plumbing they call is restated (``Arr`` below, an ndarray that carries its units and time axis):
unit conversion (``convert_units_to`` for the units these bodies use), ``resample`` with NaN-skipping means and sums
(float32 means as float64 sums rounded once to float32), ``infer_freq``, ``apply_ufunc``, ``where`` / ``concat``,
``_get_D_from_M``, the decimal year behind ``time.dt.decimal_year`` and ``amount2rate``.  Two of these are ASSUMPTIONS that
could not be executed here, because xarray and pint are absent: the decimal year is taken as
``year + (dayofyear - 1 + hour / 24) / days_in_year`` (days_in_year of the calendar), and pint's month is 365.25 / 12
days (the hydro-context ``mm/month`` of DA02).  pint's conversion factors are applied as one multiplication (or the offset
formula for temperatures).

Every case stores its inputs TIME FIRST as int16 tenths of the CF units (pr in tenths of mm/day; ``decode``), the cell
latitudes, the time axis and time of day, and the outputs ``pet`` (and ``wb`` where the water budget is checked) with
their dtype.  The first case also stores the solar tables ``ra`` [J m-2 d-1] and ``dl`` [h] of its rows and latitudes.
tests/test_pet_cpu.py and tests/test_gpu_pet.py read them.
"""

import ast
import contextlib
import os
import sys
import types

import numpy as np

REF = "/root/reference/src/xclim/indices"
HERE = os.path.dirname(os.path.abspath(__file__))
HELPERS = ["_wrap_radians", "day_angle", "solar_declination", "eccentricity_correction_factor",
           "cosine_of_solar_zenith_angle", "_sunlit_integral_of_cosine_of_solar_zenith_angle",
           "extraterrestrial_solar_radiation", "day_lengths", "wind_speed_height_conversion"]
CONVERTERS = ["_saturation_vapor_pressure_over_water", "fao_allen98", "potential_evapotranspiration", "water_budget"]
MLEN = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])
CANON = {"baierrobertson65": "BR65", "hargreaves85": "HG85", "mcguinnessbordne05": "MB05", "thornthwaite48": "TW48",
         "allen98": "FAO_PM98", "droogersallen02": "DA02"}
CANON.update({v: v for v in list(CANON.values())})
LATS = np.array([0.0, 45.0, -45.0, 67.0, -67.0, 80.0, -80.0])


# ---- the restated plumbing ------------------------------------------------------------------------------------------
def leap(y, cal):
    y = np.asarray(y)
    if cal == "julian":
        return y % 4 == 0
    if cal in ("noleap", "360_day"):
        return np.zeros(y.shape, bool)
    if cal == "all_leap":
        return np.ones(y.shape, bool)
    return ((y % 4 == 0) & (y % 100 != 0)) | (y % 400 == 0)


def mlen(y, m, cal):
    return np.full(np.shape(y), 30) if cal == "360_day" else MLEN[np.asarray(m) - 1] + ((np.asarray(m) == 2) & leap(y, cal))


class Time:
    """A time coordinate: daily rows (freq "D") or month starts (freq "MS")."""

    def __init__(self, y, m, d, cal, hour=0.0, freq="D"):
        self.year, self.month, self.day = (np.asarray(v, np.int64) for v in (y, m, d))
        self.calendar, self.hour, self.freq = cal, float(hour), freq
        self.time = self
        self.dt = self

    def __len__(self):
        return len(self.year)

    @property
    def decimal_year(self):  # ASSUMPTION (see the module docstring)
        if self.calendar == "360_day":
            doy, diy = (self.month - 1) * 30 + self.day, 360.0
        else:
            cum = np.concatenate([[0], np.cumsum(MLEN)])[:-1]
            doy = cum[self.month - 1] + self.day + ((self.month > 2) & leap(self.year, self.calendar))
            diy = 365.0 + leap(self.year, self.calendar)
        return Arr((self.year + (doy - 1 + self.hour / 24) / diy)[:, None], time=self)

    @staticmethod
    def daily(y, m, d, n, cal, hour=0.0):
        ys, ms, ds = [], [], []
        for _ in range(n):
            ys.append(y), ms.append(m), ds.append(d)
            d += 1
            if d > mlen(y, m, cal):
                d, m = 1, m + 1
                if m > 12:
                    m, y = 1, y + 1
        return Time(ys, ms, ds, cal, hour)


class Arr(np.ndarray):
    """numpy array with the units and the time axis a DataArray would carry (time on axis 0)."""

    def __new__(cls, a, units=None, time=None):
        obj = np.asarray(a).view(cls)
        obj.units, obj.time = units, time
        return obj

    def __array_finalize__(self, obj):
        self.units = getattr(obj, "units", None)
        self.time = getattr(obj, "time", None)

    def __array_wrap__(self, arr, context=None, return_scalar=False):
        out = super().__array_wrap__(arr, context, return_scalar)
        if isinstance(out, Arr) and out.time is None and context is not None:  # any operand's time axis
            out.time = next((a.time for a in context[1] if getattr(a, "time", None) is not None), None)
        return out

    chunksizes = None
    coords = ()

    @property
    def attrs(self):
        return {"units": self.units}

    def assign_attrs(self, units=None, **kw):
        out = self.view(Arr)
        out.units = units if units is not None else self.units
        return out

    def where(self, cond, other=np.nan):
        return Arr(np.where(np.asarray(cond), np.asarray(self), other), self.units, self.time)

    def rename(self, name):
        return self

    def resample(self, time):
        return Resampled(self, time)

    def isel(self, time):
        return Arr(np.asarray(self)[time], self.units, Time(self.time.year[time], self.time.month[time],
                                                             self.time.day[time], self.time.calendar, freq="MS"))

    def sel(self, time):
        return Arr(np.asarray(self)[time], self.units)


class Resampled:
    def __init__(self, da, freq):
        self.da, self.freq = da, freq
        t = da.time
        key = t.year * 12 + t.month - 1 if freq == "MS" else t.year
        self.keys, self.starts = np.unique(key, return_index=True)
        self.edges = np.append(self.starts, len(key))
        if freq == "MS":
            self.labels = Time(self.keys // 12, self.keys % 12 + 1, np.ones_like(self.keys), t.calendar, freq="MS")
        else:
            self.labels = Time(self.keys, np.ones_like(self.keys), np.ones_like(self.keys), t.calendar, freq="YS")

    @property
    def groups(self):
        return {i: np.arange(a, b) for i, (a, b) in enumerate(zip(self.edges[:-1], self.edges[1:]))}

    def _red(self, fn):
        x = np.asarray(self.da)
        out = np.stack([fn(x[a:b]) for a, b in zip(self.edges[:-1], self.edges[1:])])
        return Arr(out, self.da.units, self.labels)

    def mean(self, dim="time", keep_attrs=False):  # float32: a float64 sum rounded once
        def m(v):
            n = np.sum(~np.isnan(v), axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                return (np.nansum(v.astype(np.float64), axis=0) / n).astype(v.dtype)
        return self._red(m)

    def sum(self, dim="time"):
        return self._red(lambda v: np.nansum(v, axis=0).astype(v.dtype))


_FACTORS = {("J m-2 d-1", "cal cm-2 day-1"): 1e-4 / 4.184, ("J m-2 d-1", "MJ m-2 d-1"): 1e-6,
            ("W m-2", "MJ m-2 d-1"): 86400 / 1e6, ("Pa", "kPa"): 1e-3, ("%", "1"): None,
            ("kg m-2 s-1", "mm/month"): 365.25 / 12 * 86400, ("degrees_north", "rad"): np.pi / 180,
            ("degrees_north", "deg"): 1.0}
_SAME = {"m s-1", "kPa", "kPa degC-1", "MJ m-2 d-1", "MJ m-2 day-1", "rad", "kg m-2 s-1"}


def convert_units_to(x, target, context=None):
    if isinstance(x, str):  # quantities written in the bodies
        v, u = x.split(" ", 1)
        v = float(v)
        return {("W m-2", "J m-2 d-1"): v * 86400.0, ("m", "m"): v, ("°", "rad"): v * np.pi / 180,
                ("kPa degC", "kPa degC"): v, ("MJ m-2 day-1", "MJ m-2 day-1"): v}[(u, target)]
    src = x.units
    if src == target or (src in _SAME and target in _SAME and src.replace("day", "d") == target.replace("day", "d")):
        return x
    if (src, target) == ("K", "degC"):
        out = x - 273.15
    elif (src, target) == ("degC", "K"):
        out = x + 273.15
    elif (src, target) == ("K", "degF"):
        out = (x - (233.15 + 200 / 9)) / (5 / 9)
    elif (src, target) == ("%", "1"):
        out = x / 100
    else:
        out = x * _FACTORS[(src, target)]
    return out.assign_attrs(units=target)


def amount2rate(pet, out_units="mm/d"):
    t = pet.time
    if t is None or t.freq == "D":  # the daily bodies' products may carry the time-less solar table's metadata
        return pet.assign_attrs(units="mm/d")
    dt = mlen(t.year, t.month, t.calendar)[:, None] * 86400.0
    return ((pet / dt) * 86400.0).assign_attrs(units="mm/d")


def to_si(x, target, context=None):
    if x.units == "mm/d":
        return (x / 86400).assign_attrs(units=target)
    return convert_units_to(x, target, context)


def _get_D_from_M(time):
    y0, m0 = int(time.year[0]), int(time.month[0])
    y1, m1 = int(time.year[-1]), int(time.month[-1])
    n = int(sum(mlen(y, m, time.calendar) for y, m in _month_iter(y0, m0, y1, m1)))
    return Time.daily(y0, m0, 1, n, time.calendar)


def _month_iter(y, m, y1, m1):
    while (y, m) <= (y1, m1):
        yield y, m
        m += 1
        if m > 12:
            y, m = y + 1, 1


@contextlib.contextmanager
def _opts(**kw):
    yield


def apply_ufunc(f, *args, input_core_dims=None, dask=None):
    t = next((a.time for a in args if getattr(a, "time", None) is not None), None)
    return Arr(np.vectorize(f, otypes=[float])(*[np.asarray(a) if isinstance(a, Arr) else a for a in args]), time=t)


XR = types.SimpleNamespace(
    DataArray=Arr, set_options=_opts, apply_ufunc=apply_ufunc, concat=lambda xs, dim: Arr(np.concatenate(xs), xs[0].units),
    where=lambda c, a, b: Arr(np.where(np.asarray(c), a, np.asarray(b)), getattr(b, "units", None), getattr(b, "time", None)),
    infer_freq=lambda t: t.freq)


def extract():
    ns = {"np": np, "xr": XR, "cast": lambda t, v: v, "XR2409": True, "_chunk_like": lambda *a, chunks=None: a,
          "amount2rate": amount2rate, "ESAT_FORMULAS_COEFFICIENTS": {}, "_get_D_from_M": _get_D_from_M,
          "_gather_lat": None}

    def conv(x, target, context=None):
        return to_si(x, target, context) if target == "kg m-2 s-1" and getattr(x, "units", None) == "mm/d" else \
            convert_units_to(x, target, context)

    ns["convert_units_to"] = conv
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
        mod = ast.Module(body=body, type_ignores=[])
        ast.fix_missing_locations(mod)
        exec(compile(mod, path, "exec"), ns)
    missing = set(HELPERS + CONVERTERS) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")

    def svp(tas, ice_thresh=None, method="sonntag90"):  # converters.py:492-...: the all-water branch, in Pa
        return ns["_saturation_vapor_pressure_over_water"](conv(tas, "K"), method).assign_attrs(units="Pa")

    ns["saturation_vapor_pressure"] = svp
    return ns


# ---- cases ---------------------------------------------------------------------------------------------------------
def encode(a):
    q = np.round(np.asarray(a, np.float64) * 10)
    q[np.isnan(q)] = -32768
    return q.astype(np.int16)


def decode(q, dtype, pr=False):
    """The field the reference saw: tenths in float64 (pr: mm/day -> kg m-2 s-1), then the case's dtype; -32768 = NaN."""
    v = np.where(q == -32768, np.nan, q.astype(np.float64) / 10)
    if pr:
        v = v / 86400
    return v.astype(dtype)


def weather(rng, t, C, lats, cold=()):
    T = len(t)
    doy = np.arange(T)[:, None]
    season = np.sign(lats + 1e-9)[None, :] * np.cos(2 * np.pi * (doy - 200) / 365.0)
    base = 300 - 0.45 * np.abs(lats)[None, :] + 12 * season + rng.normal(0, 2.5, (T, C))
    for c in cold:
        base[:, c] = 262 + 4 * season[:, c] + rng.normal(0, 1.5, T)
    rng_ = rng.uniform(3, 14, (T, C))
    f = {"tasmin": base - rng_ / 2, "tasmax": base + rng_ / 2, "tas": base + rng.normal(0, 0.7, (T, C)),
         "hurs": np.clip(rng.normal(65, 18, (T, C)), 5, 100), "rsds": np.clip(rng.normal(180, 80, (T, C)), 0, 400)}
    f["rsus"] = 0.23 * f["rsds"]
    f["rlds"] = rng.uniform(250, 380, (T, C))
    f["rlus"] = f["rlds"] + rng.uniform(20, 90, (T, C))
    f["sfcWind"] = np.abs(rng.normal(4, 2, (T, C)))
    f["pr"] = np.where(rng.random((T, C)) < 0.4, rng.gamma(0.7, 8, (T, C)), 0.0)  # mm/day
    return {k: encode(v) for k, v in f.items()}


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the pet vectors can only be regenerated in the build container")
    ns = extract()
    pet_f, wb_f = ns["potential_evapotranspiration"], ns["water_budget"]
    rng = np.random.default_rng(20261015)
    C = len(LATS)
    specs = [  # name, method, dtype, calendar, start, T, hour, options
        ("br65_f32_noon", "BR65", np.float32, "standard", (2000, 2, 10), 90, 12.0, {"wb": True, "solar": True}),
        ("br65_f64", "baierrobertson65", np.float64, "noleap", (2001, 6, 1), 60, 0.0, {}),
        ("hg85_f32_tas", "HG85", np.float32, "standard", (2003, 12, 1), 70, 0.0, {"tas": True}),
        ("hg85_f64_nan", "hargreaves85", np.float64, "360_day", (2002, 3, 1), 80, 0.0, {"nan": True}),
        ("mb05_f32_custom", "MB05", np.float32, "standard", (2004, 2, 20), 60, 0.0, {"tas": True, "peta": 0.0147,
                                                                                 "petb": 0.07353}),
        ("mb05_f64_minmax", "mcguinnessbordne05", np.float64, "all_leap", (2001, 9, 1), 60, 12.0, {}),
        ("fao_f32_nan", "FAO_PM98", np.float32, "standard", (2001, 5, 1), 90, 12.0, {"nan": True}),
        ("fao_f64", "allen98", np.float64, "julian", (1900, 2, 20), 60, 0.0, {}),
        ("tw48_f32_partial", "TW48", np.float32, "standard", (2000, 3, 15), 430, 0.0, {"cold": (5,), "nan": True,
                                                                                       "wb": True}),
        ("tw48_f64_tas", "thornthwaite48", np.float64, "noleap", (2001, 1, 1), 400, 0.0, {"tas": True, "cold": (6,)}),
        ("da02_f32_partial", "DA02", np.float32, "360_day", (2001, 2, 11), 420, 0.0, {"nan": True, "wet": (2,)}),
        ("da02_f64_tas", "droogersallen02", np.float64, "standard", (2003, 11, 5), 400, 12.0, {"tas": True, "wet": (1,)}),
    ]
    out = {"names": np.array([s[0] for s in specs]), "lats": LATS}
    for name, method, dt, cal, (y, m, d), T, hour, opt in specs:
        t = Time.daily(y, m, d, T, cal, hour)
        q = weather(rng, t, C, LATS, cold=opt.get("cold", ()))
        for c in opt.get("wet", ()):  # DA02's ab < 0: more rain than the temperature range
            q["pr"][:, c] = encode(np.full(T, 60.0))
        if opt.get("nan"):
            for k in q:
                q[k][rng.random((T, C)) < 0.03] = -32768
            q["tasmax"][T // 3: T // 3 + 40, 4] = -32768  # a whole month (monthly methods) without tasmax at one cell
        use = {"tasmin", "tasmax", "pr", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind"} | (
            {"tas"} if opt.get("tas") else set())
        units = {"tasmin": "K", "tasmax": "K", "tas": "K", "hurs": "%", "rsds": "W m-2", "rsus": "W m-2", "rlds": "W m-2",
                 "rlus": "W m-2", "sfcWind": "m s-1", "pr": "kg m-2 s-1"}
        fld = {k: Arr(decode(q[k], dt, pr=k == "pr"), units[k], t) for k in use}
        lat = Arr(LATS, "degrees_north")
        kw = dict(tasmin=fld["tasmin"], tasmax=fld["tasmax"], tas=fld.get("tas"), lat=lat, hurs=fld["hurs"],
                  rsds=fld["rsds"], rsus=fld["rsus"], rlds=fld["rlds"], rlus=fld["rlus"], sfcWind=fld["sfcWind"])
        extra = {k: opt[k] for k in ("peta", "petb") if k in opt}
        with np.errstate(invalid="ignore", divide="ignore"):
            pet = pet_f(**kw, pr=fld["pr"], method=method, **extra)
            wb = wb_f(fld["pr"], **kw, method=method) if opt.get("wb") else None
        p = f"{name}/"
        reads = {"BR65": {"tasmin", "tasmax"}, "HG85": {"tasmin", "tasmax", "tas"}, "DA02": {"tasmin", "tasmax", "tas", "pr"},
                 "FAO_PM98": {"tasmin", "tasmax", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind"},
                 "MB05": {"tas"} if opt.get("tas") else {"tasmin", "tasmax"},
                 "TW48": {"tas"} if opt.get("tas") else {"tasmin", "tasmax"}}[CANON[method]]
        for k in use & (reads | ({"pr"} if opt.get("wb") else set())):  # the fields the method reads
            out[p + k] = q[k]
        out[p + "meta"] = np.array([method, np.dtype(dt).name, cal, str(hour), str(extra.get("peta", "")),
                                    str(extra.get("petb", ""))])
        out[p + "start"] = np.array([y, m, d, T])
        out[p + "pet"] = np.asarray(pet)
        out[p + "pet_dtype"] = np.array(np.asarray(pet).dtype.name)
        if wb is not None:
            out[p + "wb"] = np.asarray(wb)
        if opt.get("solar"):
            with np.errstate(invalid="ignore"):
                out[p + "ra"] = np.asarray(ns["extraterrestrial_solar_radiation"](t, lat))
                out[p + "dl"] = np.asarray(ns["day_lengths"](t, lat))
        print(name, method, np.asarray(pet).dtype, np.asarray(pet).shape, "NaN", int(np.isnan(np.asarray(pet)).sum()))
    path = os.path.join(HERE, "pet_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
