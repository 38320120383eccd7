"""Writes tests/golden/agro_vectors.npz: seeded fields and the values the numpy restatement tests/agrocpu.py gives for them,
each with its SCALE (the sum of the absolute day or month terms that went into it), for xclim_amd/csrc/agro.hip.

The restatement is the oracle (the reference's own code needs xarray); before anything is written it must reproduce every
reproducible known answer of the reference's own tests (tests/test_agro_cpu.py: check_known_answers(), on the recorded values of
tests/golden/agro_known_answers.json), and no case may sit within 1e-9 of a comparison whose outcome rounding could change:

- EGDD compares computed temperatures with its thresholds: ``min_gap`` of the restatement is the smallest distance, asserted.
- The monthly outputs compare nothing that is computed.  The hemisphere tests of CNI (lat > 0) and DI (lat >= 0) are made on
  the latitude as given, so 0.0 and -0.0, which sit on them on purpose, fall on one side whatever the arithmetic; every other
  latitude is asserted to be further than 1e-9 from 0.  ``k > 0`` of DI is made on table constants.  ``min(Pk / 5, N)`` of DI
  and the maximum of the monthly means in ``mtwm`` are continuous in their arguments: whichever side of a tie is taken, the
  value moves by no more than the rounding the bound already allows.

Run from the repository root: ``python tests/golden/make_agro_golden.py``."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import agrocpu as A  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

DAY = 86400.0
HEAT = [("hi", "huglin", "10-01"), ("hi", "interpolated", "10-01"), ("hi", "jones", "10-01"), ("bedd", "gladstones", "11-01"),
        ("bedd", "huglin", "11-01"), ("bedd", "interpolated", "11-01"), ("bedd", "icclim", "10-01"), ("bedd", "jones", "11-01"),
        ("both", "interpolated", "11-01")]
# name: dtype, calendar, start, T, units, latitudes (both sides of 0, 40, 50 and the polar circle over the set), season
# (start, {reference end -> end of this case}), freqs, water fields
CASES = {
    "midyear_f64": ("float64", "standard", "1999-03-15", 1002, "K", [35.0, 41.2, 52.0], ("04-01", {}), ("YS", "YS-JUL", "MS"), False),
    "midyear_f32": ("float32", "standard", "1999-03-15", 1002, "degC", [-33.0, -45.3, -51.0, -0.5], ("10-01", {"10-01": "04-01", "11-01": "05-01"}),
                    ("YS", "YS-JUL"), False),
    "noleap_f32": ("float32", "noleap", "2001-01-01", 730, "K", [0.0, 39.9, 67.5, -67.5], ("04-01", {}), ("YS",), False),
    "360day_f64": ("float64", "360_day", "2001-01-01", 720, "degC", [-44.0, 70.0], ("04-01", {}), ("YS", "MS"), False),
    "years_f32": ("float32", "standard", "2000-01-01", 731, "K", [45.0, -36.0], ("04-01", {}), ("YS",), True),
    "water_f64": ("float64", "standard", "2000-01-01", 731, "K", [50.0, -40.0, -0.0], ("04-01", {}), ("YS",), True),
}


def fields_of(seed, t, lat, dtype, units, water):
    rng = np.random.default_rng(seed)
    T, C = len(t), len(lat)
    doy = t.doy[:, None].astype(np.float64)
    phase = np.where(np.asarray(lat) >= 0, 105.0, 105.0 + 182.0)[None, :]
    tas = 284 + 11 * np.sin(2 * np.pi * (doy - phase) / 365) + rng.normal(0, 3, (T, C)) + np.linspace(-2, 2, C)[None, :]
    tn, tx = tas - rng.uniform(2, 9, (T, C)), tas + rng.uniform(2, 9, (T, C))
    f = dict(tas=tas, tasmin=tn, tasmax=tx)
    if units == "degC":
        f = {k: v - 273.15 for k, v in f.items()}
    if water:
        f["pr"] = np.maximum(rng.normal(2.5, 4, (T, C)), 0) / DAY
        f["evspsblpot"] = np.maximum(2.5 + 2 * np.sin(2 * np.pi * (doy - phase) / 365) + rng.normal(0, 0.5, (T, C)), 0) / DAY
    f = {k: v.astype(dtype) for k, v in f.items()}
    for v in f.values():                                 # a NaN sprinkle, and in one cell a week without tasmax inside the season
        v[rng.random((T, C)) < 0.004] = np.nan
    week = np.flatnonzero((t.month == 6) & (t.day >= 10) & (t.day <= 16))[:7]
    f["tasmax"][week, 1] = np.nan
    return f


def specs_of(season, freqs, water):
    out = []
    for freq in freqs:
        for kind, method, end in HEAT:
            if method == "jones" and not freq.startswith("YS"):
                continue
            out.append(dict(kind=kind, method=method, freq=freq, end_date=season[1].get(end, end)))
        out += [dict(kind="egdd", method=m, freq=freq) for m in ("bootsma", "qian")]
        out.append(dict(kind="monthly", freq=freq))
    return out


def spec_id(s):
    return ".".join(str(s[k]) for k in ("kind", "method", "freq") if k in s)


def main():
    from test_agro_cpu import check_known_answers

    check_known_answers()        # the restatement first: nothing is written from a restatement that misses a known answer
    arrays, meta = {}, {}
    for seed, (name, (dtype, cal, start, T, units, lat, season, freqs, water)) in enumerate(CASES.items(), 4100):
        assert all(v == 0 or abs(v) > 1e-9 for v in lat), f"{name}: a latitude within 1e-9 of the hemisphere test"
        t = TimeAxis.daily(start, T, cal)
        f = fields_of(seed, t, lat, dtype, units, water)
        sub_C = 273.15 if units == "K" else 0.0
        runs = []
        for s in specs_of(season, freqs, water):
            try:
                res = A.run(s, f, lat, t, sub_C, DAY, season)
            except AssertionError as e:          # the Jones coefficient on a set the reference would reshape (NotServed in the project)
                assert s["method"] == "jones", (name, s, e)
                continue
            except ValueError as e:
                assert s["method"] == "jones" and "below 1.0" in str(e), (name, s, e)
                continue
            gap = res.pop("min_gap", None)
            assert gap is None or gap > 1e-9, f"{name} {spec_id(s)}: a value within 1e-9 of its threshold ({gap}): change the seed"
            runs.append(s)
            for k, v in res.items():
                arrays[f"{name}/{spec_id(s)}/{k}"] = v
        for k, v in f.items():
            arrays[f"{name}/{k}"] = v
        meta[name] = dict(dtype=dtype, calendar=cal, start=start, T=T, units=units, lat=lat, season_start=season[0], runs=runs,
                          per_day=DAY)
    out = os.path.join(HERE, "agro_vectors.npz")
    np.savez_compressed(out, meta=json.dumps(meta), **arrays)
    print(out, os.path.getsize(out), "bytes;", {n: len(m["runs"]) for n, m in meta.items()})


if __name__ == "__main__":
    main()
