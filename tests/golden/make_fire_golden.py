"""Generate tests/golden/fire_vectors.npz by EXECUTING the reference's fire weather code.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_fire_golden.py

src/xclim/indices/fire/_cffwis.py cannot be imported (numba, xarray).  Its iterators and codes are AST-extracted (nothing
is copied into this repository): ``_fire_season``, ``_fire_weather_calc``, ``_fine_fuel_moisture_code``,
``_duff_moisture_code``, ``_drought_code``, ``_day_length``, ``_day_length_factor``, ``_overwintering_drought_code``,
``initial_spread_index``, ``build_up_index``, ``fire_weather_index``, ``daily_severity_rating`` and the two day-length
tables.  ``@njit`` becomes the identity; ``@vectorize`` becomes an element loop over python floats, which is numba's
float64 promotion of the float32 inputs.  The numpy index functions run as they are, on the float32 output arrays.

Every case stores its inputs with TIME LAST (the reference's layout; the weather fields as int16 multiples of
``input_scale``, see ``decode``), the parameters and the outputs of ``_fire_weather_calc``; tests/test_fire_cpu.py and
tests/test_gpu_fire.py read them.
"""

import ast
import json
import os
import sys
from collections import OrderedDict

import numpy as np

REF = "/root/reference/src/xclim/indices/fire/_cffwis.py"
HERE = os.path.dirname(os.path.abspath(__file__))
FUNCS = ["_fire_season", "_fire_weather_calc", "_fine_fuel_moisture_code", "_duff_moisture_code", "_drought_code",
         "_day_length", "_day_length_factor", "_overwintering_drought_code", "initial_spread_index", "build_up_index",
         "fire_weather_index", "daily_severity_rating"]
TABLES = ["DAY_LENGTHS", "DAY_LENGTH_FACTORS", "default_params"]


def _elementwise(fn):
    """@vectorize stand-in: broadcast, then call `fn` on python scalars (float64 arithmetic), float64 result."""

    def loop(*args):
        arrs = np.broadcast_arrays(*[np.asarray(a) for a in args])
        out = np.empty(arrs[0].shape, dtype=np.float64)
        for i in np.ndindex(out.shape):
            out[i] = fn(*[int(a[i]) if a.dtype.kind in "iu" else float(a[i]) for a in arrs])
        return out

    return loop


def extract():
    tree = ast.parse(open(REF).read())
    ns = {"np": np, "OrderedDict": OrderedDict}
    body = []
    for node in tree.body:
        if isinstance(node, (ast.Assign, ast.AnnAssign)):
            tgt = node.targets[0] if isinstance(node, ast.Assign) else node.target
            if isinstance(tgt, ast.Name) and tgt.id in TABLES:
                if isinstance(node, ast.AnnAssign):
                    node = ast.Assign(targets=[tgt], value=node.value)
                body.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name in FUNCS:
            vec = any(getattr(getattr(d, "func", d), "id", None) == "vectorize" for d in node.decorator_list)
            node.decorator_list = [ast.Name(id="_elementwise", ctx=ast.Load())] if vec else []
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            body.append(node)
    ns["_elementwise"] = _elementwise
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    missing = set(FUNCS + TABLES) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")
    return ns


def weather(rng, C, T, start_doy=0, nan_frac=0.0):
    """Seeded daily weather with a seasonal cycle, time LAST: tas [degC], pr [mm/d], hurs [%], sfcWind [km/h], snd [m]."""
    t = np.arange(T)[None, :] + start_doy
    amp = rng.uniform(8, 18, (C, 1))
    base = rng.uniform(-4, 12, (C, 1))
    tas = base + amp * np.sin(2 * np.pi * (t - 105) / 365.0) + rng.normal(0, 3.5, (C, T))
    wet = rng.random((C, T)) < 0.35
    pr = np.where(wet, rng.gamma(0.7, 6.0, (C, T)), 0.0)
    hurs = np.clip(rng.normal(65, 18, (C, T)) + 2 * pr, 5, 100)
    ws = np.abs(rng.normal(12, 7, (C, T)))
    snd = np.clip(0.4 * np.cos(2 * np.pi * (t - 20) / 365.0) - 0.05 + rng.normal(0, 0.05, (C, T)) - 0.01 * base, 0, None)
    # inputs at the precision of station data (0.1 degC, 0.1 mm, 1 %, 0.1 km/h, 1 mm of snow): the fixture stays small
    out = [np.round(a, d).astype(np.float32) for a, d in zip((tas, pr, hurs, ws, snd), (1, 1, 0, 1, 3))]
    if nan_frac:
        for a in out[:4]:
            a[rng.random(a.shape) < nan_frac] = np.nan
    return out


# The weather inputs are stored as int16 multiples of 1 / scale (NaN = -32768); decoding is float32(q / scale), which is
# bit for bit the float32 the reference was run on (np.round(x, d) is rint(x * 10**d) / 10**d in float64).
INPUT_SCALE = {"tas": 10, "pr": 10, "hurs": 1, "sfcWind": 10, "snd": 1000}
NAN_Q = -32768


def decode(q, scale):
    return np.where(q == NAN_Q, np.nan, q / float(scale)).astype(np.float32)


def quantize(a, name):
    scale = INPUT_SCALE[name]
    q64 = np.rint(np.asarray(a, dtype=np.float64) * scale)
    assert np.all(np.isnan(q64) | (np.abs(q64) < 32767))
    q = np.where(np.isnan(q64), NAN_Q, q64).astype(np.int16)
    back = decode(q, scale)
    assert np.array_equal(back, a, equal_nan=True), name  # the stored inputs are exactly the ones the reference saw
    return q


def months(T, start_month=1):
    """Month of every day of a noleap calendar starting on the 1st of `start_month`."""
    ml = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    m = []
    k = start_month - 1
    while len(m) < T:
        m.extend([k % 12 + 1] * ml[k % 12])
        k += 1
    return np.array(m[:T], dtype=np.int64)


def lats(rng, C):
    """Latitudes over the five day-length bands, their edges included."""
    edges = np.array([-90.0, -30.0, -15.0, 15.0, 30.0, 90.0, -45.0, 44.0, 60.0, -20.0, 20.0, 0.0])
    out = rng.uniform(-90, 90, C)
    out[: min(C, len(edges))] = edges[: min(C, len(edges))]
    return out


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the fire vectors can only be regenerated in the build container")
    ns = extract()
    calc = ns["_fire_weather_calc"]
    defaults = {k: v if not isinstance(v, tuple) else v[0] for k, v in ns["default_params"].items()}
    rng = np.random.default_rng(20261015)
    all_idx = ["DC", "DMC", "FFMC", "ISI", "BUI", "FWI", "DSR"]
    cases = []

    def case(name, C, T, season_method=None, indexes=all_idx, overwintering=False, dry_start=None, initial_start_up=True,
             mask=None, starts=None, winter_pr=None, nan_frac=0.0, start_month=1, boundary=False, **params):
        tas, pr, hurs, ws, snd = weather(rng, C, T, start_doy=[0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334][start_month - 1],
                                         nan_frac=nan_frac)
        if boundary:  # exact thresholds of the codes on every 7th day of the first cells
            k = np.arange(0, T, 7)
            pr[0, k], pr[1, k], pr[2, k] = 0.5, 1.5, 2.8
            hurs[3, :] = 100.0
            ws[4, :] = 0.0
            tas[5, k], tas[6, k] = -2.8, -1.1
            tas[7, k] = np.round(rng.uniform(-6, -2.8, k.size), 1)
            pr[8, :] = 0.0
        mth = np.broadcast_to(months(T, start_month), (C, T))
        lat = lats(rng, C)
        nanc = np.full(C, np.nan, np.float32)
        dc0, dmc0, ffmc0 = (nanc.copy(), nanc.copy(), nanc.copy()) if starts is None else starts(C)
        wpr = np.zeros(C, np.float32) if winter_pr is None else winter_pr(C)
        outputs = list(indexes)
        if season_method is not None and season_method != "mask":
            outputs.append("season_mask")
        if overwintering:
            outputs.append("winter_pr")
        p = dict(defaults)
        p.update(params)
        p.update(season_method=season_method, overwintering=overwintering, dry_start=dry_start,
                 initial_start_up=initial_start_up, outputs=outputs)
        m = None if mask is None else mask(tas)
        res = calc(tas, pr, hurs, ws, snd, mth, lat, m, dc0.copy(), dmc0.copy(), ffmc0.copy(), wpr.copy(), **p)
        if len(outputs) == 1:
            res = (res,)
        rec = {"tas": quantize(tas, "tas"), "pr": quantize(pr, "pr"), "hurs": quantize(hurs, "hurs"),
               "sfcWind": quantize(ws, "sfcWind"), "month": mth[0].astype(np.int8), "lat": lat,
               "dc0": dc0, "dmc0": dmc0, "ffmc0": ffmc0, "winter_pr_in": wpr}
        if season_method in ("LA08", "GFWED"):  # (the other cases never read the snow depth)
            rec["snd"] = quantize(snd, "snd")
        if m is not None:
            rec["season_mask_in"] = m.astype(bool)
        for o, r in zip(outputs, res):
            rec["out_" + o] = np.asarray(r)
        pj = {k: v for k, v in p.items() if k != "outputs"}
        pj["indexes"] = list(indexes)
        rec["params"] = np.array(json.dumps(pj))
        cases.append((name, rec))
        print(name, {o: float(np.nanmean(np.asarray(r, dtype=np.float64))) for o, r in zip(outputs, res)})

    def given(C):
        return (rng.uniform(50, 400, C).astype(np.float32), rng.uniform(2, 80, C).astype(np.float32),
                rng.uniform(60, 95, C).astype(np.float32))

    def blocks(tas):  # a fire season mask of seasonal blocks with a short shoulder season
        T = tas.shape[-1]
        d = np.arange(T) % 365
        m = ((d > 120) & (d < 280)) | ((d > 300) & (d < 310))
        m = np.broadcast_to(m, tas.shape).copy()
        m[::3] = np.roll(m[::3], 9, axis=-1)
        m[1, :5] = True
        return m

    case("none", 12, 60, nan_frac=0.01)
    case("none_boundary", 9, 80, boundary=True)
    case("mask", 2, 300, season_method="mask", mask=blocks)
    case("mask_given_no_startup", 2, 200, season_method="mask", mask=blocks, initial_start_up=False, starts=given,
         start_month=6)
    case("wf93_overwinter", 1, 400, start_month=7, season_method="WF93", overwintering=True)
    case("wf93_overwinter_cfs", 2, 400, start_month=7, season_method="WF93", overwintering=True, dry_start="CFS", prec_thresh=1.5,
         dmc_dry_factor=1.2)
    case("wf93_gfwed_dry", 1, 400, start_month=7, season_method="WF93", dry_start="GFWED", temp_condition_days=2)
    case("la08_cfs", 1, 400, start_month=7, season_method="LA08", dry_start="CFS", temp_condition_days=4, snow_condition_days=2)
    case("gfwed", 1, 400, start_month=7, season_method="GFWED", temp_start_thresh=6.0, temp_end_thresh=6.0, dry_start="GFWED")
    case("gfwed_windows", 1, 400, start_month=7, season_method="GFWED", temp_condition_days=5, snow_condition_days=7,
         overwintering=True)
    case("dc_only_overwinter", 1, 400, start_month=7, season_method="WF93", indexes=["DC"], overwintering=True,
         winter_pr=lambda C: rng.uniform(0, 300, C).astype(np.float32), starts=given)
    case("wf93_nan", 1, 400, start_month=7, season_method="WF93", overwintering=True, dry_start="CFS", nan_frac=0.01,
         temp_start_thresh=8.0)
    case("shoulder_multi_year", 1, 365 * 2, season_method="WF93", temp_start_thresh=8.0, temp_end_thresh=7.0,
         temp_condition_days=1, overwintering=True, dry_start="GFWED", start_month=7)

    out = {}
    for name, rec in cases:
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
    out["cases"] = np.array([n for n, _ in cases])
    for k, v in INPUT_SCALE.items():
        out[f"input_scale/{k}"] = np.int32(v)
    # the reference's own known answers of the helpers (tests/test_cffwis.py:122-153 of the reference)
    out["known/day_length_44_1"] = np.float64(ns["_day_length"](44, 1))
    out["known/day_length_factor_44_1"] = np.float64(ns["_day_length_factor"](44, 1))
    out["known/bui_0_0"] = np.asarray(ns["build_up_index"](0, 0), dtype=np.float64)
    path = os.path.join(HERE, "fire_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
