"""Generate tests/golden/chill_vectors.npz by EXECUTING the reference's winter-chill code.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_chill_golden.py

src/xclim/indices/_agro.py and helpers.py cannot be imported here (xarray, pint, numba, cftime).  The pieces below are
AST-extracted (nothing is copied into this repository) with their annotations dropped, and EXECUTED on numpy arrays:

  * ``_accumulate_intermediate`` and ``_chill_portion_one_season`` (_agro.py:1436-1465), whole bodies, time LAST;
  * the ``cu = xarray.where(...)`` statement of ``chill_units`` (:1574-1586), with ``xarray.where`` bound to ``np.where``;
  * ``_compute_daytime_temperature`` and ``_compute_nighttime_temperature`` (helpers.py:977-1035), whole bodies;
  * ``day_lengths`` with everything under it, the way tests/golden/make_pet_golden.py executes it (its ``extract``).

RESTATED here, because it is xarray / pint plumbing: of ``make_hourly_temperature`` (helpers.py:1090-1123) the merge / concat
of a copy of the last day, ``shift(time=-1)``, ``resample(time="h").ffill()`` (every daily value repeated 24 times),
``time.dt.hour`` (0..23 per day), ``clip(1)`` and ``xr.where``; of ``chill_portions`` (_agro.py:1533-1534 and 1468-1479)
``convert_units_to`` (degC -> K as ``+ 273.15``, K -> degC as ``- 273.15``), ``select_time(..., drop=True)`` for ``month=`` and
``date_bounds=``, ``resample_map`` over ``YS`` / ``YS-JUL`` / ``MS`` periods, ``apply_ufunc`` on the time-last array and
``.sum("time")`` (numpy's sum in the array's dtype); of ``chill_units`` (:1587-1592) ``cu.where(tas.notnull())``, the daily and
the per-period NaN-skipping sums.  ASSUMPTIONS that could not be executed: the decimal year behind ``day_lengths`` (see
make_pet_golden.py), and that a period which ``select_time`` emptied gives NaN chill portions (recorded as NaN).

Every case stores its inputs TIME FIRST — int16 tenths (``decode``), or float64 as they are where the exact value matters
(the known answers, the band edges) — its daily time axis, period offsets and selection, and the outputs: ``delta`` (rows x
cells, 0 on unselected rows), ``cp``, ``cu``, ``cu_pos`` (positive_only), ``hourly`` and ``dl`` for the daily cases.  float32
cases hold BOTH the reference's own float32 run (``delta32``, ``cp32``) and its run on the same values widened to float64
(``delta``, ``cp``), and ``gap32`` = |cp - cp32|.  The committed file must stay under 1 MiB and ``delta`` is dense (the
intermediate product sits above 1 for days on end), so the two 64-cell seasonal cases share one stored field (``tas_of``)
and record ``delta`` for a spread of their cells (``delta_cells``); every sum is recorded for every cell.

The generator ASSERTS, so that a test cannot hide a failure behind a coin toss: in every float64 run min |E - 1| over all
hours is at least 1e-9 (the release pattern ``delta > 0`` then survives a 1-ulp difference of ``exp``); and no hourly
temperature of a Utah case lies within 1e-9 of a band edge unless it EQUALS the edge as the comparison sees it (the
planted values).  tests/test_chill_cpu.py and tests/test_gpu_chill.py read the file.
"""

import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_pet_golden as P  # noqa: E402  (Time, Arr, extract: the executed day_lengths)

REF = P.REF
EDGES = (1.4, 2.4, 9.1, 12.4, 15.9, 17.9)
K2C = 273.15
KNOWN_CP = 72.2441765                    # tests/test_indices.py:375-378
KNOWN_HOURLY = [0.0, 3.90180644, 7.65366865, 11.11140466, 14.14213562, 16.62939225, 18.47759065, 19.61570561, 20.0,
                19.61570561, 18.47759065, 16.62939225, 14.14213562, 10.32039099, 8.0848137, 6.49864636, 5.26831939,
                4.26306907, 3.41314202, 2.67690173, 2.02749177, 1.44657476, 0.92107141, 0.44132444]  # tests/test_helpers.py:310-337
MARGIN = [np.inf]


def _functions(fname, names):
    tree = ast.parse(open(os.path.join(REF, fname)).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.decorator_list, node.returns = [], None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            out[node.name] = node
    missing = set(names) - set(out)
    if missing:
        raise RuntimeError(f"not found in {fname}: {missing}")
    return out


def extract():
    """The executed pieces: {name: callable}."""
    ns = {"np": np}
    agro = _functions("_agro.py", ["_accumulate_intermediate", "_chill_portion_one_season", "chill_units"])
    helpers = _functions("helpers.py", ["_compute_daytime_temperature", "_compute_nighttime_temperature"])
    body = [agro["_accumulate_intermediate"], agro["_chill_portion_one_season"], helpers["_compute_daytime_temperature"],
            helpers["_compute_nighttime_temperature"]]
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    # the one statement `cu = xarray.where(...)` of chill_units, as a function of tas
    stmt = next(n for n in agro["chill_units"].body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "cu"
                and isinstance(n.value, ast.Call) and ast.unparse(n.value.func) == "xarray.where")
    expr = ast.Expression(body=stmt.value)
    ast.fix_missing_locations(expr)
    code = compile(expr, REF, "eval")
    xarray = types.SimpleNamespace(where=np.where)
    ns["utah"] = lambda tas: eval(code, {"xarray": xarray, "tas": tas})  # noqa: S307 - the reference's own expression
    # min |E - 1| of every float64 run: _chill_portion_one_season reaches _accumulate_intermediate by global name
    acc = ns["_accumulate_intermediate"]

    def watched(prev_E, prev_xi, curr_xs, curr_ak1):
        E = acc(prev_E, prev_xi, curr_xs, curr_ak1)
        if np.asarray(E).dtype == np.float64:
            d = np.abs(np.asarray(E) - 1)
            d = d[np.isfinite(d)]
            if d.size:
                MARGIN[0] = min(MARGIN[0], float(d.min()))
        return E

    ns["_accumulate_intermediate"] = watched
    ns["day_lengths"] = P.extract()["day_lengths"]
    return ns


# ---- the restated plumbing ------------------------------------------------------------------------------------------
def encode(a):
    q = np.round(np.asarray(a, np.float64) * 10)
    q[np.isnan(q)] = -32768
    return q.astype(np.int16)


def decode(q, dtype):
    """int16 tenths (-32768 = NaN) -> the field the reference saw: tenths in float64, then the case's dtype."""
    if q.dtype != np.int16:
        return np.asarray(q, dtype)
    return np.where(q == -32768, np.nan, q.astype(np.float64) / 10).astype(dtype)


def period_offsets(t, freq):
    """Day offsets of the periods of resample(time=freq) for YS / YS-JUL / MS (the span has no empty period)."""
    if freq == "MS":
        key = t.year * 12 + t.month - 1
    else:
        anchor = {"YS": 1, "YS-JUL": 7}[freq]
        key = (t.year * 12 + t.month - anchor) // 12
    keys = np.arange(key[0], key[-1] + 1)
    return np.searchsorted(key, np.append(keys, key[-1] + 1), side="left").astype(np.int64)


def day_mask(t, indexer):
    """select_time's mask per day for month= and date_bounds= (bounds included, standard calendar: every date seen in the
    all-leap calendar, core/calendar.py:1354-1371)."""
    if not indexer:
        return None
    if "month" in indexer:
        return np.isin(t.month, indexer["month"])
    cum = np.concatenate([[0], np.cumsum([31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31])])[:-1]
    (ms, ds), (me, de) = (tuple(int(v) for v in b.split("-")) for b in indexer["date_bounds"])
    doy, s, e = cum[t.month - 1] + t.day, cum[ms - 1] + ds, cum[me - 1] + de
    return (doy >= s) & (doy <= e) if s <= e else (doy >= s) | (doy <= e)


def to_K(tas, units):
    return tas if units == "K" else tas + K2C


def to_C(tas, units):
    return tas if units == "degC" else tas - K2C


def chill_portions(ns, tas, units, seg, sel):
    """(delta (H, C), cp (P, C)) in the dtype of ``tas``: select, split, the reference's function on the time-last array of
    each period, sum("time")."""
    tas_K = to_K(tas, units)
    H, C = tas_K.shape
    rows_sel = np.ones(H, bool) if sel is None else np.repeat(sel, 24)
    delta = np.zeros((H, C), tas_K.dtype)
    cp = np.full((len(seg) - 1, C), np.nan, tas_K.dtype)
    for p, (a, b) in enumerate(zip(24 * seg[:-1], 24 * seg[1:])):
        rows = np.arange(a, b)[rows_sel[a:b]]
        if rows.size == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = ns["_chill_portion_one_season"](np.ascontiguousarray(tas_K[rows].T))
        assert d.dtype == tas_K.dtype and d.shape == (C, rows.size)
        delta[rows] = d.T
        cp[p] = np.sum(d, axis=-1)
    return delta, cp


def chill_units(ns, tas, units, seg, positive_only):
    tas_C = to_C(tas, units)
    with np.errstate(invalid="ignore"):
        cu = np.asarray(ns["utah"](tas_C), np.float64)
    cu = np.where(~np.isnan(tas_C), cu, np.nan)
    if positive_only:
        daily = np.nansum(cu.reshape(-1, 24, cu.shape[1]), axis=1)
        daily = np.where(daily > 0, daily, np.nan)
        return np.stack([np.nansum(daily[a:b], axis=0) for a, b in zip(seg[:-1], seg[1:])])
    return np.stack([np.nansum(cu[a:b], axis=0) for a, b in zip(24 * seg[:-1], 24 * seg[1:])])


def make_hourly_temperature(ns, tasmin, tasmax, dl):
    """helpers.py:1090-1123 on (D, C) arrays of one dtype and the (D, C) day lengths of the days."""
    D, C = tasmin.shape
    day, night = ns["_compute_daytime_temperature"], ns["_compute_nighttime_temperature"]
    with np.errstate(invalid="ignore", divide="ignore"):
        sunset = day(dl, tasmin, tasmax, dl)
        nxt = np.concatenate([tasmin[1:], tasmin[-1:]])   # shift(time=-1) over the data with a copy of the last day appended
        rep = lambda a: np.repeat(a, 24, axis=0)  # noqa: E731  resample("h").ffill()
        hour = np.tile(np.arange(24, dtype=np.int64), D)[:, None]
        h_dl, h_tn, h_tx, h_nxt, h_ss = rep(dl), rep(tasmin), rep(tasmax), rep(nxt), rep(sunset)
        nh = np.clip(hour + 1 - h_dl, 1, None)
        out = np.where(hour < h_dl, day(hour, h_tn, h_tx, h_dl), night(nh, h_nxt, h_ss, h_dl - 1))
    assert out.dtype == np.float64
    return out


def check_edges(name, tas_C):
    """No Utah temperature within 1e-9 of a band edge unless it equals the edge in the comparison's dtype."""
    t = np.asarray(tas_C)
    for e in EDGES:
        near = np.abs(t.astype(np.float64) - e) < 1e-9
        planted = t == t.dtype.type(e)
        bad = near & ~planted
        assert not bad.any(), f"{name}: {int(bad.sum())} temperatures within 1e-9 of the band edge {e}"


# ---- cases ----------------------------------------------------------------------------------------------------------
def seasonal(rng, t, C, mean=6.0, amp=9.0):
    """An hourly winter field in degC: seasonal cycle + diurnal cycle + weather, (24 D, C)."""
    D = len(t)
    doy = (np.arange(D)[:, None] + 0.0)
    base = mean + amp * np.cos(2 * np.pi * (doy - 200) / 365.0) + rng.normal(0, 3.0, (D, 1)) + rng.normal(0, 1.5, (D, C))
    base += np.linspace(-4, 6, C)[None, :]
    hour = np.arange(24)[None, :, None]
    f = base[:, None, :] + 5.0 * np.sin(2 * np.pi * (hour - 9) / 24.0) + rng.normal(0, 0.6, (D, 24, C))
    return f.reshape(24 * D, C)


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the chill vectors can only be regenerated in the build container")
    ns = extract()
    rng = np.random.default_rng(20261018)
    out, names = {}, []

    def hourly_case(name, tas, dtype, units, start, D, freq, indexer=None, utah=True, store=None, tas_of=None, delta_cells=None):
        """tas: (24 D, C) values; stored as int16 tenths unless ``store`` is a float64 array (kept as it is), or not at all
        when the case reads the stored field of the case ``tas_of``.  delta_cells: the cells whose delta is recorded (every
        cell when None; the sums are recorded for every cell)."""
        t = P.Time.daily(*start, D, "standard")
        if tas_of is not None:
            q = out[tas_of + "/tas"]
        else:
            q = encode(tas) if store is None else np.asarray(store, np.float64)
        x = decode(q, dtype)
        seg, sel = period_offsets(t, freq), day_mask(t, indexer)
        p = name + "/"
        if tas_of is not None:
            out[p + "tas_of"] = np.array(tas_of)
        else:
            out[p + "tas"] = q
        cells = np.arange(x.shape[1]) if delta_cells is None else np.asarray(delta_cells)
        if delta_cells is not None:
            out[p + "delta_cells"] = cells
        out[p + "meta"] = np.array([np.dtype(dtype).name, units, freq, json.dumps(indexer or {}), "hourly"])
        out[p + "start"] = np.array([*start, D])
        out[p + "seg"] = seg
        if sel is not None:
            out[p + "sel"] = sel.astype(np.uint8)
        x64 = x.astype(np.float64)
        before, MARGIN[0] = MARGIN[0], np.inf
        delta, cp = chill_portions(ns, x64, units, seg, sel)
        out[p + "delta"], out[p + "cp"] = delta[:, cells], cp
        out[p + "margin"] = np.array(MARGIN[0])
        MARGIN[0] = min(MARGIN[0], before)
        if dtype == np.float32:
            d32, c32 = chill_portions(ns, x, units, seg, sel)
            assert d32.dtype == np.float32
            out[p + "delta32"], out[p + "cp32"] = d32[:, cells], c32
            out[p + "gap32"] = np.abs(cp - c32.astype(np.float64))
        if utah and not indexer:
            if store is None:   # (a field stored as it is holds planted values only: the device reads the same bits)
                check_edges(name, to_C(x, units))
            out[p + "cu"] = chill_units(ns, x, units, seg, False)
            out[p + "cu_pos"] = chill_units(ns, x, units, seg, True)
        names.append(name)
        print(name, np.dtype(dtype).name, x.shape, "periods", len(seg) - 1, "cp", np.round(np.nanmax(cp), 4), "releases",
              int((delta > 0).sum()))
        return x, delta, cp

    # the reference's known answers, restated as inputs
    lin = np.linspace(0, 15, 120 * 24) + K2C
    _, _, cp = hourly_case("known_linspace", None, np.float64, "K", (2000, 1, 1), 120, "YS", utah=False, store=lin[:, None])
    assert abs(cp[0, 0] - KNOWN_CP) < 1.5e-7, cp   # assert_array_almost_equal(decimal=7)
    vals = np.array(10 * [1.1] + 15 * [2.0] + 20 * [5.6] + 10 * [16.0] + 5 * [20.0] + 12 * [np.nan]) + K2C  # 60 hours + half a day absent
    hourly_case("known_units", None, np.float64, "K", (2000, 1, 1), 3, "YS", store=vals[:, None])
    assert out["known_units/cu"][0, 0] == 0.5 * 15 + 20 - 0.5 * 10 - 5 and out["known_units/cu_pos"][0, 0] == 0.5 * 15 + 20 - 0.5 * 3

    # a winter of hourly data over two calendar years
    t = P.Time.daily(2001, 9, 15, 210, "standard")
    hourly_case("seasonal_f64", seasonal(rng, t, 64), np.float64, "degC", (2001, 9, 15), 210, "YS", delta_cells=np.arange(0, 64, 5))
    hourly_case("seasonal_f32", None, np.float32, "degC", (2001, 9, 15), 210, "YS", tas_of="seasonal_f64", delta_cells=np.arange(3, 64, 8))
    # the docstring's winter selection over three July-to-June years, and a selection with a gap INSIDE the period
    t = P.Time.daily(2001, 7, 1, 1096, "standard")
    hourly_case("date_bounds_3y", seasonal(rng, t, 2, mean=7.0), np.float64, "degC", (2001, 7, 1), 1096, "YS-JUL",
                {"date_bounds": ["09-01", "03-30"]})
    t = P.Time.daily(2001, 1, 1, 730, "standard")
    hourly_case("month_djf_2y", seasonal(rng, t, 2, mean=7.0) + K2C, np.float64, "K", (2001, 1, 1), 730, "YS", {"month": [12, 1, 2]})
    # NaN hours: mid-period, on the first hour of a period (both periods), an all-NaN cell
    t = P.Time.daily(2001, 1, 10, 40, "standard")
    f = seasonal(rng, t, 12, mean=4.0, amp=3.0)
    f[300, 1] = np.nan
    f[0, 2] = np.nan
    f[22 * 24, 3] = np.nan        # the first hour of February
    f[22 * 24 - 1, 4] = np.nan    # the last hour of January
    f[:, 5] = np.nan
    f[100:130, 6] = np.nan
    hourly_case("nan_hours", f, np.float64, "degC", (2001, 1, 10), 40, "MS")
    # temperatures exactly on every Utah band edge, and their neighbours on both sides
    for dt in (np.float64, np.float32):
        e = np.array(EDGES, dt)
        v = np.concatenate([e, np.nextafter(e, dt(100)), np.nextafter(e, dt(-100)), [0.0, 5.0, 10.0, 14.0, 17.0, 25.0]]).astype(dt)
        v = np.concatenate([v, v[::-1]])
        assert v.size == 48
        cells = np.stack([v, np.roll(v, 7), np.roll(v, 19)], axis=1)
        # (the float32 values are stored widened, which is exact, and decoded by rounding back, which is exact too)
        hourly_case("utah_edges_f64" if dt == np.float64 else "utah_edges_f32", None, dt, "degC", (2002, 2, 27), 2, "MS",
                    store=cells.astype(np.float64))

    # ---- daily cases: make_hourly_temperature, then the two indices on its result -----------------------------------
    def daily_case(name, tasmin, tasmax, lats, dtype, units, start, D, freq):
        t = P.Time.daily(*start, D, "standard")
        qn, qx = encode(tasmin), encode(tasmax)
        tn, tx = decode(qn, dtype), decode(qx, dtype)
        with np.errstate(invalid="ignore"):
            dl = np.asarray(ns["day_lengths"](t, P.Arr(np.asarray(lats, np.float64), "degrees_north")), np.float64)
        assert dl.shape == (D, len(lats))
        hourly = make_hourly_temperature(ns, tn, tx, dl)
        seg = period_offsets(t, freq)
        p = name + "/"
        out[p + "tasmin"], out[p + "tasmax"], out[p + "lat"], out[p + "dl"], out[p + "hourly"] = qn, qx, np.asarray(lats, np.float64), dl, hourly
        out[p + "meta"] = np.array([np.dtype(dtype).name, units, freq, "{}", "daily"])
        out[p + "start"] = np.array([*start, D])
        out[p + "seg"] = seg
        before, MARGIN[0] = MARGIN[0], np.inf
        delta, cp = chill_portions(ns, hourly, units, seg, None)
        out[p + "margin"] = np.array(MARGIN[0])
        MARGIN[0] = min(MARGIN[0], before)
        check_edges(name, to_C(hourly, units))
        out[p + "delta"], out[p + "cp"] = delta, cp
        out[p + "cu"] = chill_units(ns, hourly, units, seg, False)
        out[p + "cu_pos"] = chill_units(ns, hourly, units, seg, True)
        names.append(name)
        print(name, np.dtype(dtype).name, hourly.shape, "NaN hours", int(np.isnan(hourly).sum()), "cp", np.round(np.nanmax(cp), 4))
        return hourly

    h = daily_case("known_equator", np.array([[0.0]]), np.array([[20.0]]), [0.0], np.float64, "degC", (2000, 1, 1), 1, "YS")
    np.testing.assert_allclose(h[:, 0], KNOWN_HOURLY, rtol=1e-7, atol=1e-8)   # (np.testing.assert_allclose's default, test_helpers.py:338)
    lats = np.repeat([0.0, 45.0, -45.0, 67.0, -67.0, 80.0], 2)
    for dt, start in ((np.float64, (2001, 11, 25)), (np.float32, (2002, 5, 20))):
        D = 40
        t = P.Time.daily(*start, D, "standard")
        doy = np.arange(D)[:, None]
        base = 277.0 + 5 * np.cos(2 * np.pi * doy / 60.0) + rng.normal(0, 2.5, (D, len(lats))) + np.linspace(-3, 4, len(lats))[None, :]
        spread = rng.uniform(3, 12, (D, len(lats)))
        tn, tx = base - spread / 2, base + spread / 2
        tn[17, 1] = np.nan    # must also reach the night of day 16
        tn[D - 1, 2] = np.nan
        tx[9, 4] = np.nan
        daily_case(f"daily_{'f64' if dt == np.float64 else 'f32'}", tn, tx, lats, dt, "K", start, D, "MS")

    assert MARGIN[0] >= 1e-9, f"min |E - 1| = {MARGIN[0]:.3e}: a release hangs on the last bit of exp; change the seed"
    out["cases"] = np.array(names)
    out["min_margin"] = np.array(MARGIN[0])
    path = os.path.join(HERE, "chill_vectors.npz")
    np.savez_compressed(path, **out)
    print("min |E - 1| =", MARGIN[0])
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
