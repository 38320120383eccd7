"""Generate tests/golden/ffdi_vectors.npz by EXECUTING the reference's McArthur fire danger code.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_ffdi_golden.py

src/xclim/indices/fire/_ffdi.py cannot be imported here (numba, xarray).  Its two gufunc bodies,
``_keetch_byram_drought_index`` and ``_griffiths_drought_factor``, are AST-extracted (nothing is copied into this
repository) with their ``@guvectorize`` decorators dropped, and run per cell on float64 1-D arrays into preallocated
outputs: that is the gufunc's float64 loop.  Python's ``min`` / ``max`` and ``N**1.3`` are what numba compiles.  The FFDI
is the assignment statement of ``mcarthur_forest_fire_danger_index``, extracted the same way and evaluated on numpy
arrays of the inputs' dtype (NEP 50 promotion, as on the DataArrays).

Every case stores its inputs with TIME LAST (the reference's layout; float32 fields as int16 multiples of 0.1, see
``decode``), ``pr_annual``, ``kbdi0`` when given and ``lim``,
and the outputs: ``kbdi`` = KBDI(pr, tasmax), ``df`` = DF(pr, kbdi) with rows 0..18 NaN (the reference's ``.where``),
``ffdi`` = FFDI(df, tasmax, hurs, sfcWind), ``ffdi_df32`` = FFDI(float32 df, ...), and for cases with a separate soil
moisture deficit ``df_smd`` = DF(pr, smd).  tests/test_ffdi_cpu.py and tests/test_gpu_ffdi.py read them.
"""

import ast
import os
import sys

import numpy as np

REF = "/root/reference/src/xclim/indices/fire/_ffdi.py"
HERE = os.path.dirname(os.path.abspath(__file__))
GUFUNCS = ["_keetch_byram_drought_index", "_griffiths_drought_factor"]
FFDI_FUNC = "mcarthur_forest_fire_danger_index"


def extract():
    tree = ast.parse(open(REF).read())
    ns = {"np": np}
    body = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in GUFUNCS:
            node.decorator_list = []
            node.returns = None
            for a in node.args.args:
                a.annotation = None
            body.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name == FFDI_FUNC:
            # the one statement that computes the index, as the body of a function of the four arrays
            stmt = [s for s in node.body if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", None) == "ffdi"]
            assert len(stmt) == 1
            args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a.arg) for a in node.args.args], kwonlyargs=[],
                                 kw_defaults=[], defaults=[])
            ret = ast.Return(value=ast.Name(id="ffdi", ctx=ast.Load()))
            body.append(ast.FunctionDef(name="_ffdi_expr", args=args, body=[stmt[0], ret], decorator_list=[]))
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    missing = set(GUFUNCS + ["_ffdi_expr"]) - set(ns)
    if missing:
        raise RuntimeError(f"not found: {missing}")
    return ns


def weather(rng, C, T, dtype=np.float32, p_stay_dry=0.85, p_stay_wet=0.5, rain_scale=7.0, hot=0.0):
    """Seeded daily weather with a seasonal cycle and Markov dry / wet spells, time LAST: pr [mm/day], tasmax [degC],
    hurs [%], sfcWind [km/h].  float32 fields are rounded to 0.1 (station precision); float64 ones keep every digit."""
    t = np.arange(T)[None, :]
    tas = rng.uniform(18, 30, (C, 1)) + hot + rng.uniform(4, 12, (C, 1)) * np.sin(2 * np.pi * (t - 20) / 365.0)
    tas = tas + rng.normal(0, 3.0, (C, T))
    wet = np.zeros((C, T), bool)
    state = rng.random(C) < 0.3
    for d in range(T):
        u = rng.random(C)
        state = np.where(state, u < p_stay_wet, u >= p_stay_dry)
        wet[:, d] = state
    pr = np.where(wet, rng.gamma(0.8, rain_scale, (C, T)), 0.0)
    hurs = np.clip(rng.normal(45, 15, (C, T)) + 1.5 * pr, 3, 100)
    ws = np.abs(rng.normal(18, 9, (C, T)))
    out = []
    for a in (pr, tas, hurs, ws):
        out.append(np.round(a, 1).astype(np.float32) if dtype == np.float32 else a.astype(np.float64))
    return out


# float32 fields are stored as int16 multiples of 0.1 (NaN = -32768); decoding float32(q / 10) is bit for bit the float32
# the reference was run on (np.round(x, 1) is rint(10 x) / 10 in float64).  float64 fields are stored as they are.
INPUT_SCALE = 10
NAN_Q = -32768


def decode(q):
    return np.where(q == NAN_Q, np.nan, q / float(INPUT_SCALE)).astype(np.float32)


def quantize(a):
    q64 = np.rint(np.asarray(a, dtype=np.float64) * INPUT_SCALE)
    assert np.all(np.isnan(q64) | (np.abs(q64) < 32767))
    q = np.where(np.isnan(q64), NAN_Q, q64).astype(np.int16)
    assert np.array_equal(decode(q), a, equal_nan=True)  # the stored inputs are exactly the ones the reference saw
    return q


def main():
    if not os.path.exists(REF):
        sys.exit("reference tree not present; the ffdi vectors can only be regenerated in the build container")
    ns = extract()
    kbdi_fn, df_fn, ffdi_expr = ns["_keetch_byram_drought_index"], ns["_griffiths_drought_factor"], ns["_ffdi_expr"]
    rng = np.random.default_rng(20261016)
    cases = []

    def kbdi_all(pr, tas, pa, k0):
        out = np.empty(pr.shape, np.float64)
        for c in range(pr.shape[0]):
            kbdi_fn(pr[c].astype(np.float64), tas[c].astype(np.float64), float(pa[c]), float(k0[c]), out[c])
        return out

    def df_all(pr, smd, lim):
        out = np.full(pr.shape, np.nan)  # rows 0..18: the reference's .where
        for c in range(pr.shape[0]):
            df_fn(pr[c].astype(np.float64), smd[c].astype(np.float64), lim, out[c])
        return out

    def case(name, C, T, lim=0, dtype=np.float32, kbdi0=None, smd=None, edit=None, **wkw):
        pr, tas, hurs, ws = weather(rng, C, T, dtype, **wkw)
        pa = np.round(rng.uniform(150, 1800, C), 1)
        if edit is not None:
            edit(pr, tas, hurs, ws, pa)
        k0 = np.zeros(C) if kbdi0 is None else kbdi0(C)
        kbdi = kbdi_all(pr, tas, pa, k0)
        df = df_all(pr, kbdi, lim)
        ffdi = np.asarray(ffdi_expr(df, tas, hurs, ws))
        ffdi32 = np.asarray(ffdi_expr(df.astype(np.float32), tas, hurs, ws))
        fields = {"pr": pr, "tasmax": tas, "hurs": hurs, "sfcWind": ws}
        rec = {k: quantize(v) if dtype == np.float32 else v for k, v in fields.items()}
        rec.update({"pr_annual": pa, "lim": np.int64(lim), "kbdi": kbdi, "df": df, "ffdi": ffdi, "ffdi_df32": ffdi32})
        if kbdi0 is not None:
            rec["kbdi0"] = k0
        if smd is not None:
            s = smd(kbdi)
            rec["smd"] = s
            rec["df_smd"] = df_all(pr, s, lim)
        cases.append((name, rec))
        print(name, {k: (str(v.dtype), float(np.nanmean(v))) for k, v in rec.items() if k in ("kbdi", "df", "ffdi", "ffdi_df32")},
              "kbdi at 203.2:", int((kbdi == 203.2).sum()), "at 0:", int((kbdi == 0).sum()))

    def hot_start(C):  # the reference's indicator test starts at 1 + 203.2; then a cell at the clamp, one below
        k = rng.uniform(0, 150, C)
        n = min(C, 3)
        k[:n] = [204.2, 203.2, 190.0][:n]
        return k

    def very_hot(pr, tas, hurs, ws, pa):  # ET over 203.2 - k in one day (the reference's 100 degC known answer)
        tas[0, 40:60] = 100.0
        pr[0, 40:60] = 0.0
        pa[0] = 1.0

    def nans(pr, tas, hurs, ws, pa):
        T = pr.shape[1]
        pr[0, T // 3] = np.nan                  # KBDI NaN from there on; DF: not an event
        hurs[0, 30] = np.nan                    # FFDI only
        pr[1, [5, 40, 41]] = np.nan
        pr[1, 90] = np.nan                      # positive rain after a NaN day: r = p (Peff = 0) until a dry day
        pr[1, [95, 97]] = [4.0, 3.0]
        pr[1, 100:130] = 0.0
        ws[1, 31] = np.nan
        tas[2, T // 2] = np.nan                 # KBDI NaN from there on (and FFDI that day)

    def smd_nan(kbdi):
        s = kbdi.copy()
        s[:, 50::37] = np.nan
        s[0, :] = np.where(np.isnan(s[0]), 15.0, s[0])
        return s

    def edges(pr, tas, hurs, ws, pa):
        # 20-day windows with rain exactly 2.0 (not an event), tied maxima inside an event (the later day gives N), an
        # event on the last day of the window, and smd band edges for the discrete limits
        pr[:] = 0.0
        pr[0, [3, 4, 5]] = [2.0, 2.0, 2.0]
        pr[1, [2, 3, 4, 5]] = [5.0, 8.0, 8.0, 3.0]
        pr[2, [2, 3, 4, 8, 9]] = [8.0, 2.0, 8.0, 6.0, 6.0]
        pr[3, 19] = 20.0
        pr[4, [0, 1, 18, 19]] = [30.0, 2.1, 2.0, 7.5]
        pr[5, :] = 3.0
        pr[6, ::2] = 10.0
        pr[7, [10, 11, 12]] = [2.0, 9.0, 2.0]
        pr[8, [0, 19]] = [50.0, 50.0]
        pr[9, 5:15] = np.arange(10, 0, -1)
        pr[10, 5:15] = np.arange(1, 11)
        pr[11, :] = 0.0

    def edge_smd(kbdi):
        s = np.empty_like(kbdi)
        for c, v in enumerate([0.0, 19.999, 20.0, 25.0, 41.999, 42.0, 64.5, 65.0, 100.0, 120.0, 203.2, np.nan]):
            s[c] = v
        return s

    case("seasonal_365", 2, 365)
    case("seasonal_365_discrete_kbdi0", 2, 365, lim=1, kbdi0=hot_start)
    case("dry_clamp_1095", 1, 1095, p_stay_dry=0.97, p_stay_wet=0.2, hot=6.0, kbdi0=hot_start, edit=very_hot)
    case("wet_clamp_365", 1, 365, lim=1, p_stay_dry=0.4, p_stay_wet=0.9, rain_scale=25.0, hot=-14.0)
    case("nan_150", 3, 150, edit=nans, smd=smd_nan)
    case("nan_150_discrete", 3, 150, lim=1, edit=nans, smd=smd_nan)
    case("edges_t20_xlim", 12, 20, edit=edges, smd=edge_smd)
    case("edges_t20_discrete", 12, 20, lim=1, edit=edges, smd=edge_smd)
    case("f64_seasonal_365", 2, 365, dtype=np.float64, kbdi0=hot_start, smd=smd_nan)
    case("f64_120_discrete", 3, 120, lim=1, dtype=np.float64, p_stay_dry=0.95, edit=nans)

    out = {}
    for name, rec in cases:
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
    out["cases"] = np.array([n for n, _ in cases])
    path = os.path.join(HERE, "ffdi_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
