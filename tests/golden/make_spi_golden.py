"""Generate tests/golden/spi_vectors.npz by EXECUTING the reference's fitting code with scipy.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_spi_golden.py

src/xclim/indices/stats.py cannot be imported (xarray).  ``_fit_start`` (with its nested ``_loc_estimation``) and
``_fitfunc_1d`` are AST-extracted (nothing is copied into this repository) and run with scipy on every (group, cell) sample.
The rest of the chain is restated here in numpy:

* preprocessing: ``MS`` means and the trailing ``rolling(time=window).mean(skipna=False)``, each a float64 sum in time order
  rounded once to float32 (this package's float32 means);
* the sample of a group is the float32 preprocessed values widened to float64, zeros masked when zero-inflated
  (``da.where(da != 0)``), counts as in standardized_index_fit_params (stats.py:939-945);
* the index: ``scipy.stats.<dist>.cdf`` / ``norm.ppf`` and the zero-inflated mixture as stats.py:1156-1190 writes it.

Every case stores the daily input as int16 multiples of ``scale`` (``decode``: float32(k) * float32(scale)), its dates,
the options, the preprocessed series ``xp`` (float32), the fitted ``params`` (G, 3, C), the counts and the index; a
``reuse`` case fits on its first years and applies the parameters to the whole series.  tests/test_stdidx_cpu.py and
tests/test_gpu_stdidx.py read it.
"""

import ast
import json
import os
import warnings

import numpy as np
import pandas as pd
import scipy.stats

REF = "/root/reference/src/xclim/indices/stats.py"
HERE = os.path.dirname(os.path.abspath(__file__))


def extract():
    tree = ast.parse(open(REF).read())
    ns = {"np": np, "scipy": scipy, "warnings": warnings}
    body = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("_fit_start", "_fitfunc_1d"):
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            if node.args.kwarg is not None:
                node.args.kwarg.annotation = None
            body.append(node)
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    assert "_fit_start" in ns and "_fitfunc_1d" in ns
    return ns


def decode(codes, scale):
    return codes.astype(np.float32) * np.float32(scale)


def dates(start, T, calendar):
    if calendar == "standard":
        d = pd.date_range(start, periods=T, freq="D")
        return d.year.values, d.month.values, d.day.values
    y, m, dd = (int(p) for p in start.split("-"))
    mlen = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    out = []
    while len(out) < T:
        out.append((y, m, dd))
        dd += 1
        if dd > mlen[m - 1]:
            dd, m = 1, m + 1
            if m > 12:
                m, y = 1, y + 1
    a = np.array(out)
    return a[:, 0], a[:, 1], a[:, 2]


def doy_of(y, m, d, calendar):
    cum = np.array([0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334])
    leap = (calendar == "standard") & (((y % 4 == 0) & (y % 100 != 0)) | (y % 400 == 0))
    return cum[m - 1] + d + ((m > 2) & leap)


def mean32(vals):
    """float64 sum in order, one rounding to float32; NaN skipped (all-NaN -> NaN)."""
    s, n = 0.0, 0
    for v in vals:
        if v == v:
            s += float(v)
            n += 1
    return np.float32(s / n) if n else np.float32(np.nan)


def preprocess(x, y, m, d, freq, window):
    """(T, C) float32 daily -> (xp (T', C) float32, (y, m, d) of the rows)."""
    if freq == "MS":
        key = y * 12 + (m - 1)
        keys = np.arange(key[0], key[-1] + 1)
        xp = np.empty((len(keys), x.shape[1]), np.float32)
        for i, k in enumerate(keys):
            rows = x[key == k]
            for c in range(x.shape[1]):
                xp[i, c] = mean32(rows[:, c]) if len(rows) else np.nan
        y, m, d = keys // 12, keys % 12 + 1, np.ones(len(keys), int)
    else:
        xp = x.copy()
    if window > 1:
        out = np.full_like(xp, np.nan)
        for t in range(window - 1, len(xp)):
            w = xp[t - window + 1 : t + 1].astype(np.float64)
            for c in range(xp.shape[1]):
                col = w[:, c]
                if not np.isnan(col).any():
                    s = 0.0
                    for v in col:
                        s += float(v)
                    out[t, c] = np.float32(s / window)
        xp = out
    return xp, (y, m, d)


def fit(ns, xp, gidx, G, dist, method, zero_inflated, floc):
    C = xp.shape[1]
    params = np.full((G, 3, C), np.nan)
    nz = np.full((G, C), np.nan)
    nn = np.full((G, C), np.nan)
    failed = np.zeros((G, C), bool)
    sdist = getattr(scipy.stats, dist)
    fk = {} if floc is None else {"floc": floc}
    for g in range(G):
        rows = np.flatnonzero(gidx == g)
        if len(rows) == 0:
            continue
        for c in range(C):
            v = xp[rows, c].astype(np.float64)
            nz[g, c] = np.sum(v == 0)
            nn[g, c] = np.sum(~np.isnan(v))
            if zero_inflated:
                v = np.where(v != 0, v, np.nan)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    params[g, :, c] = ns["_fitfunc_1d"](v, dist=sdist, nparams=3, method=method, **fk)
            except Exception:  # FitError / FitDataError: the reference fails; the device gives NaN
                failed[g, c] = True
    return params, nz, nn, failed


def index(xp, gidx, params, dist, nz, nn, interp, ab):
    sdist = getattr(scipy.stats, dist)
    p = params[gidx]  # (T, 3, C)
    v = xp.astype(np.float64)
    with np.errstate(all="ignore"):
        if nz is not None:
            mask = v != 0
            pn = sdist.cdf(np.where(mask, v, np.nan), p[:, 0], p[:, 1], p[:, 2])
            z, n = nz[gidx], nn[gidx]
            alpha, beta = ab
            r1 = (1 - alpha) / (n + 1 - alpha - beta)
            rn = (z - alpha) / (n + 1 - alpha - beta)
            rf = (1 - interp) * r1 + interp * rn
            probs = np.where(mask, rn + ((1 - rn) * pn), rf)
        else:
            probs = sdist.cdf(v, p[:, 0], p[:, 1], p[:, 2])
        return np.clip(scipy.stats.norm.ppf(probs), -8.21, 8.21)


def precip(rng, T, C, doy, wet=0.35):
    seas = 1.0 + 0.6 * np.sin(2 * np.pi * (doy[:, None] - 80) / 365.0)
    amt = rng.gamma(0.7, 6.0, (T, C)) * seas
    return np.where(rng.random((T, C)) < wet, amt, 0.0)


CASES = [
    # name, dist, method, floc, zero_inflated, freq, window, years, calendar, interp, plotting, cal, kind
    ("gamma_ml_ms3", "gamma", "ML", None, True, "MS", 3, 9, "noleap", "upper", "ecdf", None, "pr"),
    ("gamma_app_ms1_center", "gamma", "APP", 0.0, True, "MS", 1, 9, "noleap", "center", "ecdf", None, "pr"),
    ("gamma_mlfloc_ms12_weibull", "gamma", "ML", 0.0, True, "MS", 12, 11, "standard", "upper", "weibull", None, "pr"),
    ("gamma_ml_ms1_float", "gamma", "ML", None, True, "MS", 1, 9, "noleap", 0.3, (0.4, 0.4), None, "pr"),
    ("fisk_app_negfloc_ms3", "fisk", "APP", -30.0, False, "MS", 3, 7, "noleap", "upper", "ecdf", None, "wb"),
    ("fisk_ml_ms1", "fisk", "ML", None, False, "MS", 1, 7, "noleap", "upper", "ecdf", None, "wb"),
    ("fisk_mlfloc_ms3", "fisk", "ML", -40.0, False, "MS", 3, 7, "noleap", "upper", "ecdf", None, "wb"),
    ("gamma_app_daily_leap", "gamma", "APP", 0.0, True, "D", 1, 4, "standard", "upper", "ecdf", None, "pr"),
    ("gamma_mlfloc_daily", "gamma", "ML", 0.0, True, "D", 1, 3, "noleap", "upper", "ecdf", None, "pr"),
    ("gamma_ml_daily_w3", "gamma", "ML", None, True, "D", 3, 3, "noleap", "upper", "ecdf", None, "pr"),
    ("gamma_ml_ms3_cal", "gamma", "ML", None, True, "MS", 3, 10, "noleap", "upper", "ecdf", ("2001-01-01", "2006-12-31"), "pr"),
    ("gamma_ml_ms3_reuse", "gamma", "ML", None, True, "MS", 3, 10, "noleap", "upper", "ecdf", "reuse", "pr"),
]


def make_case(ns, rng, spec):
    name, dist, method, floc, zi, freq, window, years, calendar, interp, plotting, cal, kind = spec
    C = 3 if freq == "MS" else 2
    T = 365 * years + (years // 4 if calendar == "standard" else 0)
    y, m, d = dates("2000-01-01", T, calendar)
    doy = doy_of(y, m, d, calendar)
    if kind == "pr":
        raw = precip(rng, T, C, doy)
        if freq == "MS":
            raw[m == 7, 0] = 0.0                                 # cell 0: July is always dry -> an all-zero group
            jul = np.flatnonzero(m == 7)
            raw[jul, 1] = 0.0
            raw[jul[40], 1] = 5.0                                 # cell 1: one wet July in the series -> one value
        scale = 0.1
    else:
        base = 1.5 + 3.0 * np.sin(2 * np.pi * (doy[:, None] - 100) / 365.0)
        raw = precip(rng, T, C, doy, 0.5) - base - rng.gamma(2.0, 1.0, (T, C))
        scale = 0.25
    codes = np.clip(np.round(raw / scale), -32000, 32000).astype(np.int16)
    x = decode(codes, scale)
    x[100:160, C - 1] = np.nan                                   # a NaN run
    if freq == "D":
        x[400:403, 0] = np.nan
    xp, (py, pm, pd_) = preprocess(x, y, m, d, freq, window)
    if freq == "MS":
        gidx, G = (pm - 1).astype(np.int32), 12
    else:
        gidx, G = (doy_of(py, pm, pd_, calendar) - 1).astype(np.int32), 366
    interp_f = {"center": 0.5, "upper": 1.0}.get(interp, interp) if isinstance(interp, str) else float(interp)
    ab = {"ecdf": (0, 1), "weibull": (0, 0)}[plotting] if isinstance(plotting, str) else plotting
    out = {"codes": codes, "scale": np.float32(scale), "year": y.astype(np.int16), "month": m.astype(np.int8), "day": d.astype(np.int8),
           "xp": xp, "gidx": gidx}
    fitrows = np.ones(len(xp), bool)
    xfit = xp
    if cal == "reuse":
        # the parameters of the first 8 years (their own preprocessing), applied to the whole series
        Ta = int(np.flatnonzero(y == 2006)[0])
        xa, (ay, am, ad) = preprocess(x[:Ta], y[:Ta], m[:Ta], d[:Ta], freq, window)
        xfit, fit_g = xa, (am - 1).astype(np.int32)
        out["reuse_T"] = np.int64(Ta)
        out["xp_fit"] = xa
    elif cal is not None:
        key = py * 10000 + pm * 100 + pd_
        lo, hi = (int(s.replace("-", "")) for s in cal)
        fitrows = (key >= lo) & (key <= hi)
        fit_g = np.where(fitrows, gidx, -1)
    else:
        fit_g = gidx
    params, nz, nn, failed = fit(ns, xfit, fit_g, G, dist, method, zi, floc)
    spi = index(xp, gidx, params, dist, nz if zi else None, nn if zi else None, interp_f, ab)
    out.update(params=params, nz=nz, nn=nn, failed=failed, spi=spi, fit_g=fit_g.astype(np.int32))
    meta = {"dist": dist, "method": method, "floc": floc, "zero_inflated": zi, "freq": freq, "window": window,
            "calendar": calendar, "interp": interp if isinstance(interp, str) else float(interp),
            "plotting": plotting if isinstance(plotting, str) else list(plotting),
            "cal": cal if (cal is None or cal == "reuse") else list(cal), "G": G}
    return out, meta


def main():
    ns = extract()
    rng = np.random.default_rng(20261015)
    arrays, metas = {}, {}
    for spec in CASES:
        out, meta = make_case(ns, rng, spec)
        for k, v in out.items():
            arrays[f"{spec[0]}__{k}"] = v
        metas[spec[0]] = meta
        print(spec[0], "fits:", int(np.isfinite(out["params"][:, 0]).sum()), "failed:", int(out["failed"].sum()),
              "spi finite:", int(np.isfinite(out["spi"]).sum()))
    arrays["meta"] = np.array(json.dumps(metas))
    path = os.path.join(HERE, "spi_vectors.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
