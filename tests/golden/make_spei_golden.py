"""Generate tests/golden/spei_vectors.npz: the standardized indices of FLOAT64 fields, by EXECUTING the reference's fitting
code with scipy.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_spei_golden.py

As tests/golden/make_spi_golden.py (whose helpers are imported), ``_fit_start`` and ``_fitfunc_1d`` of
src/xclim/indices/stats.py are AST-extracted and run with scipy on every (group, cell) sample, but here the samples are the
float64 preprocessed values themselves: nothing is rounded to float32 or widened from it, as upstream runs on a float64
field.  The rest of the chain is restated in numpy, float64 throughout, in the summation order of this package's float64
twins:

* ``MS`` means: the non-NaN values of the month added in row order from 0.0, divided by their count
  (``xh_resample_reduce_f64``);
* the trailing ``rolling(time=window).mean(skipna=False)``: the window added first row to last, divided by the window, NaN
  when any value of the window is NaN (``xh_rolling_reduce_f64``).  xarray's own rolling mean uses bottleneck's running
  sum (add the new value, subtract the old one) or numpy's sum over the window view, so its values can differ from these
  in the last bit or two (a few 1e-16 relative); its monthly means (a pairwise or axis sum) likewise.  The fits and the
  index are compared at tolerances far above that;
* the index: ``scipy.stats.<dist>.cdf`` / ``norm.ppf`` and the zero-inflated mixture (make_spi_golden.index).

Inputs are float64 values that float32 cannot represent: int32 codes times a float64 scale (``decode``: float64(k) *
scale, exact on every machine).  Water-budget-like cases (``wb``) are precipitation minus a seasonal PET, with negative
values; ``pr`` cases have exact zeros.  The ``lds_cap`` case has 36 values per group, above the 32 that the float64
instance stages in LDS, so ``auto`` takes the global work buffer.  It starts from monthly values (``monthly_input``).
tests/test_spei64_cpu.py and tests/test_gpu_spei64.py read the file.
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_spi_golden import dates, doy_of, extract, fit, index, precip  # noqa: E402

SCALE = {"pr": 0.0123456789012345, "wb": 0.00987654321098765}  # float64 steps: k * scale is not a float32 value


def decode(codes, scale):
    return codes.astype(np.float64) * np.float64(scale)


def mean64(vals):
    """the non-NaN values added in row order from 0.0, / their count (all-NaN -> NaN)."""
    s, n = 0.0, 0
    for v in vals:
        if v == v:
            s += float(v)
            n += 1
    return s / n if n else np.nan


def preprocess(x, y, m, d, freq, window, monthly_input=False):
    """(T, C) float64 -> (xp (T', C) float64, (y, m, d) of the rows)."""
    if freq == "MS" and not monthly_input:
        key = y * 12 + (m - 1)
        keys = np.arange(key[0], key[-1] + 1)
        xp = np.empty((len(keys), x.shape[1]), np.float64)
        for i, k in enumerate(keys):
            rows = x[key == k]
            for c in range(x.shape[1]):
                xp[i, c] = mean64(rows[:, c]) if len(rows) else np.nan
        y, m, d = keys // 12, keys % 12 + 1, np.ones(len(keys), int)
    else:
        xp = x.copy()
    if window > 1:
        out = np.full_like(xp, np.nan)
        for t in range(window - 1, len(xp)):
            for c in range(xp.shape[1]):
                col = xp[t - window + 1 : t + 1, c]
                if not np.isnan(col).any():
                    s = float(col[0])
                    for v in col[1:]:
                        s += float(v)
                    out[t, c] = s / window
        xp = out
    return xp, (y, m, d)


CASES = [
    # name, dist, method, floc, zero_inflated, freq, window, years, calendar, interp, plotting, cal, kind
    ("spei_gamma_ml_ms3", "gamma", "ML", None, False, "MS", 3, 6, "noleap", "upper", "ecdf", None, "wb"),
    ("spei_fisk_ml_ms1", "fisk", "ML", None, False, "MS", 1, 6, "noleap", "upper", "ecdf", None, "wb"),
    ("spei_gamma_app_negfloc_ms3", "gamma", "APP", -30.0, False, "MS", 3, 6, "noleap", "upper", "ecdf", None, "wb"),
    ("spei_fisk_app_negfloc_ms12", "fisk", "APP", -25.0, False, "MS", 12, 9, "standard", "upper", "ecdf", None, "wb"),
    ("spei_gamma_mlfloc_negfloc_ms3", "gamma", "ML", -20.0, False, "MS", 3, 6, "noleap", "upper", "ecdf", None, "wb"),
    ("spi64_gamma_ml_ms3", "gamma", "ML", None, True, "MS", 3, 7, "noleap", "upper", "ecdf", None, "pr"),
    ("spi64_gamma_app_ms1_center", "gamma", "APP", 0.0, True, "MS", 1, 7, "noleap", "center", "ecdf", None, "pr"),
    ("spi64_gamma_mlfloc_ms12_weibull", "gamma", "ML", 0.0, True, "MS", 12, 9, "standard", "upper", "weibull", None, "pr"),
    ("spei_gamma_app_daily_leap", "gamma", "APP", -30.0, False, "D", 1, 4, "standard", "upper", "ecdf", None, "wb"),
    ("spei_gamma_ml_ms3_cal", "gamma", "ML", None, False, "MS", 3, 8, "noleap", "upper", "ecdf", ("2001-01-01", "2006-12-31"), "wb"),
    ("spei_gamma_ml_ms3_reuse", "gamma", "ML", None, False, "MS", 3, 8, "noleap", "upper", "ecdf", "reuse", "wb"),
    ("spei_gamma_ml_ms1_lds_cap", "gamma", "ML", None, False, "MS", 1, 36, "noleap", "upper", "ecdf", None, "wb_monthly"),
]


def make_case(ns, rng, spec):
    name, dist, method, floc, zi, freq, window, years, calendar, interp, plotting, cal, kind = spec
    C = 3 if freq == "MS" else 2
    monthly_input = kind == "wb_monthly"
    if monthly_input:
        T = 12 * years
        y = np.repeat(np.arange(2000, 2000 + years), 12)
        m = np.tile(np.arange(1, 13), years)
        d = np.ones(T, int)
        mid = doy_of(y, m, np.full(T, 15), calendar)
        pet = 1.5 + 3.0 * np.sin(2 * np.pi * (mid[:, None] - 100) / 365.0)
        raw = rng.gamma(2.5, 1.6, (T, C)) - pet
        scale = SCALE["wb"]
    else:
        T = 365 * years + (years // 4 if calendar == "standard" else 0)
        y, m, d = dates("2000-01-01", T, calendar)
        doy = doy_of(y, m, d, calendar)
        if kind == "pr":
            raw = precip(rng, T, C, doy)
            if freq == "MS":
                raw[m == 7, 0] = 0.0                          # cell 0: July is always dry -> an all-zero group
                jul = np.flatnonzero(m == 7)
                raw[jul, 1] = 0.0
                raw[jul[40], 1] = 5.0                          # cell 1: one wet July in the series -> one value
        else:  # precipitation minus a seasonal PET [mm/day]: negative values
            pet = 1.5 + 3.0 * np.sin(2 * np.pi * (doy[:, None] - 100) / 365.0)
            raw = precip(rng, T, C, doy, 0.5) - pet - rng.gamma(2.0, 1.0, (T, C))
        scale = SCALE["pr" if kind == "pr" else "wb"]
    codes = np.round(raw / scale).astype(np.int32)
    x = decode(codes, scale)
    if monthly_input:
        x[30:42, C - 1] = np.nan                               # a NaN year
    else:
        x[100:160, C - 1] = np.nan                             # a NaN run: May is a NaN month
        if freq == "D":
            x[400:403, 0] = np.nan
    xp, (py, pm, pd_) = preprocess(x, y, m, d, freq, window, monthly_input)
    if freq == "MS":
        gidx, G = (pm - 1).astype(np.int32), 12
    else:
        gidx, G = (doy_of(py, pm, pd_, calendar) - 1).astype(np.int32), 366
    interp_f = {"center": 0.5, "upper": 1.0}.get(interp, interp) if isinstance(interp, str) else float(interp)
    ab = {"ecdf": (0, 1), "weibull": (0, 0)}[plotting] if isinstance(plotting, str) else plotting
    out = {"codes": codes, "scale": np.float64(scale), "year": y.astype(np.int16), "month": m.astype(np.int8),
           "day": d.astype(np.int8), "xp": xp, "gidx": gidx}
    xfit = xp
    if cal == "reuse":
        # the parameters of the first 6 years (their own preprocessing), applied to the whole series
        Ta = int(np.flatnonzero(y == 2006)[0])
        xa, (ay, am, ad) = preprocess(x[:Ta], y[:Ta], m[:Ta], d[:Ta], freq, window)
        xfit, fit_g = xa, (am - 1).astype(np.int32)
        out["reuse_T"] = np.int64(Ta)
        out["xp_fit"] = xa
    elif cal is not None:
        key = py * 10000 + pm * 100 + pd_
        lo, hi = (int(s.replace("-", "")) for s in cal)
        fit_g = np.where((key >= lo) & (key <= hi), gidx, -1)
    else:
        fit_g = gidx
    params, nz, nn, failed = fit(ns, xfit, fit_g, G, dist, method, zi, floc)
    si = index(xp, gidx, params, dist, nz if zi else None, nn if zi else None, interp_f, ab)
    out.update(params=params, nz=nz, nn=nn, failed=failed, spi=si, fit_g=fit_g.astype(np.int32))
    meta = {"dist": dist, "method": method, "floc": floc, "zero_inflated": zi, "freq": freq, "window": window,
            "calendar": calendar, "interp": interp if isinstance(interp, str) else float(interp),
            "plotting": plotting if isinstance(plotting, str) else list(plotting),
            "cal": cal if (cal is None or cal == "reuse") else list(cal), "G": G, "kind": kind,
            "monthly_input": monthly_input}
    return out, meta


def main():
    ns = extract()
    rng = np.random.default_rng(20261016)
    arrays, metas = {}, {}
    for spec in CASES:
        out, meta = make_case(ns, rng, spec)
        for k, v in out.items():
            arrays[f"{spec[0]}__{k}"] = v
        metas[spec[0]] = meta
        print(spec[0], "fits:", int(np.isfinite(out["params"][:, 0]).sum()), "failed:", int(out["failed"].sum()),
              "index finite:", int(np.isfinite(out["spi"]).sum()))
    arrays["meta"] = np.array(json.dumps(metas))
    path = os.path.join(HERE, "spei_vectors.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
