"""Numpy restatement of the float64 chain of the standardized indices (XCLIM_AMD_FLOAT64=native): the preprocessing of
xh_resample_reduce_f64 / xh_rolling_reduce_f64 in their summation order, then the fits and the transform of
xh_si_fit_f64 / xh_si_apply_f64, which run the same float64 arithmetic as the float32 instances once the field is read
(tests/spicpu.py, called here on the float64 values as they are).  tests/test_spei64_cpu.py checks it against
tests/golden/spei_vectors.npz (the reference's own fits on float64 samples)."""

import numpy as np

import spicpu


def month_means(x, year, month):
    """MS means of a daily (T, C) float64 field: the non-NaN values added in row order from 0.0, / their count."""
    key = year.astype(np.int64) * 12 + (month.astype(np.int64) - 1)
    keys = np.arange(key[0], key[-1] + 1)
    out = np.empty((len(keys), x.shape[1]), np.float64)
    for i, k in enumerate(keys):
        s = np.zeros(x.shape[1])
        n = np.zeros(x.shape[1], np.int64)
        for row in x[key == k]:
            ok = ~np.isnan(row)
            s = s + np.where(ok, row, 0.0)  # s starts at +0.0 and never becomes -0.0: adding 0.0 leaves it as it is
            n += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            out[i] = np.where(n > 0, s / np.maximum(n, 1), np.nan)
    return out


def rolling_mean(x, window):
    """Trailing rolling(window).mean(skipna=False): the window added first row to last, / window; NaN if incomplete."""
    out = np.full_like(x, np.nan)
    for t in range(window - 1, len(x)):
        s = x[t - window + 1].copy()
        for k in range(t - window + 2, t + 1):
            s = s + x[k]
        out[t] = s / window
    return out


def preprocess(x, year, month, freq, window, monthly_input=False):
    xp = month_means(x, year, month) if freq == "MS" and not monthly_input else np.array(x, np.float64)
    return rolling_mean(xp, window) if window > 1 else xp


fit = spicpu.fit
index = spicpu.index
