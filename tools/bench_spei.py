"""SPEI timings of float64 fields on one MI355X (XCLIM_AMD_FLOAT64=native): one JSON line per configuration.

    python tools/bench_spei.py [--reps 2] [--first] [--no-chain]

The field is a monthly water budget on 1440 x 720 cells, 70 years, built from float64 uniforms (no value is a float32), and
the SPEI-3 of it is fitted on 30 years (cal_rows = 360) with gamma ML and fisk ML.  Every configuration runs twice: on the
float64 field (xh_si_fit_f64 / xh_si_apply_f64) and on the same values rounded to float32 (xh_si_fit / xh_si_apply).  fit_ms
/ apply_ms are medians of HIP-event times of the one launch each (the 3-month means already on the device); nfev_*
summarise the Nelder-Mead objective evaluations per fit.  The chain line times converters.water_budget(..., keep=True)
(MB05 on 30 years of daily tas / pr, 1440 x 90 cells) and the SPEI-3 of its float64 device array, end to end with the
host-side calls, no host round trip.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["XCLIM_AMD_FLOAT64"] = "native"

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402


def monthly_wb(dev, years, C, seed):
    """(12 years, C) float64 and float32 (the same values rounded) device fields, uploaded a year at a time."""
    T = 12 * years
    d64 = dev.empty((T, C), np.float64)
    d32 = dev.empty((T, C), np.float32)
    rng = np.random.default_rng(seed)
    season = 2.0 + 1.5 * np.sin(2 * np.pi * (np.arange(12) - 3) / 12.0)
    shift = rng.uniform(-1.0, 1.0, C)
    for y in range(years):
        chunk = 4.0 * rng.random((12, C)) + 2.0 * rng.random((12, C)) - season[:, None] + shift[None, :]
        c32 = chunk.astype(np.float32)
        dev.copy2d(d64.ptr + y * 12 * C * 8, C * 8, chunk.ctypes.data, C * 8, C * 8, 12, "h2d")
        dev.copy2d(d32.ptr + y * 12 * C * 4, C * 4, c32.ctypes.data, C * 4, C * 4, 12, "h2d")
    return d64, d32


def run(dev, name, x, groups, G, cal_rows, dist, reps):
    T, C = x.shape
    gfit = np.where(np.arange(T) < cal_rows, groups, -1).astype(np.int32)
    fit_t, app_t = [], []
    for r in range(reps + 1):
        dev.timer_start()
        params, _, _, nfev = K.si_fit(dev, x, gfit, G, dist, "ML", want_nfev=(r == 0))
        ms = dev.timer_stop()
        if r == 0:
            nf = nfev.get()
            nf = nf[nf > 0]
        else:
            fit_t.append(ms)
        dev.timer_start()
        si = K.si_apply(dev, x, groups, params, dist)
        ms = dev.timer_stop()
        if r:
            app_t.append(ms)
        del si, params, nfev
    line = {"config": name, "dtype": np.dtype(x.dtype).name, "T": T, "cells": C, "groups": G, "cal_rows": cal_rows,
            "dist": dist, "method": "ML", "fit_ms": round(float(np.median(fit_t)), 2),
            "apply_ms": round(float(np.median(app_t)), 3), "reps": reps}
    if nf.size:
        line.update(nfev_median=int(np.median(nf)), nfev_p99=int(np.percentile(nf, 99)), nfev_max=int(nf.max()),
                    nfev_at_budget=round(float((nf >= 600).mean()), 4))
    print(json.dumps(line), flush=True)


def chain(dev, reps):
    from xclim_amd import converters as xc
    from xclim_amd import indices as xi
    from xclim_amd.timeaxis import TimeAxis

    years, ny, nx = 30, 90, 1440
    t = TimeAxis.daily("1981-01-01", 365 * years + years // 4, "standard")
    T, C = len(t), ny * nx
    doy = np.asarray(t.doy, np.float64)
    tas = K.fill_synthetic(dev, T, C, 0, 21, (283.0 + 10.0 * np.sin(2 * np.pi * (doy - 100) / 365.0)).astype(np.float32),
                           3.0)
    pr = K.fill_synthetic(dev, T, C, 1, 22, np.zeros(T, np.float32), 3e-4, 0.45)
    lat = np.repeat(np.linspace(-60.0, 70.0, ny), nx).reshape(ny, nx)
    wb_t, spei_t = [], []
    for r in range(reps + 1):
        dev.sync()
        t0 = time.perf_counter()
        wb = xc.water_budget(pr.reshape(T, ny, nx), tas=tas.reshape(T, ny, nx), lat=lat, time=t, method="MB05", device=dev,
                             keep=True)
        dev.sync()
        t1 = time.perf_counter()
        si = xi.standardized_precipitation_evapotranspiration_index(wb, t, freq="MS", window=3, device=dev, keep=True)
        dev.sync()
        t2 = time.perf_counter()
        if r:
            wb_t.append((t1 - t0) * 1e3)
            spei_t.append((t2 - t1) * 1e3)
        assert wb.dtype == np.float64 and si.dtype == np.float64
        del wb, si
    print(json.dumps({"config": "water_budget_MB05_keep_to_spei3_gamma_ML_30y_daily_1440x90", "T_daily": T, "cells": C,
                      "water_budget_ms": round(float(np.median(wb_t)), 1), "spei_ms": round(float(np.median(spei_t)), 1),
                      "chain_ms": round(float(np.median(np.add(wb_t, spei_t))), 1), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--first", action="store_true", help="only the float64 gamma ML configuration (for counter runs)")
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    dev = get_device()
    years, C = 70, 720 * 1440
    d64, d32 = monthly_wb(dev, years, C, 7)
    x64 = K.rolling_reduce(dev, d64, 3, "mean", center=False)
    x32 = K.rolling_reduce(dev, d32, 3, "mean", center=False)
    del d64, d32
    g = np.tile(np.arange(12, dtype=np.int32), years)
    for dist in ("gamma", "fisk"):
        for x in (x64, x32):
            run(dev, f"spei3_monthly_{dist}_ML_70y_cal30_1440x720", x, g, 12, 360, dist, a.reps)
            if a.first:
                return
    del x64, x32
    if not a.no_chain:
        chain(dev, a.reps)


if __name__ == "__main__":
    main()
