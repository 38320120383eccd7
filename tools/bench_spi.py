"""Standardized precipitation index timings on one MI355X: one JSON line per configuration.

    python tools/bench_spi.py [--reps 3] [--first] [--staging auto|global|lds] [--no-cpu]

fit_ms / apply_ms are medians of HIP-event times of the xh_si_fit and xh_si_apply launches (the preprocessed series
already on the device); nfev_* summarise the Nelder-Mead objective evaluations per fit (the spread that decides how long a
wave runs).  The monthly configurations start from monthly means (70 years of daily values would not fit in memory); the
daily one fits 366 day-of-year groups.  cpu_fit_s_extrapolated: scipy's own fits (``gamma.fit`` from the reference's start
values, restated in tests/spicpu.py) timed on a sample of --cpu-sample (cell, group) samples and scaled to the whole grid —
an extrapolation, not a measurement of the full grid.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402


def cpu_fit_seconds(dev, x, groups, G, method, floc, n_sample, rng):
    import scipy.stats

    import spicpu

    T, C = x.shape
    cells = rng.choice(C, n_sample, replace=True)
    gs = rng.integers(0, G, n_sample)
    xt = x.get()  # (not timed)
    t0 = time.perf_counter()
    for c, g in zip(cells, gs):
        v = xt[groups == g, c].astype(np.float64)
        v = v[~np.isnan(v) & (v != 0)]
        if len(v) <= 1:
            continue
        if method == "APP":
            spicpu.fit_start("gamma", list(v), floc)
            continue
        loc0 = spicpu.loc_estimation(list(v))
        a0, s0 = spicpu.fit_start("gamma", list(v), loc0)
        try:
            scipy.stats.gamma.fit(v, a0, loc=loc0, scale=s0, method="mle")
        except Exception:
            pass
    per_fit = (time.perf_counter() - t0) / n_sample
    return per_fit * G * C


def run(dev, name, x, groups, G, cal_rows, method, floc, reps, staging, cpu_sample, rng):
    T, C = x.shape
    gfit = np.where(np.arange(T) < cal_rows, groups, -1).astype(np.int32)
    fit_t, app_t = [], []
    for r in range(reps + 1):
        dev.timer_start()
        params, nz, nn, nfev = K.si_fit(dev, x, gfit, G, "gamma", method, floc=floc, zero_inflated=True, staging=staging,
                                        want_nfev=(r == 0))
        ms = dev.timer_stop()
        if r == 0:
            nf = nfev.get()
            nf = nf[nf > 0]
        else:
            fit_t.append(ms)
        dev.timer_start()
        si = K.si_apply(dev, x, groups, params, "gamma", nz, nn)
        ms = dev.timer_stop()
        if r:
            app_t.append(ms)
        del si, params, nz, nn, nfev
    line = {"config": name, "T": T, "cells": C, "groups": G, "cal_rows": cal_rows, "method": method, "floc": floc,
            "staging": staging, "fit_ms": round(float(np.median(fit_t)), 2), "apply_ms": round(float(np.median(app_t)), 3),
            "apply_bytes": T * C * 12, "reps": reps}
    if nf.size:
        line.update(nfev_median=int(np.median(nf)), nfev_p99=int(np.percentile(nf, 99)), nfev_max=int(nf.max()),
                    nfev_at_budget=round(float((nf >= 600).mean()), 4))
    if cpu_sample:
        s = cpu_fit_seconds(dev, x, gfit, G, method, floc, cpu_sample, rng)
        line.update(cpu_fit_s_extrapolated=round(s, 1), cpu_sample=cpu_sample)
    print(json.dumps(line), flush=True)


def monthly(dev, years, ny, nx, window, seed):
    T = 12 * years
    C = ny * nx
    base = np.tile(2.0 + 1.5 * np.sin(2 * np.pi * (np.arange(12) - 3) / 12.0), years).astype(np.float32)
    x = K.fill_synthetic(dev, T, C, 1, seed, base, 3.0, 0.93)  # monthly means: mostly wet, a few dry months
    if window > 1:
        x = K.rolling_reduce(dev, x, window, "mean", center=False)
    return x, np.tile(np.arange(12, dtype=np.int32), years)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--first", action="store_true", help="only the first configuration (for counter runs)")
    ap.add_argument("--staging", default="auto", choices=["auto", "global", "lds"])
    ap.add_argument("--cpu-sample", type=int, default=300)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = get_device()
    rng = np.random.default_rng(0)
    cpu = 0 if a.no_cpu else a.cpu_sample
    x, g = monthly(dev, 70, 720, 1440, 3, 7)
    run(dev, "spi3_monthly_gamma_ML_70y_cal30_1440x720", x, g, 12, 360, "ML", None, a.reps, a.staging, cpu, rng)
    if a.first:
        return
    run(dev, "spi3_monthly_gamma_APP_70y_cal30_1440x720", x, g, 12, 360, "APP", 0.0, a.reps, a.staging, 0, rng)
    del x
    years = 30
    from xclim_amd.timeaxis import TimeAxis

    t = TimeAxis.daily("1981-01-01", 365 * years + years // 4, "standard")
    T, C = len(t), 90 * 1440
    xd = K.fill_synthetic(dev, T, C, 1, 9, np.full(T, 2.0, np.float32), 8.0, 0.4)
    run(dev, "spi1_daily_gamma_ML_30y_1440x90", xd, (t.doy - 1).astype(np.int32), 366, T, "ML", None, a.reps, a.staging, 0, rng)


if __name__ == "__main__":
    main()
