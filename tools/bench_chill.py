"""Winter-chill timings on one MI355X: one JSON line per configuration.

    python tools/bench_chill.py [--reps 5] [--first]

ms is the median of HIP-event times of the one launch (xh_chill_daily or xh_chill_hourly; float32 inputs, the day-length
table and the float64 outputs already on the device).  bytes are the algorithmic traffic: every input field read once
(the fused path reads tasmin and tasmax, and the next day's tasmin from cache), the (day, latitude) day-length table, every
output written once.  hbm_share = bytes / ms against 8 TB/s; hours_per_s = cell-hours stepped per second, the figure that
matters for a kernel bound by float64 issue.  No CPU baseline is timed: the reference path needs xarray, which is not part
of this project's environment, and timing the test restatement (tests/chillcpu.py) would say nothing about the reference.
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.converters import day_angle  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

PEAK = 8.0e12


def report(name, rows, C, times, nbytes, hours, reps):
    ms = float(np.median(times))
    print(json.dumps({"config": name, "rows": rows, "cells": C, "ms": round(ms, 3), "bytes": int(nbytes),
                      "hbm_share": round(nbytes / (ms * 1e-3) / PEAK, 4), "hours_per_s": round(hours / (ms * 1e-3), 0),
                      "reps": reps}), flush=True)


def timed(dev, reps, launch):
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        outs = launch()
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del outs
    return times


def daily_inputs(dev, D, ny, nx):
    t = np.arange(D)
    season = (9 * np.cos(2 * np.pi * (t - 200) / 365.0)).astype(np.float32)
    C = ny * nx
    tn = K.fill_synthetic(dev, D, C, 0, 71, 274 - season, 3.0)
    tx = K.fill_synthetic(dev, D, C, 0, 72, 283 - season, 3.0)
    lats = np.linspace(-60, 60, ny)
    time = TimeAxis.daily("2001-01-01", D, "noleap")
    _, dl = K.pet_solar_table(dev, day_angle(time), lats, ra=False, dl=True)
    return tn, tx, dl, np.repeat(np.arange(ny, dtype=np.int32), nx)


def fused(dev, name, D, ny, nx, outputs, reps):
    tn, tx, dl, li = daily_inputs(dev, D, ny, nx)
    C = ny * nx
    times = timed(dev, reps, lambda: K.chill_daily(dev, tn, tx, dl, li, [0, D], outputs=outputs))
    nbytes = D * C * 8 + D * ny * 8 + C * 4 + len(outputs) * C * 8
    report(name, D, C, times, nbytes, 24 * D * C, reps)


def hourly_temperature(dev, name, D, ny, nx, reps):
    tn, tx, dl, li = daily_inputs(dev, D, ny, nx)
    C = ny * nx
    times = timed(dev, reps, lambda: K.chill_daily(dev, tn, tx, dl, li, [0, D], outputs=("hourly",)))
    report(name, D, C, times, D * C * 8 + D * ny * 8 + C * 4 + 24 * D * C * 8, 24 * D * C, reps)


def hourly(dev, name, D, ny, nx, outputs, reps):
    H, C = 24 * D, ny * nx
    h = np.arange(H)
    base = (278 - 9 * np.cos(2 * np.pi * (h / 24.0 - 200) / 365.0) + 4 * np.sin(2 * np.pi * (h - 9) / 24.0)).astype(np.float32)
    tas = K.fill_synthetic(dev, H, C, 0, 73, base, 2.0)
    times = timed(dev, reps, lambda: K.chill_hourly(dev, tas, [0, H], outputs=outputs))
    report(name, H, C, times, H * C * 4 + len(outputs) * C * 8, H * C, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="only the first configuration (for counter runs)")
    a = ap.parse_args()
    dev = get_device()
    fused(dev, "fused_cp_cu_365x1440x720", 365, 720, 1440, ("cp", "cu"), a.reps)
    if a.first:
        return
    fused(dev, "fused_cp_365x1440x720", 365, 720, 1440, ("cp",), a.reps)
    fused(dev, "fused_cu_365x1440x720", 365, 720, 1440, ("cu",), a.reps)
    hourly(dev, "hourly_cp_cu_8760x1440x90", 365, 90, 1440, ("cp", "cu"), a.reps)
    hourly(dev, "hourly_cp_8760x1440x90", 365, 90, 1440, ("cp",), a.reps)
    hourly_temperature(dev, "make_hourly_temperature_365x1440x90", 365, 90, 1440, a.reps)


if __name__ == "__main__":
    main()
