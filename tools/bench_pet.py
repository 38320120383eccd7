"""Potential evapotranspiration timings on one MI355X: one JSON line per configuration.

    python tools/bench_pet.py [--reps 5] [--first] [--cpu]

ms is the median of HIP-event times of the PET launch (xh_pet_daily / xh_pet_monthly; float32 fields already on the
device, the solar tables built before the timed window); table_ms times the table launches (xh_solar_table, and
xh_pet_month_table for the monthly methods) on their own.  bytes are the algorithmic traffic (every field the method reads
once, the float64 output written once); hbm_share = bytes / ms against 8 TB/s.  ``--cpu`` adds one line for the numpy
restatement of the tests (tests/petcpu.py) on a 365 x 1440 x 90 slab: that is this project's own restatement on one CPU
core, NOT the reference (which needs xarray and pint, absent here).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xclim_amd import converters as xc  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

PEAK = 8.0e12
READS = {"BR65": ("tasmin", "tasmax"), "HG85": ("tasmin", "tasmax"), "MB05": ("tas",), "TW48": ("tas",),
         "DA02": ("tasmin", "tasmax", "pr"),
         "FAO_PM98": ("tasmin", "tasmax", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind")}
SYNTH = {"tasmin": (0, 1, 278.0, 6.0), "tasmax": (0, 2, 288.0, 6.0), "tas": (0, 3, 283.0, 8.0), "hurs": (0, 4, 60.0, 30.0),
         "rsds": (0, 5, 180.0, 90.0), "rsus": (0, 6, 40.0, 20.0), "rlds": (0, 7, 320.0, 40.0), "rlus": (0, 8, 390.0, 40.0),
         "sfcWind": (0, 9, 5.0, 3.0), "pr": (1, 10, 0.0, 2e-4)}


def _timed(dev, fn, reps):
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        out = fn()
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del out
    return float(np.median(times))


def run(dev, method, T, ny, nx, reps, start="2001-01-01"):
    C = ny * nx
    t = TimeAxis.daily(start, T)
    f = {n: K.fill_synthetic(dev, T, C, SYNTH[n][0], SYNTH[n][1], np.full(T, SYNTH[n][2], np.float32), SYNTH[n][3])
         for n in READS[method]}
    lat_u = np.linspace(-89.875, 89.875, ny)
    li = np.repeat(np.arange(ny, dtype=np.int32), nx)
    if method in K.PET_DAILY:
        dang = xc.day_angle(t)
        sc = 1367.0 if method == "MB05" else 1361.0
        table_ms = 0.0 if method == "FAO_PM98" else _timed(dev, lambda: K.pet_solar_table(dev, dang, lat_u, sc)[0], reps)
        ra = None if method == "FAO_PM98" else K.pet_solar_table(dev, dang, lat_u, sc)[0]
        ms = _timed(dev, lambda: K.pet_daily(dev, method, f, ra, li), reps)
        rows = T
    else:
        seg, months, days, dseg, ndays = xc._months(t)
        dang = xc.day_angle(days)
        kind = 0 if method == "TW48" else 1

        def table():
            ra, dl = K.pet_solar_table(dev, dang, lat_u, ra=kind == 1, dl=kind == 0)
            return K.pet_month_table(dev, dl if kind == 0 else ra, dseg, kind)

        table_ms = _timed(dev, table, reps)
        tab = table()
        ms = _timed(dev, lambda: K.pet_monthly(dev, method, f, seg, int(months.month[0]) - 1, tab, ndays * 86400.0, li),
                    reps)
        rows = len(months)
    nbytes = T * C * 4 * len(READS[method]) + rows * C * 8
    print(json.dumps({"config": f"{method}_{T}x{nx}x{ny}", "T": T, "cells": C, "ms": round(ms, 3),
                      "table_ms": round(table_ms, 3), "bytes": nbytes, "hbm_share": round(nbytes / (ms * 1e-3) / PEAK, 3),
                      "reps": reps}), flush=True)


def cpu_baseline(method="FAO_PM98", T=365, ny=90, nx=1440):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import petcpu

    rng = np.random.default_rng(0)
    t = TimeAxis.daily("2001-01-01", T)
    C = ny * nx
    f = {n: (SYNTH[n][2] + SYNTH[n][3] * rng.random((T, C), dtype=np.float32)).astype(np.float32) for n in READS[method]}
    lat = np.repeat(np.linspace(-89, 89, ny), nx)
    t0 = time.perf_counter()
    petcpu.pet_daily(method, t, lat, **f)
    s = time.perf_counter() - t0
    print(json.dumps({"config": f"cpu_numpy_restatement_{method}_{T}x{nx}x{ny}", "what": "tests/petcpu.py on one core, not "
                      "the reference", "T": T, "cells": C, "ms": round(s * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="only the first configuration (for counter runs)")
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement on a 365 x 1440 x 90 slab")
    a = ap.parse_args()
    dev = get_device()
    run(dev, "FAO_PM98", 365, 720, 1440, a.reps)
    if a.first:
        return
    for m in ("BR65", "HG85", "MB05", "TW48", "DA02"):
        run(dev, m, 365, 720, 1440, a.reps)
    run(dev, "TW48", 10958, 90, 1440, a.reps, start="1991-01-01")
    if a.cpu:
        cpu_baseline()


if __name__ == "__main__":
    main()
