"""Fire weather system timings on one MI355X: one JSON line per configuration.

    python tools/bench_fire.py [--reps 5]

ms is the median of HIP-event times of the xh_fire_weather launch (inputs and outputs already on the device); bytes are
the algorithmic traffic (every input read once, every output written once); hbm_share = bytes / ms against 8 TB/s.
No CPU baseline is timed: the reference path needs numba and xarray, which are not part of this project's environment,
and timing the test restatement (tests/firecpu.py) would say nothing about the reference.
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.fire import _merged_params  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

PEAK = 8.0e12


def fields(dev, T, C, need_snd=False):
    t = np.arange(T)
    base = (8 + 12 * np.sin(2 * np.pi * (t - 105) / 365.0)).astype(np.float32)
    f = {"tas": K.fill_synthetic(dev, T, C, 0, 1, base, 6.0),
         "pr": K.fill_synthetic(dev, T, C, 1, 2, np.zeros(T, np.float32), 12.0, 0.35),
         "hurs": K.fill_synthetic(dev, T, C, 0, 3, np.full(T, 60.0, np.float32), 30.0),
         "sfcWind": K.fill_synthetic(dev, T, C, 0, 4, np.full(T, 14.0, np.float32), 10.0)}
    if need_snd:
        f["snd"] = K.fill_synthetic(dev, T, C, 0, 5, np.full(T, 0.05, np.float32), 0.1)
    return f


def run(dev, name, T, ny, nx, indexes, reps, **kw):
    C = ny * nx
    f = fields(dev, T, C, kw.get("season_method") in ("LA08", "GFWED"))
    if not indexes:
        f = {"tas": f["tas"]}
    lat = dev.to_device((np.linspace(-60, 80, ny)[:, None] * np.ones((1, nx))).reshape(-1))
    month = TimeAxis.daily("2001-01-01", T, "noleap").month
    starts = {"winter_pr": dev.zeros((C,), np.float32)} if kw.get("overwintering") else {}
    params = _merged_params({})
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        outs = K.fire_weather(dev, f, month, lat if indexes else None, starts, indexes, params, want_mask=kw.get("season_method") is not None,
                              want_winter_pr=bool(kw.get("overwintering")), **kw)
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del outs
    nin = len(f) * 4
    nout = 4 * len(indexes) + (1 if kw.get("season_method") else 0)
    nbytes = T * C * (nin + nout) + (C * 8 if indexes else 0)
    ms = float(np.median(times))
    print(json.dumps({"config": name, "T": T, "cells": C, "ms": round(ms, 3), "bytes": nbytes,
                      "hbm_share": round(nbytes / (ms * 1e-3) / PEAK, 3), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="only the first configuration (for counter runs)")
    a = ap.parse_args()
    dev = get_device()
    run(dev, "all7_season_none_365x1440x720", 365, 720, 1440, list(K.FIRE_INDEXES), a.reps)
    if a.first:
        return
    run(dev, "all7_wf93_overwinter_30y_1440x90", 365 * 30, 90, 1440, list(K.FIRE_INDEXES), a.reps, season_method="WF93",
        overwintering=True)
    run(dev, "fire_season_wf93_mask_only_365x1440x720", 365, 720, 1440, [], a.reps, season_method="WF93")


if __name__ == "__main__":
    main()
