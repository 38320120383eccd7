"""McArthur fire danger timings on one MI355X: one JSON line per configuration.

    python tools/bench_ffdi.py [--reps 5] [--first]

ms is the median of HIP-event times of the xh_mcarthur launch (float32 inputs and float64 outputs already on the device);
bytes are the algorithmic traffic (every input field read once, every float64 output written once, the per-cell inputs);
hbm_share = bytes / ms against 8 TB/s.  No CPU baseline is timed: the reference path needs numba and xarray, which are not
part of this project's environment, and timing the test restatement (tests/ffdicpu.py) would say nothing about the
reference.
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402

PEAK = 8.0e12
READS = {"KBDI": ("pr", "tasmax"), "DF": ("pr", "smd"), "FFDI": ("tasmax", "hurs", "sfcWind", "df")}


def fields(dev, T, C):
    t = np.arange(T)
    tas = (24 + 9 * np.sin(2 * np.pi * (t - 20) / 365.0)).astype(np.float32)
    return {"pr": K.fill_synthetic(dev, T, C, 1, 2, np.zeros(T, np.float32), 9.0, 0.3),
            "tasmax": K.fill_synthetic(dev, T, C, 0, 1, tas, 5.0),
            "hurs": K.fill_synthetic(dev, T, C, 0, 3, np.full(T, 45.0, np.float32), 20.0),
            "sfcWind": K.fill_synthetic(dev, T, C, 0, 4, np.full(T, 18.0, np.float32), 8.0),
            "smd": K.fill_synthetic(dev, T, C, 0, 5, np.full(T, 100.0, np.float32), 60.0)}


def run(dev, name, T, ny, nx, outputs, reps):
    C = ny * nx
    f = fields(dev, T, C)
    rng = np.random.default_rng(1)
    pa = dev.to_device(rng.uniform(200, 1600, C))
    k0 = dev.to_device(rng.uniform(0, 200, C))
    used = {n for o in outputs for n in READS[o]}
    if "KBDI" in outputs:
        used.discard("smd")
    if "DF" in outputs:
        used.discard("df")
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        outs = K.mcarthur(dev, f, pa, k0, outputs=outputs, lim=0)
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del outs
    nbytes = T * C * (4 * len(used) + 8 * len(outputs)) + (C * 16 if "KBDI" in outputs else 0)
    ms = float(np.median(times))
    print(json.dumps({"config": name, "T": T, "cells": C, "ms": round(ms, 3), "bytes": nbytes,
                      "hbm_share": round(nbytes / (ms * 1e-3) / PEAK, 3), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="only the first configuration (for counter runs)")
    a = ap.parse_args()
    dev = get_device()
    run(dev, "chain_365x1440x720", 365, 720, 1440, ["KBDI", "DF", "FFDI"], a.reps)
    if a.first:
        return
    run(dev, "kbdi_365x1440x720", 365, 720, 1440, ["KBDI"], a.reps)
    run(dev, "df_365x1440x720", 365, 720, 1440, ["DF"], a.reps)
    run(dev, "chain_30y_1440x90", 365 * 30, 90, 1440, ["KBDI", "DF", "FFDI"], a.reps)


if __name__ == "__main__":
    main()
