"""Time the thermal-comfort unit with HIP events (the context's timer around ONE launch, after two warm-up calls; the median of the
repetitions) and write one JSON line per case to profiles/r23/time_thermal.jsonl.

    python tools/time_thermal.py [--cells 1036800] [--days 365] [--hourly-days 31] [--reps 5] [--cpu] [--first]

Cases, float32 fields of 1440 x 720 cells: UTCI from seven fields on 365 daily rows and on 744 hourly rows; on each, UTCI with mrt
given, the mean radiant temperature alone and e_sat alone.  Each against its read-plus-write floor at 8 TB/s.  Fields, the per-row
table and the per-cell tables are on the device before the timer starts: the window holds the kernel and nothing else.
``--cpu`` adds the numpy restatement of the tests (tests/thermalcpu.py) on one core for a 1440 x 90 slab of 8 three-hourly rows: the
project's own restatement, not the reference.  ``--first`` runs the daily seven-field case once and nothing else (for a counter
run of its own)."""
import argparse
import json
import os
import sys
import time as _time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import thermal  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

NAMES = ("tas", "hurs", "sfcWind", "rsds", "rsus", "rlds", "rlus")


def host_fields(R, C, rng, only=NAMES):
    u = rng.random((R, C), dtype=np.float32)
    make = {"tas": lambda: 250 + 60 * u, "hurs": lambda: 5 + 90 * u[::-1], "sfcWind": lambda: 0.5 + 15 * u[:, ::-1], "rsds": lambda: 900 * u,
            "rsus": lambda: 180 * u, "rlds": lambda: 200 + 200 * u[::-1], "rlus": lambda: 250 + 250 * u[::-1]}
    for k in only:   # one field in host memory at a time
        yield k, np.ascontiguousarray(make[k](), dtype=np.float32)


def timed(dev, reps, call):
    call()
    call()
    ms = []
    for _ in range(reps):
        dev.timer_start()
        out = call()
        ms.append(dev.timer_stop())
        del out
    return float(np.median(ms)), [round(m, 4) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1440 * 720)
    ap.add_argument("--days", type=int, default=365)
    ap.add_argument("--hourly-days", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--first", action="store_true")
    a = ap.parse_args()
    dev = get_device(0)
    rng = np.random.default_rng(0)
    C = a.cells
    lat = np.linspace(-89.9, 89.9, C)
    lon = np.linspace(0, 359.9, C)
    latr = dev.to_device(thermal._wrap_radians(lat * (np.pi / 180)))
    lonr = dev.to_device(lon * (np.pi / 180))
    lines = []
    for name, days, sub in (("daily", a.days, None), ("hourly", a.hourly_days, thermal.SubDaily(24))):
        t = TimeAxis.daily("2001-01-01", days, "noleap")
        R = days * (sub.steps_per_day if sub else 1)
        f = {k: dev.to_device(v) for k, v in host_fields(R, C, rng)}
        rows = dev.to_device(thermal.solar_rows(t, subdaily=sub))
        mode = "subdaily" if sub else "daily"
        given = {"tas": f["tas"], "hurs": f["hurs"], "sfcWind": f["sfcWind"], "mrt": f["rlus"]}
        rad = {k: f[k] for k in ("rsds", "rsus", "rlds", "rlus")}
        cases = [(f"utci_seven_fields_{name}", 7 * 4 + 4, lambda: K.thermal_comfort(dev, f, rows, latr, lonr, mode=mode)),
                 (f"utci_mrt_given_{name}", 4 * 4 + 4, lambda: K.thermal_comfort(dev, given)),
                 (f"mrt_alone_{name}", 4 * 4 + 8, lambda: K.thermal_comfort(dev, rad, rows, latr, lonr, mode=mode, outputs=("mrt",))),
                 (f"esat_alone_{name}", 4 + 4, lambda: K.esat(dev, f["tas"], "its90"))]
        if a.first:
            cases[0][2]()
            dev.sync()
            return
        for case, bytes_per_sample, call in cases:
            ms, all_ms = timed(dev, a.reps, call)
            floor = R * C * bytes_per_sample / 8e12 * 1e3
            line = {"case": case, "rows": R, "cells": C, "dtype": "float32", "ms_median": round(ms, 4), "ms": all_ms,
                    "floor_ms_8TBs": round(floor, 4), "times_floor": round(ms / floor, 2), "device": dev.name()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        del f, given, rad, cases
    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import thermalcpu as TC

        sub, R, Cs = thermal.SubDaily(8), 8, 1440 * 90
        t = TimeAxis.daily("2001-06-20", 1, "noleap")
        f = dict(host_fields(R, Cs, rng))
        rows = thermal.solar_rows(t, subdaily=sub)
        t0 = _time.perf_counter()
        cs, _ = TC.csza(rows, thermal._wrap_radians(lat[:Cs] * (np.pi / 180)), lon[:Cs] * (np.pi / 180), "subdaily", "sunlit")
        m = TC.mrt(cs, rows[6], f["rsds"], f["rsus"], f["rlds"], f["rlus"])[0]
        TC.utci(f["tas"], f["hurs"], f["sfcWind"], m)
        sec = _time.perf_counter() - t0
        line = {"case": "numpy_restatement_one_core_utci_seven_fields (tests/thermalcpu.py; NOT the reference)", "rows": R, "cells": Cs,
                "dtype": "float32", "seconds": round(sec, 3), "ns_per_sample": round(sec / (R * Cs) * 1e9, 1)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    out_path = os.path.join(ROOT, "profiles", "r23", "time_thermal.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
