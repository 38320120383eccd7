"""Time the uncertainty-partitioning unit with HIP events (the context's timer around the launches of ONE call, after two warm-up
calls; the median of the repetitions) and write one JSON line per case to profiles/r26/time_partition.jsonl.

    python tools/time_partition.py [--cells 64800] [--years 151] [--reps 3] [--cpu 1000] [--out FILE]

Cases, float32 fields of 151 years x 80 members x 360 x 180 cells, on the device before the timer starts, output buffers allocated
outside the window: Hawkins-Sutton on 4 x 20 members (the rolling mean over 10 years, the baseline, the HS variability
pre-pass), Lafferty-Sriver on 4 x 10 x 2, and the same with a land mask (30 % of the cells all NaN); xh_ensemble_stats on 80
realizations of a 1440 x 720 map.  Each line carries the bytes the call must read and write, that floor at 8 TB/s, and the ratio.
``--cpu N`` times tests/partitioncpu.py's lafferty_sriver on one core on N cells of the same field, without NaN (one lstsq for
all series) and with one NaN year in every series (one lstsq per series, polyfit's per-series path)."""
import argparse
import json
import os
import sys
import time as _time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import partitioning  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402


def timed(dev, reps, call):
    call()
    call()
    ms = []
    for _ in range(reps):
        dev.timer_start()
        call()
        ms.append(dev.timer_stop())
    return float(np.median(ms)), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=360 * 180)
    ap.add_argument("--years", type=int, default=151)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "time_partition.jsonl"))
    a = ap.parse_args()
    dev = get_device(0)
    rng = np.random.default_rng(0)
    T, N, C = a.years, 80, a.cells
    years = np.arange(1950, 1950 + T)
    time = TimeAxis(years, np.full(T, 12), np.full(T, 31), "standard")
    q = partitioning.poly_basis(time)
    slab = min(C, 4050)   # the host draws one slab and tiles it: the kernels' time does not depend on the values' origin
    trend = np.linspace(0, 3, T, dtype=np.float32)[:, None, None]
    h = (trend * (1 + 0.3 * rng.standard_normal((1, N, 1), dtype=np.float32)) + rng.standard_normal((T, N, slab), dtype=np.float32))
    field = np.ascontiguousarray(np.tile(h, (1, 1, -(-C // slab)))[:, :, :C])
    masked = field.copy()
    masked[:, :, rng.random(C) < 0.3] = np.nan
    lines = []

    def record(case, ms, all_ms, read_b, write_b, **more):
        floor = (read_b + write_b) / 8e12 * 1e3
        line = {"case": case, "years": T, "members": N, "cells": C, "dtype": "float32", "ms_median": round(ms, 3), "ms": all_ms,
                "read_bytes": int(read_b), "write_bytes": int(write_b), "floor_ms_8TBs": round(floor, 3), "times_floor": round(ms / floor, 1),
                "device": dev.name(), **more}
        print(json.dumps(line), flush=True)
        lines.append(line)

    t0 = int(np.searchsorted(years, 2000))
    base = (int(np.searchsorted(years, 1971)), int(np.searchsorted(years, 2000)) + 1)
    for tag, host in (("", field), ("_land_mask", masked)):
        y = dev.to_device(host)
        for name, dims, kw, comps, ckw in (
                ("hawkins_sutton", [4, 20], dict(window=10, stat="mean", baseline=base, kind="+"),
                 [(0, "mean_then_var", "user"), (1, "var_then_mean", "user")], dict(weights=np.ones(20), w_axis=1, variab="hs", t0=t0, g_order=(1, 0))),
                ("lafferty_sriver", [4, 10, 2], dict(window=11, stat="var"),
                 [(0, "mean_then_var", "none"), (1, "var_then_mean", "count"), (2, "var_then_mean", "count")], dict(g_order=(1, 0, 2)))):
            outs = K.partition_smooth(dev, y, q, **kw)
            ms, all_ms = timed(dev, a.reps, lambda: K.partition_smooth(dev, y, q, outs=outs, **kw))
            record(f"partition_smooth_{name}{tag}", ms, all_ms, T * N * C * 4, 2 * T * N * C * 8 + N * C * 5 + 1)
            out, g = K.partition_components(dev, outs["sm"], outs["roll"], dims, comps, **ckw)
            ms, all_ms = timed(dev, a.reps, lambda: K.partition_components(dev, outs["sm"], outs["roll"], dims, comps, out=out, g=g, **ckw))
            record(f"partition_components_{name}{tag}", ms, all_ms, 2 * T * N * C * 8, (len(comps) + 3) * T * C * 8, components=len(comps))
            del outs, out, g
        del y
    E = 1440 * 720
    x = dev.to_device(np.ascontiguousarray(np.tile(field[0, :, :slab], (1, -(-E // slab)))[:, :E]))
    for tag, w in (("", None), ("_weighted", np.linspace(0.5, 2.0, N))):
        out = K.ensemble_stats(dev, x, w)
        ms, all_ms = timed(dev, a.reps, lambda: K.ensemble_stats(dev, x, w, out=out, ld_out=E))
        record(f"ensemble_stats{tag}", ms, all_ms, N * E * 4, 4 * E * 8, cells=E, years=1)
    if a.cpu:
        import partitioncpu as P

        n = min(a.cpu, slab)
        cube = field[:, :, :n].reshape(T, 4, 10, 2, n)
        holed = cube.copy()
        holed[rng.integers(0, T, cube.shape[1:]), np.arange(4)[:, None, None, None], np.arange(10)[None, :, None, None],
              np.arange(2)[None, None, :, None], np.arange(n)[None, None, None, :]] = np.nan
        for tag, data in (("without_nan", cube), ("with_nan", holed)):
            t_start = _time.perf_counter()
            P.lafferty_sriver(data, years)
            sec = _time.perf_counter() - t_start
            line = {"case": f"numpy_restatement_one_core_lafferty_sriver_{tag}", "cells": n, "members": N, "years": T, "seconds": round(sec, 2),
                    "seconds_for_the_map": round(sec / n * C, 0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
