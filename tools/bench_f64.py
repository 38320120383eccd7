"""float64 fields (XCLIM_AMD_FLOAT64=native) against their float32 twins, HIP-event timing on one MI355X.

    python tools/bench_f64.py  ->  one JSON line per kernel and dtype: ms, bytes from the shapes over the time, share of the
    8 TB/s peak.

The marches (compare, cdd run statistics, the fused spell statistics with window 3, the WSDI run statistics against a
float64 per-doy table) on 365 x 1440 x 720; percentile_doy
(window 5) and the tx90p count against its table on 30 years x 1440 x 90.  The float64 field is the float32 field widened
(same values, twice the bytes).  Kernel times for DESIGN come from a separate `rocprofv3 --kernel-trace --stats` run of
this script."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import Device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

dev = Device(0)


def run(name, dtype, fn, nbytes, reps=5):
    ms = bench.event_time(dev, fn, reps)
    print(json.dumps({"kernel": name, "dtype": dtype, "ms": round(ms, 4), "GB/s": round(nbytes / ms / 1e6, 1),
                      "frac": round(nbytes / ms / 1e6 / bench.HBM_PEAK_GBS, 3)}), flush=True)


def widen(x32):
    x64 = dev.to_device(x32.get().astype(np.float64))
    dev.sync()
    return x64


def marches():
    T, Y, X = 365, 1440, 720
    C = Y * X
    E = float(T) * C
    ta = TimeAxis.daily("2001-01-01", T, "noleap")
    seg, _ = ta.segments("YS")
    tas32 = K.fill_synthetic(dev, T, C, 0, 2, bench.seasonal_base(T), 3.0)
    pr32 = K.fill_synthetic(dev, T, C, 1, 3, np.zeros(T, np.float32), 40.0 / 86400.0, 0.3)
    thr = 1.0 / 86400.0
    table = dev.to_device(np.full((T, C), 291.0))  # a per-doy float64 table (WSDI: the spell condition against it)
    tidx = np.arange(T, dtype=np.int32)
    for dt, tas, pr in (("float32", tas32, pr32), ("float64", widen(tas32), widen(pr32))):
        es = 4 if dt == "float32" else 8
        run("compare_map maskf", dt, lambda: K.compare_map(dev, tas, ">", 290.0, "maskf"), (es + 4) * E)
        run("run_stats max w1 fused compare (cdd)", dt, lambda: K.run_stats(dev, pr, "max", 1, seg, cut=True, fused_op="<", thresh=thr),
            es * E)
        run("spell_run_stats w3 mean max (fused)", dt, lambda: K.spell_run_stats(dev, pr, 3, "mean", ">=", thr, "max", seg), es * E)
        run("run_stats_doy sum w6 (wsdi)", dt, lambda: K.run_stats_doy(dev, tas, ">", table, tidx, "sum", 6, seg), (es + 8) * E)
        del tas, pr


def percentiles():
    T, Y, X = 365 * 30, 1440, 90
    C = Y * X
    ta = TimeAxis.daily("1981-01-01", T, "noleap")
    seg, _ = ta.segments("YS")
    tb, _, doys = ta.doy_table()
    tidx = (ta.doy - 1).astype(np.int32)
    x32 = K.fill_synthetic(dev, T, C, 0, 5, bench.seasonal_base(T), 3.0)
    for dt, x in (("float32", x32), ("float64", widen(x32))):
        es = 4 if dt == "float32" else 8
        table = K.percentile_doy(dev, x, tb, 5, [90.0])
        tab = table.reshape(len(doys), C)
        run("percentile_doy w5 p90", dt, lambda: K.percentile_doy(dev, x, tb, 5, [90.0], out=table), es * float(T) * C + 8.0 * len(doys) * C,
            reps=2)
        run("threshold_count per-doy table (tx90p)", dt, lambda: K.threshold_count(dev, x, ">", seg, doy_table=tab, tidx=tidx),
            es * float(T) * C + 8.0 * len(doys) * C)
        del x, table, tab


if __name__ == "__main__":
    print(json.dumps({"device": dev.name()}), flush=True)
    marches()
    percentiles()
