"""The float64 twins of the period reductions (f64red.hip) against their float32 twins, HIP-event timing on one MI355X.

    python tools/bench_f64_reductions.py  ->  one JSON line per kernel and dtype: ms, bytes from the shapes over the time,
    share of the 8 TB/s peak.

Every twin on 30 years x 1440 x 90 (YS periods): degree days (cumulative_difference), temperature_sum,
thresholded_statistics(mean), the three range modes, domain_count, bivariate_count and the rolling mean of 5 and 31 days.
The degree-day and season chains of the host API (generic.cumulative_difference / generic.season on a device field,
results downloaded) on 365 x 1440 x 720.  The float64 field is the float32 field widened (same values, twice the bytes).
The bytes are those the algorithm must move: every input element once, plus the (T, C) output of the rolling statistic;
the (P, C) outputs are negligible and not counted."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["XCLIM_AMD_FLOAT64"] = "native"
import bench  # noqa: E402
from xclim_amd import generic as hgen  # noqa: E402
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


def twins():
    T, Y, X = 365 * 30, 1440, 90
    C = Y * X
    E = float(T) * C
    ta = TimeAxis.daily("1981-01-01", T, "noleap")
    seg, _ = ta.segments("YS")
    lo32 = K.fill_synthetic(dev, T, C, 0, 5, bench.seasonal_base(T) - 5.0, 3.0)
    hi32 = K.fill_synthetic(dev, T, C, 0, 6, bench.seasonal_base(T) + 5.0, 3.0)
    for dt in ("float32", "float64"):
        lo, hi = (lo32, hi32) if dt == "float32" else (widen(lo32), widen(hi32))
        es = 4 if dt == "float32" else 8
        run("thresholded_reduce mode 2 (growing degree days)", dt, lambda: K.thresholded_reduce(dev, lo, ">", 283.15, 2, "sum", seg), es * E)
        run("thresholded_reduce mode 1 (temperature_sum)", dt, lambda: K.thresholded_reduce(dev, lo, "<", 290.15, 1, "sum", seg), es * E)
        run("thresholded_reduce mode 0 mean", dt, lambda: K.thresholded_reduce(dev, lo, ">", 283.15, 0, "mean", seg), es * E)
        run("range_reduce range mean", dt, lambda: K.range_reduce(dev, lo, hi, "range", "mean", seg), 2 * es * E)
        run("range_reduce interday", dt, lambda: K.range_reduce(dev, lo, hi, "interday", "mean", seg), 2 * es * E)
        run("range_reduce extreme", dt, lambda: K.range_reduce(dev, lo, hi, "extreme", "max", seg), 2 * es * E)
        run("domain_count", dt, lambda: K.domain_count(dev, lo, ">", 275.0, "<=", 290.0, "and", seg), es * E)
        run("bivariate_count", dt, lambda: K.bivariate_count(dev, lo, hi, ">", 283.15, ">=", 295.15, "all", seg), 2 * es * E)
        for w in (5, 31):
            run(f"rolling_reduce mean w{w} centred", dt, lambda: K.rolling_reduce(dev, lo, w, "mean", True), 2 * es * E, reps=3)
        if dt == "float64":
            del lo, hi
    del lo32, hi32


def chains():
    T, Y, X = 365, 1440, 720
    C = Y * X
    E = float(T) * C
    ta = TimeAxis.daily("2001-01-01", T, "noleap")
    x32 = K.fill_synthetic(dev, T, C, 0, 2, bench.seasonal_base(T) - 10.0, 3.0)
    for dt, x in (("float32", x32), ("float64", widen(x32))):
        es = 4 if dt == "float32" else 8
        run("chain growing_degree_days (cumulative_difference, result downloaded)", dt,
            lambda: hgen.cumulative_difference(x, 278.15, ">", ta, "YS", device=dev), es * E)
        run("chain growing_season (season start / end / length, results downloaded)", dt,
            lambda: hgen.season(x, 278.15, 6, ">=", ta, "YS", "07-01", device=dev), es * E)


if __name__ == "__main__":
    print(json.dumps({"device": dev.name()}), flush=True)
    twins()
    chains()
