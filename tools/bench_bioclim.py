"""ANUCLIM BIO1-BIO19 timings on one MI355X: one JSON line per configuration.

    python tools/bench_bioclim.py [--reps 5] [--first] [--no-parent]

``single``: ms is the median of HIP-event times of the ONE launch of xh_bioclim (float32 fields and the float64 outputs already
on the device; the host tables go up inside the timed region).  ``floor_ms`` is the read floor: the bytes of the fields the
launch reads, once, over the streaming read rate measured on this box (profiles/r01/hbm_ubench.txt: 6.1 TB/s); ``of_floor``
= ms / floor_ms.  The lead-in of 12 weeks in front of every period is NOT in the floor (it is re-read traffic).

``parent``: the route the package offered for the same outputs before xh_bioclim, timed by the wall clock with the fields on
the device: the weekly resample on the device (xh_resample_reduce), the download of the weekly fields, rolling(13) and the
selections (nanargmax / nanargmin per period) in numpy, the upload of the quarter series and their period maxima and minima
on the device; for the nineteen also the period reductions of BIO1-BIO7 and BIO12-BIO15 (xh_resample_reduce,
xh_range_reduce), one launch each.  It computes float32 statistics, so it is the cheaper arithmetic.
"""

import argparse
import json
import os
import sys
import time as clock

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import anuclim  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

READ_RATE = 6.1e12
QUARTERS = ("bio8", "bio9", "bio10", "bio11", "bio16", "bio17", "bio18", "bio19")
DAY = 86400.0


def fields(dev, T, C):
    t = np.arange(T)
    season = (10 * np.sin(2 * np.pi * (t - 100) / 365.0)).astype(np.float32)
    return dict(tas=K.fill_synthetic(dev, T, C, 0, 81, 283 + season, 3.0), tasmin=K.fill_synthetic(dev, T, C, 0, 82, 279 + season, 3.0),
                tasmax=K.fill_synthetic(dev, T, C, 0, 83, 288 + season, 3.0),
                pr=K.fill_synthetic(dev, T, C, 0, 84, (3e-5 + 1e-5 * np.cos(2 * np.pi * t / 365.0)).astype(np.float32), 2e-5))


def single(dev, name, f, time, outputs, reps):
    tab = anuclim.axis_tables(time, "YS")
    T, C = f["tas"].shape
    reads = sorted({r for o in outputs for r in anuclim._READS[int(o[3:])]})
    d = {k: f[k] for k in reads}
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        outs = K.bioclim(dev, d, tab["step_off"], DAY * tab["days"], tab["seg_rows"], tab["seg_steps"], tab["W"], cv_scale=DAY,
                         outputs=outputs)
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del outs
    ms = float(np.median(times))
    nbytes = len(reads) * T * C * 4
    floor = nbytes / READ_RATE * 1e3
    rec = {"config": name, "route": "single", "rows": T, "cells": C, "periods": len(tab["seg_rows"]) - 1, "outputs": len(outputs),
           "fields_read": len(reads), "ms": round(ms, 3), "bytes_read": nbytes, "floor_ms": round(floor, 3), "of_floor": round(ms / floor, 2),
           "reps": reps}
    print(json.dumps(rec), flush=True)
    return ms


def parent(dev, name, f, time, nineteen, reps):
    """The same outputs through the entry points the package had before (see the module text)."""
    tab = anuclim.axis_tables(time, "YS")
    so, sr, ss = tab["step_off"], tab["seg_rows"], tab["seg_steps"]
    P = len(sr) - 1
    times = []
    for r in range(reps):
        dev.sync()
        t0 = clock.perf_counter()
        tw = K.resample_reduce(dev, f["tas"], "mean", so, want_valid=False)[0].get().astype(np.float64)
        pw = K.resample_reduce(dev, f["pr"], "sum", so, want_valid=False)[0].get().astype(np.float64) * DAY
        qt = np.full(tw.shape, np.nan)
        qp = np.full(pw.shape, np.nan)
        qt[12:] = np.lib.stride_tricks.sliding_window_view(tw, 13, axis=0).mean(axis=-1)
        qp[12:] = np.lib.stride_tricks.sliding_window_view(pw, 13, axis=0).sum(axis=-1)
        dq = {"t": dev.to_device(qt.astype(np.float32)), "p": dev.to_device(qp.astype(np.float32))}
        out = {}
        for k, (q, red) in {"bio10": ("t", "max"), "bio11": ("t", "min"), "bio16": ("p", "max"), "bio17": ("p", "min")}.items():
            out[k] = K.resample_reduce(dev, dq[q], red, ss, want_valid=False)[0].get()
        for p in range(P):          # _from_other_arg: a map over the periods
            a, b = int(ss[p]), int(ss[p + 1])
            for k, crit, other, arg in (("bio8", qp, qt, np.argmax), ("bio9", qp, qt, np.argmin), ("bio18", qt, qp, np.argmax),
                                        ("bio19", qt, qp, np.argmin)):
                c = crit[a:b]
                allnan = np.isnan(c).all(axis=0)
                fill = -np.inf if arg is np.argmax else np.inf
                i = arg(np.where(np.isnan(c), fill, c), axis=0)
                out.setdefault(k, []).append(np.where(allnan, np.nan, np.take_along_axis(other[a:b], i[None], 0)[0]))
        if nineteen:
            for k, (x, red) in {"bio1": ("tas", "mean"), "bio5": ("tasmax", "max"), "bio6": ("tasmin", "min"), "bio12": ("pr", "sum"),
                                "bio13": ("pr", "max"), "bio14": ("pr", "min"), "std_t": ("tas", "std"), "std_p": ("pr", "std"),
                                "mean_p": ("pr", "mean")}.items():
                out[k] = K.resample_reduce(dev, f[x], red, sr, want_valid=False)[0].get()
            out["bio2"] = K.range_reduce(dev, f["tasmin"], f["tasmax"], "range", "mean", sr, want_valid=False)[0].get()
            out["bio7"] = K.range_reduce(dev, f["tasmin"], f["tasmax"], "extreme", "max", sr, want_valid=False)[0].get()
        dev.sync()
        times.append((clock.perf_counter() - t0) * 1e3)
        del out, dq
    ms = float(np.median(times))
    print(json.dumps({"config": name, "route": "parent", "rows": int(f["tas"].shape[0]), "cells": int(f["tas"].shape[1]), "periods": P,
                      "outputs": 19 if nineteen else 8, "ms": round(ms, 1), "reps": reps}), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--first", action="store_true", help="only the single launches of the first size (for kernel-stats runs)")
    ap.add_argument("--no-parent", action="store_true")
    a = ap.parse_args()
    dev = get_device()
    for name, T, C in (("365x1440x720", 365, 1440 * 720), ("30yx1440x90", 10957, 1440 * 90)):
        time = TimeAxis.daily("1981-01-01", T)
        f = fields(dev, T, C)
        s19 = single(dev, f"all19_{name}", f, time, K.BIOCLIM_VARS, a.reps)
        s8 = single(dev, f"quarters_{name}", f, time, QUARTERS, a.reps)
        if a.first:
            return
        if not a.no_parent:
            p19 = parent(dev, f"all19_{name}", f, time, True, 2)
            p8 = parent(dev, f"quarters_{name}", f, time, False, 2)
            print(json.dumps({"config": name, "single_over_parent_all19": round(s19 / p19, 4), "single_over_parent_quarters": round(s8 / p8, 4)}),
                  flush=True)
            assert s19 <= p19 and s8 <= p8, "the single launch is slower than the route it replaces"
        del f


if __name__ == "__main__":
    main()
