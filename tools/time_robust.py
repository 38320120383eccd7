"""Time the change-robustness unit with HIP events (the context's timer around ONE launch, after two warm-up calls; the median of
the repetitions) and write one JSON line per case to profiles/r24/time_robust.jsonl.

    python tools/time_robust.py [--cells 1036800] [--members 20] [--years 30] [--reps 3] [--scipy 2000]

Cases, float32 fields of 1440 x 720 cells x 20 members of 30 / 30 annual values, on the device before the timer starts: each test
of xh_change_test (one launch), xh_ar6_gamma on the reference field (both rules), xh_robust_fractions on a test's result, and
xh_robust_coefficient.  Each line carries the read floor
(the bytes of both fields at 8 TB/s) and the read-plus-write floor.  ``--scipy N`` times what the reference runs per (cell,
realization) — the scipy call of each test, on one core, on N series pairs of the same fields — and scales it to the whole map."""
import argparse
import json
import os
import sys
import time as _time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402

OUT_BYTES = {"moments": 24, "ttest": 49, "welch": 49, "mwu": 49, "bf": 49}   # per series pair: delta, mean_ref, two counts (+ stat, df, p, status)


def timed(dev, reps, call):
    call()
    call()
    ms = []
    for _ in range(reps):
        dev.timer_start()
        out = call()
        ms.append(dev.timer_stop())
        del out
    return float(np.median(ms)), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1440 * 720)
    ap.add_argument("--members", type=int, default=20)
    ap.add_argument("--years", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy", type=int, default=2000)
    a = ap.parse_args()
    dev = get_device(0)
    rng = np.random.default_rng(0)
    R, T, C = a.members, a.years, a.cells
    slab = min(C, 1440 * 45)   # the host draws one slab and tiles it: the kernels' time does not depend on the values' origin
    reps_c = -(-C // slab)
    h_fut = (274.5 + rng.standard_normal((R, T, slab), dtype=np.float32))
    h_ref = (274.0 + 0.8 * rng.standard_normal((R, T, slab), dtype=np.float32))
    fut = dev.to_device(np.ascontiguousarray(np.tile(h_fut, (1, 1, reps_c))[:, :, :C]))
    ref = dev.to_device(np.ascontiguousarray(np.tile(h_ref, (1, 1, reps_c))[:, :, :C]))
    read = 2 * R * T * C * 4
    lines = []

    def record(case, ms, all_ms, read_b, write_b):
        line = {"case": case, "members": R, "years": [T, T], "cells": C, "dtype": "float32", "ms_median": round(ms, 3), "ms": all_ms,
                "read_floor_ms_8TBs": round(read_b / 8e12 * 1e3, 3), "read_write_floor_ms_8TBs": round((read_b + write_b) / 8e12 * 1e3, 3),
                "times_read_floor": round(ms / (read_b / 8e12 * 1e3), 1), "device": dev.name()}
        print(json.dumps(line), flush=True)
        lines.append(line)

    res = None
    for test in ("moments", "ttest", "welch", "mwu", "bf"):
        outs = K.change_test(dev, fut, ref, test)   # the output buffers are allocated once, outside the window
        ms, all_ms = timed(dev, a.reps, lambda: K.change_test(dev, fut, ref, test, outs=outs))
        record(f"change_test_{test}", ms, all_ms, read, R * C * OUT_BYTES[test])
        if test == "ttest":
            res = {k: v.get() for k, v in outs.items() if k in ("pvals", "delta")}
        del outs
    x_years = 365.0 * np.arange(T)
    blocks = np.append(np.arange(0, T, 20), T)
    for case, deg, seg in (("ar6_gamma_linear", 1, None), ("ar6_gamma_quadratic_20y_blocks", 2, blocks)):
        out = K.ar6_gamma(dev, ref, x_years, deg, 1.645, seg)
        ms, all_ms = timed(dev, a.reps, lambda: K.ar6_gamma(dev, ref, x_years, deg, 1.645, seg, out=out, ld_out=C))
        record(case, ms, all_ms, R * T * C * 4, R * C * 8)
        del out
    delta = dev.to_device(res["delta"])
    with np.errstate(invalid="ignore"):
        changed = dev.to_device((res["pvals"] < 0.05).astype(np.uint8))
    ms, all_ms = timed(dev, a.reps, lambda: K.robust_fractions(dev, delta, np.ones(R), changed=changed))
    record("robust_fractions", ms, all_ms, R * C * 9, 7 * C * 8)
    del delta, changed
    ref1 = dev.to_device(np.ascontiguousarray(np.tile(h_ref[0], (1, reps_c))[:, :C]))
    ms, all_ms = timed(dev, a.reps, lambda: K.robust_coefficient(dev, fut, ref1))
    record("robust_coefficient", ms, all_ms, (R + 1) * T * C * 4, C * 8)
    if a.scipy:
        from scipy import stats

        n = a.scipy
        # the pairs of the slab's first cells, member by member
        pairs = [(h_fut[r, :, c].astype(np.float64), h_ref[r, :, c].astype(np.float64)) for c in range(-(-n // R)) for r in range(R)][:n]
        calls = {"ttest": lambda x, y: stats.ttest_1samp(x, y.mean(), nan_policy="omit")[1],
                 "welch": lambda x, y: stats.ttest_ind(x, y, equal_var=False, nan_policy="omit")[1],
                 "mwu": lambda x, y: stats.mannwhitneyu(x, y, nan_policy="omit")[1],
                 "bf": lambda x, y: stats.levene(x, y, center="median")[1]}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for test, call in calls.items():
                t0 = _time.perf_counter()
                for x, y in pairs:
                    call(x, y)
                sec = _time.perf_counter() - t0
                line = {"case": f"scipy_one_core_{test}", "pairs": n, "us_per_pair": round(sec / n * 1e6, 1),
                        "seconds_for_the_map": round(sec / n * R * C, 0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
    out_path = os.path.join(ROOT, "profiles", "r24", "time_robust.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
