"""Streamflow and snow-melt timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_hydro.py [--reps 7] [--cells 1036800]

A timed window is ``--calls`` calls in a row (20; 4 for the Sen slope) between one pair of HIP events, 10 to 250 ms of work, and
``ms`` is the median over the reps of window / calls (float32 fields and, for the Sen slope, the period means already on the
device; outputs allocated and host tables uploaded inside the window), after one untimed warm-up window of every configuration;
the fused launch and the chain it replaces are timed in turn, rep by rep, in the same process.  ``bytes_read`` is
what the call must read once: the field (two for melt and precipitation) for the period kernels — the few halo rows of a period
are not in the floor — and the (P, C) period means for the Sen slope.  ``floor_ms`` is that over 8 TB/s, the HBM3E peak of the part;
``of_floor`` = ms / floor_ms.

The chain of the base flow index is what the library offered before this unit: ``xh_rolling_reduce`` (the centred 7-day mean, a
(T, C) float32 intermediate) + ``xh_resample_reduce`` min of it + ``xh_resample_reduce`` mean of q; it gives float32 results where
the fused launch gives float64.  The Richards-Baker index and the melt maxima have no chain to compare with: the library has no
entry point that differences consecutive rows."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import hydrology  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

PEAK = 8.0e12


def timed(dev, configs, reps, calls):
    """configs: [(name, launch, bytes, extra)].  One warm-up window each, then ``reps`` rounds that run every configuration once;
    a timed window is ``calls`` calls in a row between one pair of events, and ``ms`` is the window over ``calls``."""
    times = {name: [] for name, *_ in configs}
    for r in range(reps + 1):
        for name, launch, _, _ in configs:
            dev.timer_start()
            for _ in range(calls):
                outs = launch()      # (the outputs of the call before are released here)
            ms = dev.timer_stop() / calls
            if r:
                times[name].append(ms)
            del outs
    for name, _, nbytes, extra in configs:
        ms = float(np.median(times[name]))
        floor = nbytes / PEAK * 1e3
        print(json.dumps(dict(config=name, ms=round(ms, 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                              bytes_read=int(nbytes), floor_ms=round(floor, 3), of_floor=round(ms / floor, 2),
                              gbps=round(nbytes / ms / 1e6, 1), reps=reps, calls_per_window=calls, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cells", type=int, default=1440 * 720)
    ap.add_argument("--years", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window (the Sen slope: a fifth of it)")
    a = ap.parse_args()
    dev = get_device()
    T, C = 365, a.cells
    time = TimeAxis.daily("1981-01-01", T)
    t = np.arange(T)
    q = K.fill_synthetic(dev, T, C, 0, 71, (60 + 30 * np.sin(2 * np.pi * (t - 120) / 365.0)).astype(np.float32), 12.0)
    snw = K.fill_synthetic(dev, T, C, 0, 72, (80 + 70 * np.cos(2 * np.pi * (t - 30) / 365.0)).astype(np.float32), 6.0)
    pr = K.fill_synthetic(dev, T, C, 0, 73, (3e-5 + 1e-5 * np.cos(2 * np.pi * t / 365.0)).astype(np.float32), 2e-5)
    seg = time.segments("YS")[0]
    shape = dict(rows=T, cells=C)

    def bfi_chain():
        m7 = K.rolling_reduce(dev, q, 7, "mean", center=True)
        return K.resample_reduce(dev, m7, "min", seg, want_valid=False), K.resample_reduce(dev, q, "mean", seg, want_valid=False)

    field = T * C * 4
    timed(dev, [
        ("flow_stats_bfi+rbi", lambda: K.flow_period_stats(dev, q, seg, outputs=("bfi", "rbi")), field, shape),
        ("flow_stats_bfi", lambda: K.flow_period_stats(dev, q, seg, outputs=("bfi",)), field, shape),
        ("chain_bfi_rolling+min+mean", bfi_chain, field, dict(shape, note="floor of the fused launch; the chain moves the field four times")),
        ("melt_and_precip_max_w3", lambda: K.melt_period_max(dev, snw, seg, pr, window=3), 2 * field, shape),
        ("snow_melt_we_max_w3", lambda: K.melt_period_max(dev, snw, seg, None, window=3), field, shape),
        ("melt_and_precip_max_w31", lambda: K.melt_period_max(dev, snw, seg, pr, window=31), 2 * field, shape),
        ("antecedent_precip_w7", lambda: K.antecedent_precip(dev, pr, hydrology.api_weights(7, 0.935)), field,
         dict(shape, note="also writes a (T, C) float64 field: 2 x the bytes read")),
    ], a.reps, a.calls)
    del q, snw, pr

    # the Sen slope of 30 years of four seasons: the period means as the mirror hands them over
    Y, S = a.years, 4
    P = Y * S
    means = K.fill_synthetic(dev, P, C, 0, 74, (60 + 0.05 * np.arange(P)).astype(np.float32), 8.0)
    period_of = np.arange(P, dtype=np.int64).reshape(Y, S)
    timed(dev, [(f"sen_slope_{Y}y_x_{S}", lambda: K.sen_slope(dev, means, period_of), P * C * 4,
                 dict(years=Y, seasons=S, cells=C, series=S * C))], a.reps, max(1, a.calls // 5))


if __name__ == "__main__":
    main()
