"""Rain-season and hardiness-zone timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_rain.py [--reps 7] [--cells 1036800]

A timed window is ``--calls`` calls in a row (20) between one pair of HIP events, and ``ms`` is the median over the reps of
window / calls (the float32 field already on the device; outputs allocated and host tables uploaded inside the window), after
one untimed warm-up window of every configuration; the configurations are timed in turn, rep by rep, in the same process.
``bytes_read`` is what the call must read once: the field.  ``floor_ms`` is that over 6.1 TB/s, the read rate DESIGN.md §3
records for this part (the yardstick of the bioclim row); ``of_floor`` = ms / floor_ms; ``of_peak`` the same over the 8 TB/s
HBM3E peak the agro and hydrology rows divide by.

``xh_rain_season`` runs on 365 x 1440 x 720 float32 in kg m-2 s-1 with the reference's default parameters (wet window 3 days,
30 days without a dry sequence of 7, a dry sequence of 20 days for the end; bounds 05-01 .. 12-31 and 09-01 .. 12-31), with
both methods "per_day" and both "total" (the dry windows then come from the LDS ring: 7 and 20 additions per row).  The field
has a wet season from May to mid-October so that lanes find starts and ends (``found``: the share of cells with a value).  ``xh_rolling_zones`` runs on 30 x 1440 x 720 float32
period minima with the reference's window of 30 periods and the 27 USDA edges."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import rainseason  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

READ_RATE = 6.1e12
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
        floor = nbytes / READ_RATE * 1e3
        print(json.dumps(dict(config=name, ms=round(ms, 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                              bytes_read=int(nbytes), floor_ms=round(floor, 3), of_floor=round(ms / floor, 2),
                              of_peak=round(ms / (nbytes / PEAK * 1e3), 2), gbps=round(nbytes / ms / 1e6, 1), reps=reps,
                              calls_per_window=calls, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cells", type=int, default=1440 * 720)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    a = ap.parse_args()
    dev = get_device()
    T, C = 365, a.cells
    time = TimeAxis.daily("1981-01-01", T)
    seg = time.segments("YS-JAN")[0]
    flags = rainseason.rain_flags(time, seg)                # the reference's default dates
    # a wet season from May to mid-October (six days in ten wet, 14 to 24 mm) and a dry rest of the year (one day in fifty wet),
    # so that most lanes find a start and an end; made on the host, the generator of the library has one wet-day rate per field
    rng = np.random.default_rng(81)
    t = np.arange(T)
    p_wet = np.where((t > 120) & (t < 290), 0.6, 0.02).astype(np.float32)[:, None]
    host = rng.random((T, C), dtype=np.float32)
    host = np.where(host < p_wet, (14.0 + 10.0 * host / p_wet) / 86400.0, 0.0).astype(np.float32)
    pr = dev.to_device(host)
    del host
    shape = dict(rows=T, cells=C)
    field = T * C * 4

    def rain(method):
        return lambda: K.rain_season(dev, pr, seg, flags, time.doy, per_day=86400.0, method_dry_start=method, method_dry_end=method)

    found = {m: {k: float(np.mean(~np.isnan(v.get()))) for k, v in rain(m)().items()} for m in K.RAIN_METHODS}
    timed(dev, [(f"rain_season_{m}", rain(m), field, dict(shape, found=found[m])) for m in K.RAIN_METHODS]
          + [("rain_season_per_day_start_only", lambda: K.rain_season(dev, pr, seg, flags, time.doy, per_day=86400.0, outputs=("start",)), field, shape)],
          a.reps, a.calls)
    del pr

    P = 30
    tn_min = K.fill_synthetic(dev, P, C, 0, 82, np.full(P, 262.0, np.float32), 25.0)
    edges = rainseason.zone_edges("usda", "K")
    timed(dev, [("rolling_zones_w30_usda", lambda: K.rolling_zones(dev, tn_min, 30, edges), P * C * 4, dict(rows=P, cells=C))], a.reps, a.calls)


if __name__ == "__main__":
    main()
