"""Agroclimatic heat-sum timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/bench_agro.py [--reps 5] [--cells 1036800]

Every ``ms`` is the median of HIP-event times of ONE launch (float32 fields and the outputs already on the device; the host
tables go up inside the timed region), after one untimed warm-up launch.  ``bytes_read`` is what the launch must read once:
for the heat sums three fields over the selected span only (214 of 365 rows for 04-01 .. 11-01), for the monthly entry point
tas, pr and evspsblpot over the year and one month of tasmin, for xh_egdd its two fields once (the second walk of a period and the Qian stencil's neighbours
are re-read traffic and not in the floor).  ``floor_ms`` is that over 8 TB/s, the HBM3E peak of the part; ``of_floor`` =
ms / floor_ms.  tools/bench_bioclim.py, the yardstick of this lane pattern, divides by the 6.1 TB/s it measured: compare
``gbps``, which both can be brought to, when the two are put side by side."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import agro  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402
from xclim_amd.calendar import select_time_mask  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

PEAK = 8.0e12


def fields(dev, T, C):
    t = np.arange(T)
    season = (10 * np.sin(2 * np.pi * (t - 100) / 365.0)).astype(np.float32)
    return dict(tas=K.fill_synthetic(dev, T, C, 0, 91, 283 + season, 3.0), tasmin=K.fill_synthetic(dev, T, C, 0, 92, 278 + season, 3.0),
                tasmax=K.fill_synthetic(dev, T, C, 0, 93, 289 + season, 3.0),
                pr=K.fill_synthetic(dev, T, C, 0, 94, (3e-5 + 1e-5 * np.cos(2 * np.pi * t / 365.0)).astype(np.float32), 2e-5),
                evspsblpot=K.fill_synthetic(dev, T, C, 0, 95, (3e-5 + 2e-5 * np.sin(2 * np.pi * (t - 100) / 365.0)).astype(np.float32), 5e-6))


def timed(dev, name, launch, nbytes, reps, **extra):
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        outs = launch()
        ms = dev.timer_stop()
        if r:
            times.append(ms)
        del outs
    ms = float(np.median(times))
    floor = nbytes / PEAK * 1e3
    print(json.dumps(dict(config=name, ms=round(ms, 3), bytes_read=int(nbytes), floor_ms=round(floor, 3), of_floor=round(ms / floor, 2),
                          gbps=round(nbytes / ms / 1e6, 1), reps=reps, **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=1440 * 720)
    a = ap.parse_args()
    dev = get_device()
    T, C = 365, a.cells
    time = TimeAxis.daily("1981-01-01", T)
    f = fields(dev, T, C)
    seg = time.segments("YS")[0]
    sel = select_time_mask(time, date_bounds=("04-01", "11-01"), include_bounds=(True, False))
    lat = np.linspace(-60, 60, C)
    k_cell = dev.to_device(agro.huglin_day_length_latitude_coefficient(lat, "interpolated", 1.0))
    d_lat = dev.to_device(lat)
    shape = dict(rows=T, cells=C)
    timed(dev, "hi+bedd_04-01..11-01", lambda: K.agro_degree_sum(dev, f, seg, sel, k_cell=k_cell, outputs=("hi", "bedd")),
          3 * int(sel.sum()) * C * 4, a.reps, rows_read=int(sel.sum()), **shape)
    tabs = agro.month_tables(time, "YS")
    timed(dev, "monthly_cni+mtwm+di", lambda: K.agro_monthly(dev, f, *tabs, lat=d_lat, outputs=("cni", "mtwm", "di")), (31 + 3 * T) * C * 4, a.reps,
          **shape)
    etabs = agro.egdd_tables(time, "YS")
    for method in ("bootsma", "qian"):
        timed(dev, f"egdd_{method}", lambda m=method: K.egdd(dev, f["tasmin"], f["tasmax"], *etabs, method=m), 2 * T * C * 4, a.reps, **shape)


if __name__ == "__main__":
    main()
