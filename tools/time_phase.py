"""Snow / rain partition timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_phase.py [--reps 7] [--calls 5] [--shape year|years30|both] [--out profiles/r20/time_phase.jsonl]

Two shapes, float32 fields in mm/d and K: 365 x 1440 x 720 (one "YS" period) and 30 years x 1440 x 90 (10 957 rows, thirty "YS"
periods).  On each, two results are timed on the FUSED path (one launch of ``xh_precip_phase_period``) and on the path COMPOSED
from ``xh_precip_phase_map`` and the entry points that existed before (``xh_resample_reduce``, ``xh_domain_count``,
``xh_threshold_count``, ``xh_bivariate_count``), which writes the snow and rain fields and reads them again once per index:

  * ``totals``: the solid, liquid and total sums (what ``liquid_precip_ratio`` and the two phase totals need), method "binary";
  * ``all``: all fourteen outputs fused; composed, the ten that have an older entry point (the three sums, the four counts, the
    snow days, the days over the snow threshold, high precipitation at low temperature) — the sum over the threshold, the two
    dates and rain on frozen ground have none, so the composed time is a lower bound of what all fourteen would take.
  * ``totals_<method>``: the fused totals with each of the other methods (record only).

A timed window is ``--calls`` calls in a row between one pair of HIP events, and ``ms`` is the median over the reps of window /
calls (fields already on the device; outputs allocated and host tables uploaded inside the window), after one untimed warm-up
window of every configuration; the configurations are timed in turn, rep by rep, in the same process.  ``bytes_moved`` is the
traffic the path needs by its definition: 2 field reads for the fused path; 2 reads + 1 write per field the map stores + 1 read
per index for the composed one.  ``floor_ms`` is the two field reads over 6.1 TB/s, the bare streaming read rate DESIGN.md §3
records; ``of_floor`` = ms / floor_ms."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import phase  # noqa: E402
from xclim_amd._capi import PHASE_OUTPUTS, get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

READ_RATE = 6.1e12
TOTALS = ("pr_sum", "solid_sum", "liquid_sum")


def timed(dev, configs, reps, calls, sink):
    times = {name: [] for name, *_ in configs}
    for r in range(reps + 1):
        for name, launch, _, _ in configs:
            dev.timer_start()
            for _ in range(calls):
                outs = launch()
            ms = dev.timer_stop() / calls
            if r:
                times[name].append(ms)
            del outs
    rows = {}
    for name, _, nbytes, extra in configs:
        ms = float(np.median(times[name]))
        floor = extra.pop("floor_bytes") / READ_RATE * 1e3
        rows[name] = dict(config=name, ms=round(ms, 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                          bytes_moved=int(nbytes), gbps=round(nbytes / ms / 1e6, 1), floor_ms=round(floor, 3), of_floor=round(ms / floor, 2),
                          reps=reps, calls_per_window=calls, **extra)
        line = json.dumps(rows[name])
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    return rows


def shape_configs(dev, tag, T, C, start):
    time = TimeAxis.daily(start, T)
    seg = time.segments("YS")[0]
    t = np.arange(T)
    pr = K.fill_synthetic(dev, T, C, 0, 201, (2.5 + 1.0 * np.cos(2 * np.pi * t / 365.25)).astype(np.float32), 2.4)   # mm/d, 0.1 .. 5.9
    tas = K.fill_synthetic(dev, T, C, 0, 202, (275 - 12 * np.cos(2 * np.pi * (t - 15) / 365.25)).astype(np.float32), 6.0)
    E = T * C * 4
    shape = dict(shape=tag, rows=T, cells=C, periods=len(seg) - 1, floor_bytes=2 * E)
    lim = dict(snow_low=1.0, snow_thresh=1.0, hplt_pr=0.4, hplt_tas=272.95, rofg_pr=1.0, rofg_frz=273.15)
    parts = {m: phase.partition(m, units="K", dtype=np.float32, time=time, device=dev) for m in phase.METHODS}

    def fused(method, outputs):
        return lambda: K.precip_phase_period(dev, pr, tas, seg, parts[method], outputs, per_day=1.0, doy=time.doy, **lim)

    def composed_totals():
        f = K.precip_phase_map(dev, pr, tas, parts["binary"])
        return [K.resample_reduce(dev, x, "sum", seg, want_valid=False)[0] for x in (pr, f["snow"], f["rain"])]

    def composed_all():
        f = K.precip_phase_map(dev, pr, tas, parts["binary"])
        outs = [K.resample_reduce(dev, x, "sum", seg, want_valid=False)[0] for x in (pr, f["snow"], f["rain"])]
        outs += [K.resample_reduce(dev, x, "count", seg, want_valid=False)[0] for x in (pr, f["snow"], f["rain"], tas)]
        outs.append(K.domain_count(dev, f["snow"], ">", 1.0, "<=", phase.SNOW_HIGH, "and", seg, want_valid=False)[0])
        outs.append(K.threshold_count(dev, f["snow"], ">=", seg, scalar=1.0, want_valid=False)[0])
        outs.append(K.bivariate_count(dev, pr, tas, ">=", 0.4, "<", 272.95, "and", seg, want_valid=False)[0])
        return outs

    # composed traffic: the map reads 2 fields and writes 2; every index reads its field once (hplt reads two)
    configs = [(f"{tag}.totals.fused", fused("binary", TOTALS), 2 * E, dict(shape)),
               (f"{tag}.totals.composed", composed_totals, (2 + 2 + 3) * E, dict(shape, launches=4)),
               (f"{tag}.all.fused", fused("binary", PHASE_OUTPUTS), 2 * E, dict(shape, outputs=14)),
               (f"{tag}.all.composed_10_of_14", composed_all, (2 + 2 + 3 + 4 + 2 + 2) * E, dict(shape, launches=11, outputs=10))]
    configs += [(f"{tag}.totals_{m}.fused", fused(m, TOTALS), 2 * E, dict(shape)) for m in phase.METHODS if m != "binary"]
    # the two paths agree before they are timed
    a = {k: v.get() for k, v in fused("binary", TOTALS)().items()}
    b = [v.get() for v in composed_totals()]
    for k, v in zip(TOTALS, b):
        assert np.allclose(a[k], v, rtol=1e-4), k
    return configs, (pr, tas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--shape", default="both", choices=("year", "years30", "both"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = get_device()
    sink = open(a.out, "a") if a.out else None
    shapes = {"year": ("year_1440x720", 365, 1440 * 720, "1981-01-01"), "years30": ("years30_1440x90", 10957, 1440 * 90, "1981-01-01")}
    for key in (("year", "years30") if a.shape == "both" else (a.shape,)):
        configs, keep = shape_configs(dev, *shapes[key])
        rows = timed(dev, configs, a.reps, a.calls, sink)
        tag = shapes[key][0]
        for what in ("totals", "all"):
            f = rows[f"{tag}.{what}.fused"]["ms"]
            c = rows[[n for n in rows if n.startswith(f"{tag}.{what}.composed")][0]]["ms"]
            line = json.dumps(dict(config=f"{tag}.{what}.ratio", composed_over_fused=round(c / f, 2)))
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
        del configs, keep
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
