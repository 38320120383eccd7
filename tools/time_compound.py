"""Compound-extreme unit timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_compound.py [--reps 7] [--calls 5] [--shape year|years30|both] [--out profiles/r27/time_compound.jsonl]

Two shapes, float32 fields: 365 x 1440 x 720 (one "YS" period) and 30 years x 1440 x 90 (10 957 rows, thirty "YS" periods), with
the fields and the four (366, cells) float64 percentile tables on the device.

  * ``counts4.fused``: the four compound counts from ONE launch of ``xh_compound_doy_days``;
  * ``counts4.composed``: the same four results composed from entry points that existed before this unit, four times over:
    ``resample_doy`` of both tables (``xh_doy_broadcast``: two (T, cells) float64 threshold fields), two ``xh_compare_map_f64`` (float
    masks), and the conjunction with the period sum in ``xh_bivariate_count`` on the two masks — 20 launches;
  * ``count1.fused``: ``cold_and_dry_days`` alone (two tables);
  * ``dded``: ``xh_degree_exceedance_date``; ``dded.never``: the same with a sum that is never reached (every row is read);
  * ``snow.w3`` / ``snow.w32``: ``xh_blowing_snow_days`` with the window at 3 and at the limit;
  * ``wci``: ``xh_pair_period_sum``.

A timed window is ``--calls`` calls in a row between one pair of HIP events, and ``ms`` is the median over the reps of window /
calls (fields and tables already on the device; outputs allocated and host tables uploaded inside the window), after one untimed
warm-up window of every configuration; the configurations are timed in turn, rep by rep, in the same process (alternating runs).
``floor_bytes`` is the traffic a path cannot avoid: every field it reads once, plus, for the counts, the table rows it touches — one
table row of 8 bytes per cell for every field row on the one-year shape (each row of a table is used once), and each table once on
the thirty-year shape (the rows come back every year; what the caches return of them is the kernel's business).  ``floor_ms`` is
that over 6.1 TB/s, the bare streaming read rate DESIGN.md section 3 records; ``of_floor`` = ms / floor_ms.  ``bytes_moved`` of the
composed path counts what its launches read and write by their definition."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import compound  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import CD_OUTPUTS, get_device  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

READ_RATE = 6.1e12
OPS = {"cold_dry": ("<", "tas_lo", "<", "pr_lo"), "warm_dry": (">", "tas_hi", "<", "pr_lo"), "warm_wet": (">", "tas_hi", ">", "pr_hi"),
       "cold_wet": ("<", "tas_lo", ">", "pr_hi")}


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
    P = len(seg) - 1
    t = np.arange(T)
    season = np.cos(2 * np.pi * (t - 15) / 365.25)
    tas = K.fill_synthetic(dev, T, C, 0, 301, (283 - 9 * season).astype(np.float32), 6.0)
    pr = K.fill_synthetic(dev, T, C, 0, 302, np.full(T, 3e-5, np.float32), 3e-5)
    snd = K.fill_synthetic(dev, T, C, 0, 303, (0.6 + 0.5 * season).astype(np.float32), 0.5)
    wind = K.fill_synthetic(dev, T, C, 0, 304, np.full(T, 4.0, np.float32), 4.0)
    d = np.arange(366)
    dseason = np.cos(2 * np.pi * (d - 15) / 365.25)[:, None]
    cell = (np.arange(C) % 97 / 97.0)[None, :]
    tables = {}
    for k, tab in (("tas_lo", 280.0 - 9 * dseason + cell), ("tas_hi", 286.0 - 9 * dseason + cell), ("pr_lo", 1.5e-5 + 1e-6 * cell + 0 * dseason),
                   ("pr_hi", 4.5e-5 + 1e-6 * cell + 0 * dseason)):
        tables[k] = dev.to_device(np.ascontiguousarray(tab, dtype=np.float64))
        del tab
    tidx = (time.doy - 1).astype(np.int32)
    E = T * C * 4
    rows_touched = (T if P == 1 else 366) * C * 8       # per table: once per field row on one year, each row once on thirty
    shape = dict(shape=tag, rows=T, cells=C, periods=P)

    def fused(outputs):
        need = {n for o in outputs for n in K.CD_NEEDS[o]}
        return lambda: K.compound_doy_days(dev, tas, pr, {n: tables[n] for n in need}, tidx, seg, outputs)

    def composed():
        outs = []
        for o in CD_OUTPUTS:
            op_t, tab_t, op_p, tab_p = OPS[o]
            thr_t, thr_p = K.doy_broadcast(dev, tables[tab_t], tidx), K.doy_broadcast(dev, tables[tab_p], tidx)     # resample_doy
            m_t, m_p = K.compare_map(dev, tas, op_t, thr_t, "maskf"), K.compare_map(dev, pr, op_p, thr_p, "maskf")
            del thr_t, thr_p
            outs.append(K.bivariate_count(dev, m_t, m_p, ">", 0.5, ">", 0.5, "and", seg, want_valid=False)[0])  # the conjunction and the sum
        return outs

    start0, never = compound.exceedance_tables(time, seg, None, None)
    flags = None
    # composed traffic per index: two broadcasts write 8 B each, two compares read 4 + 8 B and write 4 B each, the count reads 4 + 4 B
    configs = [
        (f"{tag}.counts4.fused", fused(list(CD_OUTPUTS)), 2 * E + 4 * rows_touched, dict(shape, floor_bytes=2 * E + 4 * rows_touched, launches=1)),
        (f"{tag}.counts4.composed", composed, 4 * (2 * 2 * E + 2 * (E + 2 * E + E) + 2 * E), dict(shape, floor_bytes=2 * E + 4 * rows_touched, launches=20)),
        (f"{tag}.count1.fused", fused(["cold_dry"]), 2 * E + 2 * rows_touched, dict(shape, floor_bytes=2 * E + 2 * rows_touched, launches=1)),
        (f"{tag}.dded", lambda: K.degree_exceedance_date(dev, tas, seg, start0, never, time.doy, thresh=278.0, sum_thresh=1000.0), E,
         dict(shape, floor_bytes=E, note="the walk of a lane ends at its date")),
        (f"{tag}.dded.never", lambda: K.degree_exceedance_date(dev, tas, seg, start0, never, time.doy, thresh=278.0, sum_thresh=1e9), E,
         dict(shape, floor_bytes=E)),
        (f"{tag}.snow.w3", lambda: K.blowing_snow_days(dev, snd, wind, seg, flags, snd_thresh=0.3, wind_thresh=4.0, window=3), 2 * E,
         dict(shape, floor_bytes=2 * E)),
        (f"{tag}.snow.w32", lambda: K.blowing_snow_days(dev, snd, wind, seg, flags, snd_thresh=0.3, wind_thresh=4.0, window=32), 2 * E,
         dict(shape, floor_bytes=2 * E)),
        (f"{tag}.wci", lambda: K.pair_period_sum(dev, pr, pr, seg, 86400.0), 2 * E, dict(shape, floor_bytes=2 * E)),
    ]
    # the two paths agree before they are timed
    a = fused(list(CD_OUTPUTS))()
    b = composed()
    for o, v in zip(CD_OUTPUTS, b):
        got = a[o].get()
        assert np.array_equal(got, v.get().astype(np.float64)), o
        assert got.sum() > 0, o
    return configs, (tas, pr, snd, wind, tables)


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
        line = json.dumps(dict(config=f"{tag}.counts4.ratio",
                               composed_over_fused=round(rows[f"{tag}.counts4.composed"]["ms"] / rows[f"{tag}.counts4.fused"]["ms"], 2)))
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
        del configs, keep
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
