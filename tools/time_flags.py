"""Data-quality-flag timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_flags.py [--reps 5] [--calls 5] [--shapes year,30y] [--dtypes float32,float64]

``data_flags`` for ``tas`` with its six default checks (extremely high / low, above ``tasmax``, below ``tasmin``, values repeating
for 5 days, outside 5 deviations of the climatology over a window of 5) and ``dims="all"``, on 365 x 1440 x 720 ("year") and on
30 years x 1440 x 90 ("30y"), three fields of one dtype already on the device.  Two routes are timed in the same run:

(a) ``fused``: one ``xh_doy_bounds`` + one ``xh_data_flags`` with ``reduce_cells`` (what ``xclim_amd.dataflags.data_flags`` launches);
    ``fused_checks`` is the ``xh_data_flags`` launch alone, on tables made before the window.
(b) ``composed``: the same flags from the entry points that existed before this unit, float32 only: four ``xh_compare_map`` (the
    1 / 0 float mask), ``xh_suspicious_run`` and ``xh_doy_mean_std`` + ``xh_within_bnds_doy`` (uint8 masks, made float with
    ``xh_mask_u8_to_f32``), each followed by its ``any`` as ``xh_resample_reduce`` (max) over one period.  The float64 bound tables
    ``mean -+ 5 std`` that ``xh_within_bnds_doy`` takes have no device form there: they are made before the window, in favour of (b).

A timed window is ``--calls`` calls in a row between one pair of HIP events, and ``ms`` is the median over the reps of window /
calls, after one untimed warm-up window of every configuration; the configurations are timed in turn, rep by rep, in the same
process.  ``bytes_read`` of (a) is its read floor: the three fields read once plus the window pass of ``xh_doy_bounds`` counted as
one more read of the field; ``table_bytes`` are the two bound tables, written once and read once per row on top of that (as
large as the field itself when the series is one year long).  ``floor_ms`` is ``bytes_read`` over 6.1 TB/s, the read rate
DESIGN.md section 3 records for this part; ``of_floor`` = ms / floor_ms.  ``flags`` are the six answers (the fields are clean
except for the values planted in the last cell, so that every check has something to find)."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import _vp, get_device, np_ptr  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

READ_RATE = 6.1e12
SHAPES = {"year": (365, 1440 * 720, "1981-01-01"), "30y": (10957, 1440 * 90, "1981-01-01")}
HIGH, LOW = 60 + 273.15, -90 + 273.15


def timed(dev, configs, reps, calls):
    """configs: [(name, launch, bytes, extra)].  One warm-up window each, then ``reps`` rounds that run every configuration once."""
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
    out = {}
    for name, _, nbytes, extra in configs:
        ms = float(np.median(times[name]))
        floor = nbytes / READ_RATE * 1e3
        out[name] = ms
        print(json.dumps(dict(config=name, ms=round(ms, 3), min_ms=round(min(times[name]), 3), max_ms=round(max(times[name]), 3),
                              bytes_read=int(nbytes), floor_ms=round(floor, 3), of_floor=round(ms / floor, 2), gbps=round(nbytes / ms / 1e6, 1),
                              reps=reps, calls_per_window=calls, **extra)), flush=True)
    return out


def fields(dev, T, C, start, dtype):
    """tas, tasmax, tasmin (T, C) on the device: a seasonal cycle + noise of +-3 K, the companions 10 K above and below; in the
    last cell one value of each kind the checks look for."""
    time = TimeAxis.daily(start, T)
    base = (283.0 + 10.0 * np.sin(2 * np.pi * (time.doy - 110) / 365.25)).astype(np.float32)
    out = []
    for seed, off in ((91, 0.0), (92, 10.0), (93, -10.0)):
        d = K.fill_synthetic(dev, T, C, 0, seed, base + np.float32(off), 3.0)
        if off == 0.0:
            for row, value in [(5, 340.0), (T // 2, 150.0)] + [(r, 285.0) for r in range(100, 106)]:
                v = np.array([value], np.float32)
                dev.call("xh_memcpy_h2d", _vp(d.ptr + (row * C + C - 1) * 4), np_ptr(v), 4)
            dev.sync()
        if dtype == np.float64:
            wide = dev.to_device(d.get().astype(np.float64))
            d.free()
            d = wide
        out.append(d)
    return time, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--shapes", default="year,30y")
    ap.add_argument("--dtypes", default="float32,float64")
    ap.add_argument("--cells", type=int, default=0, help="override the number of cells (for a quick run)")
    a = ap.parse_args()
    dev = get_device()
    checks = [K.flag_check("cmp", ">", HIGH), K.flag_check("cmp", "<", LOW), K.flag_check("pair", ">", other=0), K.flag_check("pair", "<", other=1),
              K.flag_check("repeat", None, n=5), K.flag_check("clim")]
    for shape in a.shapes.split(","):
        T, C, start = SHAPES[shape]
        C = a.cells or C
        for dname in a.dtypes.split(","):
            dtype = np.dtype(dname).type
            esz = np.dtype(dtype).itemsize
            time, (tas, tasmax, tasmin) = fields(dev, T, C, start, dtype)
            tb, _, doys = time.doy_table()
            tidx = np.searchsorted(doys, time.doy).astype(np.int32)
            seg = np.array([0, T], np.int64)
            D = len(doys)
            info = dict(shape=shape, rows=T, cells=C, dtype=dname, table_bytes=2 * D * C * esz)
            lo, hi = K.doy_bounds(dev, tas, tb, 5, 5.0)

            def checks_only():
                return K.data_flags(dev, tas, checks, seg, y0=tasmax, y1=tasmin, tidx=tidx, lo=lo, hi=hi, reduce_cells=True)

            def fused():
                b = K.doy_bounds(dev, tas, tb, 5, 5.0)
                return K.data_flags(dev, tas, checks, seg, y0=tasmax, y1=tasmin, tidx=tidx, lo=b[0], hi=b[1], reduce_cells=True)

            flags = [int(v) for v in fused().get()[:, 0]]
            field = T * C * esz
            configs = [(f"fused_{shape}_{dname}", fused, 4 * field, dict(info, flags=flags)),
                       (f"fused_checks_{shape}_{dname}", checks_only, 3 * field, info)]
            if dtype == np.float32:
                lo64, hi64 = dev.to_device(lo.get().astype(np.float64)), dev.to_device(hi.get().astype(np.float64))

                def any_of(mask_f32, reducer="max"):
                    return K.resample_reduce(dev, mask_f32, reducer, seg, want_valid=False)[0]

                def composed():
                    outs = [any_of(K.compare_map(dev, tas, ">", np.float64(HIGH), "maskf")), any_of(K.compare_map(dev, tas, "<", np.float64(LOW), "maskf")),
                            any_of(K.compare_map(dev, tas, ">", tasmax, "maskf")), any_of(K.compare_map(dev, tas, "<", tasmin, "maskf")),
                            any_of(K.mask_to_f32(dev, K.suspicious_run(dev, tas, 5)))]
                    K.doy_mean_std(dev, tas, tb, 5)
                    outs.append(any_of(K.mask_to_f32(dev, K.within_bnds_doy(dev, tas, lo64, hi64, tidx)), "min"))   # any outside = not all within
                    return outs

                got = [o.get() for o in composed()]
                info_b = dict(info, flags=[int(np.nanmax(g)) for g in got[:5]] + [int(1 - np.nanmin(got[5]))])
                configs.append((f"composed_{shape}_{dname}", composed, 4 * field, info_b))
            ms = timed(dev, configs, a.reps, a.calls)
            if dtype == np.float32:
                print(json.dumps(dict(config=f"ratio_{shape}_{dname}", composed_over_fused=round(ms[f"composed_{shape}_{dname}"] / ms[f"fused_{shape}_{dname}"], 2))),
                      flush=True)
            for d in (tas, tasmax, tasmin, lo, hi):
                d.free()
            if dtype == np.float32:
                lo64.free(), hi64.free()
            dev.trim()


if __name__ == "__main__":
    main()
