"""Grid-reduction unit timings on one MI355X: one JSON line per configuration (record only, no gate).

    python tools/time_grid.py [--reps 7] [--calls 5] [--what dot|jet|both] [--out profiles/r28/time_grid.jsonl]

The masked dot, float32 fields on the device, weights (float64) on the device: 365 x 1440 x 1080 (a daily year of a quarter-degree
ocean grid) and 360 rows of the same grid (30 years of monthly means) —

  * ``dot.area`` / ``dot.extent``: one output of ``xh_grid_masked_dot``; ``dot.both``: both from one launch;
  * ``dot.host``: the numpy restatement of both sums (the reference's expression in float64) on ``--host-rows`` rows of the same
    field, scaled to all rows (``host_ms`` is the measured time, ``ms`` the scaled one).

The jet, float32: 365 x 3 levels x 721 x 1440 in the layouts (Z, Y, X) and (Z, X, Y), the box of the index (241 latitudes, 241
longitudes, 3 levels) — ``jet.<layout>.box_mean`` (``xh_grid_box_mean``) and ``jet.filter`` (``xh_grid_filter_argmax``, 61 weights)
separately.

A timed window is ``--calls`` calls in a row between one pair of HIP events, and ``ms`` is the median over the reps of window /
calls (fields already on the device; outputs allocated and host tables uploaded inside the window), after one untimed warm-up window
of every configuration; the configurations are timed in turn, rep by rep, in the same process (alternating runs).  ``floor_bytes``
is the traffic a path cannot avoid: the field read once (for the box mean: the selected samples once; for the filter: the zonal means
once and the outputs once).  ``floor_ms`` is that over 6.73 TB/s, the streaming read rate profiles/r27/time_compound.jsonl records
for ``xh_compound_doy_days`` (``year_1440x720.count1.fused``) — not a rate taken from the kernels timed here; ``of_floor`` = ms /
floor_ms."""

import argparse
import json
import os
import sys
import time as _time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xclim_amd import grid  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402

READ_RATE = 6.7334e12


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
    for name, _, nbytes, extra in configs:
        ms = float(np.median(times[name]))
        floor = extra.pop("floor_bytes") / READ_RATE * 1e3
        emit(sink, dict(config=name, ms=round(ms, 4), min_ms=round(min(times[name]), 4), max_ms=round(max(times[name]), 4), bytes_moved=int(nbytes),
                        gbps=round(nbytes / ms / 1e6, 1), floor_ms=round(floor, 4), of_floor=round(ms / floor, 2), reps=reps, calls_per_window=calls,
                        **extra))


def emit(sink, row):
    line = json.dumps(row)
    print(line, flush=True)
    if sink:
        sink.write(line + "\n")
        sink.flush()


def dot_configs(dev, tag, T, C, host_rows, sink):
    x = K.fill_synthetic(dev, T, C, 0, 2801, np.full(T, 45.0, np.float32), 60.0)      # concentrations around the threshold and above
    w = dev.to_device(np.random.default_rng(28).uniform(1e8, 7e8, C))
    E = T * C * 4 + C * 8
    shape = dict(shape=tag, rows=T, cells=C)
    configs = [(f"{tag}.dot.{n}", (lambda o: lambda: K.grid_masked_dot(dev, x, w, 15.0, o))(o), E, dict(shape, floor_bytes=E, launches=1))
               for n, o in (("area", ("dot",)), ("extent", ("msum",)), ("both", ("dot", "msum")))]
    # the launch agrees with the restatement on the first rows before it is timed; the restatement is timed on the way
    rows = min(host_rows, T)
    xh = dev.wrap(x.ptr, (rows, C), np.float32).get()
    wh = w.get()
    t0 = _time.perf_counter()
    with np.errstate(invalid="ignore"):
        x64 = xh.astype(np.float64)
        inside = x64 >= np.float64(np.float32(15.0))
        dot, msum = (np.where(inside, x64, 0.0) * wh).sum(1), (np.where(inside, 1.0, 0.0) * wh).sum(1)
    host_ms = (_time.perf_counter() - t0) * 1e3
    got = K.grid_masked_dot(dev, x, w, 15.0)
    for name, want in (("dot", dot), ("msum", msum)):
        g = got[name].get()[:rows]
        assert np.all(np.abs(g - want) <= 1e-12 * np.abs(want)) and want.min() > 0, name
    emit(sink, dict(config=f"{tag}.dot.host", ms=round(host_ms * T / rows, 1), host_ms=round(host_ms, 1), host_rows=rows, **shape,
                    note="numpy, float64 on the widened rows, both sums; scaled from host_rows to all rows"))
    return configs, (x, w)


def jet_configs(dev, T=365, Z=3, Y=721, X=1440):
    lat, lon = np.linspace(-90.0, 90.0, Y), np.arange(X) * 0.25
    iz, iy, ix = grid.jet_box(lat, lon, np.array([92500.0, 85000.0, 77500.0]), 75000.0, 95000.0)
    ld = Z * Y * X
    u = K.fill_synthetic(dev, T, ld, 0, 2802, np.full(T, 8.0, np.float32), 12.0)
    sel = T * len(iz) * len(iy) * len(ix) * 4
    shape = dict(rows=T, levels=Z, lats=Y, lons=X, box=[len(iz), len(iy), len(ix)])
    dz, dy, dx = (dev.to_device(np.asarray(i, np.int32)) for i in (iz, iy, ix))
    strides = {"zyx": (Y * X, X, 1), "zxy": (Y * X, 1, Y)}
    configs = [(f"jet.{lay}.box_mean", (lambda s: lambda: K.grid_box_mean(dev, u, T, ld, (Z, Y, X), s, dz, dy, dx))(s), sel + T * len(iy) * 8,
                dict(shape, layout=lay, floor_bytes=sel + T * len(iy) * 8, launches=1, field_bytes=T * ld * 4)) for lay, s in strides.items()]
    zm = K.grid_box_mean(dev, u, T, ld, (Z, Y, X), strides["zyx"], dz, dy, dx)
    wts = grid.lanczos_weights()
    fb = T * len(iy) * 8 + T * 12
    configs.append(("jet.filter", lambda: K.grid_filter_argmax(dev, zm, wts, ("smax", "jmax")), fb, dict(shape, floor_bytes=fb, launches=1)))
    out = K.grid_filter_argmax(dev, zm, wts, ("smax", "jmax"))
    assert (out["jmax"].get() >= 0).sum() == T - 60 and np.isfinite(zm.get()).all()
    return configs, (u, zm, dz, dy, dx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--what", default="both", choices=("dot", "jet", "both"))
    ap.add_argument("--host-rows", type=int, default=8, help="rows of the field the numpy restatement is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = get_device()
    sink = open(a.out, "a") if a.out else None
    if a.what in ("dot", "both"):
        for tag, T in (("daily_1440x1080", 365), ("monthly_1440x1080", 360)):
            configs, keep = dot_configs(dev, tag, T, 1440 * 1080, a.host_rows, sink)
            timed(dev, configs, a.reps, a.calls, sink)
            del configs, keep
    if a.what in ("jet", "both"):
        configs, keep = jet_configs(dev)
        timed(dev, configs, a.reps, a.calls, sink)
        del configs, keep
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
