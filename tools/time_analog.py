"""Spatial-analogue timings on one MI355X: one JSON line per step (record only, no gate).

    python tools/time_analog.py [--reps 5] [--out profiles/r21/time_analog.jsonl] [--limit 240]

Every step runs in a child process of its own (``--step``) under its own time limit, one after the other, and the run stops at
the first step that fails or runs out of time.  The steps: for each of the eight metrics, one launch of ``xh_analog`` on 30
samples x 4 indices x 1440 x 720 cells and the same on 1440 x 90 (float32 candidate fields already on the device, 0.3 plus the
synthetic generator's noise of amplitude 1.2; a normal target of 30 points; kldiv with k = 1); then ``cpu``: the per-cell time of the
restatement of tests/analogcpu.py (the reference's own scipy calls, one Python call per cell) on a 4 096-cell sample.

``ms`` is the median over ``--reps`` launches, each between one pair of HIP events (the output allocated and the target table
uploaded inside the window), after one untimed launch.  Next to it, the two bounds of the method:

  * ``read_floor_ms``: the four candidate fields read ONCE (4 x 30 x C x 4 bytes) over 6.1 TB/s, the streaming read rate DESIGN.md
    section 3 records;
  * ``fp64_floor_ms``: the float64 operations the method needs by its definition (``OPS``, below: an add, multiply, divide,
    compare, square root or logarithm counted as ONE operation each, so the bound is generous to the divisions and the
    transcendental functions) over the vector FP64 rate.  The micro-architecture notes this project works from list the FP32
    vector peak, 157.3 TFLOP/s = 2 x 78.6 T fused operations per second, and no FP64 figure; AMD's public data sheet of the
    part gives 78.6 TFLOP/s for vector FP64, half the FP32 rate, i.e. 39.3 T operations per second without contraction (the
    library is built with -ffp-contract=off, so an FMA's two operations issue as two instructions).

``of_read`` and ``of_fp64`` are ms over each; ``bound`` names the larger floor."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_RATE = 6.1e12
FP64_OPS = 39.3e12
N, M, D = 30, 30, 4
SHAPES = {"1440x90": 1440 * 90, "1440x720": 1440 * 720}   # the small one first
METHODS = ("seuclidean", "mahalanobis", "zech_aslan", "szekely_rizzo", "nearest_neighbor", "friedman_rafsky", "kolmogorov_smirnov", "kldiv")


def ops(method, n=N, m=M, d=D):
    """Float64 operations per cell by the method's definition (include/ext/xclim_hip_analog.h)."""
    tot = n + m
    pairs = n * (n - 1) // 2 + m * (m - 1) // 2 + n * m
    stats = 3 * m * d + 3 * d   # the means, the squared deviations, the divisions and roots
    return {"seuclidean": m * d + 4 * d, "mahalanobis": m * d + 2 * d * d + 2 * d,
            "zech_aslan": stats + pairs * (4 * d + 3), "szekely_rizzo": stats + pairs * (4 * d + 2),
            "nearest_neighbor": stats + tot * (tot - 1) * (4 * d + 1),
            "friedman_rafsky": (tot * (tot - 1) // 2) * (3 * d + 2),
            "kolmogorov_smirnov": tot * tot * d + tot * (2 ** d) * 3,
            "kldiv": n * m * (3 * d + 1) + 3 * n}[method]


def gpu_step(method, shape, reps):
    from xclim_amd import kernels as K
    from xclim_amd._capi import get_device

    dev = get_device()
    C = SHAPES[shape]
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (N, D))
    fields = [K.fill_synthetic(dev, M, C, 0, 300 + j, np.full(M, 0.3, np.float32), 1.2) for j in range(D)]
    par = {"zech_aslan": [1e-12], "szekely_rizzo": [1.0], "mahalanobis": np.linalg.inv(np.cov(x, rowvar=False))}.get(method)
    k = [1] if method == "kldiv" else None
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        out = K.analog(dev, method, x, fields, par=par, k=k)
        ms = dev.timer_stop()
        if r:
            times.append(ms)
    res = out.get()
    ms = float(np.median(times))
    read = D * M * C * 4 / READ_RATE * 1e3
    fp = ops(method) * C / FP64_OPS * 1e3
    return dict(step=f"{method}.{shape}", method=method, shape=shape, cells=C, n=N, m=M, d=D, ms=round(ms, 3), min_ms=round(min(times), 3),
                max_ms=round(max(times), 3), ns_per_cell=round(ms * 1e6 / C, 2), read_floor_ms=round(read, 4), ops_per_cell=ops(method),
                fp64_floor_ms=round(fp, 4), of_read=round(ms / read, 1), of_fp64=round(ms / fp, 1), bound="fp64" if fp > read else "read",
                finite=int(np.isfinite(res).sum()), reps=reps)


def cpu_step(cells=4096):
    import analogcpu as R

    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (N, D))
    y = rng.normal(0.3, 1.2, (D, M, cells)).astype(np.float32).astype(np.float64)
    row = dict(step="cpu", cells=cells, n=N, m=M, d=D)
    for method in METHODS:
        t0 = time.perf_counter()
        R.cells(method, x, y)
        row[f"{method}_us_per_cell"] = round((time.perf_counter() - t0) / cells * 1e6, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process: <method>.<shape> or cpu")
    a = ap.parse_args()
    if a.step:
        row = cpu_step() if a.step == "cpu" else gpu_step(*a.step.split("."), a.reps)
        print(json.dumps(row), flush=True)
        return 0
    steps = [f"{m}.{s}" for s in SHAPES for m in METHODS] + ["cpu"]
    sink = open(a.out, "a") if a.out else None
    for step in steps:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)], capture_output=True,
                                 text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {a.limit} s; stopping", file=sys.stderr)
            return 124
        if res.returncode != 0:
            print(f"{step}: exit status {res.returncode}; stopping\n{res.stderr[-2000:]}", file=sys.stderr)
            return res.returncode
        line = res.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if sink:
        sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
