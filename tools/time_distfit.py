"""Distribution-fit timings on one MI355X: one JSON line per step (record only, no gate).

    python tools/time_distfit.py [--reps 3] [--out profiles/r22/time_distfit.jsonl] [--limit 300]

Every step runs in a child process of its own (``--step``) under its own time limit, one after the other, and the run stops at
the first step that fails or runs out of time.  The steps, each ONE launch of ``xh_dist_fit`` on 1440 x 720 cells of 30 and of
150 annual values (float32 on the device: 65 536 distinct cells of Gumbel-distributed maxima, loc 100, scale 20, repeated over
the grid): ``norm``, ``gumbel_r``, ``gamma`` with ``floc = 0``, ``genextreme`` by maximum likelihood, and ``genextreme`` with the
fused return levels for ``t = [2, 10, 100]``; then ``cpu``: the per-cell time of the reference's ``_fitfunc_1d`` (AST-extracted
from the reference tree where it exists, see tests/golden/make_distfit_golden.py; skipped elsewhere) on one core.

``ms`` is the median over ``--reps`` launches, each between one pair of HIP events (the outputs allocated inside the window),
after one untimed launch.  ``read_floor_ms``: the field read once over 6.1 TB/s, the streaming read rate DESIGN.md section 3
records.  ``nfev_mean`` / ``at_budget``: the objective evaluations of the Nelder-Mead fits and the share that stops at 600."""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_RATE = 6.1e12
C = 1440 * 720
DISTINCT = 65536
FORMS = {"norm": ("norm", None, None), "gumbel_r": ("gumbel_r", None, None), "gamma_floc": ("gamma", 0.0, None),
         "genextreme": ("genextreme", None, None), "genextreme_levels": ("genextreme", None, [2, 10, 100])}
LENGTHS = (30, 150)


def maxima(T, cells, seed=22):
    rng = np.random.default_rng(seed)
    return (100.0 + 20.0 * rng.gumbel(size=(T, cells))).astype(np.float32)


def gpu_step(form, T, reps):
    from xclim_amd import kernels as K
    from xclim_amd import stats as S
    from xclim_amd._capi import get_device

    dev = get_device()
    dist, floc, t = FORMS[form]
    T = int(T)
    x = dev.to_device(np.tile(maxima(T, DISTINCT), (1, C // DISTINCT + 1))[:, :C])
    q = qfunc = None
    if t is not None:
        qfunc, q = S.quantile_route(1 - 1.0 / np.asarray(t, float))
    times = []
    for r in range(reps + 1):
        dev.timer_start()
        params, nfev, status, levels = K.dist_fit(dev, x, dist, "ML", floc, q=q, qfunc=qfunc or "ppf")
        ms = dev.timer_stop()
        if r:
            times.append(ms)
    nf, st = nfev.get(), status.get()
    ms = float(np.median(times))
    read = T * C * 4 / READ_RATE * 1e3
    row = dict(step=f"{form}.{T}", dist=dist, T=T, cells=C, floc=floc, levels=t, ms=round(ms, 3), min_ms=round(min(times), 3),
               max_ms=round(max(times), 3), ns_per_cell=round(ms * 1e6 / C, 2), read_floor_ms=round(read, 4), of_read=round(ms / read, 1),
               fitted=int((st == 0).sum()), at_budget=int((st == 2).sum()), nan=int((st == 1).sum()), reps=reps)
    if nf.any():
        row.update(nfev_mean=round(float(nf.mean()), 1), nfev_max=int(nf.max()))
    if levels is not None:
        row["levels_finite"] = int(np.isfinite(levels.get()).sum())
    return row


def cpu_step(cells=24):
    gen = os.path.join(ROOT, "tests", "golden")
    sys.path.insert(0, gen)
    import make_distfit_golden as G

    if not os.path.exists(G.REF):
        return dict(step="cpu", skipped="no reference tree")
    import scipy.stats

    ns = G.extract()
    row = dict(step="cpu", cells=cells)
    for T in LENGTHS:
        x = maxima(T, cells).astype(np.float64)
        for dist in ("norm", "gumbel_r", "genextreme"):
            t0 = time.perf_counter()
            for c in range(cells):
                ns["_fitfunc_1d"](x[:, c], dist=getattr(scipy.stats, dist), nparams=2 if dist != "genextreme" else 3, method="ML")
            row[f"{dist}_{T}_ms_per_cell"] = round((time.perf_counter() - t0) / cells * 1e3, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300, help="seconds a step may take")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process: <form>.<T> or cpu")
    a = ap.parse_args()
    if a.step:
        row = cpu_step() if a.step == "cpu" else gpu_step(*a.step.split("."), a.reps)
        print(json.dumps(row), flush=True)
        return 0
    steps = [f"{f}.{T}" for T in LENGTHS for f in FORMS] + ["cpu"]
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
