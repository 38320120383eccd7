"""Time the humidity, heat-stress and wind unit with HIP events (the context's timer around the launches of one case, after two
warm-up calls; the median of the repetitions and their spread) and write one JSON line per case to time_humidity.jsonl in the next
free profiles/rNN (or ``--out``).

    python tools/time_humidity.py [--cells 1036800] [--rows 365] [--reps 7] [--out DIR] [--first]

Cases, float32 fields of 365 x 1440 x 720, fields and outputs on the device before the timer starts (the window holds the kernels
and nothing else): each single output of xh_air_moisture from just the fields it needs, the fused launch (tas, tdps, ps) -> (hurs,
huss, humidex, heat_index), and uas_vas_to_sfcwind, each against its read-plus-write floor at 8 TB/s.  Two comparisons in the same
session: relative_humidity(tas, tdps) as ONE launch against the two xh_esat launches that served it before this unit (which still
leave the division to the host), and the fused launch against the sum of its four single-output launches.  ``--first`` runs the fused
launch once and nothing else (for a counter run of its own)."""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xclim_amd import kernels as K  # noqa: E402
from xclim_amd._capi import get_device  # noqa: E402

NEEDS = {"esat": ("tas",), "vp": ("huss", "ps"), "vpd": ("tas", "hurs"), "hurs": ("tas", "tdps"), "huss": ("tas", "hurs", "ps"),
         "huss_dew": ("tdps", "ps"), "tdps": ("huss", "ps"), "humidex": ("tas", "tdps"), "heat_index": ("tas", "hurs")}
FUSED = ("hurs", "huss", "humidex", "heat_index")


def next_free_profile_dir():
    taken = [int(m.group(1)) for m in (re.search(r"r(\d+)$", p) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(taken, default=0) + 1:02d}")


def host_field(name, R, C, rng):
    u = rng.random((R, C), dtype=np.float32)
    return {"tas": lambda: 250 + 60 * u, "tdps": lambda: 245 + 55 * u, "hurs": lambda: 5 + 90 * u, "huss": lambda: 1e-4 + 0.02 * u,
            "ps": lambda: 60000 + 45000 * u, "uas": lambda: -15 + 30 * u, "vas": lambda: 15 - 30 * u}[name]().astype(np.float32)


def timed(dev, reps, call):
    call()
    call()
    ms = []
    for _ in range(reps):
        dev.timer_start()
        out = call()
        ms.append(dev.timer_stop())
        del out
    return float(np.median(ms)), [round(m, 4) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1440 * 720)
    ap.add_argument("--rows", type=int, default=365)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--first", action="store_true")
    a = ap.parse_args()
    dev = get_device(0)
    rng = np.random.default_rng(0)
    R, C = a.rows, a.cells
    f = {k: dev.to_device(host_field(k, R, C, rng)) for k in ("tas", "tdps", "hurs", "huss", "ps", "uas", "vas")}
    bufs = {o: dev.empty((R, C), np.float32) for o in FUSED}   # the outputs, allocated once: the window holds no allocation

    def moisture(outputs, fields):
        return K.air_moisture(dev, {k: f[k] for k in fields}, outputs, outs={o: bufs[FUSED[i]] for i, o in enumerate(outputs)})

    if a.first:
        moisture(FUSED, ("tas", "tdps", "ps"))
        dev.sync()
        return
    lines = []

    def record(case, passes, call, **extra):
        ms, all_ms = timed(dev, a.reps, call)
        floor = R * C * 4 * passes / 8e12 * 1e3
        line = {"case": case, "rows": R, "cells": C, "dtype": "float32", "field_passes": passes, "ms_median": round(ms, 4), "ms_min": min(all_ms),
                "ms_max": max(all_ms), "ms": all_ms, "floor_ms_8TBs": round(floor, 4), "times_floor": round(ms / floor, 2), "device": dev.name(), **extra}
        print(json.dumps(line), flush=True)
        lines.append(line)
        return line

    single = {o: record(f"single_{o}", len(need) + 1, lambda o=o, need=need: moisture((o,), need)) for o, need in NEEDS.items()}
    fused = record("fused_hurs_huss_humidex_heat_index_from_tas_tdps_ps", 3 + 4, lambda: moisture(FUSED, ("tas", "tdps", "ps")))
    record("uas_vas_to_sfcwind", 2 + 2, lambda: K.wind_map(dev, "from_uv", f["uas"], f["vas"], [0.5], outputs=(0, 1), outs={0: bufs["hurs"], 1: bufs["huss"]}))

    def two_esat():   # what served relative_humidity(tas, tdps) before this unit: two launches, four passes, the division left to the host
        K.esat(dev, f["tdps"], "sonntag90", out=bufs["hurs"], ld_out=C)
        return K.esat(dev, f["tas"], "sonntag90", out=bufs["huss"], ld_out=C)

    pair = record("two_xh_esat_launches_tdps_and_tas", 4, two_esat)
    four = sum(single[o]["ms_median"] for o in FUSED)
    summary = {"case": "comparisons", "relative_humidity_one_launch_ms": single["hurs"]["ms_median"], "two_xh_esat_launches_ms": pair["ms_median"],
               "relative_humidity_not_slower": single["hurs"]["ms_median"] <= pair["ms_median"], "fused_ms": fused["ms_median"],
               "sum_of_its_four_single_launches_ms": round(four, 4), "fused_faster_than_the_sum": fused["ms_median"] < four,
               "spread": {k: [v["ms_min"], v["ms_max"]] for k, v in (("hurs", single["hurs"]), ("two_esat", pair), ("fused", fused),
                                                                    *((f"single_{o}", single[o]) for o in FUSED))}}
    print(json.dumps(summary), flush=True)
    lines.append(summary)
    out_dir = a.out or next_free_profile_dir()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_humidity.jsonl"), "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
