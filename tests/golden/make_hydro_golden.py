"""Writes tests/golden/hydro_vectors.npz from the numpy restatement tests/hydrocpu.py: the inputs (seeded fields with the NaN
patterns of hydrocpu.synth) and the expected outputs of every run of every case, with a scale per value where the bound is
relative to one.  Run from the repository root: ``python tests/golden/make_hydro_golden.py``."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import hydrocpu as H  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

FREQS = ("YS", "YS-JUL", "YS-OCT", "QS-DEC", "MS")
LONG_RUNS = ([dict(kind="flow", freq=f) for f in FREQS]
             + [dict(kind="melt", window=3, freq="YS-JUL", pr="pr"), dict(kind="melt", window=3, freq="YS-JUL", pr="nopr"),
                dict(kind="melt", window=31, freq="MS", pr="pr"), dict(kind="melt", window=1, freq="YS", pr="pr"),
                dict(kind="melt", window=5, freq="QS-DEC", pr="nopr"), dict(kind="melt", window=32, freq="YS-OCT", pr="pr")]
             + [dict(kind="api", window=7, p_exp=0.935), dict(kind="api", window=1, p_exp=0.935), dict(kind="api", window=31, p_exp=0.9)]
             + [dict(kind="sen", freq="QS-DEC"), dict(kind="sen", freq="YS"), dict(kind="sen", freq="MS")])
SHORT_RUNS = [dict(kind="flow", freq="YS"), dict(kind="melt", window=3, freq="YS", pr="pr"), dict(kind="melt", window=7, freq="YS", pr="nopr"),
              dict(kind="api", window=7, p_exp=0.935), dict(kind="api", window=1, p_exp=0.935)]
CASES = {
    "std_f64": dict(start="2000-01-01", T=800, calendar="standard", dtype="float64", C=5, runs=LONG_RUNS),
    "noleap_f32": dict(start="2000-01-01", T=800, calendar="noleap", dtype="float32", C=5, runs=LONG_RUNS),
    "midyear_f32": dict(start="1998-11-17", T=800, calendar="standard", dtype="float32", C=5, runs=LONG_RUNS),
    "short_f64": dict(start="2000-01-01", T=5, calendar="standard", dtype="float64", C=3, runs=SHORT_RUNS),
}


def main():
    arrays, meta = {}, {}
    for name, c in CASES.items():
        time = TimeAxis.daily(c["start"], c["T"], c["calendar"])
        fields = H.synth(time, c["C"], np.dtype(c["dtype"]))
        for k, v in fields.items():
            arrays[f"{name}/{k}"] = v
        for s in c["runs"]:
            for k, v in H.run(s, fields, time).items():
                arrays[f"{name}/{H.spec_id(s)}/{k}"] = v
        meta[name] = c
    arrays["meta"] = np.array(json.dumps(meta))
    out = os.path.join(HERE, "hydro_vectors.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
