"""Writes tests/golden/phase_vectors.npz: fields and the outputs of the period kernel as the numpy restatement
(tests/phasecpu.py) gives them, one family per decision of the kernel.  Run from the repository root:

    python tests/golden/make_phase_golden.py

Every case is a series of 800 days from 1999-06-10 (its "YS" periods: a partial 1999 that holds row 0, the leap year 2000, a short
2001 that holds row T - 1; "YS-JUL" and "MS" likewise touch both ends).  The exact families use the "binary" method on "mm/d"
fields with amounts on a 0.25 mm grid, so every sum is exact in any order; the random temperatures lie on a 1/64 grid, which
keeps the file small."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import phasecpu as R  # noqa: E402

START, T = "1999-06-10", 800
NEW_YEAR = 205    # the row of 2000-01-01: the boundary of the "YS" periods
K = 273.15


def amounts(rng, C, scale=1.0):
    """Daily amounts on a 0.25 grid, about a third of the days wet."""
    return np.where(rng.random((T, C)) < 0.35, np.round(rng.gamma(0.9, 6.0, (T, C)) * 4) / 4, 0.0) * scale


def temps(rng, C, mean, spread=6.0):
    t = np.arange(T)[:, None]
    return np.round((mean + 12 * np.cos(2 * np.pi * (t - 35) / 365.25) + rng.normal(0, spread, (T, C))) * 64) / 64


def exact_case(dtype):
    """binary, K, "mm/d": every decision on a column of its own."""
    rng = np.random.default_rng(11)
    C = 12
    thr = dtype(K)
    pr = amounts(rng, C).astype(dtype)
    tas = temps(rng, C, K).astype(dtype)
    pr[:, :3] = np.where(pr[:, :3] == 0, 0.25, pr[:, :3])
    tas[:, 0] = thr                                    # at the threshold: snow
    tas[:, 1] = np.nextafter(thr, dtype(0))            # one ulp below: snow
    tas[:, 2] = np.nextafter(thr, dtype(1e4))          # one ulp above: no snow day in any period
    tas[:, 3] = np.nan                                 # NaN tas: snow 0, rain pr
    pr[::3, 4] = np.nan                                # NaN pr, warm: snow 0, rain NaN
    tas[:, 4] = thr + dtype(5)
    pr[::3, 5] = np.nan                                # NaN pr, cold: both NaN
    tas[:, 5] = thr - dtype(5)
    pr[NEW_YEAR:NEW_YEAR + 366, 6] = np.nan            # the year 2000 all NaN (both fields)
    tas[NEW_YEAR:NEW_YEAR + 366, 6] = np.nan
    pr[:, 7] = np.where(np.arange(T) % 2, 1.0, 0.75)   # amounts at the snow threshold of 1 mm and just below
    tas[:, 7] = thr - dtype(1)
    # rain on frozen ground: frozen everywhere, wet everywhere, thaws placed by hand
    for c in (8, 9, 10):
        tas[:, c] = thr - dtype(2)
        pr[:, c] = 2.0
    tas[6, 8] = thr + dtype(1)                         # a thaw on row 6 of the series: only six rows before it, never counts
    tas[30, 8] = thr + dtype(1)                        # (a thaw after a long freeze, for contrast)
    tas[7, 9] = thr + dtype(1)                         # a thaw on row 7: the first row that can count
    tas[8, 10] = thr + dtype(1)                        # and on row 8
    tas[NEW_YEAR - 8, 9] = thr + dtype(1)              # a freeze run of 7 rows up to the boundary, then a thaw ...
    tas[NEW_YEAR + 2, 9] = thr + dtype(1)              # ... on the third row of the new period: the run crosses the boundary
    tas[NEW_YEAR - 5, 10] = np.nan                     # (a NaN inside the run counts as frozen)
    tas[NEW_YEAR, 10] = thr + dtype(1)                 # a thaw on the first row of a period
    tas[NEW_YEAR + 366 - 3, 10] = thr + dtype(1)       # and two thaws fewer than 7 rows apart around the next boundary
    tas[NEW_YEAR + 366 + 2, 10] = thr + dtype(1)
    fam = ["at_thresh", "nan_pr", "no_snow_day", "all_nan_period", "rofg_early_thaw", "rofg_boundary", "rofg_first_row"]
    params = {"method": "binary", "thresh": K, "units": "K", "snow_low": 0.75, "snow_thresh": 1.0, "pr_thresh": 1.0, "tas_thresh": K + 0.5,
              "rofg_thresh": 1.0}
    return pr, tas, fam, params


def cases():
    out = {}
    for dtype, freq in ((np.float32, "YS"), (np.float64, "MS")):
        pr, tas, fam, params = exact_case(dtype)
        out[f"exact.{np.dtype(dtype).name}"] = (pr, tas, fam, params, "mm/d", freq, False)
    frac = {"snow_low": 0.3, "snow_thresh": 0.9}
    rng = np.random.default_rng(12)
    # brown: tas at thresh, at upper, one ulp inside either end
    C = 8
    pr, tas = amounts(rng, C), temps(rng, C, K + 1, 3.0)
    tas[:, 0], tas[:, 1] = K + 0.5, (K + 0.5 - K + 2) + K
    tas[:, 2], tas[:, 3] = np.nextafter(K + 0.5, 1e4), np.nextafter((K + 0.5 - K + 2) + K, 0)
    out["brown.float64"] = (pr, tas, ["brown_upper", "random"], {"method": "brown", "thresh": K + 0.5, "units": "K", **frac}, "mm/d", "YS-JUL", False)
    # auer with thresh = 0 K: dtas is tas itself, so the columns sit exactly on the nodes
    pr, tas = amounts(rng, C), temps(rng, C, 2.0, 3.0)
    nodes = R.auer_nodes()[0]
    for c, v in enumerate((nodes[1], nodes[2], nodes[100], nodes[101], -0.5, 6.5)):
        tas[:, c] = v
    out["auer.float64"] = (pr, tas, ["auer_nodes", "random"], {"method": "auer", "thresh": 0.0, "units": "K", **frac}, "mm/d", "YS", False)
    pr, tas = (amounts(rng, 4) / 86400).astype(np.float32), temps(rng, 4, 1.0, 3.0).astype(np.float32)
    out["auer.float32"] = (pr, tas, ["random"], {"method": "auer", "thresh": -0.5, "units": "degC", **frac}, "kg m-2 s-1", "MS", False)
    # dai_annual with clip_temp: tas at -clip, +clip and beyond
    pr, tas = amounts(rng, C), temps(rng, C, 0.0, 3.0)
    for c, v in enumerate((-2.0, 2.0, -2.5, 2.5, np.nextafter(2.0, 0), np.nextafter(-2.0, 0))):
        tas[:, c] = v
    out["dai_clip.float64"] = (pr, tas, ["dai_clip", "random"], {"method": "dai_annual", "units": "degC", "clip_temp": 2.0, "landmask": False, **frac},
                               "mm/d", "YS", False)
    # land and ocean cells side by side, seasons changing inside the "YS" periods
    pr, tas = amounts(rng, C).astype(np.float32), temps(rng, C, K + 1, 3.0).astype(np.float32)
    tas[:, 1] = tas[:, 0]
    pr[:, 1] = pr[:, 0]
    land = [True, False] * (C // 2)
    out["dai_seasonal.float32"] = (pr, tas, ["land_ocean", "season_change", "random"],
                                   {"method": "dai_seasonal", "units": "K", "landmask": land, **frac}, "mm/d", "YS", False)
    pr = amounts(rng, C).astype(np.float32)
    prsn = np.where(rng.random((T, C)) < 0.5, pr, 0).astype(np.float32)
    prsn[::7, 2] = np.nan
    out["given.float32"] = (pr, prsn, ["random"], {"snow_low": 0.5, "snow_thresh": 1.0}, "mm/d", "YS-JUL", True)
    return out


def main():
    arrays, meta = {}, {}
    for name, (pr, second, fam, params, flux, freq, given) in cases().items():
        time = R.otime(START, T)
        kw = dict(params)
        if isinstance(kw.get("landmask"), list):
            kw["landmask"] = np.array(kw["landmask"], bool)
        exp = R.period_outputs(pr, second, time, freq, given=given, per_day=R.PER_DAY[flux], **kw)
        arrays[f"{name}/pr"], arrays[f"{name}/second"] = pr, second
        for o, v in exp.items():
            arrays[f"{name}/{o}"] = v
        meta[name] = {"family": fam, "params": params, "flux_units": flux, "freq": freq, "given": given, "start": START, "dtype": pr.dtype.name,
                      "outputs": list(exp)}
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "phase_vectors.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
