"""One bad sample (NaN, -9999, 1e20, the netCDF fill value) in one cell of a field of the compound-extreme unit moves only the
results whose period (for the window of blowing_snow: whose periods) hold it, and bitwise nothing in any other cell
(tests/footprint.py).  Positions: four rows in different periods, at the first cell, the wave seam (cells 63 and 64) and the ragged
tail (cell 69 of 70: with float32 fields cells 68 and 69 are the partial last 16-byte group of xh_compound_doy_days).  The reference
is the numpy restatement tests/compoundcpu.py, which adds in the kernels' order: every comparison is exact."""
import numpy as np
import pytest

import compoundcpu as CC
import footprint as FP
from poisoned import poisoned_outputs  # noqa: F401
from test_compound_cpu import COUNTS, TABLES, TABLE_ARGS, golden_otime, golden_time
from xclim_amd import compound

pytestmark = pytest.mark.gpu

C = 70
TIME, OTIME = golden_time("std"), golden_otime("std")
T = len(TIME)
ROWS = (85, 178, 270, 360)      # a few days into four consecutive quarters of QS-DEC (and into four different months)
CELLS = (0, 63, 64, 69)
THRESH, SUM_THRESH = 278.0, 150.0
WINDOW = 3


def compound_fields(rng, kind, dtype):
    """Random fields and tables; at the perturbed positions the sample takes part in a count: cold and dry at the first and third,
    warm and wet at the second and fourth (so that every perturbation of either field moves a count at one of them at least)."""
    f = {"tas": FP.kelvin(rng, T, C, dtype), "pr": FP.flux(rng, T, C, dtype),
         "tas_lo": 280.0 + rng.normal(0, 0.5, (366, C)), "tas_hi": 286.0 + rng.normal(0, 0.5, (366, C)),
         "pr_lo": rng.uniform(5e-6, 2e-5, (366, C)), "pr_hi": rng.uniform(5e-5, 2e-4, (366, C))}
    for k, (r, c) in enumerate(zip(ROWS, CELLS)):
        f["tas"][r, c], f["pr"][r, c] = (270.0, 0.0) if k % 2 == 0 else (295.0, 1e-3)
    return f


def compound_device(dev, f):
    out = compound.compound_days(f["tas"], f["pr"], **{TABLE_ARGS[k]: f[k] for k in TABLE_ARGS}, freq="MS", time=TIME, device=dev)
    return [out[n] for n in COUNTS]


def compound_ref(f):
    return [CC.compound_days(n, f["tas"], f["pr"], f[TABLES[n][0]], f[TABLES[n][1]], OTIME, "MS") for n in COUNTS]


def dded_fields(rng, kind, dtype):
    tas = FP.kelvin(rng, T, C, dtype)
    for r, c in zip(ROWS, CELLS):
        tas[r, c] = THRESH + 30.0      # a warm day before the sum of its quarter is reached: without it the date moves
    return {"tas": tas}


def snow_fields(rng, kind, dtype):
    snd = np.abs(np.cumsum(rng.normal(0, 0.2, (T, C)), axis=0))
    wind = rng.uniform(0, 9, (T, C))
    for r, c in zip(ROWS, CELLS):      # snow that keeps falling in a wind around the position: every window there counts
        snd[r - 5:r + 6, c] = 1.0 + np.arange(11.0)
        wind[r - 5:r + 6, c] = 9.0
    return {"snd": snd.astype(dtype), "sfcWind": wind.astype(dtype)}


def wci_fields(rng, kind, dtype):
    pr, ev = FP.flux(rng, T, C, dtype), FP.flux(rng, T, C, dtype)
    for r, c in zip(ROWS, CELLS):
        pr[r, c] = ev[r, c] = 1e-4
    return {"pr": pr, "evspsbl": ev}


def _case(name, make, device, ref, target, nout, **kw):
    return FP.Case(name=name, lib="compound", make=make, device=device, ref=ref, target=target, rows=ROWS, cells=CELLS, C=C,
                   tol=(None,) * nout, tol_from="tests/test_gpu_compound.py (exact)", kinds=("kelvin",), **kw)


NO_COUNT = "-9999 leaves a cold (dry) sample cold (dry), 1e20 a warm (wet) one warm (wet): its counts stay; the other positions move"
CASES = [
    _case("compound-tas", compound_fields, compound_device, compound_ref, "tas", 4, may_be_empty=NO_COUNT),
    _case("compound-pr", compound_fields, compound_device, compound_ref, "pr", 4, may_be_empty=NO_COUNT),
    _case("dded", dded_fields,
          lambda dev, f: [compound.degree_days_exceedance_date(f["tas"], THRESH, SUM_THRESH, freq="QS-DEC", time=TIME, device=dev)],
          lambda f: [CC.degree_days_exceedance_date(f["tas"], OTIME, THRESH, SUM_THRESH, freq="QS-DEC")], "tas", 1),
    _case("snow-snd", snow_fields,
          lambda dev, f: [compound.blowing_snow(f["snd"], f["sfcWind"], 0.5, 4.0, WINDOW, "MS", time=TIME, device=dev)],
          lambda f: [CC.blowing_snow(f["snd"], f["sfcWind"], OTIME, 0.5, 4.0, WINDOW, "MS")], "snd", 1),
    _case("snow-wind", snow_fields,
          lambda dev, f: [compound.blowing_snow(f["snd"], f["sfcWind"], 0.5, 4.0, WINDOW, "MS", time=TIME, device=dev)],
          lambda f: [CC.blowing_snow(f["snd"], f["sfcWind"], OTIME, 0.5, 4.0, WINDOW, "MS")], "sfcWind", 1,
          dropped={"1e20": "a wind above the threshold, as the clean sample is: nothing moves", "ncfill": "as 1e20"}),
    _case("wci", wci_fields,
          lambda dev, f: [compound.water_cycle_intensity(f["pr"], f["evspsbl"], "MS", time=TIME, device=dev)],
          lambda f: [CC.water_cycle_intensity(f["pr"], f["evspsbl"], OTIME, "MS")], "pr", 1),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_bad_sample_stays_in_its_period_and_its_cell(dev, case, dtype):
    FP.check(dev, case, "kelvin", dtype)
