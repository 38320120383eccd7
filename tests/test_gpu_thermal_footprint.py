"""One bad sample (NaN, -9999, 1e20, the netCDF fill value) in each of the seven fields of xh_thermal_comfort changes the outputs of
that sample and no other (tests/footprint.py).  Positions: the last row, at the wave seam (cells 63 and 64), the first cell and the
ragged tail (cell 69 of 70).  The reference is the numpy restatement end to end, so its bound carries the cosine's: csza is good to
1e-12 absolute and enters i_star = direct / csza only where csza > 0.001, which amplifies it to at most 1e-9 relative in the
bracket and a quarter of that in mrt (rtol 1e-9 asserted); UTCI then moves by at most its slope in the radiant temperature (below
2 degC per K) times 1e-9 * 330 K, under 1e-6 degC, plus 1e-12 of the polynomial of magnitudes (a bad humidity is not masked and
gives a UTCI of 1e10) and one float32 ulp of the value for float32 fields: the third array the reference returns."""
import numpy as np
import pytest

import footprint as FP
import thermalcpu as TC
from poisoned import poisoned_outputs  # noqa: F401
from xclim_amd import _capi, thermal
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

SUB = thermal.SubDaily(8)
TIME = TimeAxis.daily("2001-06-20", 3, "standard")
R, C = 24, 70
LAT, LON = np.linspace(-80, 80, C), np.linspace(-170, 350, C)
FIELDS = ("tas", "hurs", "sfcWind", "rsds", "rsus", "rlds", "rlus")


def make(rng, kind, dtype):
    tas = rng.uniform(265, 310, (R, C))
    f = {"tas": tas, "hurs": rng.uniform(10, 95, (R, C)), "sfcWind": rng.uniform(0.6, 15, (R, C)), "rsds": rng.uniform(5, 300, (R, C)),
         "rlds": 0.8 * 5.67e-8 * tas**4, "rlus": 5.67e-8 * tas**4}
    f["rsus"] = 0.2 * f["rsds"]
    return {k: f[k].astype(dtype) for k in FIELDS}


def device(dev, f):
    res = thermal.universal_thermal_climate_index(**f, lat=LAT, lon=LON, time=TIME, subdaily=SUB, outputs=("utci", "mrt"), device=dev)
    return [res["utci"], res["mrt"]]


def ref(f):
    rows = thermal.solar_rows(TIME, subdaily=SUB)
    cs, _ = TC.csza(rows, TC.wrap(LAT * (np.pi / 180)), LON * (np.pi / 180), "subdaily", "sunlit")
    m = TC.mrt(cs, rows[_capi.THERMAL_ROWS["inv_d2"]], f["rsds"], f["rsus"], f["rlds"], f["rlus"])[0]
    u, scale = TC.utci(f["tas"], f["hurs"], f["sfcWind"], m)
    dt = f["tas"].dtype
    with np.errstate(over="ignore"):
        u = u.astype(dt)
        bound = 1e-12 * scale + 1e-6 + (np.spacing(np.abs(u)).astype(np.float64) if dt == np.float32 else 0.0)
    return [u, m, bound]


CASES = [FP.Case(name=f"thermal-{n}-{np.dtype(dt).name}", lib="thermal", make=make, device=device, ref=ref, target=n, rows=(R - 1,),
                 tol=(dict(scale=2, rtol=1.0), dict(rtol=1e-9)), tol_from="this module's docstring",
                 kinds=("kelvin",), dtypes=(dt,)) for n in FIELDS for dt in (np.float32, np.float64)]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_bad_sample_stays_in_its_sample(dev, case):
    FP.check(dev, case, "kelvin", case.dtypes[0])
