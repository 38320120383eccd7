"""One bad sample (NaN, -9999, 1e20, the netCDF fill value; inf in a test of its own) in one series of one cell changes that
series' sm and roll, that cell's components and g, and bitwise nothing in any other cell (tests/footprint.py).  The perturbed field
is ONE series of the cube, (time, cell); the other members are fixed, so the harness's (row, cell) positions address a sample.
Positions: the first and last year, two years inside, at the first cell, the wave seam (cells 63 and 64) and the ragged tail
(cell 69 of 70).  A polynomial fit reads its whole series, so the footprint may be the whole cell (``whole_cell``).  The reference
is the numpy restatement with its series solved one by one, so that no series' bits depend on which others share a LAPACK call; the
bounds are its own (tests/partitioncpu.py)."""
import numpy as np
import pytest

import footprint as FP
import partitioncpu as P
from poisoned import poisoned_outputs  # noqa: F401
from xclim_amd import kernels as K
from xclim_amd import partitioning
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

C = 70
YEARS = np.arange(1980, 2020)
TIME = TimeAxis(YEARS, np.full(40, 12), np.full(40, 31), "standard")
SERIES = {"hs": (1, 2), "ls": (1, 0, 1)}   # the member whose series is perturbed
MEMBERS = {"hs": (2, 3), "ls": (2, 3, 2)}


def make(func):
    def fields(rng, kind, dtype):
        cube = P._field(91 if func == "hs" else 92, YEARS, MEMBERS[func], dtype, base=5.0)[..., :C]
        return {"series": np.ascontiguousarray(cube[(slice(None),) + SERIES[func]]), "cube": cube}
    return fields


def _cube(func, f):
    cube = f["cube"].copy()
    cube[(slice(None),) + SERIES[func]] = f["series"]
    return cube


def device(func):
    def run(dev, f):
        cube = _cube(func, f)
        T = cube.shape[0]
        if func == "hs":
            g, u, sm = partitioning.hawkins_sutton(cube, baseline=("1981", "2000"), kind="*", time=TIME, device=dev, keep=True)
            roll = K.partition_smooth(dev, dev.to_device(np.ascontiguousarray(cube.reshape(T, -1, C))), partitioning.poly_basis(TIME), window=10,
                                      stat="mean", outputs=("roll",))["roll"]
        else:
            g, u, sm = partitioning.lafferty_sriver(cube, time=TIME, device=dev, keep=True)
            roll = K.partition_smooth(dev, dev.to_device(np.ascontiguousarray(cube.reshape(T, -1, C))), partitioning.poly_basis(TIME),
                                      outputs=("roll",))["roll"]
        return [sm.get(), roll.get(), g, u]
    return run


def ref(func):
    def run(f):
        cube = _cube(func, f)
        T = cube.shape[0]
        with np.errstate(all="ignore"):
            if func == "hs":
                g, u, bg, bu = P.hawkins_sutton(cube, YEARS, baseline=(1981, 2000), kind="*", batched=False)
            else:
                g, u, bg, bu = P.lafferty_sriver(cube, YEARS, batched=False)
            sm, e = P.smooth(cube, P.stamps_ns(YEARS), batched=False)
            e = e + P.restatement_slack(cube)   # (sm is compared with the restatement here, not with an exact fit)
            window, stat = (10, "mean") if func == "hs" else (11, "var")
            roll = P.rolling(cube.astype(np.float64) - sm, window, stat)
            wtol = P._winmax(e, window)
            b_roll = wtol + P.RTOL * np.abs(roll) if func == "hs" else P._vbound(roll, wtol)
            if func == "hs":   # the written sm is divided by the baseline mean
                rows = sm[1:21]
                base = np.nansum(rows, axis=0) / (~np.isnan(rows)).sum(axis=0)
                e = (e + np.abs(sm / base) * np.nanmax(e[1:21], axis=0)) / np.abs(base) + P.RTOL * np.abs(sm / base)
                sm = sm / base
        flat = lambda a: np.ascontiguousarray(a.reshape(T, -1, C))   # noqa: E731
        return [flat(sm), flat(roll), g, u, flat(e), flat(b_roll), bg, bu]
    return run


SCALED = tuple(dict(scale=k, rtol=1.0) for k in (4, 5, 6, 7))
CASES = [FP.Case(name=f"partition-{func}-{np.dtype(dt).name}", lib="partition", make=make(func), device=device(func), ref=ref(func),
                 target="series", rows=(0, 14, 39, 22), tol=SCALED, tol_from="tests/partitioncpu.py", kinds=("kelvin",), dtypes=(dt,),
                 whole_cell=True) for func, dt in (("hs", np.float32), ("ls", np.float64))]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_bad_sample_stays_in_its_cell(dev, case):
    FP.check(dev, case, "kelvin", case.dtypes[0])


@pytest.mark.parametrize("func", ["hs", "ls"])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_bad_sample_changes_only_its_series_and_its_cell(dev, func, bad):
    """device(clean) against device(perturbed), bit for bit: sm and roll of every other series, and everything of every other
    cell, stay as they are; the perturbed series and its cell's components do change."""
    f = make(func)(None, "kelvin", np.float64)
    clean = device(func)(dev, f)
    n = int(np.ravel_multi_index(SERIES[func], MEMBERS[func]))
    for t, c in ((0, 0), (14, 63), (39, 64), (22, 69)):
        g = dict(f)
        g["series"] = f["series"].copy()
        g["series"][t, c] = bad
        pert = device(func)(dev, g)
        for k, (a, b) in enumerate(zip(clean, pert)):
            same = FP.same_bits(a, b)
            assert np.delete(same, c, axis=-1).all(), f"output {k}: another cell changed"
            if k < 2:
                assert np.delete(same[..., c], n, axis=1).all(), f"output {k}: another series of the cell changed"
                assert not same[:, n, c].all(), f"output {k}: the series did not change"
            else:
                assert not same[..., c].all(), f"output {k}: the cell did not change"
