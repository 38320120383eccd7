"""One bad sample (NaN, -9999, 1e20, the netCDF fill value) in a field of the grid-reduction unit moves only what holds it, and
bitwise nothing else (tests/footprint.py).  For the masked dot that is the sums of the sample's own ROW: the harness perturbs
``field[t, c]`` and looks for the footprint in column ``c`` of the outputs, so the field is handed to it transposed, (cells, rows) —
its "row" is the cell (the first and the last lane of a wave, the seam of the two halves of a chunk, the seam of two chunks, the
ragged last cell) and its "cell" is the row, whose two sums are the whole column (``whole_cell``).  For the jet it is one sample of
the line of samples at one level and one longitude, (T, latitudes): the zonal mean moves on its row and the filtered wind on the rows
whose window (15 weights here) holds it, both at its latitude only.  The reference is the numpy restatement tests/gridcpu.py with the 1e-12 bound
of tests/test_gpu_grid.py."""
import numpy as np
import pytest

import footprint as FP
import gridcpu as G
from poisoned import poisoned_outputs  # noqa: F401
from test_grid_cpu import CHUNK, ROWS
from xclim_amd import kernels as K

pytestmark = pytest.mark.gpu

C_DOT, T_DOT = 2 * CHUNK + 3, ROWS + 1
DOT_CELLS = (0, 63, 64, CHUNK // 2 - 1, CHUNK // 2, CHUNK - 1, CHUNK, C_DOT - 1)
DOT_ROWS = (0, 3, ROWS, 5, 1, ROWS - 1, 2, 6)
THRESH = 15.0
T_JET, Z, Y, X = 64, 2, 10, 8
JET_ROWS, JET_CELLS = (9, 25, 40, 55), (0, 3, 4, 9)     # latitudes: the first and the last wave of a workgroup of k_box_mean_x, and the next workgroup
Z0, X0 = 1, 5
TOL = 1e-12
# 15 weights between 1/8 and 17/8: a window of 15 rows is a quarter of the 64 rows at most, the share of a cell the harness allows a
# footprint.  (Not the Lanczos weights either: five of those are below 1e-17, where a moved sample is lost in the rounding of the
# reference's sum but not always of the device's, whose zonal means differ in their last bits: the footprint, which comes from the
# reference alone, would then miss a row that the window does hold.)
WEIGHTS = ((np.arange(15) * 5) % 17 + 1) / 8.0


def dot_fields(rng, kind, dtype):
    xT = rng.uniform(0.0, 100.0, (C_DOT, T_DOT))
    for c, t in zip(DOT_CELLS, DOT_ROWS):
        xT[c, t] = 50.0                          # a counted sample: every perturbation moves a sum of its row
    return {"xT": xT.astype(dtype), "w": rng.uniform(1e8, 1.2e10, C_DOT)}


def dot_device(dev, f):
    out = K.grid_masked_dot(dev, dev.to_device(np.ascontiguousarray(f["xT"].T)), dev.to_device(f["w"]), THRESH)
    return [out["dot"].get(), out["msum"].get()]


def dot_ref(f):
    return list(G.masked_dot_terms(np.ascontiguousarray(f["xT"].T), f["w"], THRESH))


def jet_fields(rng, kind, dtype):
    rest = rng.normal(8.0, 6.0, (T_JET, Z, Y, X)).astype(dtype)
    return {"rest": rest, "line": rest[:, Z0, :, X0].copy()}


def _jet_u(f):
    u = f["rest"].copy()
    u[:, Z0, :, X0] = f["line"]
    return u


def jet_device(dev, f):
    zm = K.grid_box_mean(dev, dev.to_device(_jet_u(f)), T_JET, Z * Y * X, (Z, Y, X), (Y * X, X, 1), np.arange(Z), np.arange(Y), np.arange(X))
    return [zm.get(), K.grid_filter_argmax(dev, zm, WEIGHTS, ("f",))["f"].get()]


def jet_ref(f):
    zm, zterms = G.box_mean_terms(_jet_u(f), np.arange(Z), np.arange(Y), np.arange(X))
    flt, fterms = G.filter_terms(zm, WEIGHTS)
    # the device filters ITS zonal means, each within 1e-12 x zterms of the restatement's: the scale of f is the sum of its own
    # absolute terms plus the sum of |weight| x zterms over its window
    return [zm, flt, zterms, fterms + G.filter_terms(zterms, np.abs(WEIGHTS))[0]]


CASES = [
    FP.Case(name="masked-dot", lib="grid", make=dot_fields, device=dot_device, ref=dot_ref, target="xT", rows=DOT_CELLS, cells=DOT_ROWS,
            C=T_DOT, tol=(dict(scale=2, rtol=TOL), dict(scale=3, rtol=TOL)), tol_from="tests/test_gpu_grid.py (1e-12 x the absolute terms)",
            kinds=("kelvin",), whole_cell=True),
    FP.Case(name="jet-line", lib="grid", make=jet_fields, device=jet_device, ref=jet_ref, target="line", rows=JET_ROWS, cells=JET_CELLS, C=Y, tol=(dict(scale=2, rtol=TOL), dict(scale=3, rtol=TOL)),
            tol_from="tests/test_gpu_grid.py (1e-12 x the absolute terms)", kinds=("kelvin",)),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_bad_sample_stays_in_its_row_or_its_window_and_latitude(dev, case, dtype):
    FP.check(dev, case, "kelvin", dtype)
