"""Generate tests/golden/grid_known_answers.json and tests/golden/grid_vectors.npz.

grid_known_answers.json holds, as data only, the inputs and the expectations of the reference's own tests of the three bodies of the
grid-reduction unit — the sea-ice geometry of tests/conftest.py:233-251 and tests/test_seaice.py, the jet case of
tests/test_indices.py:2283-2336 — and the 61 Lanczos weights, recorded by EXECUTING the reference's
``_compute_low_pass_filter_weights`` (src/xclim/indices/_synoptic.py:103-116) behind a stand-in ``xarray.DataArray``.  Run in the
build container only (needs the reference tree, which does not exist on the GPU box); without it the weights of the existing file
are kept.

grid_vectors.npz holds the inputs of tests/test_gpu_grid.py in compact integer encodings (the tests decode them, tests/test_grid_cpu.py
``decode``): concentrations in quarter percents, cell areas that are integers below 2^20, winds in 1/64 m s-1 — every sum of such
values is exact in float64 in ANY order, so the device must equal the restatement bit for bit — and one random family per kernel,
compared within 1e-12 x the sum of a value's absolute terms.  The expectations are not stored: tests/gridcpu.py computes them."""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/xclim/indices/_synoptic.py"
KNOWN = os.path.join(HERE, "grid_known_answers.json")
VECTORS = os.path.join(HERE, "grid_vectors.npz")
CHUNK, ROWS = 2048, 8   # XH_GRID_CHUNK, XH_GRID_ROWS (tests/test_grid_cpu.py checks them against the header)


def reference_weights():
    """The reference's own function, executed: its ``xarray.DataArray(values, dims=[...])`` returns the values."""
    tree = ast.parse(open(REF).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_compute_low_pass_filter_weights"]
    for node in body:
        node.decorator_list, node.returns = [], None
        for a in node.args.args:
            a.annotation = None
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "xarray": types.SimpleNamespace(DataArray=lambda values, dims=None: np.asarray(values))}
    exec(compile(mod, REF, "exec"), ns)
    return ns["_compute_low_pass_filter_weights"](window_size=61, cutoff=1 / 10)


def known_answers(weights):
    return {
        "sea_ice": {
            # conftest.py:233-251: a 1 degree grid on a sphere of radius r; test_seaice.py: 10 % south of the equator, 50 % north
            "r": 6100000, "south": 10, "north": 50, "rows": 2, "thresh": "15 %", "decimals": 3,
            "extent_over": "2 pi r^2", "area_over": "pi r^2", "numpy_ratio": 1.0000127,
            "cases": [{"name": "simple", "siconc_units": "%", "siconc_scale": 1.0, "area_units": "m2", "area_scale": 1.0},
                      {"name": "dimensionless", "siconc_units": "", "siconc_scale": 0.01, "area_units": "m2", "area_scale": 1.0},
                      {"name": "area_units", "siconc_units": "%", "siconc_scale": 1.0, "area_units": "km2", "area_scale": 1e-6}]},
        "jet": {
            # test_indices.py:2283-2336: 66 days, (time, Z, X, Y), ones at the middle latitude
            "T": 66, "dims": ["time", "Z", "X", "Y"], "Z": [75000, 85000, 100000], "X": [120, 121, 122], "Y": [15, 16, 17],
            "value_by_Y": [0.0, 1.0, 0.0], "ua_units": "m s-1", "Z_units": "Pa", "Y_units": "degrees_north", "X_units": "degrees_east",
            "error_with_X_as_given": "ValueError", "shift_X": -180, "not_nan": 6, "jetlat_max": 16.0, "jetstr_max": 0.999276877412766},
        "lanczos_weights_61_0.1": [float(v) for v in weights],
    }


def vectors():
    rng = np.random.default_rng(28)
    C, T = 2 * CHUNK + 3, ROWS + 1
    z = {}
    # masked dot, exact: concentrations 0 .. 100 % in quarter percents (a fifth of the cells below the threshold), integer areas
    q = rng.integers(0, 401, (T, C)).astype(np.uint16)
    q[rng.random((T, C)) < 0.2] = 0
    z["dot/exact/q"] = q
    z["dot/exact/area"] = rng.integers(1, 1 << 20, C).astype(np.uint32)
    # masked dot, random: float32 concentrations, float64 areas of a 1 degree grid scale
    z["dot/random/x"] = rng.uniform(0, 100, (T, C)).astype(np.float32)
    z["dot/random/area"] = rng.uniform(1e8, 1.2e10, C)
    # jet, exact: winds in 1/64 m s-1 on a base (T, Z, Y, X) block that the tests tile along Y and X
    z["jet/exact/q"] = rng.integers(-1024, 1025, (130, 4, 8, 16)).astype(np.int16)
    # jet, random: one float32 block at the largest shape of the tests' random family
    z["jet/random/u"] = rng.normal(8.0, 6.0, (66, 3, 5, 67)).astype(np.float32)
    z["filter/random/zm"] = rng.normal(8.0, 6.0, (130, 65))
    z["meta"] = np.array(json.dumps({"chunk": CHUNK, "rows": ROWS, "seed": 28}))
    return z


if __name__ == "__main__":
    if os.path.exists(REF):
        w = reference_weights()
    elif os.path.exists(KNOWN):
        w = json.load(open(KNOWN))["lanczos_weights_61_0.1"]
        print("reference tree not present: the recorded weights are kept", file=sys.stderr)
    else:
        sys.exit("reference tree not present; the weights can only be recorded in the build container")
    with open(KNOWN, "w") as f:
        json.dump(known_answers(w), f, indent=1)
        f.write("\n")
    np.savez_compressed(VECTORS, **vectors())
    print(KNOWN, os.path.getsize(KNOWN), VECTORS, os.path.getsize(VECTORS))
