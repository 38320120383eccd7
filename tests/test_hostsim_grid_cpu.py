"""The grid-reduction unit WITHOUT a GPU: tests/hostsim/simdevice.py builds grid.hip, unchanged, into a small simulation library,
and this module re-runs tests/test_gpu_grid.py, tests/test_gpu_grid_footprint.py and tests/test_gpu_grid_adapter.py on it in a child
pytest, the way tests/test_hostsim_compound_cpu.py does for the compound unit.  The lanes of k_masked_dot, k_dot_finish,
k_box_mean_x and k_filter_argmax talk through shuffles, static LDS and workgroup barriers, so the unit is compiled on fibers (no
``extern __shared__`` declaration to rewrite: 0).  The mirror calls no entry point beside its own.  The second half builds the
unit's stand-alone program (tests/hostsim/standalone/grid_driver.cpp: its own main, g++ -fsanitize=address,undefined, nothing loaded
into Python) that calls the three entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

simdevice.UNIT_LIBRARIES["grid"] = (("grid",), ("grid",), "grid_driver.cpp")
simdevice.UNIT_LIBRARY_FIBER_UNITS["grid"] = 0
GPU_MODULES = ["tests/test_gpu_grid.py", "tests/test_gpu_grid_footprint.py", "tests/test_gpu_grid_adapter.py"]
ENTRY_POINTS = ("xh_grid_masked_dot", "xh_grid_box_mean", "xh_grid_filter_argmax")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "grid", tmp_path_factory.mktemp("hostsim_grid")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert all(hasattr(dll, n) for n in ENTRY_POINTS)
    assert sim.lib.xh_grid_masked_dot.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_compound_doy_days


def test_the_known_answers_on_the_simulation(sim):
    from test_grid_cpu import check_known_answers, mirror_api

    check_known_answers(mirror_api(sim))


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=70)


def test_standalone_sanitizer_run(tmp_path):
    """The three entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes, at the small shapes of tests/test_gpu_grid.py (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "grid", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
