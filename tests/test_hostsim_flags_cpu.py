"""The data-quality-flag unit WITHOUT a GPU: tests/hostsim/simdevice.py builds dataflags.hip, unchanged, into a small simulation
library (one lane per cell, plain stores, no traffic between lanes: thread by thread) together with the units of the entry
points its cross-check calls, and this module re-runs tests/test_gpu_flags.py and tests/test_gpu_flags_adapter.py on it in a child
pytest, the way tests/test_hostsim_units_cpu.py re-runs the other units'.  The second half builds the unit's stand-alone program
(tests/hostsim/standalone/flags_driver.cpp: its own main, g++ -fsanitize=address,undefined, nothing loaded into Python) that
calls the two entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

# dataflags.hip; spell.hip (xh_suspicious_run; it links against the launchers of window.hip) and elemwise.hip (xh_compare_map,
# xh_within_bnds_doy) hold the entry points of the cross-check with what existed before.  The driver holds the unit alone.
simdevice.UNIT_LIBRARIES["flags"] = (("dataflags", "spell", "window", "elemwise"), ("dataflags",), "flags_driver.cpp")
ENTRY_POINTS = ("xh_data_flags", "xh_doy_bounds", "xh_suspicious_run", "xh_compare_map", "xh_within_bnds_doy")
GPU_MODULES = ["tests/test_gpu_flags.py", "tests/test_gpu_flags_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "flags", tmp_path_factory.mktemp("hostsim_flags")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_known_answers_on_the_simulation(sim):
    from test_flags_cpu import check_known_answers, mirror_api

    check_known_answers(mirror_api(sim))


def test_the_refusals_on_the_simulation(sim):
    from test_flags_cpu import refusals

    refusals(sim)


def test_the_gpu_modules_on_the_simulation(sim):
    # (of tests/test_gpu_footprint.py: the cases on this unit's entry points, by their id "flags-...", and the test named "flags")
    _child_run(sim, GPU_MODULES + ["tests/test_gpu_footprint.py"], skip="footprint and not (flags- or test_flags)", at_least=60 + 6)


def test_standalone_sanitizer_run(tmp_path):
    """The two entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes: runs that touch row 0 and row T - 1, the stores into earlier periods with P = T, window rows before row 0 and after row
    T - 1, 1, 65 and 260 cells, float32 and float64 (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "flags", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
