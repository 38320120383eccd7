"""The snow / rain partition unit WITHOUT a GPU: tests/hostsim/simdevice.py builds phase.hip, unchanged, into a small simulation
library together with the units of the entry points its cross-check calls, and this module re-runs tests/test_gpu_phase.py and
tests/test_gpu_phase_adapter.py on it in a child pytest, the way tests/test_hostsim_flags_cpu.py does for the data-quality flags.
Thread by thread suffices: both kernels have one lane per (cell, period) or per cell group, read the auer table and the dai
coefficients from global memory (nothing is staged in LDS), and have no barrier and no traffic between lanes.  The second half
builds the unit's stand-alone program (tests/hostsim/standalone/phase_driver.cpp: its own main, g++ -fsanitize=address,undefined,
nothing loaded into Python) that calls the two entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

# phase.hip; f64.hip (xh_resample_reduce_f64, xh_threshold_count_f64; it links against the launchers of window.hip) holds the entry
# points of the cross-check with what existed before, reduce.hip + tcount.hip their float32 twins.  The driver holds the unit alone.
simdevice.UNIT_LIBRARIES["phase"] = (("phase", "f64", "reduce", "tcount", "window"), ("phase",), "phase_driver.cpp")
ENTRY_POINTS = ("xh_precip_phase_map", "xh_precip_phase_period", "xh_resample_reduce_f64", "xh_threshold_count_f64")
GPU_MODULES = ["tests/test_gpu_phase.py", "tests/test_gpu_phase_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "phase", tmp_path_factory.mktemp("hostsim_phase")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    for name in ENTRY_POINTS:
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_known_answers_on_the_simulation(sim):
    from test_phase_cpu import check_known_answers, mirror_api

    assert check_known_answers(mirror_api(sim)) == 33


def test_the_refusals_on_the_simulation(sim):
    from test_phase_cpu import refusals

    refusals(sim)


def test_the_gpu_modules_on_the_simulation(sim):
    # (of tests/test_gpu_footprint.py: the cases on this unit's entry points, by their id "phase-...")
    _child_run(sim, GPU_MODULES + ["tests/test_gpu_footprint.py"], skip="footprint and not phase-", at_least=100 + 6)


def test_standalone_sanitizer_run(tmp_path):
    """The two entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes: a one-row series, periods on row 0 and on row T - 1, the frozen-ground warm-up at row 0, 1, 65 and 260 cells, float32 and
    float64, every method (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "phase", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
