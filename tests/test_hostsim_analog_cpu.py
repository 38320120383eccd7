"""The spatial-analogue unit WITHOUT a GPU: tests/hostsim/simdevice.py builds analog.hip, unchanged, into a small simulation library,
and this module re-runs tests/test_gpu_analog.py and tests/test_gpu_analog_adapter.py on it in a child pytest, the way
tests/test_hostsim_phase_cpu.py does for the snow / rain partition.  The kernel copies the target table to LDS behind one
workgroup barrier, so the unit runs on fibers (its one ``extern __shared__`` declaration becomes the launch's LDS block); there
is no other traffic between lanes.  The entry point is not in ``_capi.SIGNATURES``, from which the simulation's library handle
takes its ``argtypes``: the wrapper converts every argument itself (kernels._ext_call), which this run exercises.  The second
half builds the unit's stand-alone program (tests/hostsim/standalone/analog_driver.cpp: its own main, g++
-fsanitize=address,undefined, nothing loaded into Python) that calls the entry point on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

simdevice.UNIT_LIBRARIES["analog"] = (("analog",), ("analog",), "analog_driver.cpp")
simdevice.UNIT_LIBRARY_FIBER_UNITS["analog"] = 1
GPU_MODULES = ["tests/test_gpu_analog.py", "tests/test_gpu_analog_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "analog", tmp_path_factory.mktemp("hostsim_analog")))


def test_is_simulated(sim):
    assert hasattr(ctypes.CDLL(sim.path), "xh_analog")
    assert sim.lib.xh_analog is not None and sim.lib.xh_analog.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=25)


def test_standalone_sanitizer_run(tmp_path):
    """The entry point under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands' sizes:
    every method on 1, 65 and 260 cells in both dtypes, the limits of the header and one past each (exit status 4: a property
    that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "analog", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
