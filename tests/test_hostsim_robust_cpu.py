"""The change-robustness unit WITHOUT a GPU: tests/hostsim/simdevice.py builds robust.hip, unchanged, into a small simulation
library, and this module re-runs tests/test_gpu_robust.py, tests/test_gpu_robust_footprint.py and tests/test_gpu_robust_adapter.py
on it in a child pytest, the way
tests/test_hostsim_thermal_cpu.py does for the thermal unit.  xh_robust_coefficient sorts in LDS by the whole wave (barriers), so
the unit is compiled on fibers; a translation unit has one mode, so the lane kernels of xh_change_test and xh_robust_fractions run
on fibers as well (they have no traffic between lanes: the result is that of a thread-by-thread run).  Both `extern __shared__`
declarations are rewritten.  The second half builds the unit's stand-alone program (tests/hostsim/standalone/robust_driver.cpp:
its own main, g++ -fsanitize=address,undefined, nothing loaded into Python) that calls the four entry points on exact-size heap
blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

# f64.hip and reduce.hip + tcount.hip + window.hip: the annual means of a daily reference (xh_resample_reduce, _f64), as in "hydro"
simdevice.UNIT_LIBRARIES["robust"] = (("robust", "f64", "reduce", "tcount", "window"), ("robust",), "robust_driver.cpp")
simdevice.UNIT_LIBRARY_FIBER_UNITS["robust"] = 2
GPU_MODULES = ["tests/test_gpu_robust.py", "tests/test_gpu_robust_footprint.py", "tests/test_gpu_robust_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "robust", tmp_path_factory.mktemp("hostsim_robust")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert all(hasattr(dll, n) for n in ("xh_change_test", "xh_ar6_gamma", "xh_robust_fractions", "xh_robust_coefficient"))
    assert sim.lib.xh_change_test.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):
        sim.lib.xh_fill_synthetic


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=67)


def test_standalone_sanitizer_run(tmp_path):
    """The four entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes: every test on 1, 65 and 130 cells, both staging backings, both dtypes, a ref with and without realizations; fields and
    outputs a call does not need are NULL (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "robust", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
