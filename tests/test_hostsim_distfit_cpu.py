"""The distribution-fit unit WITHOUT a GPU: tests/hostsim/simdevice.py builds distfit.hip, unchanged, into a small simulation library,
and this module re-runs tests/test_gpu_distfit.py and tests/test_gpu_distfit_adapter.py on it in a child pytest, the way
tests/test_hostsim_analog_cpu.py does for the spatial analogues.  k_dist_fit stages every lane's sample in a private LDS column
(lds + threadIdx.x, stride FIT_BLOCK), so the unit runs thread by thread and its one ``extern __shared__`` declaration becomes the
launch's LDS block, as stdidx.hip's does.  The library also holds the units of the entry points frequency_analysis is built on
(the rolling mean and the period extremes).  The entry points are not in ``_capi.SIGNATURES``, from which the simulation's library
handle takes its ``argtypes``: the wrappers convert every argument themselves (kernels._ext_call).  The second half builds the
unit's stand-alone program (tests/hostsim/standalone/distfit_driver.cpp: its own main, g++ -fsanitize=address,undefined, nothing
loaded into Python) that calls both entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

# f64.hip and reduce.hip + tcount.hip + window.hip: the period extremes and the rolling mean (reduce.hip links against the launchers
# of tcount.hip, f64.hip against window.hip)
simdevice.UNIT_LIBRARIES["distfit"] = (("distfit", "f64", "reduce", "tcount", "window"), ("distfit",), "distfit_driver.cpp")
if "distfit" not in simdevice.DYN_LDS_UNITS:
    simdevice.DYN_LDS_UNITS = (*simdevice.DYN_LDS_UNITS, "distfit")
GPU_MODULES = ["tests/test_gpu_distfit.py", "tests/test_gpu_distfit_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "distfit", tmp_path_factory.mktemp("hostsim_distfit")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert hasattr(dll, "xh_dist_fit") and hasattr(dll, "xh_dist_eval")
    assert sim.lib.xh_dist_fit.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_gpu_modules_on_the_simulation(sim):
    # (of tests/test_gpu_footprint.py: the cases on this unit's entry points, by their id "distfit-...")
    _child_run(sim, GPU_MODULES + ["tests/test_gpu_footprint.py"], skip="footprint and not distfit-", at_least=100 + 8)


def test_standalone_sanitizer_run(tmp_path):
    """Both entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands' sizes:
    every distribution and method on 1, 65 and 260 cells in both dtypes, T of 1, 2, 3, 32 and 33, 0, 16 and 17 fused levels
    (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "distfit", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
