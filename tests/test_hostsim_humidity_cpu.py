"""The humidity, heat-stress and wind unit WITHOUT a GPU: tests/hostsim/simdevice.py builds humidity.hip, unchanged, into a small
simulation library, and this module re-runs tests/test_gpu_humidity.py, tests/test_gpu_humidity_footprint.py and
tests/test_gpu_humidity_adapter.py on it in a child pytest, the way tests/test_hostsim_thermal_cpu.py does for the thermal-comfort
unit (thermal.hip is linked too: the adapter module calls ``saturation_vapor_pressure``).  Both kernels are element-wise, without
LDS and without traffic between lanes: thread by thread.  The entry points are not in ``_capi.SIGNATURES``, from which the
simulation's library handle takes its ``argtypes``: the wrappers convert every argument themselves (kernels._ext_call).  The second
half builds the unit's stand-alone program (tests/hostsim/standalone/humidity_driver.cpp: its own main, g++
-fsanitize=address,undefined, nothing loaded into Python) that calls both entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

simdevice.UNIT_LIBRARIES["humidity"] = (("humidity", "thermal"), ("humidity",), "humidity_driver.cpp")
GPU_MODULES = ["tests/test_gpu_humidity.py", "tests/test_gpu_humidity_footprint.py", "tests/test_gpu_humidity_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "humidity", tmp_path_factory.mktemp("hostsim_humidity")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert hasattr(dll, "xh_air_moisture") and hasattr(dll, "xh_wind_map")
    assert sim.lib.xh_air_moisture.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=40)


def test_standalone_sanitizer_run(tmp_path):
    """Both entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands' sizes:
    3 rows by 1, 3, 4, 5, 65 and 130 cells, both dtypes, every single output with just its fields, the full and the fused sets, every
    e_sat method and case, the four wind operations; fields and outputs a call does not need are NULL (exit status 4: a property
    that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "humidity", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
