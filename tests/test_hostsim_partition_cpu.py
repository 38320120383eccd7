"""The uncertainty-partitioning unit WITHOUT a GPU: tests/hostsim/simdevice.py builds partition.hip, unchanged, into a small
simulation library, and this module re-runs tests/test_gpu_partition.py, tests/test_gpu_partition_footprint.py and
tests/test_gpu_partition_adapter.py on it in a child pytest, the way tests/test_hostsim_robust_cpu.py does for the robustness unit.
The unit has no LDS and no traffic between lanes, so its kernels run thread by thread.  The second half builds the unit's
stand-alone program (tests/hostsim/standalone/partition_driver.cpp: its own main, g++ -fsanitize=address,undefined, nothing
loaded into Python) that calls the three entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

simdevice.UNIT_LIBRARIES["partition"] = (("partition",), ("partition",), "partition_driver.cpp")
GPU_MODULES = ["tests/test_gpu_partition.py", "tests/test_gpu_partition_footprint.py", "tests/test_gpu_partition_adapter.py"]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "partition", tmp_path_factory.mktemp("hostsim_partition")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert all(hasattr(dll, n) for n in ("xh_partition_smooth", "xh_partition_components", "xh_ensemble_stats"))
    assert sim.lib.xh_partition_smooth.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):
        sim.lib.xh_fill_synthetic


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=60)


def test_standalone_sanitizer_run(tmp_path):
    """The three entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes: 1, 65 and 130 cells, both dtypes, every degree and both windows, a given sm, both baselines, with the optional outputs
    NULL in turn (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "partition", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
