"""The compound-extreme unit WITHOUT a GPU: tests/hostsim/simdevice.py builds compound.hip, unchanged but for the declaration of
its dynamic LDS, into a small simulation library, and this module re-runs tests/test_gpu_compound.py,
tests/test_gpu_compound_footprint.py and tests/test_gpu_compound_adapter.py on it in a child pytest, the way
tests/test_hostsim_partition_cpu.py does for the partitioning unit.  The ring of k_blowing_snow is dynamic LDS in lane-private
columns, so the unit is compiled like rainseason.hip: on fibers, the LDS of a launch a heap block of exactly its size.  The library
also holds the units of the entry points the mirror calls beside its own: the period counts of the missing mask (reduce.hip,
f64.hip with tcount.hip and window.hip) and the re-gridding of a 365-row table (xh_doy_interp of quantile.hip, which links against
core.hip and the three pdoy units).  The second half
builds the unit's stand-alone program (tests/hostsim/standalone/compound_driver.cpp: its own main, g++
-fsanitize=address,undefined, nothing loaded into Python) that calls the four entry points on exact-size heap blocks."""
import ctypes
import subprocess

import pytest

from test_hostsim_cpu import _child_run
from test_hostsim_units_cpu import _built
from tests.hostsim import simdevice

simdevice.UNIT_LIBRARIES["compound"] = (("compound", "f64", "reduce", "tcount", "window", "quantile", "core", "pdoy_top", "pdoy_walk", "pdoy_quad"), ("compound",),
                                        "compound_driver.cpp")
simdevice.UNIT_LIBRARY_FIBER_UNITS["compound"] = 1
simdevice.UNIT_DEFINES["compound"] = ["-DSIM_EXACT_DYN_LDS=1"]
GPU_MODULES = ["tests/test_gpu_compound.py", "tests/test_gpu_compound_footprint.py", "tests/test_gpu_compound_adapter.py"]
ENTRY_POINTS = ("xh_compound_doy_days", "xh_degree_exceedance_date", "xh_blowing_snow_days", "xh_pair_period_sum")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, "compound", tmp_path_factory.mktemp("hostsim_compound")))


def test_is_simulated(sim):
    dll = ctypes.CDLL(sim.path)
    assert all(hasattr(dll, n) for n in ENTRY_POINTS + ("xh_resample_reduce", "xh_resample_reduce_f64", "xh_doy_interp"))
    assert sim.lib.xh_compound_doy_days.argtypes is None   # (no prototype from SIGNATURES: the wrapper's job)
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_rain_season


def test_the_known_answers_on_the_simulation(sim):
    from test_compound_cpu import check_known_answers, mirror_api

    check_known_answers(mirror_api(sim))


def test_the_gpu_modules_on_the_simulation(sim):
    _child_run(sim, GPU_MODULES, at_least=120)


def test_standalone_sanitizer_run(tmp_path):
    """The four entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly the operands'
    sizes: 1, 65, 130 and 132 cells, both dtypes, all 15 output sets, the start row on the first and on the last row of a period
    and absent, windows 1, 2 and 32 (exit status 4: a property that needs no reference does not hold)."""
    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, "compound", tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
