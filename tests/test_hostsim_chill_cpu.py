"""tests/test_gpu_chill.py WITHOUT a GPU.  chill.hip has one lane per (cell, period) and no traffic between lanes, so it runs
thread by thread on the host simulation (tests/hostsim).  This module builds it, unchanged, into a small simulation library of
its own with the helpers of tests/hostsim/simdevice.py — chill.hip, pet.hip (xh_solar_table gives the day lengths) and
sim_runtime.cpp; the shared library of tests/test_hostsim_cpu.py is left as it is — and re-runs the whole GPU module on it in
a child pytest, the way that module re-runs the other units': the golden cases of the reference through both entry points,
the edge shapes, the padded views, the adapter."""
import os
import shutil
import subprocess

import pytest

from test_hostsim_cpu import _child_run

UNITS = ("chill", "pet")

# What the child run leaves out, and why.
DESELECTED = {
    "tests/test_gpu_chill.py::test_30_years_1440x8_fused_against_restatement":
        "too slow on a CPU (30 years x 11 520 cells x 24 hours), and its fields come from xh_fill_synthetic, which this library does not hold",
}


def build(workdir: str) -> str:
    """g++ the sources of UNITS + sim_runtime.cpp into workdir/libxclimhip_hostsim_chill.so, with the flags of simdevice.build."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC]
    objs = sd._compile_all(UNITS, workdir, flags)
    out = os.path.join(workdir, "libxclimhip_hostsim_chill.so")
    subprocess.run(["g++", "-shared", "-o", out, *objs], check=True)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:
        pytest.skip("host simulation not built here: no g++")
    try:
        path = build(str(tmp_path_factory.mktemp("hostsim_chill")))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"chill.hip no longer compiles for the host simulation: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
    return simdevice.SimDevice(path)


def test_chill_is_simulated(sim):
    import ctypes

    dll = ctypes.CDLL(sim.path)
    for name in ("xh_chill_hourly", "xh_chill_daily", "xh_solar_table"):
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_chill_module_on_the_simulation(sim):
    _child_run(sim, ["tests/test_gpu_chill.py"], deselect=sorted(DESELECTED), at_least=76)
