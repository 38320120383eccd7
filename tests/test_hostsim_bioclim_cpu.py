"""tests/test_gpu_bioclim.py WITHOUT a GPU.  bioclim.hip has one lane per (cell, period) and no traffic between lanes, so it runs
thread by thread on the host simulation (tests/hostsim).  This module builds it, unchanged, into a small simulation library of
its own with the helpers of tests/hostsim/simdevice.py — bioclim.hip, the units of the entry points the cross-checks call
(f64.hip: xh_resample_reduce_f64, f64red.hip: xh_range_reduce_f64) and sim_runtime.cpp — and
re-runs the whole GPU module on it in a child pytest.  The second half builds a stand-alone program (its own main, g++
-fsanitize=address,undefined, nothing loaded into Python) that calls xh_bioclim on exact-size heap blocks."""
import os
import shutil
import subprocess

import pytest

from test_hostsim_cpu import _child_run

UNITS = ("bioclim", "f64", "f64red")

# What the child run leaves out, and why.
DESELECTED = {}

HERE = os.path.dirname(os.path.abspath(__file__))


def build(workdir: str) -> str:
    """g++ the sources of UNITS + sim_runtime.cpp into workdir/libxclimhip_hostsim_bioclim.so, with the flags of simdevice.build."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC]
    objs = sd._compile_all(UNITS, workdir, flags)
    out = os.path.join(workdir, "libxclimhip_hostsim_bioclim.so")
    subprocess.run(["g++", "-shared", "-o", out, *objs], check=True)
    return out


def build_driver(workdir: str) -> str:
    """The stand-alone sanitizer program: bioclim.hip + sim_runtime.cpp + tests/hostsim/standalone/bioclim_driver.cpp, all with
    -fsanitize=address,undefined -fno-sanitize-recover=all, the sanitizer runtimes linked statically."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-g", "-fno-var-tracking", "-O1", "-ffp-contract=off", f"-fsanitize={sd.STANDALONE_SANITIZE}",
             "-fno-sanitize-recover=all", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC, "-I", os.path.join(sd.ROOT, "include")]
    objs = sd._compile_all(("bioclim",), workdir, flags, sd.STANDALONE_SANITIZE)
    out = os.path.join(workdir, "bioclim_driver")
    subprocess.run(["g++", *flags, "-static-libasan", "-static-libubsan", "-o", out,
                    os.path.join(sd.HERE, "standalone", "bioclim_driver.cpp"), *objs], check=True)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:
        pytest.skip("host simulation not built here: no g++")
    try:
        path = build(str(tmp_path_factory.mktemp("hostsim_bioclim")))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"bioclim.hip no longer compiles for the host simulation: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
    return simdevice.SimDevice(path)


def test_bioclim_is_simulated(sim):
    import ctypes

    dll = ctypes.CDLL(sim.path)
    for name in ("xh_bioclim", "xh_resample_reduce_f64", "xh_range_reduce_f64"):
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_bioclim_module_on_the_simulation(sim):
    _child_run(sim, ["tests/test_gpu_bioclim.py", "tests/test_gpu_anuclim_adapter.py"], deselect=sorted(DESELECTED), at_least=55)


def test_standalone_sanitizer_run(tmp_path):
    """xh_bioclim under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly T * C elements: the
    series that starts mid-year (the lead-in before the first step of a period is where a read before the block would hide;
    the last bin of one day where a read past it would) and the series shorter than 13 weeks, float32 and float64, every
    output requested, and the quarter outputs alone.  The program checks that every call returns XH_OK and that the short series
    gives NaN quarters and step indices of -1 (exit status 4 otherwise); a sanitizer report aborts it."""
    if shutil.which("g++") is None:
        pytest.skip("stand-alone sanitizer program not built here: no g++")
    try:
        driver = build_driver(str(tmp_path))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the stand-alone bioclim driver does not build: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
