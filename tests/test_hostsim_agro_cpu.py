"""tests/test_gpu_agro.py and tests/test_gpu_agro_adapter.py WITHOUT a GPU.  agro.hip has one lane per (cell, period) or per
cell and no traffic between lanes, so it runs thread by thread on the host simulation (tests/hostsim).  This module builds it,
unchanged, into a small simulation library of its own with the helpers of tests/hostsim/simdevice.py — agro.hip, pet.hip (the
solar table behind the Gladstones and Jones coefficients), f64.hip (xh_resample_reduce_f64 of the warmest-month cross-check) and
sim_runtime.cpp — and re-runs the two GPU modules on it in a child pytest.  The second half builds a stand-alone program (its
own main, g++ -fsanitize=address,undefined, nothing loaded into Python) that calls the five entry points on exact-size heap
blocks."""
import os
import shutil
import subprocess

import pytest

from test_hostsim_cpu import _child_run

UNITS = ("agro", "pet", "f64")
ENTRY_POINTS = ("xh_agro_degree_sum", "xh_agro_monthly", "xh_egdd", "xh_corn_heat_units", "xh_qian_wma")

# What the child run leaves out, and why.
DESELECTED = {}

HERE = os.path.dirname(os.path.abspath(__file__))


def build(workdir: str) -> str:
    """g++ the sources of UNITS + sim_runtime.cpp into workdir/libxclimhip_hostsim_agro.so, with the flags of simdevice.build."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC]
    objs = sd._compile_all(UNITS, workdir, flags)
    out = os.path.join(workdir, "libxclimhip_hostsim_agro.so")
    subprocess.run(["g++", "-shared", "-o", out, *objs], check=True)
    return out


def build_driver(workdir: str) -> str:
    """The stand-alone sanitizer program: agro.hip + sim_runtime.cpp + tests/hostsim/standalone/agro_driver.cpp, all with
    -fsanitize=address,undefined -fno-sanitize-recover=all, the sanitizer runtimes linked statically."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-g", "-fno-var-tracking", "-O1", "-ffp-contract=off", f"-fsanitize={sd.STANDALONE_SANITIZE}",
             "-fno-sanitize-recover=all", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC, "-I", os.path.join(sd.ROOT, "include")]
    objs = sd._compile_all(("agro",), workdir, flags, sd.STANDALONE_SANITIZE)
    out = os.path.join(workdir, "agro_driver")
    subprocess.run(["g++", *flags, "-static-libasan", "-static-libubsan", "-o", out,
                    os.path.join(sd.HERE, "standalone", "agro_driver.cpp"), *objs], check=True)
    return out


_SIM = []


def sim_device(tmp_path_factory):
    """The SimDevice of one build per test session, shared with tests/test_agro_cpu.py (which takes its refusals from it); skips
    without g++."""
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:
        pytest.skip("host simulation not built here: no g++")
    if not _SIM:
        try:
            path = build(str(tmp_path_factory.mktemp("hostsim_agro")))
        except subprocess.CalledProcessError as e:
            pytest.fail(f"agro.hip no longer compiles for the host simulation: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
        _SIM.append(simdevice.SimDevice(path))
    return _SIM[0]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return sim_device(tmp_path_factory)


def test_agro_is_simulated(sim):
    import ctypes

    dll = ctypes.CDLL(sim.path)
    for name in ENTRY_POINTS + ("xh_solar_table", "xh_resample_reduce_f64"):
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_agro_modules_on_the_simulation(sim):
    _child_run(sim, ["tests/test_gpu_agro.py", "tests/test_gpu_agro_adapter.py"], deselect=sorted(DESELECTED), at_least=170)


def test_standalone_sanitizer_run(tmp_path):
    """The five entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly T * C
    elements: the series that starts mid-year (1999-03-15 + 1002 days), a one-row series, the Qian stencil at both series ends
    (xh_qian_wma and the "qian" start of xh_egdd on periods that touch row 0 and row T - 1), and a season span that ends on the
    last row; float32 and float64.  The program checks that every call returns XH_OK and a few properties that need no reference
    (exit status 4 otherwise); a sanitizer report aborts it."""
    if shutil.which("g++") is None:
        pytest.skip("stand-alone sanitizer program not built here: no g++")
    try:
        driver = build_driver(str(tmp_path))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the stand-alone agro driver does not build: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
