"""tests/test_gpu_rain.py and tests/test_gpu_rain_adapter.py WITHOUT a GPU.  rainseason.hip is built, unchanged, into a small
simulation library of its own with the helpers of tests/hostsim/simdevice.py — rainseason.hip, f64.hip and reduce.hip + tcount.hip + window.hip (the period
minima of hardiness_zones and the counts of the missing mask) and sim_runtime.cpp; the shared library of tests/test_hostsim_cpu.py
is left as it is.  The ring of k_rain_season is dynamic LDS, so rainseason.hip is compiled like the fiber units of the
simulation (tests/hostsim/simt.h): its dynamic LDS declaration becomes a pointer to the workgroup's LDS block, which is a heap
block of exactly the launch's size.  The two GPU modules are re-run on it in a child pytest.  The second half builds a
stand-alone program (its own main, g++ -fsanitize=address,undefined, nothing loaded into Python) that calls the two entry points
on exact-size heap blocks at the limit windows."""
import os
import shutil
import subprocess

import pytest

from test_hostsim_cpu import _child_run

UNITS = ("f64", "reduce", "tcount", "window")   # (reduce.hip links against the launchers of tcount.hip, f64.hip against window.hip)
ENTRY_POINTS = ("xh_rain_season", "xh_rolling_zones")

HERE = os.path.dirname(os.path.abspath(__file__))


def _compile_rain(sd, workdir, flags):
    """rainseason.hip as a fiber unit: the rewrite simdevice._prepare_unit gives the units of its FIBER_UNITS list."""
    text = open(os.path.join(sd.CSRC, "rainseason.hip")).read()
    text, nsub = sd._DYN_LDS.subn(lambda m: f"{m.group(1)}* {m.group(2)} = ({m.group(1)}*)sim_dynamic_lds();", text)
    if nsub != 1:
        raise RuntimeError("rainseason.hip: the `extern __shared__` declaration the simulation rewrites has changed")
    src, obj = os.path.join(workdir, "rainseason.sim.cpp"), os.path.join(workdir, "rainseason.o")
    open(src, "w").write(text)
    subprocess.run(["g++", "-x", "c++", *flags, "-DSIM_FIBERS=1", "-D__shared__=static", "-DSIM_EXACT_DYN_LDS=1", "-c", src, "-o", obj],
                   check=True, capture_output=True, text=True)
    return obj


def build(workdir: str) -> str:
    """g++ rainseason.hip (on fibers), the sources of UNITS and sim_runtime.cpp into workdir/libxclimhip_hostsim_rain.so."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC]
    objs = [_compile_rain(sd, workdir, flags)] + sd._compile_all(UNITS, workdir, flags)
    out = os.path.join(workdir, "libxclimhip_hostsim_rain.so")
    subprocess.run(["g++", "-shared", "-o", out, *objs], check=True)
    return out


def build_driver(workdir: str) -> str:
    """The stand-alone sanitizer program: rainseason.hip + sim_runtime.cpp + tests/hostsim/standalone/rain_driver.cpp, all with
    -fsanitize=address,undefined -fno-sanitize-recover=all, the sanitizer runtimes linked statically."""
    from tests.hostsim import simdevice as sd

    os.makedirs(workdir, exist_ok=True)
    sd._prepare_headers(workdir)
    flags = ["-std=c++17", "-g", "-fno-var-tracking", "-O1", "-ffp-contract=off", f"-fsanitize={sd.STANDALONE_SANITIZE}",
             "-fno-sanitize-recover=all", "-I", workdir, "-I", sd.HERE, "-I", sd.CSRC, "-I", os.path.join(sd.ROOT, "include")]
    objs = [_compile_rain(sd, workdir, flags)] + sd._compile_all((), workdir, flags, sd.STANDALONE_SANITIZE)
    out = os.path.join(workdir, "rain_driver")
    subprocess.run(["g++", *flags, "-static-libasan", "-static-libubsan", "-o", out,
                    os.path.join(sd.HERE, "standalone", "rain_driver.cpp"), *objs], check=True)
    return out


_SIM = []


def sim_device(tmp_path_factory):
    """The SimDevice of one build per test session; skips without g++."""
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:
        pytest.skip("host simulation not built here: no g++")
    if not _SIM:
        try:
            path = build(str(tmp_path_factory.mktemp("hostsim_rain")))
        except subprocess.CalledProcessError as e:
            pytest.fail(f"rainseason.hip no longer compiles for the host simulation: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
        _SIM.append(simdevice.SimDevice(path))
    return _SIM[0]


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return sim_device(tmp_path_factory)


def test_rainseason_is_simulated(sim):
    import ctypes

    dll = ctypes.CDLL(sim.path)
    for name in ENTRY_POINTS + ("xh_resample_reduce", "xh_resample_reduce_f64"):
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_known_answers_on_the_simulation(sim):
    from test_rain_cpu import check_known_answers, mirror_api

    check_known_answers(mirror_api(sim))


def test_the_rain_modules_on_the_simulation(sim):
    _child_run(sim, ["tests/test_gpu_rain.py", "tests/test_gpu_rain_adapter.py"], at_least=90)


def test_standalone_sanitizer_run(tmp_path):
    """The two entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly T * C
    elements: periods on row 0 and on row T - 1, empty periods, periods shorter than every window, all four method
    combinations, the sum windows at 1 and at the limit of 32 (the largest ring), a per-day dry window beyond the ring (the
    second read of the decision row), float32 and float64; 1, 65 and 260 cells; the zones with windows 1, 30 and one longer than
    the series.  The program checks that every call returns XH_OK and a few properties that need no reference (exit status 4
    otherwise); a sanitizer report aborts it."""
    if shutil.which("g++") is None:
        pytest.skip("stand-alone sanitizer program not built here: no g++")
    try:
        driver = build_driver(str(tmp_path))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the stand-alone rain driver does not build: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
