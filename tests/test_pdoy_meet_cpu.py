"""tests/test_gpu_pdoy_meet.py WITHOUT a GPU: the whole module in a child pytest against the host simulation (tests/hostsim:
quantile.hip is a fibre unit, so the waves of a workgroup, their barrier and their votes run as written), built once per
session the way tests/test_hostsim_cpu.py builds it.  No other CPU test runs k_pdoy_slide at forced chunk lengths."""
import os
import shutil
import subprocess
import sys

import pytest


@pytest.fixture(scope="module")
def sim_lib(tmp_path_factory):
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:   # (a unit that no longer compiles is tests/test_hostsim_cpu.py::test_the_simulation_builds's failure)
        pytest.skip("host simulation not built here: no g++")
    return simdevice.build_shared(str(tmp_path_factory.getbasetemp()))


def test_the_meeting_chunks_module_on_the_simulation(sim_lib):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, XH_TEST_DEVICE="hostsim", HOSTSIM_LIB=sim_lib)
    cmd = [sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "--timeout", "600", "tests/test_gpu_pdoy_meet.py"]
    try:   # (the tests are independent and seeded one by one: four workers where pytest-xdist is installed)
        import xdist  # noqa: F401

        cmd += ["-n", str(min(4, os.cpu_count() or 1))]
    except ImportError:
        pass
    res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True)
    tail = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else res.stderr[-500:]
    assert res.returncode == 0, res.stdout[-3000:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= 166, tail
