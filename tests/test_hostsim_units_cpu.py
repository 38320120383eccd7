"""The GPU modules of the units that have a simulation library of their own WITHOUT a GPU: tests/test_gpu_chill.py,
tests/test_gpu_bioclim.py (+ the ANUCLIM adapter), tests/test_gpu_agro*.py, tests/test_gpu_hydro*.py and tests/test_gpu_rain*.py.
tests/hostsim/simdevice.py builds each unit, unchanged, into a small library (UNIT_LIBRARIES there says what each holds and why)
and this module re-runs the unit's GPU modules on it in a child pytest, the way tests/test_hostsim_cpu.py re-runs the other
units': the golden cases of the reference, the edge shapes, the padded views, the adapters.  The second half builds each
unit's stand-alone program (its own main, g++ -fsanitize=address,undefined, nothing loaded into Python) that calls the unit's
entry points on exact-size heap blocks."""
import shutil
import subprocess

import pytest

from test_hostsim_cpu import _child_run

# unit -> (the entry points that must resolve: the unit's own and those of the units linked with it,
#          the GPU modules of the child run, the least number of tests that must pass there: the unit's own and, where
#          tests/test_gpu_footprint.py has cases on the unit's entry points, those)
UNITS = {
    "chill": (("xh_chill_hourly", "xh_chill_daily", "xh_solar_table"), ["tests/test_gpu_chill.py", "tests/test_gpu_footprint.py"], 76 + 4),
    "bioclim": (("xh_bioclim", "xh_resample_reduce_f64", "xh_range_reduce_f64"),
                ["tests/test_gpu_bioclim.py", "tests/test_gpu_anuclim_adapter.py", "tests/test_gpu_footprint.py"], 55 + 4),
    "agro": (("xh_agro_degree_sum", "xh_agro_monthly", "xh_egdd", "xh_corn_heat_units", "xh_qian_wma", "xh_solar_table", "xh_resample_reduce_f64"),
             ["tests/test_gpu_agro.py", "tests/test_gpu_agro_adapter.py", "tests/test_gpu_footprint.py"], 170 + 12),
    "hydro": (("xh_flow_period_stats", "xh_melt_period_max", "xh_antecedent_precip", "xh_sen_slope",
               "xh_resample_reduce", "xh_resample_reduce_f64", "xh_threshold_count_doy", "xh_nan_quantile_f64"),
              ["tests/test_gpu_hydro.py", "tests/test_gpu_hydro_adapter.py", "tests/test_gpu_footprint.py"], 100 + 20),
    "rain": (("xh_rain_season", "xh_rolling_zones", "xh_resample_reduce", "xh_resample_reduce_f64"),
             ["tests/test_gpu_rain.py", "tests/test_gpu_rain_adapter.py", "tests/test_gpu_footprint.py"], 90 + 6),
}

# What the child runs leave out, and why.
DESELECTED = {
    "tests/test_gpu_chill.py::test_30_years_1440x8_fused_against_restatement":
        "too slow on a CPU (30 years x 11 520 cells x 24 hours), and its fields come from xh_fill_synthetic, which this library does not hold",
    "tests/test_gpu_hydro.py::test_quantile_indices_against_restatement[float32]":
        "the float32 whole-series quantile goes through the selection kernels (quantile.hip, select*.hip), which this library does not hold",
}


def _built(what: str, build, name: str, workdir) -> str:
    """build(name, workdir) of simdevice; skips without g++, and a unit that no longer compiles FAILS with the compiler's words."""
    if shutil.which("g++") is None:
        pytest.skip(f"{what} not built here: no g++")
    try:
        return build(name, str(workdir))
    except subprocess.CalledProcessError as e:
        pytest.fail(f"{what} of {name} no longer builds: {' '.join(map(str, e.cmd))[-400:]}\n{(e.stderr or '')[-2000:]}")


_SIM = {}


def sim_device(name: str, tmp_path_factory):
    """The SimDevice of one library build per test session and unit, shared with tests/test_agro_cpu.py and
    tests/test_hydro_cpu.py (which take their refusals from it); skips without g++."""
    from tests.hostsim import simdevice

    if name not in _SIM:
        _SIM[name] = simdevice.SimDevice(_built("the host simulation", simdevice.build_unit_library, name, tmp_path_factory.mktemp(f"hostsim_{name}")))
    return _SIM[name]


@pytest.fixture(params=list(UNITS))
def unit(request):
    return request.param


@pytest.fixture
def sim(unit, tmp_path_factory):
    return sim_device(unit, tmp_path_factory)


def test_is_simulated(unit, sim):
    import ctypes

    dll = ctypes.CDLL(sim.path)
    for name in UNITS[unit][0]:
        assert hasattr(dll, name), name
        assert getattr(sim.lib, name) is not None
    with pytest.raises(NotImplementedError, match="not simulated"):   # what the library does not hold raises, never a no-op
        sim.lib.xh_fill_synthetic


def test_the_known_answers_of_rain_on_the_simulation(tmp_path_factory):
    from test_rain_cpu import check_known_answers, mirror_api

    check_known_answers(mirror_api(sim_device("rain", tmp_path_factory)))


def test_the_gpu_modules_on_the_simulation(unit, sim):
    _, files, at_least = UNITS[unit]
    # (of tests/test_gpu_footprint.py: the cases whose entry points this library holds, by their id "<unit>-...")
    _child_run(sim, files, skip=f"footprint and not {unit}-", deselect=sorted(d for d in DESELECTED if d.split("::")[0] in files),
               at_least=at_least)


# Every program runs its entry points under AddressSanitizer and UBSan in a process of its own, on malloc blocks of exactly
# T * C elements, checks that every call returns XH_OK and a few properties that need no reference (exit status 4 otherwise);
# a sanitizer report aborts it.
@pytest.mark.parametrize("unit", [
    # xh_bioclim: the series that starts mid-year (the lead-in before the first step of a period is where a read before the
    # block would hide; the last bin of one day where a read past it would) and the series shorter than 13 weeks, float32 and
    # float64, every output requested, and the quarter outputs alone; the short series gives NaN quarters and step indices of -1
    "bioclim",
    # the five entry points: the series that starts mid-year (1999-03-15 + 1002 days), a one-row series, the Qian stencil at both
    # series ends (xh_qian_wma and the "qian" start of xh_egdd on periods that touch row 0 and row T - 1), and a season span
    # that ends on the last row; float32 and float64
    "agro",
    # the four entry points: periods that touch row 0 and row T - 1 (the 7-day window, the melt window and the API halo all reach
    # for rows outside the series there), series shorter than the windows, the largest window, Sen series of 2, 3, 64 and the
    # largest number of years with absent years; float32 and float64; 1, 65 and 260 cells
    "hydro",
    # the two entry points: periods on row 0 and on row T - 1, empty periods, periods shorter than every window, all four method
    # combinations, the sum windows at 1 and at the limit of 32 (the largest ring), a per-day dry window beyond the ring (the
    # second read of the decision row), float32 and float64; 1, 65 and 260 cells; the zones with windows 1, 30 and one longer
    # than the series
    "rain",
])
def test_standalone_sanitizer_run(unit, tmp_path):
    from tests.hostsim import simdevice

    driver = _built("the stand-alone sanitizer program", simdevice.build_unit_driver, unit, tmp_path)
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, f"exit status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "cases clean" in res.stdout, res.stdout[-2000:]
