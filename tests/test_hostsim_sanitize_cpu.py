"""The 22 entry points of fire.hip, ffdi.hip, pet.hip, stdidx.hip, f64red.hip and f64run.hip under AddressSanitizer and
UndefinedBehaviorSanitizer, WITHOUT a GPU and without Python in the sanitized process (tests/hostsim/standalone).

tests/hostsim/simdevice.py builds san_driver (the rewritten unit sources + sim_runtime.cpp + standalone/san_driver.cpp, all with
-g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all; nothing is preloaded).  The checks of tests/newunit_cases.py —
the ones tests/test_gpu_edges_new_units.py runs on the device, with the seeded generators of the GPU tests — run here on a
ReplayDevice: every call of one of the 22 entry points becomes a case directory (a manifest and the raw arrays), the driver
copies each array into a malloc block of EXACTLY its size, calls the entry point through the C ABI and dumps the blocks.  A
case must end with exit status 0 and no sanitizer report, and the dumped outputs then pass the same comparisons with the
restatements (ffdicpu, petcpu, spicpu, firecpu, oracle) at the GPU tests' tolerances: a clean run with wrong numbers fails.

Row widths 1, 2, 3, 63, 65, 130, 257 (and 131 for the float64 marches: two cells per lane on even widths, one on odd ones —
hostargs.h's xh_pick_vec64 — each with an odd tail); k_percentile_doy_f64 runs on ucontext fibers that are announced to ASan
(simt.h), so every kernel of the six units gets both sanitizers.  Run plainly (one process): the last test reads what the
others replayed."""
import shutil
import subprocess

import numpy as np
import pytest

import newunit_cases as nc

WIDTHS = [1, 2, 3, 63, 65, 130, 257]
F64_WIDTHS = WIDTHS + [131]


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    from tests.hostsim import simdevice

    if shutil.which("g++") is None:
        pytest.skip("no g++")
    # (a compile error is a failure here, never a skip: subprocess.CalledProcessError propagates)
    # (the whole simulation library — shared with tests/test_hostsim_cpu.py: the public functions also call entry points of the
    # older units, which run in this process — is built while the driver compiles)
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(2) as pool:
        lib = pool.submit(simdevice.build_shared, str(tmp_path_factory.getbasetemp()))
        driver = pool.submit(simdevice.build_standalone, str(tmp_path_factory.mktemp("san_driver")))
        lib, driver = lib.result(), driver.result()
    return simdevice.ReplayDevice(lib, driver, str(tmp_path_factory.mktemp("san_cases")))


@pytest.fixture
def native(monkeypatch):
    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "native")


def test_the_driver_aborts_on_a_one_element_over_read(san, tmp_path):
    """The net itself: a field handed over one element short (T * C - 1 values for a (T, C) call) must end in a heap-buffer-overflow
    report — the exact-size blocks are what makes the clean runs below mean something."""
    from tests.hostsim import simdevice

    T, C = 4, 3
    case = tmp_path / "short"
    case.mkdir()
    (case / "b0.in").write_bytes(np.ones(T * C - 1, np.float32).tobytes())
    (case / "b1.in").write_bytes(np.ones(T * C, np.float32).tobytes())
    (case / "b2.in").write_bytes(np.zeros(T * C, np.float32).tobytes())
    (case / "manifest.txt").write_text("entry xh_overwintering_dc\nbuf b0 %d\nbuf b1 %d\nbuf b2 %d\narg ctx\narg p b0 0\narg p b1 0\n"
                                       "arg i %d\narg d 0.75\narg d 0.75\narg d 15\narg p b2 0\n" % (4 * (T * C - 1), 4 * T * C, 4 * T * C, T * C))
    res = subprocess.run([san.lib._driver, str(case)], capture_output=True, text=True)
    assert res.returncode != 0 and "heap-buffer-overflow" in res.stderr, res.stderr[-2000:]
    assert simdevice.STANDALONE_SANITIZE == "address,undefined"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mcarthur(san, dtype):
    for C in WIDTHS:
        nc.check_mcarthur(san, 60, (C,), dtype)
    for T in (1, 19, 20, 21):   # the 20-day window of the drought factor
        nc.check_mcarthur(san, T, (3,), dtype, "discrete")
        nc.check_mcarthur(san, T, (65,), dtype)
    nc.check_mcarthur(san, 21, (2,), dtype, all_nan=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_pet_daily_and_monthly(san, dtype):
    """75 days from mid-March (three calendar months, the outer two cut), all six methods."""
    for method in nc.PET_METHODS:
        nc.check_pet(san, method, dtype, (65,))
        nc.check_pet(san, method, dtype, (3,), T=1)
    for C in WIDTHS:
        nc.check_pet(san, "FAO_PM98" if dtype == np.float32 else "HG85", dtype, (C,))
        nc.check_pet(san, "TW48" if dtype == np.float32 else "DA02", dtype, (C,))


@pytest.mark.parametrize("staging", ["global", "lds"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_standardized_index_kernels(san, dtype, staging):
    """36 monthly steps in 12 groups, and 9 steps in 3 groups of 3 values; gamma APP, gamma ML with floc = 0 (zero-inflated), one
    fisk ML (23 values per group: a 3-parameter fit of 3 values has no maximum to compare); the sample staged in LDS (a heap block of exactly the launch's size) and in the global work buffer."""
    for C in WIDTHS:
        nc.check_si_kernels(san, dtype, C, 36, 12, "gamma", "ML", 0.0, True, staging)
    nc.check_si_kernels(san, dtype, 65, 36, 12, "gamma", "APP", 0.0, False, staging)
    nc.check_si_kernels(san, dtype, 3, 9, 3, "gamma", "ML", 0.0, True, staging)
    nc.check_si_kernels(san, dtype, 3, 9, 3, "gamma", "APP", 0.0, False, staging)
    nc.check_si_kernels(san, dtype, 3, 276, 12, "fisk", "ML", None, False, staging)
    nc.check_si_kernels(san, dtype, 3, 36, 12, "gamma", "ML", 0.0, True, staging, all_nan=True)


def test_standardized_index_public(san, native):
    for dtype in (np.float32, np.float64):
        nc.check_si_public(san, dtype, (65,))
        nc.check_si_public(san, dtype, (3,), months=1)
        nc.check_si_public(san, dtype, (2,), all_nan=True)


@pytest.mark.parametrize("mode", sorted(nc.FIRE_MODES))
def test_fire_weather(san, mode):
    for T, C in ((1, 3), (2, 63), (37, 65), (37, 1), (2, 130), (1, 257), (37, 2)):
        nc.check_fire(san, T, C, mode)
    nc.check_fire(san, 37, 3, mode, all_nan=True)


def test_float64_reductions(san, native):
    for C in F64_WIDTHS:   # (the float32 / float64 mixed pairs on the widths of both lane layouts only)
        nc.check_f64_reductions(san, (C,), 60, mixed=C in (1, 2, 130, 131))
    nc.check_f64_reductions(san, (3,), 1)
    nc.check_f64_reductions(san, (2,), 40, all_nan=True)


def test_float64_run_lengths(san, native):
    for C in F64_WIDTHS:
        nc.check_f64_runs(san, (C,), 60)
    nc.check_f64_runs(san, (3,), 1)
    nc.check_f64_runs(san, (2,), 40, all_nan=True)
    # 17 periods: enough workgroups x periods for the two-cells-per-lane form of k_spell_runs_f64 on the simulation's 2 CUs
    nc.check_f64_runs(san, (130,), 500)


def test_float64_rolling(san, native):
    for C in F64_WIDTHS:   # (mean and var are the sum's and the std's kernels with one more division: the edges file runs them)
        nc.check_f64_rolling(san, C, 40, windows=(1, 8, 9, 31), reducers=("sum", "min", "max", "std"))
    nc.check_f64_rolling(san, 2, 1, windows=(1, 8))
    nc.check_f64_rolling(san, 3, 40, windows=(9,), reducers=("sum", "std"), all_nan=True)


@pytest.mark.parametrize("years, window", [(2, 5), (2, 31), (5, 5), (5, 31)])
def test_float64_percentile_doy(san, native, years, window):
    for C in (1, 2, 3, 65):
        nc.check_f64_percentile_doy_days(san, C, years, window)
    nc.check_f64_percentile_doy_days(san, 2, years, window, all_nan=True)


def test_float64_warm_spells_against_a_day_of_year_table(san, native):
    """xh_run_stats_doy_f64 (through warm_spell_duration_index) on both lane layouts.  The whole-year percentile table is only its
    input: those launches (365 workgroups on fibers, half a minute under ASan) run in this process, the sanitized ones are
    test_float64_percentile_doy's."""
    san.lib.in_process = ("xh_percentile_doy_f64",)
    try:
        for C in (2, 3, 130, 131):
            nc.check_f64_percentile_doy(san, (C,), 2, 5)
        nc.check_f64_percentile_doy(san, (2,), 2, 5, all_nan=True)
    finally:
        san.lib.in_process = ()


_RAN = set()


@pytest.fixture(autouse=True)
def _note_what_ran(request):
    yield
    _RAN.add(request.node.originalname)


def test_every_entry_point_ran_sanitized_on_every_width(san, request):
    """The tally of the module: all 22 entry points ran sanitized, each on every row width.  It needs the other tests of this
    module to have run in this process; selected alone, or with the module spread over xdist workers, it checks only that what
    did run belongs to the 22."""
    from tests.hostsim import simdevice

    ran = san.lib.replayed
    assert set(ran) <= set(simdevice.NEW_ENTRY_POINTS)
    siblings = {i.originalname for i in request.session.items if i.module is request.module} - {request.node.originalname}
    if not siblings <= _RAN:
        return
    assert sorted(ran) == sorted(simdevice.NEW_ENTRY_POINTS), sorted(set(simdevice.NEW_ENTRY_POINTS) - set(ran))
    for name in ("xh_mcarthur", "xh_pet_daily", "xh_pet_monthly", "xh_si_fit", "xh_si_apply", "xh_si_fit_f64", "xh_si_apply_f64",
                 "xh_fire_weather"):
        assert {a[1] for a in ran[name]} >= set(WIDTHS), name
    assert {a[0] for a in ran["xh_overwintering_dc"]} >= set(WIDTHS)   # (its one size is the number of cells)
    for name in ("xh_thresholded_reduce_f64", "xh_range_reduce_f64", "xh_domain_count_f64", "xh_bivariate_count_f64",
                 "xh_rolling_reduce_f64", "xh_compare_map_f64", "xh_run_stats_f64", "xh_spell_mask_f64", "xh_spell_run_stats_f64"):
        assert {a[1] for a in ran[name]} >= set(F64_WIDTHS), name
