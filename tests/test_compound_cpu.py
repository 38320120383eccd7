"""The compound-extreme unit without a GPU (xclim_amd.compound, include/units/xclim_hip_compound.h): the numpy restatement
tests/compoundcpu.py reproduces the known answers of the reference's own tests (tests/golden/compound_known_answers.json) and the
recorded vectors (tests/golden/compound_vectors.npz), the conditions of the random families hold, the mirrors of the header's
``#define``s, the host tables of the mirror against the restatement's own calendar arithmetic, and every ``NotServed`` /
``ValueError`` path, which is taken before a device is asked for.  Also the helpers that tests/test_gpu_compound*.py import."""
import json
import os
import re

import numpy as np
import pytest

import compoundcpu as CC
from oracle import calendar as ocal
from xclim_amd import _capi as capi
from xclim_amd import compound
from xclim_amd import kernels as K
from xclim_amd.calendar import DoyPercentile
from xclim_amd.timeaxis import TimeAxis

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "units", "xclim_hip_compound.h")
KNOWN = json.load(open(os.path.join(HERE, "golden", "compound_known_answers.json")))
_Z = np.load(os.path.join(HERE, "golden", "compound_vectors.npz"))
_META = json.loads(str(_Z["meta"]))
AXES, META = _META["axes"], _META["cases"]
CASES = {kind: [n for n, m in META.items() if m["kind"] == kind] for kind in ("compound", "dded", "snow", "wci")}
COUNTS = tuple(compound.COMPOUND_OUTPUTS)
TABLES = {"cold_and_dry_days": ("tas_lo", "pr_lo"), "warm_and_dry_days": ("tas_hi", "pr_lo"), "warm_and_wet_days": ("tas_hi", "pr_hi"),
          "cold_and_wet_days": ("tas_lo", "pr_hi")}
TABLE_ARGS = {"tas_lo": "tas_per_low", "tas_hi": "tas_per_high", "pr_lo": "pr_per_low", "pr_hi": "pr_per_high"}


class NoDevice:
    """Handed in as ``device=``: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


def same(got, want, what=""):
    """Exactly equal, NaN where NaN: every result of this unit is an integer, a day of year, an exact sum or NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert got.dtype == np.float64, f"{what}: dtype {got.dtype}"
    np.testing.assert_array_equal(got, want, err_msg=what)


def golden_time(axis) -> TimeAxis:
    a = AXES[axis]
    return TimeAxis.daily(a["start"], a["T"], a["calendar"])


def golden_otime(axis):
    a = AXES[axis]
    return CC.otime(a["calendar"], a["start"], a["T"])


def get(name, key):
    return _Z[f"{name}/{key}"]


def tile(a, cells, use=None):
    """The columns ``use`` (default: all) of ``a`` repeated to ``cells`` columns."""
    use = np.arange(a.shape[1]) if use is None else np.asarray(use)
    return np.ascontiguousarray(a[:, use[np.arange(cells) % len(use)]])


# ---- the restatement against the reference's known answers ----------------------------------------------------------------------
def _edited(n, fill, edits):
    x = np.full(n, float(fill))
    for lo, hi, v in edits:
        x[lo:hi] = 0.0 if v == "=0" else x[lo:hi] + v
    return x[:, None]


def check_known_answers(api):
    """``api``: the seven functions as ``f(fields..., time=(calendar, start, n), **kw) -> (P, C)``; the restatement here, the
    mirror on the device in tests/test_gpu_compound.py."""
    for k in KNOWN["compound"]:
        t = ("standard", k["start"], k["n"])
        ot = CC.otime(*t)
        tas, pr = _edited(k["n"], k["tas_fill"], k["tas_edits"]), _edited(k["n"], k["pr_fill"], k["pr_edits"])
        tp, td = ocal.percentile_doy(tas, ot, k["window"], float(k["tas_per"]))
        pp, pd_ = ocal.percentile_doy(pr, ot, k["window"], float(k["pr_per"]))
        out = api[k["function"]](tas, pr, (tp[..., 0], td), (pp[..., 0], pd_), freq=k["freq"], time=t)
        assert out[0, 0] == k["first_value"], k["function"]
    for k in KNOWN["degree_days_exceedance_date"]:
        tas = np.full((k["n"], 1), k["tas_fill"])
        out = api["degree_days_exceedance_date"](tas, thresh=k["thresh_K"], sum_thresh=k["sum_thresh"], op=k["op"], after_date=k["after_date"],
                                                 time=("standard", k["start"], k["n"]))
        assert out[0, 0] == k["first_value"], k
    k = KNOWN["blowing_snow"]
    out = api["blowing_snow"](np.array(k["snd"])[:, None], np.array(k["sfcWind"], float)[:, None], snd_thresh=k["snd_thresh_m"],
                              sfcWind_thresh=k["sfcWind_thresh_kmh"], window=k["window"], freq=k["freq"], time=("standard", k["start"], len(k["snd"])))
    assert out[:, 0].tolist() == k["value"]
    k = KNOWN["water_cycle_intensity"]
    out = api["water_cycle_intensity"](np.full((k["n"], 1), k["pr_fill"]), np.full((k["n"], 1), k["evspsbl_fill"]), freq=k["freq"],
                                       time=("standard", k["start"], k["n"]))
    np.testing.assert_allclose(out[:, 0], k["value"], rtol=1e-7)   # the reference's own assert_allclose


def restatement_api():
    api = {n: (lambda n: lambda tas, pr, tp, pp, freq, time: CC.compound_days(n, tas, pr, tp[0], pp[0], CC.otime(*time), freq, tp[1], pp[1]))(n)
           for n in COUNTS}
    api["degree_days_exceedance_date"] = lambda tas, time, **kw: CC.degree_days_exceedance_date(tas, CC.otime(*time), **kw)
    api["blowing_snow"] = lambda snd, w, time, **kw: CC.blowing_snow(snd, w, CC.otime(*time), **kw)
    api["water_cycle_intensity"] = lambda pr, ev, time, **kw: CC.water_cycle_intensity(pr, ev, CC.otime(*time), **kw)
    return api


def mirror_api(dev):
    def axis(time):
        return TimeAxis.daily(time[1], time[2], time[0])

    def count(n):
        def fn(tas, pr, tp, pp, freq, time):
            pers = [DoyPercentile(None, d, [np.nan], (1,), {}, host=np.asarray(p, np.float64)[None], device=dev) for p, d in (tp, pp)]
            return getattr(compound, n)(tas, pr, *pers, freq=freq, time=axis(time), device=dev)
        return fn

    api = {n: count(n) for n in COUNTS}
    api["degree_days_exceedance_date"] = lambda tas, time, **kw: compound.degree_days_exceedance_date(tas, time=axis(time), device=dev, **kw)
    api["blowing_snow"] = lambda snd, w, time, **kw: compound.blowing_snow(snd, w, time=axis(time), device=dev, **kw)
    api["water_cycle_intensity"] = lambda pr, ev, time, **kw: compound.water_cycle_intensity(pr, ev, time=axis(time), device=dev, **kw)
    return api


def test_the_restatement_reproduces_the_reference_s_known_answers():
    check_known_answers(restatement_api())
    assert len(KNOWN["compound"]) == 4 and len(KNOWN["degree_days_exceedance_date"]) == 3
    assert [k["first_value"] for k in KNOWN["compound"]] == [10, 20, 20, 10]
    assert [k["first_value"] for k in KNOWN["degree_days_exceedance_date"]] == [151, 151, 256]


# ---- the vectors are the restatement's, and the conditions of the fixture hold --------------------------------------------------
def test_the_vectors_are_what_the_restatement_gives():
    for name in CASES["compound"]:
        m, t = META[name], golden_otime(META[name]["axis"])
        for n in COUNTS:
            a, b = TABLES[n]
            same(CC.compound_days(n, get(name, "tas"), get(name, "pr"), get(name, a), get(name, b), t, "QS-DEC"), get(name, f"QS-DEC/{n}"), f"{name} {n}")
        assert m["ndoy"] == get(name, "tas_lo").shape[0]
    for name in CASES["dded"]:
        m, t = META[name], golden_otime("std")
        for s, p in m["sets"].items():
            kw = {k: p[k] for k in ("op", "after_date", "never_reached")}
            same(CC.degree_days_exceedance_date(get(name, "tas"), t, m["thresh"], m["sum_thresh"], freq="YS-JUL", **kw), get(name, f"{s}/YS-JUL"), f"{name} {s}")
    for name in CASES["snow"]:
        m, t = META[name], golden_otime("std")
        for i, ind in m["indexers"].items():
            same(CC.blowing_snow(get(name, "snd"), get(name, "sfcWind"), t, m["snd_thresh"], m["sfcWind_thresh"], m["window"], "YS", **ind),
                 get(name, f"{i}/YS"), f"{name} {i}")
    for name in CASES["wci"]:
        same(CC.water_cycle_intensity(get(name, "pr"), get(name, "evspsbl"), golden_otime("std"), "MS"), get(name, "MS"), name)


def test_the_built_families_lie_on_their_grids():
    for name in CASES["compound"]:
        if not META[name]["random"]:
            tas, pr = get(name, "tas"), get(name, "pr")
            assert np.all((tas * 4 == np.round(tas * 4)) | np.isnan(tas)) and np.all((pr * 2.0 ** 22 == np.round(pr * 2.0 ** 22)) | np.isnan(pr))
            assert np.array_equal(tas.astype(np.float32), tas, equal_nan=True) and np.array_equal(pr.astype(np.float32), pr, equal_nan=True)
    tas = get("dded.built", "tas")
    assert np.all((tas * 4 == np.round(tas * 4)) | np.isnan(tas))
    for w in (1, 2, 3, 32):
        snd, wind = get(f"snow.w{w}", "snd"), get(f"snow.w{w}", "sfcWind")
        assert np.all((snd * 64 == np.round(snd * 64)) | np.isnan(snd)) and np.all(wind * 4 == np.round(wind * 4))
        assert np.nanmax(np.abs(snd)) < 2 ** 10    # ... so every window sum of differences is exact in float32 as well
    pr, ev = get("wci.built", "pr"), get("wci.built", "evspsbl")
    for x in (pr, ev):
        assert np.all((x * 2.0 ** 22 == np.round(x * 2.0 ** 22)) | np.isnan(x)) and np.nanmax(x) * 2.0 ** 22 * 400 < 2 ** 24


def test_the_random_families_keep_their_distance_from_every_threshold():
    """A condition of the fixture, not a tolerance: 1e-6 relative between every field value and its table value, and between
    every running or window sum and its threshold."""
    t = golden_otime("std")
    name = "compound.random"
    assert META[name]["random"] and get(name, "tas").dtype == np.float32
    assert CC.compound_margin(get(name, "tas"), get(name, "pr"), {k: get(name, k) for k in K.CD_TABLES}, t) >= 1e-6
    m = META["dded.random"]
    assert get("dded.random", "tas").dtype == np.float32
    for s, p in m["sets"].items():
        for freq in p["freqs"]:
            assert CC.exceedance_margin(get("dded.random", "tas"), t, m["thresh"], m["sum_thresh"], p["op"], p["after_date"], freq) >= 1e-6
    m = META["snow.random"]
    assert get("snow.random", "snd").dtype == np.float32
    assert CC.blowing_snow_margin(get("snow.random", "snd"), get("snow.random", "sfcWind"), m["snd_thresh"], m["sfcWind_thresh"], m["window"]) >= 1e-6
    # the interpolated 365-row tables: the two interpolations (scipy's, the device's) may round differently
    name = "compound.tab365"
    use = META[name]["use"]
    for k in K.CD_TABLES:
        thr = ocal.resample_doy(get(name, k), np.arange(1, 366), t)[:, use]
        x = get(name, "tas" if k.startswith("tas") else "pr")[:, use]
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.nanmin(np.abs(x - thr) / np.maximum(np.abs(x), np.abs(thr))) >= 1e-6


def test_every_decision_of_the_families_is_taken():
    c = META["dded.built"]["columns"].index
    ys = get("dded.built", "plain/YS")
    assert ys[1, c("exact")] == 201 and np.isnan(ys[1:3, c("first_row")]).all() and ys[2, c("last_row")] == 365
    assert get("dded.built", "plain/MS")[21, c("last_row")] == 366 and get("dded.built", "plain/YS-JUL")[1, c("last_row")] == 182
    assert get("dded.built", "apr15/YS")[2, c("first_row")] == 105                       # on the start row, which is not the period's first
    assert (get("dded.built", "plain.300/YS")[:, c("never")] == 300).all() and get("dded.built", "plain.300/YS")[1, c("never_equal")] == 300
    assert get("dded.built", "feb01.dec01/YS")[1:, c("never")].tolist() == [336.0, 335.0, 335.0]   # "12-01" in a leap year and in two others
    assert np.isnan(get("dded.built", "feb01.dec01/YS")[0]).all() and np.isnan(get("dded.built", "jun15.200/YS")[3]).all()
    assert np.isnan(get("dded.built", "feb29/YS")[[0, 2, 3]]).all() and not np.isnan(get("dded.built", "feb29/YS")[1]).all()
    assert not np.array_equal(get("dded.built", "plain/YS")[:, c("nan_run")], get("dded.built", "plain/YS")[:, c("generic")])
    c = META["snow.w3"]["columns"].index
    for w in (1, 2, 3, 32):
        ys = get(f"snow.w{w}", "all/YS")
        assert ys[:, c("nan_inside")].sum() == 0 < ys[:, c("nan_outside")].sum()
        assert ys[0, c("first_rows")] == 2 and ys[:, c("halo")].sum() >= 5 and ys[:, c("equal")].sum() > 10
        assert 0 < get(f"snow.w{w}", "winter/YS")[:, c("halo")].sum() < ys[:, c("halo")].sum()
    c = META["compound.tab366"]["columns"].index
    ys = get("compound.tab366", "YS/cold_and_wet_days")
    assert ys[1, c("doy366")] >= 1


# ---- the mirrors of the header's #defines ------------------------------------------------------------------------------------------
def test_the_mirrors_of_the_header_s_defines():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(XH_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    assert defines == capi.UNIT_DEFINES["xclim_hip_compound.h"]
    assert [f"XH_CD_{k.upper()}" for k in capi.CD_OUTPUTS] == ["XH_CD_COLD_DRY", "XH_CD_WARM_DRY", "XH_CD_WARM_WET", "XH_CD_COLD_WET"]
    assert list(capi.CD_OUTPUTS.values()) == [1, 2, 4, 8] and capi.CD_NOUT == len(capi.CD_OUTPUTS)
    assert capi.BS_MAX_WINDOW == capi.HYDRO_MAX_WINDOW == compound.BS_MAX_WINDOW == 32
    assert list(compound.COMPOUND_OUTPUTS.values()) == list(capi.CD_OUTPUTS) and set(K.CD_NEEDS) == set(capi.CD_OUTPUTS)
    for n, (a, b) in TABLES.items():
        assert K.CD_NEEDS[compound.COMPOUND_OUTPUTS[n]] == (a, b)
    assert compound.ADAPTED == compound.multivariate.ADAPTED + compound.threshold.ADAPTED and len(compound.ADAPTED) == 7


# ---- the host tables of the mirror ----------------------------------------------------------------------------------------------------
def test_the_table_rows_are_those_of_resample_doy():
    for axis, ndoy in (("std", 366), ("std", 365), ("noleap", 365)):
        t, ot = golden_time(axis), golden_otime(axis)
        tab = np.arange(1.0, ndoy + 1)[:, None]
        per = DoyPercentile(None, np.arange(1, ndoy + 1), [np.nan], (1,), {}, host=tab[None])
        tidx = compound.compound_table_rows({"tas_lo": per}, t)
        want = ocal.resample_doy(np.arange(1.0, (366 if axis == "std" else 365) + 1)[:, None], np.arange(1, (366 if axis == "std" else 365) + 1), ot)[:, 0]
        assert np.array_equal(tidx + 1, want)      # after adjust_doy_calendar the table of a standard axis has 366 rows


def test_the_exceedance_tables_are_those_of_the_reference_s_date_arithmetic():
    t, ot = golden_time("std"), golden_otime("std")
    from oracle.timeutil import groups

    for freq in ("YS", "YS-JUL", "MS", "QS-DEC"):
        seg = t.segments(freq)[0]
        g = groups(ot, freq)
        assert [int(i[0]) for _, i in g] == seg[:-1].tolist()
        for after, never in ((None, None), ("04-15", 300), ("02-29", "12-01"), ("06-15", "02-29")):
            start, nv = compound.exceedance_tables(t, seg, after, never)
            for p, (_, idx) in enumerate(g):
                sub = ot.isel(idx)
                hit = np.flatnonzero((sub.month == int(after[:2])) & (sub.day == int(after[3:]))) if after else np.array([0])
                assert start[p] == (idx[hit[0]] if hit.size else -1)
                if never is None:
                    assert np.isnan(nv[p])
                elif isinstance(never, str) and never == "02-29":
                    pass
                else:
                    assert nv[p] == (never if not isinstance(never, str) else CC.doy_from_string(never, int(sub.year[0]), "standard"))
    assert compound.exceedance_tables(t, t.segments("YS")[0], None, "12-01")[1].tolist() == [335.0, 336.0, 335.0, 335.0]
    assert compound.blowing_snow_periods([0, 1, 32]) == 1 and compound.blowing_snow_periods([0, 2, 32]) == 0 and compound.blowing_snow_periods([0]) == 0


# ---- every refusal is made before a device is asked for ------------------------------------------------------------------------------
def refusals(dev):
    t = golden_time("std")
    T = len(t)
    x = np.full((T, 3), 280.0, np.float32)
    tab = np.full((366, 3), 279.0)
    gappy = TimeAxis(np.r_[t.year[:40], t.year[50:]], np.r_[t.month[:40], t.month[50:]], np.r_[t.day[:40], t.day[50:]], "standard")
    monthly = TimeAxis([2000] * 12, range(1, 13), [1] * 12)

    def rows(time):
        return x if time is None else x[:len(time)]

    calls = {
        "compound_days": lambda time, **kw: compound.compound_days(rows(time), rows(time), tab, tab, tab, tab, time=time, device=dev, **kw),
        "degree_days_exceedance_date": lambda time, **kw: compound.degree_days_exceedance_date(rows(time), time=time, device=dev, **kw),
        "blowing_snow": lambda time, **kw: compound.blowing_snow(rows(time), rows(time), time=time, device=dev, **kw),
        "water_cycle_intensity": lambda time, **kw: compound.water_cycle_intensity(rows(time), rows(time), time=time, device=dev, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(compound.NotServed):
            call(gappy)
        with pytest.raises(compound.NotServed):
            call(monthly)
        with pytest.raises(compound.NotServed):
            call(t, freq="3h")
        with pytest.raises(TypeError, match="Freq must be a string"):
            call(t, freq=5)
        with pytest.raises(TypeError, match="TimeAxis"):
            call(None)
        with pytest.raises(ValueError, match="mask_missing=False"):
            call(t, keep=True, mask_missing=True)
        with pytest.raises(ValueError, match="rows"):
            compound.water_cycle_intensity(x, x, time=TimeAxis.daily("2000-01-01", 10), device=dev)
    # the tables: one that does not cover the axis, two on different axes, several percentiles, other cells
    holed = DoyPercentile(None, np.r_[np.arange(1, 60), np.arange(61, 367)], [np.nan], (3,), {}, host=np.zeros((1, 365, 3)))
    with pytest.raises(compound.NotServed, match="does not cover"):    # it ends on day 366, so it is not re-gridded, and has no day 60
        compound.cold_and_dry_days(x, x, holed, tab, time=t, device=dev)
    shifted = DoyPercentile(None, np.arange(1, 366), [np.nan], (3,), {}, host=np.zeros((1, 365, 3)))
    with pytest.raises(compound.NotServed, match="share their day-of-year axis"):
        compound.cold_and_dry_days(x[:365], x[:365], shifted, tab, time=TimeAxis.daily("2001-01-01", 365), device=dev)
    two = DoyPercentile(None, np.arange(1, 367), [10.0, 90.0], (3,), {}, host=np.zeros((2, 366, 3)))
    with pytest.raises(ValueError, match="select one percentile"):
        compound.warm_and_wet_days(x, x, two, tab, time=t, device=dev)
    with pytest.raises(ValueError, match="cells"):
        compound.warm_and_wet_days(x, x, tab[:, :2], tab, time=t, device=dev)
    with pytest.raises(ValueError, match="need tas_per_high"):
        compound.compound_days(x, x, tab, None, tab, tab, time=t, device=dev)
    with pytest.raises(ValueError, match="outputs must be"):
        compound.compound_days(x, x, tab, tab, tab, tab, outputs=("hot_days",), time=t, device=dev)
    with pytest.raises(ValueError, match="outputs must be"):
        compound.compound_days(x, x, tab, tab, tab, tab, outputs=(), time=t, device=dev)
    with pytest.raises(ValueError, match="differs from"):
        compound.cold_and_dry_days(x, x[:, :2], tab, tab, time=t, device=dev)
    # the exceedance date
    with pytest.raises(NotImplementedError, match="op: '=='"):
        compound.degree_days_exceedance_date(x, op="==", time=t, device=dev)
    with pytest.raises(ValueError, match="units must be one of"):
        compound.degree_days_exceedance_date(x, units="degF", time=t, device=dev)
    with pytest.raises(ValueError, match="MM-DD"):
        compound.degree_days_exceedance_date(x, never_reached="2000-12-01", time=t, device=dev)
    with pytest.raises(TypeError, match="never_reached"):
        compound.degree_days_exceedance_date(x, never_reached=300.5, time=t, device=dev)
    with pytest.raises(ValueError, match="More than 1 instance"):   # a period of three years holds the date three times (max_idxs=1)
        compound.exceedance_tables(t, np.array([0, T]), "04-15")
    # blowing snow
    with pytest.raises(compound.NotServed, match="up to 32"):
        compound.blowing_snow(x, x, window=33, time=t, device=dev)
    for w in (0, 2.0, True):
        with pytest.raises(ValueError, match="window must be an integer"):
            compound.blowing_snow(x, x, window=w, time=t, device=dev)
    # water cycle intensity
    with pytest.raises(ValueError, match="flux_units must be one of"):
        compound.water_cycle_intensity(x, x, flux_units="m/s", time=t, device=dev)
    # empty results need no device either
    assert compound.compound_days(x[:, :0], x[:, :0], tab[:, :0], tab[:, :0], tab[:, :0], tab[:, :0], time=t, device=dev)["cold_and_dry_days"].shape == (4, 0)
    assert compound.degree_days_exceedance_date(x[:, :0], time=t, device=dev).shape == (4, 0)
    assert compound.blowing_snow(x[:, :0], x[:, :0], time=t, device=dev).shape == (4, 0)
    assert compound.blowing_snow(x[:1], x[:1], time=t.subset(slice(0, 1)), device=dev).shape == (0, 3)
    assert compound.water_cycle_intensity(x[:, :0], x[:, :0], freq="MS", time=t, device=dev).shape == (37, 0)


def test_refusals_need_no_device():
    refusals(NoDevice())


def test_the_kernel_wrappers_refuse_before_the_call():
    class Arr(capi.DeviceArray):
        def __init__(self, shape, dtype):   # a device array that owns nothing: only its shape and dtype are looked at
            self.shape, self.dtype, self.ptr = tuple(shape), np.dtype(dtype), 0

        def __del__(self):
            pass

    dev, x, x64, tab = NoDevice(), Arr((10, 4), np.float32), Arr((10, 4), np.float64), Arr((366, 4), np.float64)
    seg = [0, 10]
    with pytest.raises(TypeError, match="all float32 or all float64"):
        K.compound_doy_days(dev, x, x64, {"tas_lo": tab, "pr_lo": tab}, np.zeros(10), seg, ["cold_dry"])
    with pytest.raises(ValueError, match="need the tables"):
        K.compound_doy_days(dev, x, x, {"tas_lo": tab}, np.zeros(10), seg, ["cold_dry"])
    with pytest.raises(ValueError, match="non-empty subset"):
        K.compound_doy_days(dev, x, x, {"tas_lo": tab, "pr_lo": tab}, np.zeros(10), seg, ["hot"])
    with pytest.raises(TypeError, match="float64"):
        K.compound_doy_days(dev, x, x, {"tas_lo": tab, "pr_lo": Arr((366, 4), np.float32)}, np.zeros(10), seg, ["cold_dry"])
    with pytest.raises(ValueError, match="tidx must have 10 entries"):
        K.compound_doy_days(dev, x, x, {"tas_lo": tab, "pr_lo": tab}, np.zeros(9), seg, ["cold_dry"])
    with pytest.raises(ValueError, match="up to 32"):
        K.blowing_snow_days(dev, x, x, seg, snd_thresh=0.5, wind_thresh=4.0, window=33)
    with pytest.raises(ValueError, match="selection must be"):
        K.blowing_snow_days(dev, x, x, seg, np.zeros(9, bool), snd_thresh=0.5, wind_thresh=4.0)
    with pytest.raises(ValueError, match="start must have 1 entries"):
        K.degree_exceedance_date(dev, x, seg, [0, 0], [np.nan], np.ones(10), thresh=0.0, sum_thresh=1.0)
    with pytest.raises(ValueError, match="offsets must be non-decreasing"):
        K.pair_period_sum(dev, x, x, [0, 11])
