"""rain_season and hardiness_zones without a GPU: the numpy restatement tests/raincpu.py reproduces the known answers of the
reference's own tests (tests/golden/rain_known_answers.json: eight for rain_season, six for hardiness_zones) and the golden file
tests/golden/rain_vectors.npz; the flag byte of ``xclim_amd.rainseason.rain_flags`` against ``select_time_mask`` applied period by
period; what the mirror does not serve; the mirrors of the header's #defines (tests/test_abi_cpu.py checks header, ctypes table and library).  ``refusals`` and ``check_known_answers`` are
shared with tests/test_gpu_rain.py (the device) and tests/test_hostsim_units_cpu.py (the host simulation).

Every result is an integer (a day of year, a number of days, a zone) or NaN: every comparison is exact."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import raincpu as R
import stridedabi as S
from stridedabi import RAIN_TABLE
from xclim_amd import _capi, rainseason
from xclim_amd.calendar import select_time_mask
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "xclim_hip_rain.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rain_vectors.npz")
_vp = ctypes.c_void_p
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "rain_known_answers.json")))
OUTPUTS = ("start", "end", "length")


def same(got, want, what):
    """Equal element by element, NaN where NaN is expected."""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---- the reference's known answers ---------------------------------------------------------------------------------------
class Restated:
    """The two functions on the restatement, with the signature ``mirror_api`` gives the mirror."""

    @staticmethod
    def rain_season(pr, time, flux_units, **kw):
        return R.rain_season(pr, time, "YS-JAN", flux_units, **kw)

    @staticmethod
    def hardiness_zones(tasmin, time, method, units):
        return R.hardiness_zones(tasmin, time, 30, method, "YS", units)


def mirror_api(dev):
    """xclim_amd.rainseason on ``dev`` behind the same two signatures."""

    class Mirror:
        @staticmethod
        def rain_season(pr, time, flux_units, **kw):
            return tuple(rainseason.rain_season(pr, time=time, flux_units=flux_units, device=dev, **kw))

        @staticmethod
        def hardiness_zones(tasmin, time, method, units):
            return rainseason.hardiness_zones(tasmin, method=method, time=time, units=units, device=dev)

    return Mirror


def check_known_answers(f=Restated):
    k = KNOWN["rain_season"]
    ax = k["axis"]
    time = TimeAxis.daily(ax["start"], ax["rows"], ax["calendar"])
    n = 0
    for method in k["method_dry_start"]:
        for kind, r in k["results"].items():
            pr = np.full((ax["rows"], 1), np.nan)
            for lo, hi, v in k["base"]["spans"] + r["spans"]:
                pr[lo:hi] = v
            got = f.rain_season(pr, time, ax["units"], method_dry_start=method, **k["arguments"])
            want = [np.nan if v is None else v for v in r["expected"]]
            same(np.array([g[0, 0] for g in got]), want, f"rain_season {method} {kind}")
            n += 1
    z = KNOWN["hardiness_zones"]
    ax = z["axis"]
    time = TimeAxis.daily(ax["start"], ax["rows"], ax["calendar"])
    for case in z["cases"]:
        t = np.full((ax["rows"], 1), float(z["base"]["fill"]))
        t[time.doy == 1] = case["tmin"]
        got = f.hardiness_zones(t, time, case["method"], ax["units"])
        assert got.shape == (30, 1) and np.isnan(got[:-1]).all(), case
        same(got[-1], [np.nan if case["zone"] is None else case["zone"]], f"hardiness_zones {case}")
        n += 1
    assert n == 14


def test_restatement_reproduces_the_known_answers():
    check_known_answers()


def test_zone_edges_of_the_mirror_and_of_the_restatement():
    for method in ("usda", "anbg", "USDA"):
        for units in ("K", "degC"):
            e = rainseason.zone_edges(method, units)
            np.testing.assert_array_equal(e, R.zone_edges(method, units))
            assert len(e) == (27 if method.lower() == "usda" else 8) and (np.diff(e) > 0).all() and len(e) <= _capi.ZONES_MAX_EDGES
    np.testing.assert_array_equal(rainseason.zone_edges("anbg", "degC"), np.arange(-15.0, 25.0, 5.0))
    np.testing.assert_allclose(rainseason.zone_edges("usda", "degC")[[0, 18, -1]], [-51.0 - 1 / 9, -1.0 - 1 / 9, 21.0 + 1 / 9], rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError, match="Method must be one of `usda` or `anbg`. Got rhs."):
        rainseason.zone_edges("rhs")
    # get_zones of the restatement on the edges themselves: left-closed bins, the last one closed on the right, NaN outside
    e = np.array([0.0, 5.0, 10.0])
    same(R.get_zones([-0.1, 0.0, 4.9, 5.0, 10.0, 10.1, np.nan, np.inf], e), [np.nan, 0, 0, 1, 1, np.nan, np.nan, np.nan], "get_zones")


# ---- the flag byte ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,T,freq,dates", [
    ("1999-01-01", 365 + 366 + 300, "YS-JAN", dict(date_min_start="05-01", date_max_start="12-31", date_min_end="09-01", date_max_end="12-31")),
    ("1999-01-01", 365 + 366 + 200, "YS-JAN", dict(date_min_start="02-10", date_max_start="06-30", date_min_end="04-15", date_max_end="12-31")),
    # a July year: the start window (08-15 .. 06-30), the start bounds and the end bounds all wrap around 31 December, and the
    # first period holds 29 February 2000
    ("1999-07-01", 366 + 365 + 150, "YS-JUL", dict(date_min_start="08-15", date_max_start="03-15", date_min_end="10-01", date_max_end="06-30")),
    ("1999-07-01", 366 + 365, "YS-JUL", dict(date_min_start="02-29", date_max_start="03-15", date_min_end="02-28", date_max_end="02-29")),
], ids=["jan-defaults", "jan", "jul-wrapping", "jul-feb29"])
def test_flags_against_select_time_mask_period_by_period(start, T, freq, dates):
    time = TimeAxis.daily(start, T)
    seg = np.asarray(time.segments(freq)[0])
    flags = rainseason.rain_flags(time, seg, **dates)
    assert flags.dtype == np.uint8 and flags.shape == (T,) and len(seg) == (4 if T > 731 else 3)
    for k in range(len(seg) - 1):
        rows = slice(int(seg[k]), int(seg[k + 1]))
        sub = time.subset(rows)
        last = f"{int(sub.month[-1]):02d}-{int(sub.day[-1]):02d}"
        want = (select_time_mask(sub, date_bounds=(dates["date_min_start"], last)) * _capi.RAIN_START_WINDOW
                + select_time_mask(sub, date_bounds=(dates["date_min_start"], dates["date_max_start"])) * _capi.RAIN_START_BOUNDS
                + select_time_mask(sub, date_bounds=(dates["date_min_end"], dates["date_max_end"])) * _capi.RAIN_END_BOUNDS)
        np.testing.assert_array_equal(flags[rows], want)
        for j, m in enumerate(R.period_masks(time, rows, **dates)):
            np.testing.assert_array_equal((flags[rows] >> j) & 1, m)
        w = (flags[rows] & 1) != 0
        assert w[-1] and (np.diff(w.astype(int)) >= 0).all()          # the start window is the tail of the period
    if freq == "YS-JUL":
        feb29 = np.flatnonzero((time.month == 2) & (time.day == 29))
        assert len(feb29) == 1 and flags[feb29[0]] & 1
        if dates["date_min_start"] == "02-29":      # the window of the leap year starts on 29 February, the other years' on 1 March
            assert not flags[feb29[0] - 1] & 1 and (flags[feb29[0]] & 2) and flags[feb29[0]] & 4


def test_restatement_from_dates_and_from_flags_agree():
    time = TimeAxis.daily("1999-07-01", 366 + 365 + 150)
    dates = dict(date_min_start="08-15", date_max_start="03-15", date_min_end="10-01", date_max_end="06-30")
    rng = np.random.default_rng(3)
    pr = np.where(rng.random((len(time), 40)) < 0.5, np.round(rng.gamma(1.0, 8.0, (len(time), 40)) * 4) / 4, 0.0)
    seg = time.segments("YS-JUL")[0]
    a = R.rain_season(pr, time, "YS-JUL", "mm/d", window_not_dry_start=10, window_dry_end=5, **dates)
    b = R.rain_season_flags(pr, seg, rainseason.rain_flags(time, seg, **dates), time.doy, "mm/d", window_not_dry_start=10, window_dry_end=5)
    for x, y, k in zip(a, b, OUTPUTS):
        same(x, y, k)
    assert 0 < np.isnan(a[0]).sum() < a[0].size and 0 < np.isnan(a[1]).sum() < a[1].size


# ---- the golden file -------------------------------------------------------------------------------------------------------
_Z = np.load(GOLDEN) if os.path.exists(GOLDEN) else None      # (absent only while tests/golden/make_rain_golden.py writes it)
META = json.loads(str(_Z["meta"])) if _Z is not None else {}
CASES = sorted(META)
ZONE_CASES = sorted({k.split("/")[0] for k in (_Z.files if _Z is not None else ()) if k.startswith("zones.")})
FAMILIES = ("reach", "nan", "same_row", "bounds", "none", "random")


def golden_case(name):
    """(meta, pr, seg, flags, doy, {start, end, length}) of one case."""
    return (META[name], _Z[f"{name}/pr"], _Z[f"{name}/seg"], _Z[f"{name}/flags"], _Z[f"{name}/doy"], {k: _Z[f"{name}/{k}"] for k in OUTPUTS})


def golden_time(m, T):
    """The time axis of a case that has one (the cases with hand-made flags do not)."""
    return TimeAxis.daily(m["time"]["start"], T, m["time"]["calendar"])


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    fams = {f for m in META.values() for f in m["family"]}
    assert fams == set(FAMILIES)
    sums = {(m["params"]["window_wet_start"]) for m in META.values()}
    assert {1, 2, 32} <= sums
    for key, method in (("window_dry_start", "method_dry_start"), ("window_dry_end", "method_dry_end")):
        assert {1, 2, 32} <= {m["params"][key] for m in META.values() if m["params"][method] == "total"}
    assert {(m["params"]["method_dry_start"], m["params"]["method_dry_end"]) for m in META.values()} == {
        (a, b) for a in ("per_day", "total") for b in ("per_day", "total")}
    assert any(m["params"]["window_dry_start"] > 32 for m in META.values())      # the second read of the decision row
    assert {m["dtype"] for m in META.values()} == {"float32", "float64"}
    assert {len(_Z[f"{n}/seg"]) - 1 for n in CASES} == {1, 3}
    for name in CASES:                                                            # every case decides both ways
        m, pr, seg, flags, doy, exp = golden_case(name)
        assert pr.dtype == np.dtype(m["dtype"]) and pr.shape[1] == len(m["columns"]) == exp["start"].shape[1]
        if name != "bounds_single_row" and "random" not in m["family"]:
            assert any(0 < np.isnan(exp[k]).sum() < exp[k].size for k in ("start", "end")), name
        if "random" not in m["family"]:                                           # the 0.25 mm grid, in mm per day
            assert m["flux_units"] == "mm/d"
            v = pr[~np.isnan(pr)].astype(np.float64)
            np.testing.assert_array_equal(v * 4, np.round(v * 4))
    assert len(ZONE_CASES) == 4


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden_file(name):
    m, pr, seg, flags, doy, exp = golden_case(name)
    got = R.rain_season_flags(pr, seg, flags, doy, m["flux_units"], **m["params"])
    for g, k in zip(got, OUTPUTS):
        same(g, exp[k], f"{name} {k}")
        assert np.array_equal(g[~np.isnan(g)], np.round(g[~np.isnan(g)]))
    if m["dates"] is not None:        # the cases on a calendar: the same from the dates, period by period
        time = golden_time(m, len(flags))
        np.testing.assert_array_equal(rainseason.rain_flags(time, seg, **m["dates"]), flags)
        np.testing.assert_array_equal(time.doy, doy)
        for g, k in zip(R.rain_season(pr, time, m["time"]["freq"], m["flux_units"], **m["params"], **m["dates"]), OUTPUTS):
            same(g, exp[k], f"{name} {k} from the dates")


@pytest.mark.parametrize("name", [n for n in CASES if "random" in META[n]["family"]])
def test_random_fields_keep_their_distance_from_the_thresholds(name):
    """No window sum (and no single amount compared per day) lies within 1e-6 relative of its threshold: the answers of the random
    float32 fields do not depend on the order of the additions or on float32 arithmetic."""
    m, pr, seg, flags, _, _ = golden_case(name)
    assert m["flux_units"] == "kg m-2 s-1" and pr.dtype == np.float32
    assert (R.margin(pr, seg, flags, m["flux_units"], **m["params"]) > 1e-6).all()


@pytest.mark.parametrize("name", ZONE_CASES)
def test_restatement_reproduces_the_golden_zones(name):
    method, units = name.split(".")[1:]
    x, e = _Z[f"{name}/x"], R.zone_edges(method, units)
    n = len(e)
    for w in (1, 2, 30):
        same(R.rolling_zones(x, w, e), _Z[f"{name}/w{w}"], f"{name} window {w}")
    z = _Z[f"{name}/w1"][0]
    same(z[:n], list(range(n - 1)) + [n - 2], "a value on an edge is in the zone to its right; the last edge closes the last zone")
    same(z[n:2 * n], list(range(n - 1)) + [np.nan], "just above an edge")
    same(z[2 * n:3 * n], [np.nan] + list(range(n - 1)), "just below an edge")
    same(z[3 * n:3 * n + 3], [np.nan] * 3, "below the first edge, above the last, NaN")
    w30 = _Z[f"{name}/w30"]
    assert np.isnan(w30[:29]).all() and np.isnan(w30[29:, -12:-8]).all() and not np.isnan(w30[30, -8:]).any()   # the NaN period 13


# ---- what the mirror does not serve -----------------------------------------------------------------------------------------
def test_axes_and_arguments_that_are_not_served():
    t = TimeAxis.daily("2000-01-01", 400)
    pr = np.ones((400, 2))
    gappy = t.subset(np.r_[0:10, 11:400])
    with pytest.raises(rainseason.NotServed):
        rainseason.rain_season(pr[:399], time=gappy)
    with pytest.raises(rainseason.NotServed):
        rainseason.hardiness_zones(pr[:399], time=gappy)
    for kw in (dict(window_wet_start=33), dict(window_dry_start=33, method_dry_start="total"), dict(window_dry_end=33, method_dry_end="total")):
        with pytest.raises(rainseason.NotServed, match="up to 32"):
            rainseason.rain_season(pr, time=t, **kw)
    with pytest.raises(rainseason.NotServed, match="start bounds"):      # the 35 rows of 2001 end on 4 February
        rainseason.rain_season(pr, time=t)
    with pytest.raises(rainseason.NotServed, match="end bounds"):
        rainseason.rain_season(pr, time=t, date_min_start="01-01")
    with pytest.raises(rainseason.NotServed):
        rainseason.rain_season(pr, time=t, freq="7D")
    with pytest.raises(ValueError, match="Unknown method_dry_start: weekly."):
        rainseason.rain_season(pr, time=t, method_dry_start="weekly")
    with pytest.raises(ValueError, match="Unknown method_dry_end: weekly."):
        rainseason.rain_season(pr, time=t, method_dry_end="weekly")
    with pytest.raises(ValueError, match="flux_units"):
        rainseason.rain_season(pr, time=t, flux_units="in/d")
    with pytest.raises(ValueError, match="window_dry_start"):
        rainseason.rain_season(pr, time=t, window_dry_start=0)
    with pytest.raises(ValueError, match="keep=True"):
        rainseason.rain_season(pr, time=t, keep=True, mask_missing=True)
    with pytest.raises(TypeError):
        rainseason.rain_season(pr, time=t, freq=3)
    with pytest.raises(NotImplementedError, match="Method must be one of"):
        rainseason.hardiness_zones(pr, method="rhs", time=t)
    with pytest.raises(ValueError, match="units"):
        rainseason.hardiness_zones(pr, time=t, units="degF")
    assert (rainseason.RAIN_MAX_WINDOW, _capi.HYDRO_MAX_WINDOW) == (32, 32)
    txt = open(HEADER).read()
    assert "#define XH_RAIN_MAX_WINDOW 32" in txt and "#define XH_ZONES_MAX_EDGES 32" in txt
    assert rainseason.ADAPTED == ("rain_season", "hardiness_zones")


# ---- the C ABI (tests/test_abi_cpu.py checks the header against the ctypes table, the library and the registry) ---------
def test_the_unit_is_built_and_its_operand_table_is_the_header_s():
    assert set(S.prototypes(HEADER)) == set(RAIN_TABLE)
    make = open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()
    assert "rainseason.hip" in make and "xclim_hip_rain.h" in make
    assert '#include "xclim_hip.h"' in open(HEADER).read()
    assert len(re.findall(r"/\* host \*/", open(HEADER).read())) == 4      # the host tables are marked


def test_the_flag_bits_mirror_the_header():
    assert (_capi.RAIN_START_WINDOW, _capi.RAIN_START_BOUNDS, _capi.RAIN_END_BOUNDS) == (1, 2, 4)
    for bit, name in ((1, "START_WINDOW"), (2, "START_BOUNDS"), (4, "END_BOUNDS")):
        assert re.search(rf"#define XH_RAIN_{name} {bit}\b", open(HEADER).read())


def test_entry_points_reject_a_null_context():
    lib = _capi.load_library()
    null, some = _vp(0), _vp(64)   # never dereferenced: the check fails first
    assert lib.xh_rain_season(null, 10, 4, 4, 0, some, 1.0, 1, some, some, some, 25.0, 3, 30, 1.0, 7, 0, 0.0, 20, 0, some, some, some,
                              4) == _capi.XH_ERR_ARG
    assert lib.xh_rolling_zones(null, 10, 4, 4, 0, some, 3, 8, some, some, 4) == _capi.XH_ERR_ARG


def refusals(dev):
    """Every refusal is a code that answers before anything is launched: the sentinel in the outputs is intact afterwards, and the
    same call with nothing wrong then runs.  On the device (tests/test_gpu_rain.py) and, through it, on the host simulation."""
    from newunit_cases import shared_refusals

    ARG, LAYOUT, LIMIT = _capi.XH_ERR_ARG, _capi.XH_ERR_LAYOUT, _capi.XH_ERR_LIMIT
    T, C, P = 40, 8, 2
    x = dev.to_device(np.linspace(1.0, 9.0, T * C).reshape(T, C))
    out = dev.to_device(np.full((T, C), -7.0))
    p = lambda a: _vp(0) if a is None else a.ctypes.data_as(_vp)  # noqa: E731
    d = lambda a: _vp(0) if a is None else _vp(a.ptr)             # noqa: E731
    seg = np.array([0, 20, T], np.int64)
    many = np.zeros(65538, np.int64)
    flags = np.full(T, 7, np.uint8)
    doy = np.arange(1, T + 1, dtype=np.int32)
    rs, rz = (getattr(dev.lib, n) for n in RAIN_TABLE)

    def rain(ld=C, ld_out=C, seg=seg, P=P, pr=x, flags=flags, doy=doy, ww=3, wnd=5, wd=4, ts=0, we=3, te=0, s=out, e=out, ln=out, T=T, C=C,
             ctx=dev.ctx):
        return rs(ctx, T, C, ld, 1, d(pr), 1.0, P, p(seg), p(flags), p(doy), 25.0, ww, wnd, 1.0, wd, ts, 0.0, we, te, d(s), d(e), d(ln), ld_out)

    assert rain(ld=C - 1) == LAYOUT and rain(ld_out=C - 1) == LAYOUT                       # a pitch below the row width
    assert rain(seg=None) == ARG and rain(pr=None) == ARG and rain(flags=None) == ARG and rain(doy=None) == ARG and rain(T=-1) == ARG
    assert rain(seg=np.array([0, 30, 20], np.int64)) == ARG                                  # a decreasing seg
    assert rain(seg=np.array([0, 20, T + 1], np.int64)) == ARG and rain(seg=np.array([-1, 20, T], np.int64)) == ARG
    assert rain(seg=many, P=65536) == LIMIT                                                  # more than 65535 periods
    assert rain(s=None, e=None, ln=None) == ARG                                              # no output requested
    assert rain(ww=0) == ARG and rain(wd=0) == ARG and rain(we=0) == ARG and rain(wnd=-1) == ARG
    M = rainseason.RAIN_MAX_WINDOW
    assert rain(ww=M + 1) == LIMIT and rain(wd=M + 1, ts=1) == LIMIT and rain(we=M + 1, te=1) == LIMIT     # one row beyond the limit
    holed = flags.copy()
    holed[30] = 6                                                                            # a start window with a hole
    assert rain(flags=holed) == ARG
    bad = doy.copy()
    bad[7] = 367
    assert rain(doy=bad) == ARG
    bad[7] = 0
    assert rain(doy=bad) == ARG
    shared_refusals(rain, T, C, [("seg", seg, T, dict(seg=many, P=65536))])

    edges = np.array([0.0, 2.0, 4.0, 6.0])

    def zones(ld=C, ld_out=C, xx=x, window=3, n=4, e=edges, o=out, P=T, C=C, ctx=dev.ctx):
        return rz(ctx, P, C, ld, 1, d(xx), window, n, p(e), d(o), ld_out)

    assert zones(ld=C - 1) == LAYOUT and zones(ld_out=C - 1) == LAYOUT
    assert zones(xx=None) == ARG and zones(e=None) == ARG and zones(o=None) == ARG and zones(window=0) == ARG and zones(P=-1) == ARG
    assert zones(n=1) == ARG and zones(e=np.array([0.0, 2.0, 2.0, 6.0])) == ARG and zones(e=np.array([0.0, np.nan, 2.0, 6.0])) == ARG
    assert zones(n=_capi.ZONES_MAX_EDGES + 1, e=np.arange(40.0)) == LIMIT
    shared_refusals(lambda T=T, **kw: zones(P=T, **kw), T, C)

    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((T, C), -7.0))          # nothing was launched: the sentinels are intact
    assert rain(wd=M + 1, we=M + 1) == 0                                     # "per_day" windows have no limit
    dev.sync()
    assert (out.get()[:P] != -7.0).all() and (out.get()[P:] == -7.0).all()
    assert zones() == 0
    dev.sync()
    got = out.get()
    assert np.isnan(got[:2]).all() and (got[2:] != -7.0).all()
