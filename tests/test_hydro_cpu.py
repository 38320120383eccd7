"""The hydrology unit without a GPU: the numpy restatement tests/hydrocpu.py against the reference's known answers
(tests/golden/hydro_known_answers.json, recorded from its tests/test_hydrology.py) and against tests/golden/hydro_vectors.npz; what
of the C ABI is the unit's own (tests/test_abi_cpu.py checks header, ctypes table and library); the host tables of the mirror; the refusals and the known answers
on the host simulation of hydro.hip.

Tolerance of the unit family: |got - want| <= 1e-12 * scale, the scale being the sum of the absolute terms of the value (hydrocpu
carries it); counts, n and NaN patterns exactly; the Sen slope bit for bit; p within 1e-12 absolute."""

import ctypes
import json
import os
import types

import numpy as np
import pytest

import hydrocpu as H
import stridedabi as S
from stridedabi import HYDRO_TABLE
from xclim_amd import _capi, hydrology
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "xclim_hip_hydro.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "hydro_vectors.npz")
RTOL = 1e-12
P_ATOL = 1e-12
_vp = ctypes.c_void_p
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "hydro_known_answers.json")))


# ---- the comparison ------------------------------------------------------------------------------------------------------
def check(got, want, scale, what):
    """Integers (``scale`` None) exactly; floats: the same NaN pattern and |got - want| <= RTOL * scale."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if scale is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    bad = err > RTOL * np.asarray(scale)
    assert not bad.any(), f"{what}: {int(bad.sum())} values beyond {RTOL} * scale, worst {np.nanmax(err / np.maximum(scale, 1e-300)):.3g} of scale"


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def check_run(got, exp, what):
    """The outputs of one run against the expected ones: slope bit for bit (NaN where NaN), p within P_ATOL, integers exactly,
    everything else within RTOL of its scale."""
    for k, v in got.items():
        if k == "slope":
            np.testing.assert_array_equal(np.isnan(v), np.isnan(exp[k]), err_msg=f"{what} slope: NaN pattern")
            np.testing.assert_array_equal(np.nan_to_num(v), np.nan_to_num(exp[k]), err_msg=f"{what} slope: not the same bits")
        elif k == "p":
            np.testing.assert_array_equal(np.isnan(v), np.isnan(exp[k]), err_msg=f"{what} p: NaN pattern")
            assert (np.abs(np.nan_to_num(v) - np.nan_to_num(exp[k])) <= P_ATOL).all(), f"{what} p"
        else:
            check(v, exp[k], exp.get(k + "_scale"), f"{what} {k}")


# ---- the reference's known answers ---------------------------------------------------------------------------------------
def _series(k, key="spans", fill=None):
    a = np.full(k["T"], k.get("fill", 0.0) if fill is None else fill, np.float64)
    for lo, hi, v in k.get(key, []):
        a[lo:hi] = v
    for lo, hi, first, step in k.get("ramps", []):
        a[lo:hi] = first + step * np.arange(hi - lo)
    return a[:, None]


class Restated:
    """The functions of xclim_amd.hydrology on the restatement, for one signature of the known-answer checks."""

    @staticmethod
    def flow_stats(q, freq, time):
        r = H.flow_period_stats(q, time.segments(freq)[0])
        return r["bfi"], r["rbi"]

    @staticmethod
    def melt(snw, pr, window, freq, time, per_day):
        return H.melt_period_max(snw, pr, per_day, window, time.segments(freq)[0])["out"]

    @staticmethod
    def api(pr, window, p_exp, per_day):
        return H.antecedent_precip(pr, per_day, H.api_weights(window, p_exp))["out"]

    flow_index = staticmethod(H.flow_index)

    @staticmethod
    def high(q, factor, freq, time):
        return H.high_flow_frequency(q, factor, time.segments(freq)[0])

    @staticmethod
    def low(q, factor, freq, time):
        return H.low_flow_frequency(q, factor, time.segments(freq)[0])

    @staticmethod
    def aridity(pr, pet, freq, time):
        return H.aridity_index(pr, pet, time.segments(freq)[0])

    @staticmethod
    def sen(q, freq, time):
        seg = time.segments(freq)[0]
        table, seasons, _ = H.season_year_table(time, freq)
        r = H.sen_slope(H.period_mean(q, seg), table)
        return r["slope"], r["p"], seasons

    @staticmethod
    def bfi_ratio(q, time):
        return H.seasonal_bfi_ratio(q, time)[1]


def mirror_api(dev):
    """The same signatures on xclim_amd.hydrology with the device ``dev`` (a GPU or the host simulation)."""
    flux = {H.DAY: "kg m-2 s-1", 1.0: "mm/d"}
    kw = dict(device=dev)

    def sen(q, freq, time):
        s = hydrology.sen_slope(q, freq, time=time, **kw)
        return s.sen_slope, s.p_value, s.seasons

    return types.SimpleNamespace(
        flow_stats=lambda q, freq, time: tuple(hydrology.flow_stats(q, freq, time=time, **kw)),
        melt=lambda snw, pr, window, freq, time, per_day: (
            hydrology.snow_melt_we_max(snw, window, freq, time=time, **kw) if pr is None else
            hydrology.melt_and_precip_max(snw, pr, window, freq, time=time, flux_units=flux[per_day], **kw)),
        api=lambda pr, window, p_exp, per_day: hydrology.antecedent_precipitation_index(pr, window, p_exp, flux_units=flux[per_day], **kw),
        flow_index=lambda q, p: hydrology.flow_index(q, p, **kw),
        high=lambda q, factor, freq, time: hydrology.high_flow_frequency(q, factor, freq, time=time, **kw),
        low=lambda q, factor, freq, time: hydrology.low_flow_frequency(q, factor, freq, time=time, **kw),
        aridity=lambda pr, pet, freq, time: hydrology.aridity_index(pr, pet, freq, time=time, **kw),
        sen=sen,
        bfi_ratio=lambda q, time: hydrology.base_flow_index_seasonal_ratio(q, time=time, **kw).ratio)


def check_known_answers(f=Restated):
    """Every reproducible known answer of the reference's tests/test_hydrology.py."""
    k = KNOWN["base_flow_index"]
    a, t = _series(k), TimeAxis.daily(k["start"], k["T"])
    bfi, _ = f.flow_stats(a, k["freq"], t)
    np.testing.assert_array_equal(bfi, [[1.0 / a.mean()]])
    k = KNOWN["rb_flashiness_index"]
    _, rbi = f.flow_stats(_series(k), k["freq"], TimeAxis.daily(k["start"], k["T"]))
    np.testing.assert_array_equal(rbi, [[k["want"]]])
    k = KNOWN["snow_melt_we_max"]
    np.testing.assert_array_equal(f.melt(_series(k), None, k["window"], k["freq"], TimeAxis.daily(k["start"], k["T"]), 1.0), [[k["want"]]])
    k = KNOWN["melt_and_precip_max"]
    out = f.melt(_series(k, "snw_spans"), _series(k, "pr_spans"), k["window"], k["freq"], TimeAxis.daily(k["start"], k["T"]), H.DAY)
    np.testing.assert_array_equal(out, [[k["want"]]])
    k = KNOWN["flow_index"]
    np.testing.assert_array_equal(f.flow_index(_series(k), k["p"]), [k["want"]])
    for name, fn in (("high_flow_frequency", f.high), ("low_flow_frequency", f.low)):
        k = KNOWN[name]
        np.testing.assert_array_equal(fn(_series(k), k["factor"], k["freq"], TimeAxis.daily(k["start"], k["T"]))[:, 0], k["want"])
    # the four cases of the antecedent precipitation index
    k = KNOWN["antecedent_precipitation_index"]
    w, pe = k["window"], k["p_exp"]
    out = f.api(_series(k["simple"]), w, pe, 1.0)
    assert abs(np.nanmax(out) - k["simple"]["max"]) <= k["simple"]["atol"] and abs(np.nanmin(out) - k["simple"]["min"]) <= k["simple"]["atol"]
    a = _series(k["nan_present"])
    a[k["nan_present"]["nan_row"]] = np.nan
    assert np.isnan(f.api(a, w, pe, 1.0)[k["nan_present"]["nan_row"]]).all()
    out = f.api(_series(k["nan_start_window"]), w, pe, 1.0)
    assert np.isnan(out[:w - 1]).all() and not np.isnan(out[w - 1:]).any()
    a = _series(k["manual_calc"])
    manual = np.full(a.shape, np.nan)
    for idx in range(a.shape[0] - w + 1):
        weights = list(reversed([pe ** (ii + 1 - 1) for ii in range(w)]))
        manual[idx + w - 1] = (a[idx:idx + w, 0] * weights).sum()
    np.testing.assert_allclose(f.api(a, w, pe, 1.0), manual, atol=k["manual_calc"]["atol"])
    k = KNOWN["aridity_index"]
    out = f.aridity(_series(k, "pr"), _series(k, "pet"), k["freq"], TimeAxis.daily(k["start"], k["T"]))
    np.testing.assert_allclose(out[:, 0], k["want"], rtol=k["rtol"], atol=0)
    k = KNOWN["base_flow_index_seasonal_ratio"]
    t = TimeAxis.daily(k["start"], k["T"])
    q = _series(k)
    q[np.isin(t.month, (12, 1, 2))] = k["DJF"]
    q[np.isin(t.month, (6, 7, 8))] = k["JJA"]
    ratio = f.bfi_ratio(q, t)
    np.testing.assert_allclose(ratio[~np.isnan(ratio)], k["want"], atol=k["atol"])
    assert (~np.isnan(ratio)).sum() >= 1
    # Sen slopes: the four seasons of QS-DEC (sorted: DJF, JJA, MAM, SON), then the year of YS-DEC
    k = KNOWN["sen_slope"]
    t = TimeAxis.daily(k["start"], k["T"])
    q = np.arange(k["T"], dtype=np.float64)[:, None]
    for factor in (1.0, k["sim_factor"]):
        got = [f.sen(q * factor, fr, t) for fr in k["freqs"]]
        assert got[0][2] == ["DJF", "JJA", "MAM", "SON"] and got[1][2] == ["annual"]
        slope = np.concatenate([g[0][:, 0] for g in got])
        np.testing.assert_allclose(slope, np.asarray(k["slope"]) * factor, atol=1e-15 if factor == 1.0 else 1e-12)
        np.testing.assert_allclose(np.concatenate([g[1][:, 0] for g in got]), k["p"], rtol=k["p_tol"], atol=k["p_tol"])
        if factor == 1.0:
            obs = slope
    np.testing.assert_allclose(obs / slope, k["ratio"], atol=1e-15)


def test_restatement_reproduces_the_known_answers():
    check_known_answers()


# ---- the golden file -----------------------------------------------------------------------------------------------------
_Z = np.load(GOLDEN) if os.path.exists(GOLDEN) else None      # (absent only while tests/golden/make_hydro_golden.py writes it)
META = json.loads(str(_Z["meta"])) if _Z is not None else {}
CASES = sorted(META)
RUNS = [(n, H.spec_id(s)) for n in CASES for s in META[n]["runs"]]


def golden_case(name):
    m = META[name]
    c = types.SimpleNamespace(name=name, **{k: m[k] for k in ("start", "T", "calendar", "dtype", "C", "runs")})
    c.time = TimeAxis.daily(m["start"], m["T"], m["calendar"])
    c.fields = {k: np.array(_Z[f"{name}/{k}"]) for k in ("q", "snw", "pr")}
    c.expected = {}
    for s in m["runs"]:
        rid = H.spec_id(s)
        c.expected[rid] = {key.split("/", 2)[2]: np.array(_Z[key]) for key in _Z.files if key.startswith(f"{name}/{rid}/")}
    return c


def spec_of(case, run):
    return next(s for s in case.runs if H.spec_id(s) == run)


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 500_000
    assert {META[n]["dtype"] for n in CASES} == {"float32", "float64"} and {META[n]["calendar"] for n in CASES} == {"standard", "noleap"}
    freqs = {s["freq"] for n in CASES for s in META[n]["runs"] if "freq" in s}
    assert freqs == {"YS", "YS-JUL", "YS-OCT", "QS-DEC", "MS"}
    windows = {s["window"] for n in CASES for s in META[n]["runs"] if s["kind"] == "melt"}
    assert {1, 3, 31, hydrology.HYDRO_MAX_WINDOW} <= windows
    c = golden_case("std_f64")
    ys = c.time.segments("YS")[0]
    q = c.fields["q"]
    assert np.isnan(q[0, 1]) and np.isnan(q[ys[1] - 1, 1])                  # row 0, and the last row of a period
    assert np.isnan(q[ys[1]:ys[2], 2]).all() and not np.isnan(q[:31, 2]).any()       # a whole NaN period
    assert np.isnan(q[:, 3]).all() and not np.isnan(q[:, 0]).any()                    # a whole NaN cell, a clean one
    e = c.expected["flow.YS"]
    assert np.isnan(e["bfi"][1, 2]) and e["valid"][1, 2] == 0 and not np.isnan(e["bfi"][0, 0])
    assert np.isnan(e["bfi"][:, 3]).all() and np.isnan(e["rbi"][:, 3]).all() and (e["sum"][:, 3] == 0).all()
    s = golden_case("short_f64").expected                                   # shorter than the 7-day window
    assert np.isnan(s["flow.YS"]["bfi"]).all() and np.isnan(s["api.7.0.935"]["out"]).all() and not np.isnan(s["api.1.0.935"]["out"][:, 0]).any()
    m = c.expected["melt.31.MS.pr"]["out"]                                   # a period shorter than the window still has a value
    assert np.isnan(m[0]).all() and not np.isnan(m[1:, 0]).any()
    assert c.expected["sen.QS-DEC"]["period_of"].min() == -1


@pytest.mark.parametrize("name,run", RUNS)
def test_restatement_reproduces_the_golden_file(name, run):
    c = golden_case(name)
    got = H.run(spec_of(c, run), c.fields, c.time)
    exp = c.expected[run]
    assert set(got) == set(exp)
    if "x" in exp:           # the Sen slope of the recorded period means, whatever this machine's numpy makes of the field
        got = dict(H.sen_slope(exp["x"], exp["period_of"]), x=exp["x"], period_of=exp["period_of"])
    check_run({k: v for k, v in got.items() if not k.endswith("_scale") and k not in ("x", "period_of")}, exp, f"{name} {run}")


def test_identities_of_the_restatement():
    c = golden_case("std_f64")
    q, seg = H.widen(c.fields["q"]), c.time.segments("YS-OCT")[0]
    r = H.flow_period_stats(q, seg)
    m = H.m7(q)[0]
    assert np.isnan(m[:3]).all() and np.isnan(m[-3:]).all() and not np.isnan(m[3:-3, 0]).any()
    np.testing.assert_allclose(m[10, 0], q[7:14, 0].mean(), rtol=1e-14)
    np.testing.assert_allclose(r["mean"][1, 0], q[seg[1]:seg[2], 0].mean(), rtol=1e-14)
    np.testing.assert_allclose(r["rbi"][1, 0], np.abs(np.diff(q[seg[1] - 1:seg[2], 0])).sum() / q[seg[1]:seg[2], 0].sum(), rtol=1e-13)
    snw = H.widen(c.fields["snw"])
    w3 = H.melt_period_max(snw, None, 1.0, 3, seg)["out"]
    np.testing.assert_allclose(w3[1, 0], max(snw[i - 3, 0] - snw[i, 0] for i in range(seg[1], seg[2])), rtol=1e-12)
    # a constant series, ties, and the two-value series
    assert H.mann_kendall(np.full(9, 3.0))[:2] == (0.0, 1.0)
    s, p, n = H.mann_kendall(np.array([1.0, np.nan, 3.0]))
    assert (s, n) == (1.0, 2) and abs(p - 1.0) < 1e-15
    assert np.isnan(H.mann_kendall(np.array([np.nan, 2.0]))[0])


def test_season_tables_of_the_mirror_match_the_restatement():
    for start, T, cal in (("2000-01-01", 1825, "standard"), ("1998-11-17", 800, "noleap"), ("2000-12-01", 365, "standard")):
        t = TimeAxis.daily(start, T, cal)
        for freq in ("YS", "YS-DEC", "YS-JUL", "QS-DEC", "QS", "QS-FEB", "MS"):
            a, b = hydrology.season_year_table(t, freq), H.season_year_table(t, freq)
            np.testing.assert_array_equal(a[0], b[0])
            assert list(a[1]) == list(b[1]) and list(a[2]) == list(b[2])
    table, seasons, years = hydrology.season_year_table(TimeAxis.daily("2000-01-01", 1825), "QS-DEC")
    assert seasons == ["DJF", "JJA", "MAM", "SON"] and list(years) == list(range(1999, 2005))
    assert list(table[:, 0]) == [0, 4, 8, 12, 16, 20] and list(table[:, 2]) == [1, 5, 9, 13, 17, -1]
    np.testing.assert_array_equal(hydrology.api_weights(7, 0.935), H.api_weights(7, 0.935))
    assert hydrology.api_weights(3, 0.5).tolist() == [0.25, 0.5, 1.0]


def test_axes_and_arguments_that_are_not_served():
    t = TimeAxis.daily("2000-01-01", 400)
    q = np.ones((400, 2))
    gappy = t.subset(np.r_[0:10, 11:400])
    with pytest.raises(hydrology.NotServed):
        hydrology.base_flow_index(q[:399], time=gappy)
    with pytest.raises(hydrology.NotServed):
        hydrology.snow_melt_we_max(q, window=hydrology.HYDRO_MAX_WINDOW + 1, time=t)
    with pytest.raises(hydrology.NotServed):
        hydrology.antecedent_precipitation_index(q, window=hydrology.HYDRO_MAX_WINDOW + 1)
    for freq in ("2QS", "7D", "W"):
        with pytest.raises(hydrology.NotServed):
            hydrology.sen_slope(q, freq, time=t)
    long = TimeAxis.daily("1800-01-01", 366 * (hydrology.SEN_MAX_YEARS + 1), "noleap")
    with pytest.raises(hydrology.NotServed, match="years"):
        hydrology.sen_slope(np.ones((len(long), 1), np.float32), "YS", time=long)
    with pytest.raises(ValueError, match="flux_units"):
        hydrology.melt_and_precip_max(q, q, time=t, flux_units="in/d")
    with pytest.raises(ValueError, match="window"):
        hydrology.snow_melt_we_max(q, window=0, time=t)
    with pytest.raises(TypeError):
        hydrology.base_flow_index(q, freq=3, time=t)
    with pytest.raises(ValueError, match="keep=True"):
        hydrology.rb_flashiness_index(q, time=t, keep=True, mask_missing=True)
    assert (hydrology.HYDRO_MAX_WINDOW, hydrology.SEN_MAX_YEARS) == (32, 181)
    txt = open(HEADER).read()
    assert "#define XH_HYDRO_MAX_WINDOW 32" in txt and "#define XH_SEN_MAX_YEARS 181" in txt


# ---- the C ABI (tests/test_abi_cpu.py checks the header against the ctypes table, the library and the registry) ---------
def test_the_unit_is_built_and_its_operand_table_is_the_header_s():
    assert set(S.prototypes(HEADER)) == set(HYDRO_TABLE)
    make = open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()
    assert "hydro.hip" in make and "xclim_hip_hydro.h" in make
    assert '#include "xclim_hip.h"' in open(HEADER).read()


def test_the_integer_outputs_are_the_header_s():
    for name, decl in S.header_declarations(HEADER).items():
        text = {n: t for t, n in decl}
        for op in HYDRO_TABLE[name]:               # the dtype of the table is the declared one
            assert op.mode == "r" or ("int32_t" in text[op.ptr]) == (op.dtype == "i4"), (name, op.ptr)


def test_entry_points_reject_a_null_context():
    lib = _capi.load_library()
    null, some = _vp(0), _vp(64)   # never dereferenced: the check fails first
    assert lib.xh_flow_period_stats(null, 10, 4, 4, 0, some, 1, some, some, some, null, null, null, 4) == _capi.XH_ERR_ARG
    assert lib.xh_melt_period_max(null, 10, 4, 4, 0, some, some, 86400.0, 3, 1, some, some, 4) == _capi.XH_ERR_ARG
    assert lib.xh_antecedent_precip(null, 10, 4, 4, 0, some, 86400.0, 7, some, some, 4) == _capi.XH_ERR_ARG
    assert lib.xh_sen_slope(null, 10, 4, 4, 0, some, 5, 1, some, some, some, null, 4) == _capi.XH_ERR_ARG


def refusals(dev):
    """Every refusal is a code that answers before anything is launched: the sentinel in the outputs is intact afterwards, and the
    same call with nothing wrong then runs.  On the device (tests/test_gpu_hydro.py) and on the host simulation (below)."""
    from newunit_cases import shared_refusals

    ARG, LAYOUT, LIMIT = _capi.XH_ERR_ARG, _capi.XH_ERR_LAYOUT, _capi.XH_ERR_LIMIT
    T, C, P = 40, 8, 2
    x = dev.to_device(np.linspace(1.0, 9.0, T * C).reshape(T, C))
    out = dev.to_device(np.full((T, C), -7.0))
    cnt = dev.to_device(np.full((P, C), -7, np.int32))
    p = lambda a: _vp(0) if a is None else a.ctypes.data_as(_vp)  # noqa: E731
    d = lambda a: _vp(0) if a is None else _vp(a.ptr)             # noqa: E731
    seg = np.array([0, 20, T], np.int64)
    many = np.zeros(65538, np.int64)
    fl, me, ap, se = (getattr(dev.lib, n) for n in HYDRO_TABLE)

    def flow(ld=C, ld_out=C, seg=seg, P=P, q=x, bfi=out, rbi=out, valid=cnt, T=T, C=C, ctx=dev.ctx):
        return fl(ctx, T, C, ld, 1, d(q), P, p(seg), d(bfi), d(rbi), _vp(0), _vp(0), d(valid), ld_out)

    assert flow(ld=C - 1) == LAYOUT and flow(ld_out=C - 1) == LAYOUT                       # a pitch below the row width
    assert flow(seg=None) == ARG and flow(q=None) == ARG and flow(T=-1) == ARG              # NULL arguments, a negative shape
    assert flow(seg=np.array([0, 30, 20], np.int64)) == ARG                                  # a decreasing seg
    assert flow(seg=np.array([0, 20, T + 1], np.int64)) == ARG and flow(seg=np.array([-1, 20, T], np.int64)) == ARG
    assert flow(seg=many, P=65536) == LIMIT                                                  # more than 65535 periods
    assert flow(bfi=None, rbi=None, valid=None) == ARG                                       # no output requested
    shared_refusals(flow, T, C, [("seg", seg, T, dict(seg=many, P=65536))])

    def melt(ld=C, ld_out=C, seg=seg, P=P, snw=x, pr=x, window=3, o=out, T=T, C=C, ctx=dev.ctx):
        return me(ctx, T, C, ld, 1, d(snw), d(pr), 86400.0, window, P, p(seg), d(o), ld_out)

    assert melt(ld=C - 1) == LAYOUT and melt(ld_out=C - 1) == LAYOUT
    assert melt(seg=None) == ARG and melt(snw=None) == ARG and melt(o=None) == ARG and melt(window=0) == ARG
    assert melt(seg=np.array([0, 30, 20], np.int64)) == ARG and melt(seg=many, P=65536) == LIMIT
    assert melt(window=hydrology.HYDRO_MAX_WINDOW + 1) == LIMIT
    shared_refusals(melt, T, C, [("seg", seg, T, dict(seg=many, P=65536))])

    w = H.api_weights(7, 0.935)

    def api(ld=C, ld_out=C, pr=x, window=7, weights=w, o=out, T=T, C=C, ctx=dev.ctx):
        return ap(ctx, T, C, ld, 1, d(pr), 1.0, window, p(weights), d(o), ld_out)

    assert api(ld=C - 1) == LAYOUT and api(ld_out=C - 1) == LAYOUT
    assert api(pr=None) == ARG and api(weights=None) == ARG and api(o=None) == ARG and api(window=0) == ARG
    assert api(window=hydrology.HYDRO_MAX_WINDOW + 1, weights=np.ones(40)) == LIMIT
    shared_refusals(api, T, C)

    Y = 10
    po = np.arange(Y, dtype=np.int64).reshape(Y, 1)
    slope, pv, n1 = dev.to_device(np.full((1, C), -7.0)), dev.to_device(np.full((1, C), -7.0)), dev.to_device(np.full((1, C), -7, np.int32))

    def sen(ld=C, ld_out=C, xx=x, po=po, Y=Y, K=1, s=slope, pp=pv, T=T, C=C, ctx=dev.ctx):
        return se(ctx, T, C, ld, 1, d(xx), Y, K, p(po), d(s), d(pp), d(n1), ld_out)

    assert sen(ld=C - 1) == LAYOUT and sen(ld_out=C - 1) == LAYOUT
    assert sen(xx=None) == ARG and sen(po=None) == ARG and sen(s=None, pp=None) == ARG and sen(Y=-1) == ARG
    bad = po.copy()
    bad[3] = T
    assert sen(po=bad) == ARG                                                                # a row outside x
    bad[3] = -2
    assert sen(po=bad) == ARG
    big = hydrology.SEN_MAX_YEARS + 1
    assert sen(po=np.zeros((big, 1), np.int64), Y=big) == LIMIT                              # one year beyond the limit
    assert sen(po=np.zeros((1, 65536), np.int64), Y=1, K=65536) == LIMIT
    shared_refusals(sen, T, C)

    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((T, C), -7.0))          # nothing was launched: the sentinels are intact
    np.testing.assert_array_equal(cnt.get(), np.full((P, C), -7, np.int32))
    for a in (slope, pv):
        np.testing.assert_array_equal(a.get(), np.full((1, C), -7.0))
    np.testing.assert_array_equal(n1.get(), np.full((1, C), -7, np.int32))
    assert flow() == 0 and sen() == 0 and api() == 0
    dev.sync()
    assert (out.get() != -7.0).all() and (cnt.get() == 20).all() and (n1.get() == Y).all() and (slope.get() > 0).all()
    assert melt() == 0
    dev.sync()
    assert (out.get()[:P] != -7.0).all()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from test_hostsim_units_cpu import sim_device

    return sim_device("hydro", tmp_path_factory)    # the one build of the session


def test_refusals_answer_before_any_launch(sim):
    refusals(sim)


def test_the_simulated_kernels_give_the_known_answers(sim):
    """The same known answers through xclim_amd.hydrology on the host simulation of hydro.hip (and of the existing kernels the
    other indices are built from)."""
    check_known_answers(mirror_api(sim))
