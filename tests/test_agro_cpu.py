"""The agroclimatic heat-sum unit without a GPU: the numpy restatement tests/agrocpu.py against the known answers of the
reference's own tests and against tests/golden/agro_vectors.npz; the host tables and coefficients of xclim_amd.agro against the
restatement's; what of the C ABI of include/xclim_hip_agro.h is the unit's own (tests/test_abi_cpu.py checks header, ctypes table,
library and the operand table of tests/stridedabi.py); the refusals, on the host simulation.  ``golden_case``, ``check``,
``launch`` and ``refusals`` are what tests/test_gpu_agro.py runs on the device.

Tolerance (check): |got - want| <= 1e-12 * scale, for float32 and float64 fields alike, because both widen the same values;
scale is the sum of the absolute day or month terms that went into the value (the mean's for a mean), stored next to it.  At
most 366 terms, a handful of roundings each, eps = 1.1e-16: about 2e-13; 1e-12 is the project's float64 bound elsewhere.
Counts, the EGDD start / end days and the NaN patterns must match exactly."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import agrocpu as A
import stridedabi as S
from stridedabi import AGRO_TABLE
from xclim_amd import _capi, agro
from xclim_amd.calendar import select_time_mask
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "xclim_hip_agro.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "agro_vectors.npz")
RTOL = 1e-12
K2C = 273.15
_vp = ctypes.c_void_p


# ---- the known answers of the reference's tests ----------------------------------------------------------------------
# tests/golden/agro_known_answers.json holds the recorded inputs and expected values (degC, null = NaN); the assertions made on
# them are below.
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "agro_known_answers.json")))


def _nan(v):
    return np.array([np.nan if x is None else x for x in v], np.float64)


def _column(v):
    return (np.asarray(v, np.float64) + K2C)[:, None]


BEDD_ANSWERS = [tuple(r) for r in KNOWN["bedd"]["rows"]]
JONES_ANSWERS = [tuple(r) for r in KNOWN["jones"]["rows"]]
HUGLIN_LATS = np.asarray(KNOWN["huglin"]["lat"], np.float64)
HUGLIN_OUT = [(m, np.nan if cap is None else cap, _nan(want)) for m, cap, want in KNOWN["huglin"]["rows"]]


def bedd_inputs():
    """The axis, latitudes, tasmin field (K) and the two tasmax - tasmin offsets of the BEDD known answers."""
    b = KNOWN["bedd"]
    tn = np.zeros((b["T"], len(b["lat"]))) + b["tasmin"] + K2C
    return TimeAxis.daily(b["start"], b["T"]), np.asarray(b["lat"], np.float64), tn, [tx - b["tasmin"] for tx in b["tasmax"]]


def _bedd(method, end_date, freq, tx_offset):
    t, lat, tn, _ = bedd_inputs()
    spec = dict(kind="bedd", method=method, freq=freq, end_date=end_date)
    return A.run(spec, dict(tasmin=tn, tasmax=tn + tx_offset), lat, t, K2C, 86400.0, (KNOWN["bedd"]["start_date"],))["bedd"].T   # (lat, time)


def check_bedd(method, end_date, freq, deg_days, max_deg_days, run=_bedd):
    """Every assertion of the reference's test_bedd for one of its parameter sets; ``run(method, end_date, freq, tasmax -
    tasmin)`` gives the (lat, time) result (the restatement's, or the device's in tests/test_gpu_agro.py)."""
    warm, hotter = bedd_inputs()[3]
    if method == "jones" and freq == "MS":
        with pytest.raises(NotImplementedError):
            run(method, end_date, freq, warm)
        return
    bedd, hot = run(method, end_date, freq, warm), run(method, end_date, freq, hotter)
    if freq == "YS":
        np.testing.assert_allclose(np.array([deg_days] * 3), bedd[1][:3], atol=0.125)
        np.testing.assert_allclose(np.array([max_deg_days] * 3), hot[0][:3], atol=0.1)
        if method == "icclim":
            np.testing.assert_array_equal(bedd[0], bedd[-1])
        elif method in ("huglin", "interpolated"):
            np.testing.assert_array_equal(bedd[0][0], bedd[0][1])
        else:
            np.testing.assert_array_less(bedd[0], bedd[1])
            np.testing.assert_array_less(bedd[1], bedd[2])
    else:
        last = [deg_days] if method != "icclim" else [0]
        np.testing.assert_allclose(np.array([deg_days] * 6 + last), bedd[0][3:10], rtol=0.125)
        np.testing.assert_allclose(np.array([max_deg_days] * 6 + ([max_deg_days] if method != "icclim" else [0])), hot[0][3:10], rtol=0.1)
        if method == "icclim":
            np.testing.assert_array_equal(bedd[0][3:10], bedd[-1][3:10])
        elif method in ("huglin", "interpolated"):
            np.testing.assert_array_equal(bedd[0][3:10], bedd[0][15:22])
        else:
            np.testing.assert_array_less(bedd[0][3:9], bedd[1][3:9])
            np.testing.assert_array_less(bedd[1][9], bedd[0][9])
            np.testing.assert_array_less(bedd[1][3:9], bedd[2][3:9])
            np.testing.assert_array_less(bedd[2][9], bedd[1][9])


def check_jones(method, start_date, end_date, freq, floor, results):
    """The Jones and Gladstones coefficient table, 2 decimals."""
    start, n = KNOWN["jones"]["axes"][freq]
    t = TimeAxis.daily(start, n)
    lats = np.asarray(KNOWN["jones"]["lat"], np.float64)
    if results is None:
        with pytest.raises(ValueError):
            A.jones_k_period(t, lats, start_date, end_date, freq, drop=True)
        return
    k = A.jones_k_period(t, lats, start_date, end_date, freq, drop=True)
    if method == "gladstones":
        k = 1.1135 * k - 0.1352
    if floor:
        k = np.where(k >= 1.0, k, 1.0)
    np.testing.assert_array_almost_equal(k[0], results, 2)


def egdd_series():
    e = KNOWN["egdd"]
    tas = np.asarray(e["tas"], np.float64)
    return TimeAxis.daily(e["start"], len(tas)), _column(tas - e["half_range"]), _column(tas + e["half_range"])


def check_known_answers(chu=A.corn_heat_units, qian=A.qian_wma, egdd=None, huglin=A.huglin_coefficient, tables=True):
    """Every reproducible known answer of the reference's tests, to the tolerance each is asserted with.  The callables default
    to the restatement; tests/test_gpu_agro.py hands in the device's."""
    c, q, e = KNOWN["chu"], KNOWN["qian"], KNOWN["egdd"]
    np.testing.assert_allclose(chu(_column(c["tasmin"]), _column(c["tasmax"]))[:, 0], c["out"])
    out = qian(_column(q["tas"]))[:, 0]
    np.testing.assert_array_equal(out[q["first"]:q["first"] + len(q["out_K"])], q["out_K"])      # exact
    assert out[50] < 10 + K2C and out[51] > K2C
    t, tn, tx = egdd_series()
    for method, want in e["out"].items():
        got = egdd(t, tn, tx, method) if egdd else A.egdd(tn, tx, *A.egdd_tables(t, e["freq"]), method=method)["egdd"]
        np.testing.assert_array_equal(np.asarray(got)[:, 0], _nan(want))                          # exact
    for method, cap, want in HUGLIN_OUT:
        np.testing.assert_array_almost_equal(huglin(HUGLIN_LATS, method, cap), want, decimal=2)
    if tables:
        for row in BEDD_ANSWERS:
            check_bedd(*row)
        for row in JONES_ANSWERS:
            check_jones(*row)


def test_chu_qian_egdd_and_huglin_coefficient_known_answers():
    check_known_answers(tables=False)


@pytest.mark.parametrize("method,end_date,freq,deg_days,max_deg_days", BEDD_ANSWERS)
def test_bedd_known_answers(method, end_date, freq, deg_days, max_deg_days):
    check_bedd(method, end_date, freq, deg_days, max_deg_days)


@pytest.mark.parametrize("row", JONES_ANSWERS, ids=lambda r: f"{r[0]}-{r[3]}-{r[1]}")
def test_jones_coefficient_known_answers(row):
    check_jones(*row)


def test_the_mirror_coefficient_keeps_the_quirk_beyond_fifty_degrees():
    """helpers.py:604 is full_like(lat_abs, cap + 1): "huglin" gives cap_value + 1 beyond 50 degrees, "interpolated" cap_value."""
    for method, cap, want in HUGLIN_OUT:
        np.testing.assert_array_almost_equal(agro.huglin_day_length_latitude_coefficient(HUGLIN_LATS, method, cap), np.array(want), decimal=2)
    lat = np.array([30.0, 45.0, 50.0, 50.5, -70.0])
    np.testing.assert_array_equal(agro.huglin_day_length_latitude_coefficient(lat, "huglin", 1.0), [1.0, 1.04, 1.06, 2.0, 2.0])
    np.testing.assert_array_equal(agro.huglin_day_length_latitude_coefficient(lat, "interpolated", 1.0)[3:], [1.0, 1.0])
    np.testing.assert_array_equal(agro.huglin_day_length_latitude_coefficient(lat, "huglin", 1.0), A.huglin_coefficient(lat, "huglin", 1.0))
    with pytest.raises(TypeError):
        agro.huglin_day_length_latitude_coefficient(lat, "huglin", 1)
    with pytest.raises(NotImplementedError):
        agro.huglin_day_length_latitude_coefficient(lat, "smoothed", 1.0)


# ---- the golden file -------------------------------------------------------------------------------------------------
_Z = np.load(GOLDEN) if os.path.exists(GOLDEN) else None      # (absent only while tests/golden/make_agro_golden.py writes it)
META = json.loads(str(_Z["meta"])) if _Z is not None else {}
CASES = sorted(META)
FIELDS = ("tas", "tasmin", "tasmax", "pr", "evspsblpot")


def spec_id(s):
    return ".".join(str(s[k]) for k in ("kind", "method", "freq") if k in s)


def golden_case(name):
    m = META[name]
    c = types.SimpleNamespace(name=name, **m)
    c.fields = {k: _Z[f"{name}/{k}"] for k in FIELDS if f"{name}/{k}" in _Z.files}
    c.time = TimeAxis.daily(m["start"], m["T"], m["calendar"])
    c.lat = np.asarray(m["lat"], np.float64)
    c.sub_C = K2C if m["units"] == "K" else 0.0
    c.season = (m["season_start"],)
    c.expected = {spec_id(s): {k.split("/")[2]: _Z[k] for k in _Z.files if k.startswith(f"{name}/{spec_id(s)}/")} for s in m["runs"]}
    return c


RUNS = [(n, spec_id(s)) for n in CASES for s in META[n]["runs"]]


def spec_of(case, run):
    return next(s for s in case.runs if spec_id(s) == run)


def check(got, want, scale, what):
    """One output against its expected value (the module text): integers and the EGDD bound days exactly, the same NaN pattern,
    everything else within RTOL * scale."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if scale is None:
        np.testing.assert_array_equal(got, want, err_msg=what)
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    bad = err > RTOL * np.asarray(scale)
    assert not bad.any(), f"{what}: {int(bad.sum())} values beyond {RTOL} * scale, worst {np.nanmax(err / np.maximum(scale, 1e-300)):.3g} of scale"


def check_run(got, exp, what):
    for k, v in got.items():
        check(v, exp[k], exp.get(k + "_scale"), f"{what} {k}")


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 500_000
    assert {"midyear_f64", "midyear_f32", "noleap_f32", "360day_f64", "years_f32", "water_f64"} <= set(CASES)
    assert {META[n]["dtype"] for n in CASES} == {"float32", "float64"}
    assert {META[n]["calendar"] for n in CASES} == {"standard", "noleap", "360_day"}
    assert {s["freq"] for n in CASES for s in META[n]["runs"]} == {"YS", "YS-JUL", "MS"}
    assert META["midyear_f64"]["start"] == "1999-03-15" and META["midyear_f64"]["T"] == 1002
    lats = np.abs(np.concatenate([META[n]["lat"] for n in CASES]))
    for edge in (40, 50, 66.56):
        assert (lats < edge).any() and (lats > edge).any()
    assert any(np.signbit(v) for n in CASES for v in META[n]["lat"]) and any(v > 0 for n in CASES for v in META[n]["lat"])
    kinds = {(s["kind"], s.get("method")) for n in CASES for s in META[n]["runs"]}
    assert {("hi", "huglin"), ("hi", "interpolated"), ("hi", "jones"), ("bedd", "gladstones"), ("bedd", "icclim"), ("bedd", "jones"),
            ("both", "interpolated"), ("egdd", "bootsma"), ("egdd", "qian"), ("monthly", None)} <= kinds
    c = golden_case("midyear_f64")
    week = np.flatnonzero(np.isnan(c.fields["tasmax"][:, 1]) & (c.time.month == 6) & (c.time.day >= 10) & (c.time.day <= 16))
    assert len(week) >= 7                                                        # the NaN week inside the season
    e = c.expected["bedd.huglin.YS"]
    full = select_time_mask(c.time, date_bounds=("04-01", "11-01"), include_bounds=(True, False))
    seg = c.time.segments("YS")[0]
    assert e["valid"][0, 1] <= full[seg[0]:seg[1]].sum() - 7 and c.time.year[week[0]] == 1999
    assert "di" in golden_case("water_f64").expected["monthly.YS"] and "di" not in c.expected["monthly.YS"]
    assert any(np.isnan(golden_case(n).expected[r]["egdd"]).any() and not np.isnan(golden_case(n).expected[r]["egdd"]).all()
               for n, r in RUNS if r.startswith("egdd"))


@pytest.mark.parametrize("name,run", RUNS)
def test_restatement_reproduces_the_golden_file(name, run):
    c = golden_case(name)
    got = A.run(spec_of(c, run), c.fields, c.lat, c.time, c.sub_C, c.per_day, c.season)
    got.pop("min_gap", None)
    exp = c.expected[run]
    assert set(got) == set(exp)
    for k in exp:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{name} {run} {k}")


def test_the_restated_day_length_is_the_solar_table_s():
    import petcpu
    from xclim_amd import converters as xc

    t = TimeAxis.daily("1999-03-15", 500)
    lats = np.array([-67.5, -40.0, 0.0, 35.0, 40.0, 70.0])
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(A.day_lengths(t, lats), petcpu.solar_table(xc.day_angle(t), lats)[1])


def test_identities_of_the_restatement():
    """What the reference's data-file tests would pin, as identities: di(wo=300) == di(wo=200) + 100; CNI of an all-north field is
    the September mean; HI with k = 1 on an all-north and an all-south latitude set."""
    c = golden_case("water_f64")
    tabs = A.month_tables(c.time, "YS")
    f = c.fields
    a = A.monthly(f["tasmin"], None, f["pr"], f["evspsblpot"], c.lat, *tabs, sub_C=c.sub_C, wo=200.0)
    b = A.monthly(f["tasmin"], None, f["pr"], f["evspsblpot"], c.lat, *tabs, sub_C=c.sub_C, wo=300.0)
    np.testing.assert_allclose(b["di"], a["di"] + 100, rtol=1e-13)
    north = A.monthly(f["tasmin"], None, None, None, None, *tabs, hemisphere="north", sub_C=c.sub_C)["cni"]
    sep = np.array([np.nanmean(f["tasmin"][(c.time.year == y) & (c.time.month == 9)] - c.sub_C, axis=0) for y in (2000, 2001)])
    np.testing.assert_allclose(north, sep, rtol=1e-13)
    seg = c.time.segments("YS")[0]
    sel = select_time_mask(c.time, date_bounds=("04-01", "10-01"), include_bounds=(True, False))
    plain = A.degree_sum(f["tas"], None, f["tasmax"], seg, sel, None, None, sub_C=c.sub_C)["hi"]
    for lats in (np.array([10.0, 25, 39]), -np.array([10.0, 25, 39])):      # |lat| <= 40: k = 1 in both hemispheres
        k = A.huglin_coefficient(lats, "huglin", 1.0)
        np.testing.assert_array_equal(A.degree_sum(f["tas"], None, f["tasmax"], seg, sel, k, None, sub_C=c.sub_C)["hi"], plain)


@pytest.mark.parametrize("name", CASES)
def test_host_tables_match_the_restatement(name):
    c = golden_case(name)
    for freq in sorted({s["freq"] for s in c.runs}):
        for got, want in zip(agro.month_tables(c.time, freq), A.month_tables(c.time, freq)):
            np.testing.assert_array_equal(got, want)
            assert got.dtype == want.dtype
        for got, want in zip(agro.egdd_tables(c.time, freq), A.egdd_tables(c.time, freq)):
            np.testing.assert_array_equal(got, want)
            assert got.dtype == want.dtype


def test_axes_and_arguments_that_are_not_served():
    t = TimeAxis.daily("2001-01-01", 400)
    x = np.full((400, 2), 280.0)
    gappy = t.subset(np.r_[0:100, 101:400])
    with pytest.raises(agro.NotServed):
        agro.huglin_index(x[:399], x[:399], [45.0, 46.0], method="huglin", time=gappy)
    with pytest.raises(agro.NotServed):
        agro.dryness_index(x, x, "north", time=TimeAxis.daily("2001-01-02", 400))
    with pytest.raises(agro.NotServed):
        agro.cool_night_index(x[:30], "north", time=TimeAxis.daily("2001-04-01", 30))
    with pytest.raises(ValueError, match="Freq not allowed"):
        agro.cool_night_index(x, "north", freq="YS-JUL", time=t)
    with pytest.raises(ValueError, match="Freq not allowed"):
        agro.dryness_index(x, x, "north", freq="MS", time=t)
    with pytest.raises(NotImplementedError):       # the reference's own default method is one it does not implement
        agro.huglin_index(x, x, [45.0, 46.0], time=t)
    with pytest.raises(NotImplementedError):
        agro.biologically_effective_degree_days(x, x, [45.0, 46.0], method="smoothed", time=t)
    with pytest.raises(NotImplementedError, match="Method: toto"):
        agro.effective_growing_degree_days(x, x, method="toto", time=t)
    with pytest.raises(ValueError, match="units"):
        agro.corn_heat_units(x, x, units="F")
    with pytest.raises(ValueError, match="flux_units"):
        agro.dryness_index(x[:365], x[:365], "north", time=TimeAxis.daily("2001-01-01", 365), flux_units="in/d")


# ---- the C ABI (tests/test_abi_cpu.py checks the header against the ctypes table, the library and the registry) ---------
def test_the_unit_is_built_and_its_operand_table_is_the_header_s():
    assert set(S.prototypes(HEADER)) == set(AGRO_TABLE)
    assert "agro.hip" in open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()
    assert '#include "xclim_hip.h"' in open(HEADER).read()


def test_the_outputs_have_the_rows_and_the_integer_type_of_the_header():
    for name, decl in S.header_declarations(HEADER).items():
        text = {n: t for t, n in decl}
        for op in AGRO_TABLE[name]:                # the dtype of the table is the declared one
            assert op.mode == "r" or ("int32_t" in text[op.ptr]) == (op.dtype == "i4"), (name, op.ptr)
        out_rows = {op.rows for op in AGRO_TABLE[name] if op.mode == "w"}
        assert out_rows == ({"T"} if name in ("xh_corn_heat_units", "xh_qian_wma") else {"P"})


def test_entry_points_reject_a_null_context():
    lib = _capi.load_library()
    null, some = _vp(0), _vp(64)   # never dereferenced: the check fails first
    assert lib.xh_agro_degree_sum(null, 10, 4, 4, 0, some, some, some, 1, some, null, null, null, null, 0, null, 0.0, 10.0, 10.0, 1, 10.0,
                                  13.0, 9.0, some, some, null, 4) == _capi.XH_ERR_ARG
    assert lib.xh_agro_monthly(null, 10, 4, 4, 0, some, some, some, some, 1, some, some, some, 1, some, some, 0, 0.0, 1.0, 200.0, some, some,
                               some, null, 4) == _capi.XH_ERR_ARG
    assert lib.xh_egdd(null, 10, 4, 4, 0, some, some, 1, some, some, some, some, some, some, some, 0, 0.0, 5.0, some, null, null, null,
                       4) == _capi.XH_ERR_ARG
    assert lib.xh_corn_heat_units(null, 10, 4, 4, 0, some, some, 0.0, 4.44, 10.0, some, 4) == _capi.XH_ERR_ARG
    assert lib.xh_qian_wma(null, 10, 4, 4, 0, some, some, 4) == _capi.XH_ERR_ARG


def refusals(dev):
    """Every refusal is a code that answers before anything is launched: the sentinel in the outputs is intact afterwards, and the
    same call with nothing wrong then runs.  On the device (tests/test_gpu_agro.py) and on the host simulation (below)."""
    from newunit_cases import shared_refusals

    ARG, LAYOUT, LIMIT = _capi.XH_ERR_ARG, _capi.XH_ERR_LAYOUT, _capi.XH_ERR_LIMIT
    T, C, P = 40, 8, 2
    x = dev.to_device(np.full((T, C), 290.0))
    out = dev.to_device(np.full((T, C), -7.0))
    cnt = dev.to_device(np.full((P, C), -7, np.int32))
    kc = dev.to_device(np.ones(C))
    kd = dev.to_device(np.ones((T, 1)))
    li = dev.to_device(np.zeros(C, np.int32))
    p = lambda a: _vp(0) if a is None else a.ctypes.data_as(_vp)  # noqa: E731
    d = lambda a: _vp(0) if a is None else _vp(a.ptr)             # noqa: E731
    seg = np.array([0, 20, T], np.int64)
    many = np.zeros(65538, np.int64)

    deg = dev.lib.xh_agro_degree_sum

    def degree(ld=C, ld_out=C, seg=seg, P=P, tas=x, tasmin=x, tasmax=x, k_cell=None, k_day=None, lat_idx=None, L=0, hi=out, bedd=out,
               T=T, C=C, ctx=dev.ctx):
        return deg(ctx, T, C, ld, 1, d(tas), d(tasmin), d(tasmax), P, p(seg), _vp(0), d(k_cell), d(k_day), _vp(0), L, d(lat_idx), K2C,
                   10.0, 10.0, 1, 10.0, 13.0, 9.0, d(hi), d(bedd), d(cnt), ld_out)

    assert degree(ld=C - 1) == LAYOUT and degree(ld_out=C - 1) == LAYOUT                   # a pitch below the row width
    assert degree(seg=None) == ARG and degree(tasmax=None) == ARG and degree(tas=None) == ARG and degree(tasmin=None) == ARG   # NULL arguments
    assert degree(seg=np.array([0, 30, 20], np.int64)) == ARG                              # a decreasing seg
    assert degree(seg=np.array([0, 20, T + 1], np.int64)) == ARG and degree(seg=np.array([-1, 20, T], np.int64)) == ARG
    assert degree(seg=many, P=65536) == LIMIT                                              # more than 65535 periods
    assert degree(hi=None, bedd=None) == ARG                                               # no output requested
    assert degree(k_cell=kc, k_day=kd, lat_idx=li, L=1) == ARG                             # both k_cell and k_day
    assert degree(k_day=kd, L=1) == ARG                                                    # k_day without lat_idx
    shared_refusals(degree, T, C, [("seg", seg, T, dict(seg=many, P=65536))])

    mo, mc, md, sm = np.array([0, 31, T], np.int64), np.array([1, 2], np.int32), np.array([31, 28], np.int32), np.array([0, 1, 2], np.int64)
    mon = dev.lib.xh_agro_monthly

    def monthly(mo=mo, mc=mc, md=md, sm=sm, lat=kc, hemisphere=0, cni=out, di=out, pr=x, ld=C, ld_out=C, P=P, T=T, C=C, ctx=dev.ctx):
        return mon(ctx, T, C, ld, 1, d(x), d(x), d(pr), d(x), 2, p(mo), p(mc), p(md), P, p(sm), d(lat), hemisphere, K2C, 86400.0, 200.0,
                   d(cni), _vp(0), d(di), d(cnt), ld_out)

    assert monthly(ld=C - 1) == LAYOUT
    for k in ("mo", "mc", "md", "sm"):
        assert monthly(**{k: None}) == ARG, k
    assert monthly(mo=np.array([0, 35, 31], np.int64)) == ARG and monthly(mo=np.array([0, 31, T + 1], np.int64)) == ARG
    assert monthly(sm=np.array([0, 2, 1], np.int64)) == ARG and monthly(sm=np.array([0, 1, 3], np.int64)) == ARG
    assert monthly(mc=np.array([1, 13], np.int32)) == ARG and monthly(md=np.array([31, 0], np.int32)) == ARG
    assert monthly(cni=None, di=None) == ARG and monthly(pr=None) == ARG
    assert monthly(hemisphere=3) == ARG and monthly(lat=None) == ARG
    shared_refusals(monthly, T, C, [("sm", sm, 2, dict(sm=many, P=65536)), ("mo", mo, T, None)])

    doy = np.arange(1, T + 1, dtype=np.int32)
    sf, ef, d0 = np.array([0, 20], np.int64), np.array([5, -1], np.int64), np.zeros(P, np.int64)
    ldoy, ldays = np.ones(P, np.int32), np.full(P, 365, np.int32)
    eg = dev.lib.xh_egdd

    def egdd(seg=seg, doy=doy, sf=sf, ef=ef, d0=d0, ldoy=ldoy, ldays=ldays, method=0, o=out, tasmin=x, ld_out=C, ld=C, P=P, T=T, C=C,
             ctx=dev.ctx):
        return eg(ctx, T, C, ld, 1, d(tasmin), d(x), P, p(seg), p(doy), p(sf), p(ef), p(d0), p(ldoy), p(ldays), method, K2C, 5.0, d(o),
                  _vp(0), _vp(0), d(cnt), ld_out)

    assert egdd(ld_out=C - 1) == LAYOUT and egdd(tasmin=None) == ARG and egdd(o=None) == ARG and egdd(method=2) == ARG
    for k in ("seg", "doy", "sf", "ef", "d0", "ldoy", "ldays"):
        assert egdd(**{k: None}) == ARG, k
    assert egdd(seg=np.array([0, 30, 20], np.int64)) == ARG
    assert egdd(sf=np.array([0, 5], np.int64)) == ARG and egdd(ef=np.array([25, -1], np.int64)) == ARG     # a row outside its period
    assert egdd(doy=np.zeros(T, np.int32)) == ARG and egdd(ldays=np.full(P, 300, np.int32)) == ARG
    shared_refusals(egdd, T, C, [("seg", seg, T, dict(seg=many, P=65536))])

    chu, qian = dev.lib.xh_corn_heat_units, dev.lib.xh_qian_wma
    assert chu(dev.ctx, T, C, C - 1, 1, d(x), d(x), K2C, 4.44, 10.0, d(out), C) == LAYOUT
    assert chu(dev.ctx, T, C, C, 1, d(x), _vp(0), K2C, 4.44, 10.0, d(out), C) == ARG
    assert chu(dev.ctx, T, C, C, 1, d(x), d(x), K2C, 4.44, 10.0, _vp(0), C) == ARG
    assert qian(dev.ctx, T, C, C, 1, d(x), d(out), C - 1) == LAYOUT and qian(dev.ctx, T, C, C, 1, _vp(0), d(out), C) == ARG
    assert qian(dev.ctx, -1, C, C, 1, d(x), d(out), C) == ARG
    shared_refusals(lambda ctx=dev.ctx, T=T, C=C, ld=C, ld_out=C: chu(ctx, T, C, ld, 1, d(x), d(x), K2C, 4.44, 10.0, d(out), ld_out), T, C)
    shared_refusals(lambda ctx=dev.ctx, T=T, C=C, ld=C, ld_out=C: qian(ctx, T, C, ld, 1, d(x), d(out), ld_out), T, C)

    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((T, C), -7.0))          # nothing was launched: the sentinels are intact
    np.testing.assert_array_equal(cnt.get(), np.full((P, C), -7, np.int32))
    assert degree(bedd=None) == 0 and monthly(di=None) == 0 and egdd() == 0 and qian(dev.ctx, T, C, C, 1, d(x), d(out), C) == 0
    dev.sync()
    assert (out.get() != -7.0).all() and (cnt.get() == 20).all()


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    from test_hostsim_units_cpu import sim_device

    return sim_device("agro", tmp_path_factory)    # the one build of the session


def test_refusals_answer_before_any_launch(sim):
    refusals(sim)


def test_the_simulated_kernels_give_the_known_answers(sim):
    """The same known answers through xclim_amd.agro on the host simulation of agro.hip."""
    egdd = lambda t, tn, tx, m: agro.effective_growing_degree_days(tx, tn, method=m, time=t, device=sim)   # noqa: E731
    check_known_answers(chu=lambda tn, tx: agro.corn_heat_units(tn, tx, device=sim), qian=lambda x: agro.qian_weighted_mean_average(x, device=sim),
                        egdd=egdd, huglin=agro.huglin_day_length_latitude_coefficient, tables=False)
