"""The ANUCLIM variables without a GPU: the numpy restatement tests/anuclimcpu.py against tests/golden/anuclim_vectors.npz and
the known answers of the reference's own tests (stored there as cases "ka_*"), the host tables of xclim_amd.anuclim against
the restatement's, the single-pass formula's measured distance, and the C ABI of xh_bioclim (header, ctypes, refusals with a
NULL context).  ``golden_case`` is what tests/test_gpu_bioclim.py loads its cases with."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import anuclimcpu as A
import stridedabi as S
from xclim_amd import _capi, anuclim
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
GOLDEN = os.path.join(ROOT, "tests", "golden", "anuclim_vectors.npz")
RTOL64, RTOL32 = 1e-12, 1e-6      # the standing bounds for float64 units and for means of float32 fields
FIELDS = ("tas", "tasmin", "tasmax", "pr")
_Z = np.load(GOLDEN)
META = json.loads(str(_Z["meta"]))
CV_BOUND = 4 * float(_Z["cv_single_pass_dev"])   # BIO4 / BIO15: four times the measured distance of the single-pass formula
CASES = sorted(META)
KNOWN = [n for n in CASES if n.startswith("ka_")]
SEEDED = [n for n in CASES if not n.startswith("ka_")]


def time_axis(kind, start, T, calendar):
    if kind == "D":
        return TimeAxis.daily(start, T, calendar)
    if kind == "W":
        return TimeAxis.daily(start, 7 * T, calendar).subset(slice(None, None, 7))
    y, m, _ = (int(p) for p in start.split("-"))
    mo = y * 12 + m - 1 + np.arange(T)
    return TimeAxis(mo // 12, mo % 12 + 1, np.ones(T, np.int64), calendar)


def golden_case(name):
    m = META[name]
    c = types.SimpleNamespace(name=name, **m)
    c.fields = {k: _Z[f"{name}/{k}"] for k in FIELDS if f"{name}/{k}" in _Z.files}
    c.time = time_axis(m["kind"], m["start"], m["T"], m["calendar"])
    c.days = {"D": np.ones(m["T"]), "W": np.full(m["T"], 7.0)}.get(m["kind"])
    if c.days is None:
        c.days = c.time.days_in_month().astype(np.float64)
    c.factor = m["per_day"] * c.days
    c.expected = {f: {k.split("/")[2]: _Z[k] for k in _Z.files if k.startswith(f"{name}/{f}/")} for f in m["freqs"]}
    c.tables = lambda freq: A.tables(c.time.year, c.time.month, m["kind"], freq)
    # the keywords of xclim_amd.anuclim that describe the same units
    c.units = "degC" if m["kelvin"] else "K"
    c.pr_units = {(86400.0, 86400.0): "kg m-2 s-1", (1.0, 1.0): "mm/d", (1 / 7, 1.0): "mm/week", (12 / 365.25, 1.0): "mm/month"}[
        (m["per_day"], m["cv_scale"])]
    return c


def check(got, exp, name, dtype, what=""):
    """One output against its expected value: the step indices and counts exactly, BIO4 / BIO15 within the measured bound of
    the single-pass formula, everything else within the standing bound of the fields' dtype; the same NaN pattern."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, name, got.shape, exp.shape)
    if exp.dtype.kind == "i":
        np.testing.assert_array_equal(got, exp, err_msg=f"{what} {name}")
        return
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{what} {name}: NaN pattern")
    rtol = RTOL32 if np.dtype(dtype) == np.float32 else RTOL64
    if name in ("bio4", "bio15"):   # float32 rows are widened before the accumulation: the measured bound holds for them too
        rtol = CV_BOUND
    np.testing.assert_allclose(got, exp, rtol=rtol, atol=0, equal_nan=True, err_msg=f"{what} {name}")


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert len(KNOWN) >= 20 and {"midyear_f64", "midyear_nan_f32", "short_f64", "noleap_f32", "360day_f64", "weekly_f64", "monthly_f32",
                                 "constant_f64", "tropical_f64", "midyear_thresh_f64"} <= set(SEEDED)
    assert {META[n]["dtype"] for n in SEEDED} == {"float32", "float64"}
    assert 0 < CV_BOUND <= 4e-10, "the single-pass formula would have been rejected above 1e-10"


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden_file(name):
    c = golden_case(name)
    for freq, exp in c.expected.items():
        so, sr, ss, W = c.tables(freq)
        got = A.bioclim(c.fields, so, c.factor, sr, ss, W, c.kind == "D", c.kelvin, c.cv_scale, c.thresh)
        assert set(got) == set(exp)
        for k in exp:
            np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{name} {freq} {k}")


@pytest.mark.parametrize("name", KNOWN)
def test_known_answers_of_the_reference(name):
    """tests/test_indices.py:2797-3085 of the reference, to the 6 decimals it asserts them with."""
    c = golden_case(name)
    assert c.answers
    for key, want in c.answers.items():
        np.testing.assert_array_almost_equal(c.expected["YS"][key][:, 0], want, decimal=6)


@pytest.mark.parametrize("name", CASES)
def test_single_pass_formula_stays_within_its_measured_distance(name):
    c = golden_case(name)
    for freq, exp in c.expected.items():
        so, sr, ss, W = c.tables(freq)
        one = A.bioclim(c.fields, so, c.factor, sr, ss, W, c.kind == "D", c.kelvin, c.cv_scale, c.thresh, single_pass=True)
        for k in ("bio4", "bio15"):
            if k in exp:
                np.testing.assert_allclose(one[k], exp[k], rtol=CV_BOUND / 4, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", CASES)
def test_host_tables_match_the_restatement(name):
    c = golden_case(name)
    for freq in c.freqs:
        so, sr, ss, W = c.tables(freq)
        tab = anuclim.axis_tables(c.time, freq)
        assert tab["kind"] == c.kind and tab["W"] == W and tab["binned"] == (c.kind == "D")
        for k, v in (("step_off", so), ("seg_rows", sr), ("seg_steps", ss)):
            np.testing.assert_array_equal(tab[k], v, err_msg=k)
        np.testing.assert_array_equal(tab["days"], c.days)


def test_the_cases_hold_what_they_are_there_for():
    c = golden_case("midyear_f64")
    e = c.expected["YS"]
    so, sr, ss, _ = c.tables("YS")
    assert ss[1] - ss[0] > 12 and so[-1] - so[-2] == 1            # (YS: 42 steps in 1999; a last bin of one day)
    so, sr, ss, _ = c.tables("YS-JUL")
    assert ss[1] - ss[0] == 16 and (c.expected["YS-JUL"]["wettest"][0] >= 12).all()   # a first period of few steps: 4 quarters
    c = golden_case("short_f64")
    e = c.expected["YS"]
    assert all(np.isnan(e[f"bio{k}"]).all() for k in (8, 9, 10, 11, 16, 17, 18, 19)) and all((e[w] == -1).all() for w in A.WHICH)
    assert not np.isnan(e["bio1"]).any()
    e = golden_case("midyear_nan_f32").expected["YS"]
    assert np.isnan(e["bio1"][:, 3]).all() and (e["bio12"][:, 3] == 0).all() and (e["warmest"][:, 3] == -1).all()
    assert e["warmest"][1, 4] == -1 and np.isnan(e["bio18"][1, 4]) and e["wettest"][1, 4] >= 0     # a criterion that is all NaN
    assert np.isnan(e["bio8"][1, 4]) and not np.isnan(e["bio16"][1, 4])                            # a picked value that is NaN
    e = golden_case("constant_f64").expected["YS"]
    assert (e["wettest"][0] == 12).all() and (e["warmest"] == [[12], [53]]).all() and (e["bio4"] == 0).all()
    c = golden_case("tropical_f64")
    x = c.fields["tas"][:365].astype(np.float64)
    naive = 100 * np.sqrt(np.maximum((x ** 2).sum(0) / 365 - (x.sum(0) / 365) ** 2, 0)) / (x.sum(0) / 365)
    assert (np.abs(naive - c.expected["YS"]["bio4"][0]) > 1e-10 * c.expected["YS"]["bio4"][0]).any()   # the naive sum of squares fails it


def test_axes_that_are_not_served():
    t = TimeAxis.daily("2001-01-01", 400)
    gappy = t.subset(np.r_[0:100, 101:400])
    for bad in (gappy, t.subset(slice(None, None, 3)), t.subset(slice(0, 2))):
        with pytest.raises(anuclim.NotServed):
            anuclim.axis_tables(bad, "YS")
    with pytest.raises(anuclim.NotServed):
        anuclim.axis_tables(t, "7D")
    for fn, args in ((anuclim.tg_mean_warmcold_quarter, (None, t, "wettest")), (anuclim.prcptot_wetdry_quarter, (None, t, "toto")),
                     (anuclim.tg_mean_wetdry_quarter, (None, None, t, "warmest")), (anuclim.prcptot_warmcold_quarter, (None, None, t, "x"))):
        with pytest.raises(NotImplementedError):
            fn(*args)
    with pytest.raises(NotImplementedError):
        anuclim.prcptot_wetdry_period(None, t, op="toto")


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_entry_point_header_ctypes_and_exports():
    lib = _capi.load_library()
    assert hasattr(lib, "xh_bioclim")
    decl = S.header_declarations()["xh_bioclim"]
    sig = _capi.SIGNATURES["xh_bioclim"]
    assert len(decl) == 24 == len(sig)
    for (d, _), s in zip(decl, sig):
        assert S.is_ctypes_kind(d, s) and (s is ctypes.c_void_p or "*" not in d), (d, s)
    assert "bioclim.hip" in open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()


def test_entry_point_rejects_a_null_context():
    lib = _capi.load_library()
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(64)   # never dereferenced: the check fails first
    assert lib.xh_bioclim(null, 10, 4, 4, 0, some, some, some, some, 2, some, some, 1, 1, some, some, 13, 0.0, 1.0, 0.0, some, null, null,
                          4) == _capi.XH_ERR_ARG
