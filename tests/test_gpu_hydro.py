"""The hydrology unit on the device (xclim_amd/csrc/hydro.hip, xclim_amd.hydrology) against tests/golden/hydro_vectors.npz and, at
the cell counts no golden value exists for, against the numpy restatement tests/hydrocpu.py; the host mirrors bit for bit against
the kernel calls; every output subset of xh_flow_period_stats against the launch with all of them; the Sen slope at the series
lengths that change its sort (one pair, odd and even numbers of slopes, the largest length) and on series with ties, absent and
NaN years; on padded, poisoned row views (tests/stridedabi.py); the refusals.  Every test runs on poisoned output buffers, and
after every call of an entry point no output element may still hold the poison (tests/unwritten.py: watch, on the operand table
of tests/stridedabi.py).

Tolerance (tests/test_hydro_cpu.py: check, check_run): |got - want| <= 1e-12 * scale, the scale being the sum of the absolute terms
of the value; counts, n and the NaN patterns exactly; the Sen slope bit for bit; p within 1e-12 absolute."""

import numpy as np
import pytest

import hydrocpu as H
import stridedabi as S
from stridedabi import HYDRO_TABLE
from test_hydro_cpu import (RUNS, bits, check, check_known_answers, check_run, golden_case, mirror_api, refusals,
                            spec_of)
from xclim_amd import hydrology
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis
from unwritten import watched  # noqa: F401  (autouse: after every call of an entry point no output element may still hold the poison)
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
FLUX = "kg m-2 s-1"


def _host(outs):
    return {k: v.get() for k, v in outs.items()}


# ---- one run, through kernels.py and through the mirror ---------------------------------------------------------------
def launch(dev, s, fields, time, exp=None):
    kind = s["kind"]
    if kind == "flow":
        return _host(K.flow_period_stats(dev, dev.to_device(fields["q"]), time.segments(s["freq"])[0], outputs=K.FLOW_OUTPUTS))
    if kind == "melt":
        pr = dev.to_device(fields["pr"]) if s["pr"] == "pr" else None
        return {"out": K.melt_period_max(dev, dev.to_device(fields["snw"]), time.segments(s["freq"])[0], pr, window=s["window"],
                                         per_day=H.DAY).get()}
    if kind == "api":
        return {"out": K.antecedent_precip(dev, dev.to_device(fields["pr"]), H.api_weights(s["window"], s["p_exp"]), per_day=H.DAY).get()}
    return _host(K.sen_slope(dev, dev.to_device(exp["x"]), exp["period_of"], outputs=K.SEN_OUTPUTS))


def mirror(dev, s, fields, time):
    """The mirror's value of a run and the kernel call it must equal bit for bit."""
    kind, kw = s["kind"], dict(time=time, device=dev)
    if kind == "flow":
        both = hydrology.flow_stats(fields["q"], s["freq"], **kw)
        return {"bfi": hydrology.base_flow_index(fields["q"], s["freq"], **kw), "rbi": hydrology.rb_flashiness_index(fields["q"], s["freq"], **kw),
                "bfi2": both.base_flow_index, "rbi2": both.rb_flashiness_index}
    if kind == "melt":
        if s["pr"] == "pr":
            return {"out": hydrology.melt_and_precip_max(fields["snw"], fields["pr"], s["window"], s["freq"], flux_units=FLUX, **kw)}
        return {"out": hydrology.snow_melt_we_max(fields["snw"], s["window"], s["freq"], **kw)}
    if kind == "api":
        return {"out": hydrology.antecedent_precipitation_index(fields["pr"], s["window"], s["p_exp"], flux_units=FLUX, **kw)}
    r = hydrology.sen_slope(fields["q"], s["freq"], **kw)
    return {"slope": r.sen_slope, "p": r.p_value}


def _same_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


@pytest.mark.parametrize("name,run", RUNS)
def test_golden_cases(dev, name, run):
    c = golden_case(name)
    s, exp = spec_of(c, run), c.expected[run]
    got = launch(dev, s, c.fields, c.time, exp)
    assert set(got) == {k for k in exp if not k.endswith("_scale") and k not in ("x", "period_of")}
    check_run(got, exp, f"{name} {run}")
    m = mirror(dev, s, c.fields, c.time)
    if s["kind"] == "sen":      # the mirror's own chain: xh_resample_reduce (the field's dtype), then xh_sen_slope
        means, _ = K.resample_reduce(dev, dev.to_device(c.fields["q"]), "mean", c.time.segments(s["freq"])[0], want_valid=False)
        got = _host(K.sen_slope(dev, means, exp["period_of"]))
        tol = 1e-12 if c.dtype == "float64" else 2e-6       # the device's period means against numpy's: float32 means round to 6e-8
        np.testing.assert_allclose(means.get(), exp["x"], rtol=tol, equal_nan=True)
    for k, v in m.items():
        _same_bits(v, got[k.rstrip("2")], f"{name} {run} {k}: mirror")


# ---- cell counts: one lane, a wave less one, a wave, a wave and one, more than one workgroup's worth of waves -------------
_SYNTH = {}
_RUNS = ([dict(kind="flow", freq=f) for f in ("YS", "YS-JUL", "YS-OCT", "QS-DEC", "MS")]
         + [dict(kind="melt", window=3, freq="YS-JUL", pr="pr"), dict(kind="melt", window=3, freq="YS-JUL", pr="nopr"),
            dict(kind="melt", window=31, freq="MS", pr="pr"), dict(kind="melt", window=1, freq="QS-DEC", pr="nopr")]
         + [dict(kind="api", window=7, p_exp=0.935), dict(kind="api", window=1, p_exp=0.935), dict(kind="api", window=31, p_exp=0.9),
            dict(kind="api", window=32, p_exp=0.97)]      # (the largest window: more than 64 KiB of LDS with the weights)
         + [dict(kind="sen", freq="QS-DEC")])


def _synth(C, T, dtype, calendar):
    """Seeded fields on T days and C cells, and the restatement's values for them: once per key."""
    key = (C, T, np.dtype(dtype).name, calendar)
    if key not in _SYNTH:
        t = TimeAxis.daily("2000-01-01", T, calendar)
        f = H.synth(t, C, np.dtype(dtype))
        _SYNTH[key] = (t, f, [(s, H.run(s, f, t)) for s in _RUNS if T > 5 or s["kind"] != "sen"])
    return _SYNTH[key]


@pytest.mark.parametrize("dtype,calendar", [(np.float64, "standard"), (np.float32, "noleap")])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_cell_counts_against_restatement(dev, C, dtype, calendar):
    t, f, runs = _synth(C, 800, dtype, calendar)
    for s, exp in runs:
        check_run(launch(dev, s, f, t, exp), exp, f"C={C} {H.spec_id(s)}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_series_shorter_than_the_windows(dev, dtype):
    t, f, runs = _synth(65, 5, dtype, "standard")
    for s, exp in runs:
        got = launch(dev, s, f, t, exp)
        check_run(got, exp, f"T=5 {H.spec_id(s)}")
        if s["kind"] == "flow":
            assert np.isnan(got["bfi"]).all() and not np.isnan(got["rbi"][:, 0]).any()
        if s["kind"] == "api" and s["window"] >= 7:
            assert np.isnan(got["out"]).all()
        if s["kind"] == "melt" and s["window"] >= 5:
            assert np.isnan(got["out"]).all()


def test_empty_first_middle_and_last_periods(dev):
    t, f, _ = _synth(65, 800, np.float32, "noleap")
    seg = np.array([0, 0, 300, 300, 800, 800], np.int64)
    empty = np.array([True, False, True, False, True])
    got = _host(K.flow_period_stats(dev, dev.to_device(f["q"]), seg, outputs=K.FLOW_OUTPUTS))
    check_run(got, H.flow_period_stats(f["q"], seg), "empty periods: flow")
    assert np.isnan(got["bfi"][empty]).all() and np.isnan(got["mean"][empty]).all() and (got["valid"][empty] == 0).all()
    assert (got["sum"][empty] == 0).all()
    out = K.melt_period_max(dev, dev.to_device(f["snw"]), seg, dev.to_device(f["pr"]), window=3).get()
    check_run({"out": out}, H.melt_period_max(f["snw"], f["pr"], H.DAY, 3, seg), "empty periods: melt")
    assert np.isnan(out[empty]).all() and not np.isnan(out[1, 0])


# ---- output subsets, and pr against no pr -------------------------------------------------------------------------------
def test_every_output_subset_of_the_flow_kernel_equals_the_full_launch(dev):
    t, f, _ = _synth(65, 800, np.float32, "noleap")
    q, seg = dev.to_device(f["q"]), t.segments("YS-OCT")[0]
    full = _host(K.flow_period_stats(dev, q, seg, outputs=K.FLOW_OUTPUTS))
    n = len(K.FLOW_OUTPUTS)
    for mask in range(1, 2 ** n):
        names = [o for i, o in enumerate(K.FLOW_OUTPUTS) if mask >> i & 1]
        got = _host(K.flow_period_stats(dev, q, seg, outputs=names))
        assert list(got) == names
        for k, v in got.items():
            assert v.dtype == full[k].dtype
            if k == "valid":
                np.testing.assert_array_equal(v, full[k])
            else:
                _same_bits(v, full[k], f"{names}: {k}")


def test_melt_with_and_without_precipitation(dev):
    t, f, _ = _synth(65, 800, np.float64, "standard")
    snw, seg = dev.to_device(f["snw"]), t.segments("YS-JUL")[0]
    without = K.melt_period_max(dev, snw, seg, None, window=3).get()
    with_pr = K.melt_period_max(dev, snw, seg, dev.to_device(f["pr"]), window=3).get()
    zero = K.melt_period_max(dev, snw, seg, dev.to_device(np.zeros_like(f["pr"])), window=3).get()
    _same_bits(zero, without + 0.0, "zero precipitation adds nothing")       # (+ 0.0: 0.0 + -0.0 of the kernel's first term)
    ok = ~np.isnan(with_pr)
    assert ok.any() and (with_pr[ok] >= without[ok]).all() and (with_pr[ok] > without[ok]).any()


# ---- xh_sen_slope ---------------------------------------------------------------------------------------------------------
def _sen_case(Y, C=65, K_=2, dtype=np.float64, seed=0):
    """(x (Y * K, C), period_of (Y, K)): a noisy trend; column 1 constant, 2 with ties, 3 with NaN years in the middle, 4 with one
    value, 5 with none; the first year of season 0 absent (period_of = -1)."""
    rng = np.random.default_rng(50 + Y + seed)
    x = (0.3 * (np.arange(Y * K_) // K_)[:, None] + rng.normal(0, 2.0, (Y * K_, C))).astype(dtype)
    po = np.arange(Y * K_, dtype=np.int64).reshape(Y, K_)
    po[0, 0] = -1
    if C > 5:
        x[:, 1] = 4.25
        x[:, 2] = np.round(x[:, 2])
        x[po[Y // 3:Y // 3 + max(1, Y // 5)].ravel(), 3] = np.nan
        x[:, 4] = np.nan
        x[po[-1], 4] = 1.5
        x[:, 5] = np.nan
    return x, po


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("Y", [2, 3, 4, 5, 6, 30, 64, hydrology.SEN_MAX_YEARS])
def test_sen_slope_lengths_and_series(dev, Y, dtype):
    C = 65 if Y <= 64 else 9
    x, po = _sen_case(Y, C, dtype=dtype)
    got = _host(K.sen_slope(dev, dev.to_device(x), po, outputs=K.SEN_OUTPUTS))
    want = H.sen_slope(x, po)
    check_run(got, want, f"Y={Y}")
    k = 1                                   # the season whose every year is present
    assert (got["n"][k, 0] == Y) and (got["n"][0, 0] == Y - 1)
    assert got["slope"][k, 1] == 0.0 and got["p"][k, 1] == 1.0 and got["n"][k, 1] == Y          # a constant series
    assert got["n"][k, 4] == 1 and np.isnan(got["slope"][k, 4]) and np.isnan(got["p"][k, 4])     # one value
    assert got["n"][k, 5] == 0 and np.isnan(got["slope"][k, 5]) and np.isnan(got["p"][k, 5])     # none
    assert got["n"][k, 3] < Y and (Y < 4 or not np.isnan(got["slope"][k, 3]))                    # NaN years in the middle
    if Y >= 30:
        assert len(np.unique(x[po[:, k], 2])) < Y and 0 <= got["p"][k, 2] < 1                    # ties (a strong trend: p may round to 0)
    # slope alone and p alone give the same bits
    for name in ("slope", "p"):
        one = _host(K.sen_slope(dev, dev.to_device(x), po, outputs=(name,)))
        assert list(one) == [name]
        _same_bits(one[name], got[name], f"Y={Y} {name} alone")


def test_sen_slope_uses_the_original_year_positions(dev):
    """A NaN year between two values halves the pair's slope: (x_2 - x_0) / 2, not the slope of neighbours."""
    x = np.array([[1.0], [np.nan], [3.0], [np.nan], [9.0]])
    got = _host(K.sen_slope(dev, dev.to_device(x), np.arange(5).reshape(5, 1), outputs=K.SEN_OUTPUTS))
    assert got["n"][0, 0] == 3 and got["slope"][0, 0] == 2.0            # slopes 1, 2, 3 over the distances 2, 4, 2
    check_run(got, H.sen_slope(x, np.arange(5).reshape(5, 1)), "positions")


# ---- the indices built from the existing kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_quantile_indices_against_restatement(dev, dtype):
    t, f, _ = _synth(65, 800, dtype, "standard")
    q = f["q"].copy()
    q[:, 3] = f["q"][:, 0] * 0.5            # (a whole NaN cell has no median: tested below)
    seg = t.segments("YS-OCT")[0]
    fi = hydrology.flow_index(q, 0.95, device=dev)
    want = H.flow_index(q, 0.95)
    if dtype == np.float64:
        check(fi, want, 4 * np.abs(want), "flow_index")                  # two quantiles (an interpolation each) and a division
    else:   # xh_nan_quantile interpolates float32 samples in float32, as numpy does for a float32 array: 6e-8 per quantile
        np.testing.assert_allclose(fi, want, rtol=4 * 2.0 ** -24)
    # The counts are exact when no value of the series lies within the device's error of a threshold, which is asserted on the
    # restatement's own thresholds.  The error: float64, a median or mean below 128 is good to 1e-12; float32, the
    # median is interpolated in float32 (two ulp of 128 = 1.5e-5, times the factor) and the mean of the field is a float32 mean
    # (xh_resample_reduce: within 1e-6 of the float64 one, asserted below, = 1e-4 at 128, times the factor)
    w = H.widen(q)
    hi, lo = hydrology.high_flow_frequency(q, 1.25, "YS-OCT", time=t, device=dev), hydrology.low_flow_frequency(q, 0.8, "YS-OCT", time=t, device=dev)
    med = np.nanquantile(w, 0.5, axis=0)
    mean = np.nansum(np.nan_to_num(w), axis=0) / np.maximum((~np.isnan(w)).sum(axis=0), 1)
    near_hi, near_lo = (1e-9, 1e-9) if dtype == np.float64 else (1.25 * 1.6e-5, 0.8 * 1.3e-4)
    assert np.nanmax(med) < 128 and mean.max() < 128 and np.nanmin(np.abs(w - 1.25 * med[None])) > near_hi and np.nanmin(np.abs(w - 0.8 * mean[None])) > near_lo
    np.testing.assert_array_equal(hi, H.high_flow_frequency(q, 1.25, seg))
    np.testing.assert_array_equal(lo, H.low_flow_frequency(q, 0.8, seg))
    dmean = K.resample_reduce(dev, dev.to_device(q), "mean", np.array([0, 800]), want_valid=False)[0].get()[0].astype(np.float64)
    has = (~np.isnan(w)).any(axis=0)
    np.testing.assert_allclose(dmean[has], mean[has], rtol=1e-12 if dtype == np.float64 else 1e-6)
    assert hi.sum() > 0 and lo.sum() > 0 and hi.dtype == np.int32
    ai = hydrology.aridity_index(f["pr"], f["q"], "YS", time=t, device=dev)
    want = H.aridity_index(f["pr"], f["q"], t.segments("YS")[0])
    np.testing.assert_allclose(ai, want, rtol=1e-12 if dtype == np.float64 else 1e-5, equal_nan=True)
    assert np.isnan(hydrology.flow_index(f["q"], device=dev)[3])


def test_seasonal_ratio_and_sen_slope_ratio_of_the_mirror(dev):
    t, f, _ = _synth(65, 800, np.float64, "standard")
    got = hydrology.base_flow_index_seasonal_ratio(f["q"], time=t, device=dev)
    bfi, ratio, seasons = H.seasonal_bfi_ratio(f["q"], t)
    assert got.seasons == seasons == ["DJF", "JJA", "MAM", "SON"] and list(got.years) == [1999, 2000, 2001]
    np.testing.assert_allclose(got.bfi, bfi, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got.ratio, ratio, rtol=1e-12, equal_nan=True)
    r = hydrology.sen_slope_ratio(f["q"], f["q"] * 2, "QS-DEC", time=t, device=dev)
    ok = ~np.isnan(r.ratio)
    assert ok.any() and (r.ratio[ok] == 0.5).all() and r.seasons == seasons
    _same_bits(r.p_value, r.p_value_sim, "doubling a series keeps its ranks")


# ---- padded, poisoned row views ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C,pitch", [(65, 80), (130, 144)])
def test_padded_views_give_the_same_bits(dev, monkeypatch, C, pitch, dtype):
    """Every strided operand of the four entry points in rows of `pitch` elements, NaN / 1e30 in the extra columns of the inputs and
    in front of their first row, 0xA5 bytes in those of the outputs (tests/stridedabi.py: padded, which asserts that they stay)."""
    for name, ops in HYDRO_TABLE.items():
        for op in ops:
            assert {op.ptr, op.stride} <= set(S.parameters(name)), (name, op)
    t, f, _ = _synth(C, 800, dtype, "standard" if dtype == np.float64 else "noleap")
    seg = t.segments("QS-DEC")[0]
    po = H.season_year_table(t, "QS-DEC")[0]

    def run():
        d = {k: dev.to_device(v) for k, v in f.items()}
        out = {"flow." + k: v for k, v in K.flow_period_stats(dev, d["q"], seg, outputs=K.FLOW_OUTPUTS).items()}
        out["melt"] = K.melt_period_max(dev, d["snw"], seg, d["pr"], window=5)
        out["api"] = K.antecedent_precip(dev, d["pr"], H.api_weights(7, 0.935))
        out.update({"sen." + k: v for k, v in K.sen_slope(dev, out["flow.mean"], po, outputs=K.SEN_OUTPUTS).items()})
        return _host(out)

    plain = run()
    with S.padded(dev, monkeypatch, pads=(pitch - C, pitch - C), shift=5) as log:
        got = run()
    assert set(got) == set(plain) and len(got) == 10
    for k, g in got.items():
        p = plain[k]
        same = (g == p) | (np.isnan(g) & np.isnan(p)) if g.dtype.kind == "f" else g == p
        assert g.shape == p.shape and same.all(), f"{k} differs under row pitches {log}"
    assert [n for n, _ in log] == list(HYDRO_TABLE)
    assert all(used == {"ld": (pitch, C), "ld_out": (pitch, C)} for _, used in log), log


def test_every_output_operand_was_armed_and_checked(dev, watched):
    """The watch of this module sees the outputs of all four entry points poisoned before the call (they come from Device.empty
    under the fixture) and written after it."""
    t, f, _ = _synth(65, 800, np.float32, "noleap")
    d = {k: dev.to_device(v) for k, v in f.items()}
    seg = t.segments("YS")[0]
    flow = K.flow_period_stats(dev, d["q"], seg, outputs=K.FLOW_OUTPUTS)
    K.melt_period_max(dev, d["snw"], seg, d["pr"], window=3)
    K.antecedent_precip(dev, d["pr"], H.api_weights(7, 0.935))
    K.sen_slope(dev, flow["mean"], np.arange(len(seg) - 1).reshape(-1, 1), outputs=K.SEN_OUTPUTS)
    seen = {n: armed for n, armed in watched if n in HYDRO_TABLE}
    assert set(seen) == set(HYDRO_TABLE)
    for name, armed in seen.items():
        assert set(armed) == {op.ptr for op in HYDRO_TABLE[name] if op.mode == "w"} and all(armed.values()), (name, armed)


# ---- the reference's known answers, the missing mask, the refusals ---------------------------------------------------------
def test_known_answers_on_the_device(dev):
    check_known_answers(mirror_api(dev))


def test_missing_mask_and_keep(dev):
    c = golden_case("std_f64")
    q, e = c.fields["q"], c.expected["flow.YS"]
    kw = dict(time=c.time, device=dev)
    full = c.time.expected_count("YS")[:, None]
    m = hydrology.flow_stats(q, "YS", mask_missing=True, **kw)
    for got, k in ((m.base_flow_index, "bfi"), (m.rb_flashiness_index, "rbi")):
        want = np.where(e["valid"] != full, np.nan, e[k])
        assert not np.isnan(want[0, 0]) and np.isnan(want[0, 1]) and np.isnan(want[-1]).all()    # a NaN row; the partial last year
        check(got, want, e[k + "_scale"], f"masked {k}")
    kept = hydrology.base_flow_index(q, "YS", keep=True, **kw)
    check(kept.get(), e["bfi"], e["bfi_scale"], "kept bfi")
    melt = hydrology.melt_and_precip_max(c.fields["snw"], c.fields["pr"], 3, "YS-JUL", mask_missing=True, **kw)
    em = c.expected["melt.3.YS-JUL.pr"]
    assert np.isnan(melt[0]).all() and np.isnan(melt[:, 1]).all()
    check(melt[1, 0], em["out"][1, 0], em["out_scale"][1, 0], "masked melt")
    with pytest.raises(ValueError, match="keep=True"):
        hydrology.base_flow_index(q, "YS", keep=True, mask_missing=True, **kw)
    assert hydrology.base_flow_index(q[:, :0], "YS", **kw).shape == (3, 0)
    assert hydrology.antecedent_precipitation_index(q[:0], device=dev).shape == (0, 5)
    with pytest.raises(ValueError, match="up to 32"):          # kernels.py refuses before the call; the mirror says NotServed
        K.antecedent_precip(dev, dev.to_device(q), np.ones(33))


def test_refusals(dev):
    refusals(dev)
