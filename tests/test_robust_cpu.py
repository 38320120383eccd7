"""The change-robustness unit without a GPU: the numpy restatement (tests/robustcpu.py) against the reference's own closures and
scipy 1.15 as recorded by tests/golden/make_robust_golden.py and against the known answers of the reference's tests; the exact
Mann-Whitney null distribution against scipy's; the mirrors of the header's #defines; the NotServed rules and the reference's
three error messages (which answer before a device is asked for).

The restatement's tails are scipy.special's own, its sums numpy's: it agrees with the recorded statistics to a few ulp except
where a NaN was dropped, where the reference's mean("time") adds zeros in place (np.nanmean) and scipy adds the compacted series.
RTOL_STAT bounds that: the two means differ by at most n ulp of the sum, and enter t through (mean - popmean), so the bound is
n 2^-53 |mean| / |mean - popmean| <= 40 * 1.1e-16 * 275 / 1e-3 for the families here, whose deltas are above 1e-3: 1.3e-9."""
import numpy as np
import pytest

import robustcpu as RC
from xclim_amd import _capi, ensembles
from xclim_amd.fields import NotServed

RTOL_STAT = 1.3e-9
RTOL_P = 1e-7   # |dp / p| <= |t f(t) / sf(t)| |dt / t|, and t f / sf <= t^2 + 1 < 80 for the recorded |t| < 9 (p > 1e-12)


def _close(got, want, rtol, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaN pattern differs"
    ok = ~np.isnan(want)
    fin = ok & np.isfinite(want)
    assert np.array_equal(got[ok & ~fin], want[ok & ~fin]), what
    err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
    assert err.size == 0 or err.max() <= rtol, f"{what}: relative difference {err.max():.3e} > {rtol:.1e}"


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_restatement_reproduces_the_reference(family):
    v = RC.vectors()
    fut, ref = v[f"{family}/fut"], v[f"{family}/ref"]
    T1, T2 = fut.shape[1], ref.shape[1]
    for test in RC.TESTS:
        res = RC.change_test(fut, ref, test)
        p, stat = res["pvals"].copy(), res["stat"].copy()
        pend = res["status"] == RC.PENDING
        for r, c in zip(*np.nonzero(pend)):   # the host's part of the exact route
            n1, n2 = int(res["n_fut"][r, c]), int(res["n_ref"][r, c])
            u = max(stat[r, c], n1 * n2 - stat[r, c])
            p[r, c] = min(1.0, 2 * ensembles.mwu_exact_sf(n1, n2)[int(u)])
        if test == "mwu":   # the reference's statistic is U of the REFERENCE sample (its parameters are named the other way round)
            stat = res["n_fut"] * res["n_ref"] - stat
        # rows whose guard answered before scipy have no recorded statistic
        want_stat = v[f"{family}/{test}/stat"]
        _close(np.where(np.isnan(want_stat), np.nan, stat), want_stat, RTOL_STAT, f"{family}/{test}/stat")
        _close(p, v[f"{family}/{test}/p"], RTOL_P, f"{family}/{test}/p")
        if test in ("ttest", "welch"):
            want_df = v[f"{family}/{test}/df"]
            _close(np.where(np.isnan(want_df), np.nan, res["df"]), want_df, 1e-12, f"{family}/{test}/df")
        with np.errstate(invalid="ignore"):
            assert np.array_equal(p < 0.05, v[f"{family}/{test}/p"] < 0.05)
    if family == "pending":
        assert (RC.change_test(fut, ref, "mwu")["status"][:, ::2] == RC.PENDING).all()
        assert (RC.change_test(fut, ref, "mwu")["status"][:, 1::2] == RC.DONE).all()
    assert (T1, T2) == (fut.shape[1], ref.shape[1])


def test_known_answers_of_the_reference_s_tests():
    k = RC.known()
    fut, ref = np.array(k["robust_data"]["fut"]), np.array(k["robust_data"]["ref"])
    names = {v: key for key, v in ensembles.ROBUSTNESS_TESTS.items()}
    for case in k["fractions"]:
        test = case["test"]
        key = ensembles.ROBUSTNESS_TESTS.get(test, "moments")
        res = RC.change_test(fut, ref, key)
        valid = (res["n_fut"] == fut.shape[1]) & (res["n_ref"] == ref.shape[1])
        with np.errstate(all="ignore"):
            if key != "moments":
                changed = res["pvals"] < 0.05
                assert changed.T.astype(int).tolist() == case["changed_table"], test
            elif test == "ipcc-ar6-c":
                changed = np.abs(res["delta"]) > RC.ar6_gamma(ref, 365.0 * np.arange(40), False)[0]
            elif "abs_thresh" in case["kwargs"]:
                changed = np.abs(res["delta"]) > case["kwargs"]["abs_thresh"]
            elif "rel_thresh" in case["kwargs"]:
                changed = np.abs(res["delta"] / res["mean_ref"]) > case["kwargs"]["rel_thresh"]
            else:
                changed = None
        fr = RC.fractions(res["delta"], None, changed, valid)
        rows = _capi.RF_ROWS
        np.testing.assert_array_almost_equal(fr[rows["changed"]], case["changed"])
        np.testing.assert_array_almost_equal(fr[rows["changed_positive"]], case["changed_positive"])
        for name, want in k["common"].items():
            np.testing.assert_array_almost_equal(fr[rows[name]], want)
    assert set(names) == set(RC.TESTS)
    res = RC.change_test(fut, ref, "moments")
    valid = (res["n_fut"] == 40) & (res["n_ref"] == 40)
    fr = RC.fractions(res["delta"], k["weighted"]["weights"], None, valid)
    np.testing.assert_array_equal(fr[_capi.RF_ROWS["changed"]], k["weighted"]["changed"])
    np.testing.assert_array_almost_equal(fr[_capi.RF_ROWS["changed_positive"]], k["weighted"]["changed_positive"])
    for case in k["delta"]:
        d = np.array(case["delta"], float)[:, None]
        changed = np.abs(d) > case["abs_thresh"] if case["abs_thresh"] is not None else None
        fr = RC.fractions(d, case["weights"], changed, None, case["strict_sign"])
        for name in ("changed", "changed_positive", "positive", "agree"):
            if name in case:
                np.testing.assert_array_equal(fr[_capi.RF_ROWS[name]], [case[name]])
    cat = k["categories"]
    got, attrs = ensembles.robustness_categories(np.array(cat["changed"]), np.array(cat["agree"]))
    assert got.tolist() == cat["expected"] and attrs["flag_values"] == cat["flag_values"] and attrs["flag_meanings"] == cat["flag_meanings"]
    assert ensembles.robustness_categories({"changed": np.array([1.0]), "agree": np.array([1.0]), "valid": np.array([0.0])})[0].tolist() == [99]
    for case in k["coefficient"]:
        got = RC.coefficient(np.array(case["fut"])[:, :, None], np.array(case["ref"])[:, None])[0, 0]
        np.testing.assert_almost_equal(got, case["expected"], case["decimals"])
        assert abs(got - case["reference"]) <= 1e-12 * (1 + abs(1 - got))


@pytest.mark.parametrize("tag", ["coef", "coef32"])
def test_coefficient_restatement_reproduces_the_reference(tag):
    v = RC.vectors()
    got, a1, a2 = RC.coefficient(v[f"{tag}/fut"], v[f"{tag}/ref"])
    want = v[f"{tag}/R"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
    ok = ~np.isnan(want)
    terms = v[f"{tag}/fut"].shape[0] * (v[f"{tag}/fut"].shape[1] + 1)
    bound = max(1e-12, (2 * terms + 8) * 2.0 ** -53) * (1 + a1[ok] / a2[ok])
    assert (np.abs(got[ok] - want[ok]) <= bound).all()


@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 30), (3, 5), (8, 12), (12, 8), (8, 8), (7, 40), (8, 512)])
def test_mwu_exact_sf_against_scipy(n1, n2):
    from math import comb

    from scipy.stats._mannwhitneyu import _MWU

    counts = ensembles.mwu_exact_counts(n1, n2)
    assert sum(counts) == comb(n1 + n2, n1) and counts == counts[::-1] and min(counts) >= 1 and max(counts) < 2 ** 63
    sf = ensembles.mwu_exact_sf(n1, n2)
    assert sf.shape == (n1 * n2 + 1,) and sf[0] == 1.0 and np.all(np.diff(sf) <= 0) and sf[-1] > 0
    k = np.arange((n1 * n2 + 1) // 2, n1 * n2 + 1)   # scipy's sf is called with max(U1, U2) only
    assert np.abs(_MWU(n1, n2).sf(k) - sf[k]).max() <= (n1 * n2 + 8) * 2.0 ** -53


def test_the_mirrors_of_the_header():
    d = _capi.UNIT_DEFINES["xclim_hip_robust.h"]
    assert d["XH_CT_MAX_T"] == RC._capi.CT_MAX_T == 512 and d["XH_CT_LDS_SLOTS"] == 64 and d["XH_RC_MAX_POOL"] == 8192
    assert [d[f"XH_RF_{k.upper()}"] for k in ensembles.FRACTIONS] == list(range(7)) and d["XH_RF_NFRAC"] == 7
    assert ensembles.FRACTIONS == ("changed", "positive", "changed_positive", "negative", "changed_negative", "valid", "agree")
    assert set(ensembles.ROBUSTNESS_TESTS.values()) | {"moments"} == set(_capi.CT_TESTS)
    assert (RC.DONE, RC.NAN, RC.PENDING) == (0, 1, 2)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


def test_errors_and_not_served_answer_before_the_device():
    dev = _NoDevice()
    f, r = np.zeros((4, 10, 3)), np.zeros((4, 12, 3))
    with pytest.raises(ValueError, match=r"When deltas are given \(ref=None\), 'test' must be None or 'threshold'\."):
        ensembles.robustness_fractions(np.zeros((4, 3)), test="ttest", device=dev)
    with pytest.raises(ValueError, match="One and only one of abs_thresh or rel_thresh must be given if test='threshold'."):
        ensembles.robustness_fractions(f, r, test="threshold", device=dev)
    with pytest.raises(ValueError, match="One and only one of abs_thresh or rel_thresh"):
        ensembles.robustness_fractions(f, r, test="threshold", abs_thresh=1, rel_thresh=2, device=dev)
    with pytest.raises(ValueError, match="Statistical test mytest must be one of ttest, welch-ttest, mannwhitney-utest, brownforsythe-test, ipcc-ar6-c."):
        ensembles.robustness_fractions(f, r, test="mytest", device=dev)
    from xclim_amd.timeaxis import TimeAxis

    with pytest.raises(NotServed, match="ipcc-ar6-c needs ref_time"):
        ensembles.robustness_fractions(f, r, test="ipcc-ar6-c", device=dev)
    every_other = TimeAxis(np.arange(2000, 2024, 2), np.ones(12, int), np.ones(12, int), "standard")
    monthly = TimeAxis(np.full(12, 2000), np.arange(1, 13), np.ones(12, int), "standard")
    for axis in (every_other, monthly):
        with pytest.raises(NotServed, match="neither annual nor daily without gaps"):
            ensembles.robustness_fractions(f, r, test="ipcc-ar6-c", ref_time=axis, device=dev)

    class MissingPct:
        pass

    with pytest.raises(NotServed, match="invalid=MissingPct"):
        ensembles.robustness_fractions(f, r, test="ttest", invalid=MissingPct(), device=dev)
    with pytest.raises(NotServed, match="integer"):
        ensembles.robustness_fractions(f.astype(np.int32), r, device=dev)
    with pytest.raises(NotServed, match="integer"):
        ensembles.robustness_coefficient(f.astype(np.int64), r[0], device=dev)
    with pytest.raises(NotServed, match="integer deltas"):
        ensembles.robustness_fractions(np.zeros((4, 3), np.int32), device=dev)

    class Chunked:
        chunks, shape, dtype = ((1,),), (4, 10, 3), np.dtype(np.float64)

    with pytest.raises(NotServed, match="chunked"):
        ensembles.robustness_coefficient(Chunked(), r[0], device=dev)


def test_sizes_beyond_the_limits_and_mixed_dtypes_are_not_served():
    class Dev:   # to_device hands the array back: the limits are checked on the shapes before any launch
        def to_device(self, a):
            return a

    with pytest.raises(NotServed, match="up to 512"):
        ensembles.robustness_fractions(np.zeros((2, 513, 3)), np.zeros((2, 10, 3)), test="ttest", device=Dev())
    with pytest.raises(NotServed, match="float64 and ref float32"):
        ensembles.robustness_fractions(np.zeros((2, 10, 3)), np.zeros((2, 10, 3), np.float32), test="ttest", device=Dev())
    with pytest.raises(NotServed, match="pools of up to 8192"):
        ensembles.robustness_coefficient(np.zeros((20, 500, 3)), np.zeros((30, 3)), device=Dev())
    with pytest.raises(NotServed, match="float32 and ref float64"):
        ensembles.robustness_coefficient(np.zeros((2, 10, 3), np.float32), np.zeros((30, 3)), device=Dev())
