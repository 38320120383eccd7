"""The change-robustness unit on the device against the reference's own closures and scipy 1.15 (tests/golden/robust_vectors.npz)
and against the numpy restatement (tests/robustcpu.py).

EXACT: the counts, 2 U and the tie term of the Mann-Whitney test, the status byte, the NaN pattern, `changed` (p < 0.05: the
generator keeps every recorded p 1e-6 relative away from 0.05), the exact-route p (bit for bit the table's value) and the
fractions under dyadic weights; other weights within (R + 8) 2^-53.  Statistics and p-values are compared with the golden.  The
largest relative differences measured on an MI355X over ALL families are written next to MEASURED below and in DESIGN.md section 3;
ten times each is asserted, df included.  One exception, with the bound derived in tests/test_robust_cpu.py: the one-sample t-test
of a pair whose REFERENCE series has a dropped NaN, where the reference's popmean is mean("time") = np.nanmean (zeros added in
place) and the device's is the mean of the compacted series.  The coefficient is
checked within max(1e-12, (2 terms + 8) 2^-53) (1 + A1 / A2): all terms are non-negative."""
import numpy as np
import pytest

import robustcpu as RC
from poisoned import poisoned_outputs  # noqa: F401
from test_robust_cpu import RTOL_P, RTOL_STAT
from xclim_amd import _capi, ensembles
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

# measured on an MI355X: the largest relative difference to the golden of (statistic, p-value, df) per test.  Every statistic came out
# bit for bit (0: the sums are in numpy's order, sqrt and the divisions are IEEE), so ten times that asserts equality; the p-values
# carry the prefactor exp(lgamma ...) of the incomplete beta function, whose error grows with df (the largest are the 500 / 511
# family's: df up to 1009).  Welch's df differs by one ulp in places (scipy squares with pow).
MEASURED = {"ttest": (0.0, 1.650e-12, 0.0), "welch": (0.0, 1.347e-12, 2.145e-16), "mwu": (0.0, 7.115e-15, 0.0), "bf": (0.0, 1.903e-12, 0.0)}


def _run(dev, fut, ref, test):
    return ensembles.change_test(fut, ref, test, device=dev)


def _rel(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaN pattern differs"
    ok = ~np.isnan(want)
    fin = ok & np.isfinite(want)
    assert np.array_equal(got[ok & ~fin], want[ok & ~fin]), what
    zero = fin & (want == 0)
    assert np.array_equal(got[zero], want[zero]), what
    fin &= want != 0
    return float((np.abs(got[fin] - want[fin]) / np.abs(want[fin])).max()) if fin.any() else 0.0


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_families_against_the_reference(dev, family):
    v = RC.vectors()
    fut, ref = v[f"{family}/fut"], v[f"{family}/ref"]
    for test in RC.TESTS:
        res = _run(dev, fut, ref, test)
        cpu = RC.change_test(fut, ref, test)
        for k in ("n_fut", "n_ref"):
            assert np.array_equal(res[k], cpu[k]), (test, k)
        raw = {k: a.get() for k, a in K.change_test(dev, dev.to_device(fut), dev.to_device(ref), test,
                                                    ensembles.mwu_exact_sf(fut.shape[1], ref.shape[1]) if test == "mwu" and min(fut.shape[1], ref.shape[1]) <= 8 else None).items()}
        assert np.array_equal(raw["status"], cpu["status"]), (test, "status")
        stat = res["stat"]
        if test == "mwu":
            assert np.array_equal(2 * raw["stat"][raw["status"] != RC.NAN], cpu["twoU"][cpu["status"] != RC.NAN]), "2 U"
            assert np.array_equal(raw["df"][raw["status"] != RC.NAN], cpu["ties"][cpu["status"] != RC.NAN]), "the tie term"
            pend = raw["status"] == RC.PENDING
            assert np.isnan(raw["pvals"][pend]).all() and (res["status"][pend] == RC.DONE).all()
            stat = res["n_fut"] * res["n_ref"] - stat   # the reference's statistic is U of the reference sample
        want_stat, want_p, want_df = v[f"{family}/{test}/stat"], v[f"{family}/{test}/p"], v[f"{family}/{test}/df"]
        got_stat, got_p = np.where(np.isnan(want_stat), np.nan, stat), res["pvals"]
        if test == "ttest":   # the pairs whose popmean the reference took with np.nanmean over a NaN: the derived bound
            loose = np.broadcast_to(np.isnan(ref).any(axis=1), want_p.shape) & ~np.isnan(want_p)
            if loose.any():
                assert _rel(got_stat[loose], want_stat[loose], "stat") <= RTOL_STAT and _rel(got_p[loose], want_p[loose], "p") <= RTOL_P
            got_stat, got_p, want_stat, tight_p = (np.where(loose, np.nan, a) for a in (got_stat, got_p, want_stat, want_p))
        else:
            tight_p = want_p
        es = _rel(got_stat, want_stat, f"{family}/{test}/stat")
        ep = _rel(got_p, tight_p, f"{family}/{test}/p")
        ed = 0.0 if test == "mwu" else _rel(np.where(np.isnan(want_df), np.nan, res["df"]), want_df, f"{family}/{test}/df")
        print(f"measured {family} {test}: stat {es:.3e} p {ep:.3e} df {ed:.3e}")
        assert es <= 10 * MEASURED[test][0] and ep <= 10 * MEASURED[test][1] and ed <= 10 * MEASURED[test][2], (family, test, es, ep, ed)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(res["pvals"] < 0.05, want_p < 0.05), "changed"
        # the moments are written by every test, and are the same bits
        mom = _run(dev, fut, ref, "moments")
        assert np.array_equal(mom["delta"], res["delta"], equal_nan=True) and np.array_equal(mom["mean_ref"], res["mean_ref"], equal_nan=True)
        assert np.array_equal(res["delta"], cpu["delta"], equal_nan=True), "numpy's pairwise mean of the compacted series, bit for bit"


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("C", [1, 65, 130])
def test_cell_counts(dev, C, dtype):
    v = RC.vectors()
    fam = "main" if dtype == "float64" else "main32"
    fut, ref = np.ascontiguousarray(v[f"{fam}/fut"][:, :, :C]), np.ascontiguousarray(v[f"{fam}/ref"][:, :, :C])
    assert fut.dtype == np.dtype(dtype)
    for test in RC.TESTS:
        res = _run(dev, fut, ref, test)
        want = v[f"{fam}/{test}/p"][:, :C]
        assert _rel(res["pvals"], want, test) <= 10 * MEASURED[test][1]
        assert np.array_equal(res["pvals"] < 0.05, want < 0.05)
    # a ref without realizations: stride 0
    one = _run(dev, fut, np.ascontiguousarray(ref[0]), "welch")
    full = _run(dev, fut, np.ascontiguousarray(np.broadcast_to(ref[0], ref.shape)), "welch")
    for k in one:
        assert np.array_equal(one[k], full[k], equal_nan=True), k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_split_of_the_pairwise_sum(dev, rng, dtype):
    """The means against np.mean, bit for bit, at the lengths where numpy's split changes shape: one block, two leaves, the first
    third level (265 = 128 + 137) and every length from 489 to 512, where a part of the second level is split again."""
    lengths = [1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 264, 265, 272, 300, 384, 385] + list(range(489, 513))
    for T in lengths:
        fut, ref = rng.normal(274, 1, (2, T, 3)).astype(dtype), rng.normal(274, 1, (T // 2 + 1, 3)).astype(dtype)
        res = ensembles.change_test(fut, ref, "ttest", device=dev)
        mf = np.stack([[np.mean(np.ascontiguousarray(fut[r, :, c]).astype(np.float64)) for c in range(3)] for r in range(2)])
        mr = np.array([np.mean(np.ascontiguousarray(ref[:, c]).astype(np.float64)) for c in range(3)])
        assert np.array_equal(res["mean_ref"], np.broadcast_to(mr, (2, 3))), T
        assert np.array_equal(res["delta"], mf - mr, equal_nan=True), T
        cpu = RC.change_test(fut, ref, "ttest")
        assert np.array_equal(res["stat"], cpu["stat"], equal_nan=True), T   # the variance's sum has the same split


def test_exact_route_is_the_table_bit_for_bit(dev):
    v = RC.vectors()
    fut, ref = v["mwu_8_12/fut"], v["mwu_8_12/ref"]
    sf = ensembles.mwu_exact_sf(8, 12)
    raw = {k: a.get() for k, a in K.change_test(dev, dev.to_device(fut), dev.to_device(ref), "mwu", sf).items()}
    assert (raw["status"] == RC.DONE).all() and (raw["df"] == 0).all()
    u = np.maximum(raw["stat"], 96 - raw["stat"]).astype(int)
    assert np.array_equal(raw["pvals"], np.minimum(1.0, 2.0 * sf[u]))
    pend = ensembles.change_test(v["pending/fut"], v["pending/ref"], "mwu", device=dev)
    cpu = RC.change_test(v["pending/fut"], v["pending/ref"], "mwu")
    sel = cpu["status"] == RC.PENDING
    u = np.maximum(cpu["stat"][sel], 96 - cpu["stat"][sel]).astype(int)
    assert sel.any() and np.array_equal(pend["pvals"][sel], np.minimum(1.0, 2.0 * sf[u]))


@pytest.mark.parametrize("strict", [True, False])
def test_fractions(dev, strict):
    v = RC.vectors()
    rows = _capi.RF_ROWS
    for fam in ("zero_delta", "main", "nan_one", "allnan"):
        fut, ref = v[f"{fam}/fut"], v[f"{fam}/ref"]
        R = fut.shape[0]
        mom = RC.change_test(fut, ref, "moments")
        valid = (mom["n_fut"] == fut.shape[1]) & (mom["n_ref"] == ref.shape[1])
        if fam == "zero_delta":
            assert (mom["delta"] == 0).any() and (mom["delta"] > 0).any() and (mom["delta"] < 0).any()
        for weights, exact in ((None, True), ([1, 0.5, 2, 0.25], True), ([1, 0.1, 3.5, 5], False)):
            for test, kw in ((None, {}), ("ttest", {}), ("threshold", {"abs_thresh": 0.5}), ("threshold", {"rel_thresh": 0.001})):
                got = ensembles.robustness_fractions(fut, ref, test, weights, strict_sign=strict, device=dev, **kw)
                if test == "ttest":
                    with np.errstate(invalid="ignore"):
                        changed = v[f"{fam}/ttest/p"] < 0.05
                    assert np.array_equal(got["pvals"] < 0.05, changed)
                elif "abs_thresh" in kw:
                    changed = np.abs(mom["delta"]) > 0.5
                elif "rel_thresh" in kw:
                    with np.errstate(all="ignore"):
                        changed = np.abs(mom["delta"] / mom["mean_ref"]) > 0.001
                else:
                    changed = None
                want = RC.fractions(mom["delta"], weights, changed, valid, strict)
                for name, k in rows.items():
                    if exact:
                        assert np.array_equal(got[name], want[k]), (fam, weights, test, name)
                    else:
                        assert np.abs(got[name] - want[k]).max() <= (R + 8) * 2.0 ** -53, (fam, weights, test, name)
    # the three-way maximum: a cell whose members all have delta == 0 agrees on "no change"
    z = ensembles.robustness_fractions(np.zeros((3, 2)), device=dev, strict_sign=True)
    assert (z["agree"] == 1).all() and (z["positive"] == 0).all() and (z["changed"] == 1).all()
    z = ensembles.robustness_fractions(np.full((3, 2), np.nan), device=dev)
    assert all((z[k] == 0).all() for k in rows)


def test_known_answers_through_the_mirror(dev):
    k = RC.known()
    fut, ref = np.array(k["robust_data"]["fut"]), np.array(k["robust_data"]["ref"])
    for case in k["fractions"]:
        test = case["test"].split("/")[0]
        test = None if test == "None" else test
        kw = {"ref_time": TimeAxis(np.arange(2000, 2040), np.ones(40, int), np.ones(40, int), "noleap")} if test == "ipcc-ar6-c" else {}
        fr = ensembles.robustness_fractions(fut, ref, test, device=dev, **case["kwargs"], **kw)
        np.testing.assert_array_almost_equal(fr["changed"], case["changed"])
        np.testing.assert_array_almost_equal(fr["changed_positive"], case["changed_positive"])
        for name, want in k["common"].items():
            np.testing.assert_array_almost_equal(fr[name], want)
        if case["changed_table"] is not None:
            assert (fr["pvals"] < 0.05).T.astype(int).tolist() == case["changed_table"]
        else:
            assert "pvals" not in fr
    fr = ensembles.robustness_fractions(fut, ref, None, k["weighted"]["weights"], device=dev)
    np.testing.assert_array_equal(fr["changed"], k["weighted"]["changed"])
    np.testing.assert_array_almost_equal(fr["changed_positive"], k["weighted"]["changed_positive"])
    for case in k["delta"]:
        kw = {"abs_thresh": case["abs_thresh"]} if case["abs_thresh"] is not None else {}
        fr = ensembles.robustness_fractions(np.array(case["delta"], float), None, "threshold" if kw else None, case["weights"],
                                            strict_sign=case["strict_sign"], device=dev, **kw)
        for name in ("changed", "changed_positive", "positive", "agree"):
            if name in case:
                np.testing.assert_array_almost_equal(fr[name], case[name], 15)
    # the empty case: all NaN gives 0 everywhere
    fr = ensembles.robustness_fractions(np.full((20, 10), np.nan), np.full((20, 10), np.nan), "ttest", device=dev)
    assert fr["changed"] == 0 and fr["valid"] == 0
    # AtLeastNValid(n=20): the second half of fut missing in cell 3 keeps its members valid
    half = fut.copy()
    half[:, 20:, 3] = np.nan
    fr = ensembles.robustness_fractions(half, ref, "ttest", invalid=("at_least_n", 20), device=dev)
    assert fr["valid"][3] == 0.5 and (fr["valid"][:3] == 1).all()
    for case in k["coefficient"]:
        got = ensembles.robustness_coefficient(np.array(case["fut"])[:, :, None], np.array(case["ref"])[:, None], device=dev)
        np.testing.assert_almost_equal(got[0], case["expected"], case["decimals"])


@pytest.mark.parametrize("tag", ["coef", "coef32"])
def test_coefficient(dev, tag):
    v = RC.vectors()
    fut, ref = v[f"{tag}/fut"], v[f"{tag}/ref"]
    R, a1, a2 = (a.get() for a in K.robust_coefficient(dev, dev.to_device(fut), dev.to_device(ref), parts=True))
    want = v[f"{tag}/R"]
    cpu = RC.coefficient(fut, ref)
    for got, ref_ in ((R, want), (R, cpu[0]), (a1, cpu[1]), (a2, cpu[2])):
        assert np.array_equal(np.isnan(got), np.isnan(ref_)) and np.isnan(ref_).sum() == 1
    ok = ~np.isnan(want)
    terms = fut.shape[0] * (fut.shape[1] + 1)
    rel = max(1e-12, (2 * terms + 8) * 2.0 ** -53)
    assert (np.abs(R[ok] - want[ok]) <= rel * (1 + cpu[1][ok] / cpu[2][ok])).all()
    assert (np.abs(a1[ok] - cpu[1][ok]) <= rel * cpu[1][ok]).all() and (np.abs(a2[ok] - cpu[2][ok]) <= rel * cpu[2][ok]).all()
    for C in (1, 7):
        part = ensembles.robustness_coefficient(np.ascontiguousarray(fut[:, :, :C]), np.ascontiguousarray(ref[:, :C]), device=dev)
        assert np.array_equal(part, R[:C])


def test_the_largest_pool(dev, rng):
    """R T1 + R = 8192 exactly: 16 members of 511 values, and a reference of 8176 + 16 = 8192 pooled values."""
    fut, ref = rng.normal(1.0, 1.0, (16, 511, 2)), rng.normal(0.0, 1.0, (500, 2))
    got = ensembles.robustness_coefficient(fut, ref, device=dev)
    cpu = RC.coefficient(fut, ref)
    rel = max(1e-12, (2 * 8192 + 8) * 2.0 ** -53)
    assert (np.abs(got - cpu[0]) <= rel * (1 + cpu[1] / cpu[2])).all()
    with pytest.raises(_capi.XclimHipError):
        K.robust_coefficient(dev, dev.to_device(rng.normal(0, 1, (16, 512, 1))), dev.to_device(ref[:, :1].copy()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("years", [60, 50])
def test_ar6_gamma_against_the_restatement(dev, years, dtype):
    """gamma within 1e-12 of the sum of the absolute terms of a residual (|y| + |trend|, times the factor), with and without blocks;
    then the whole test through the mirror: annual stamps, and the same years as daily rows (the annual means on the device)."""
    v = RC.vectors()
    ref, fut, x = v[f"ar6_{years}/ref"].astype(dtype), v[f"ar6_{years}/fut"].astype(dtype), v[f"ar6_{years}/x"]
    seg = np.append(np.arange(0, years, 20), years)
    for with_pi, tag in ((False, "lin"), (True, "pi")):
        got = K.ar6_gamma(dev, dev.to_device(ref), x, 2 if with_pi else 1, np.sqrt(2) * 1.645 if with_pi else np.sqrt(2 / 20) * 1.645,
                          seg if with_pi else None).get()
        want, scale = RC.ar6_gamma(ref, x, with_pi)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).any()
        err = np.abs(got - want) / scale
        print(f"measured ar6 {years} {tag} {np.dtype(dtype).name}: {err.max():.3e} of the scale")
        assert err.max() <= 1e-12
        if dtype == np.float64:
            assert np.abs(want - v[f"ar6_{years}/gamma_{tag}"]).max() == 0
        time = TimeAxis(np.arange(1950, 1950 + years), np.ones(years, int), np.ones(years, int), "noleap")
        fr = ensembles.robustness_fractions(fut, ref, "ipcc-ar6-c", ref_time=time, device=dev, **({"ref_pi": True} if with_pi else {}))
        mom = RC.change_test(fut, ref, "moments")
        valid = (mom["n_fut"] == fut.shape[1]) & (mom["n_ref"] == years)
        exp = RC.fractions(mom["delta"], None, np.abs(mom["delta"]) > want, valid)
        for name, k in _capi.RF_ROWS.items():
            assert np.array_equal(fr[name], exp[k]), (tag, name)
        assert "pvals" not in fr
    # a short gamma: one member with two years only has no quadratic fit
    short = ref[:, :8].copy()
    short[0, 2:, 0] = np.nan
    got = K.ar6_gamma(dev, dev.to_device(short), x[:8], 2, 1.0).get()
    assert np.isnan(got[0, 0]) and np.isfinite(got[1:]).all()


def test_ar6_from_daily_rows(dev, rng):
    """500 daily noleap rows from 1 December: three calendar years of 31, 365 and 104 rows (xh_change_test takes 512 rows at most,
    so a daily reference is served up to there).  The annual means come from xh_resample_reduce, the labels are each year's
    1 January."""
    time = TimeAxis.daily("2000-12-01", 500, "noleap")
    ref = (274 + rng.normal(0, 1, (3, 500, 5))).astype(np.float64)
    fut = (274.3 + rng.normal(0, 1, (3, 40, 5))).astype(np.float64)
    fr = ensembles.robustness_fractions(fut, ref, "ipcc-ar6-c", ref_time=time, device=dev)
    cuts = [0, 31, 396, 500]
    annual = np.stack([ref[:, a:b].mean(axis=1) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    want, scale = RC.ar6_gamma(annual, 365.0 * np.arange(3), False)
    mom = RC.change_test(fut, ref, "moments")
    # the device's annual means add the rows in another order than numpy: gamma moves by about 1e-13; no |delta| is that close
    assert (np.abs(np.abs(mom["delta"]) - want) > 1e-6).all() and (want > 1e-3).all()
    exp = RC.fractions(mom["delta"], None, np.abs(mom["delta"]) > want, np.ones((3, 5), bool))
    for name, k in _capi.RF_ROWS.items():
        assert np.array_equal(fr[name], exp[k]), name
    gappy = time.subset(np.r_[0:400, 402:500])
    with pytest.raises(ensembles.NotServed, match="neither annual nor daily"):
        ensembles.robustness_fractions(fut, ref[:, :len(gappy)], "ipcc-ar6-c", ref_time=gappy, device=dev)
    long = TimeAxis.daily("2001-01-01", 730, "noleap")
    with pytest.raises(ensembles.NotServed, match="up to 512"):
        ensembles.robustness_fractions(fut, np.zeros((3, 730, 5)), "ipcc-ar6-c", ref_time=long, device=dev)


def test_fused_route_equals_the_composed_one(dev):
    v = RC.vectors()
    fut, ref = v["nan_one/fut"], v["nan_one/ref"]
    fused = ensembles.robustness_fractions(fut, ref, "welch-ttest", [1, 0.1, 3.5, 5], device=dev)
    d_f, d_r = dev.to_device(fut), dev.to_device(ref)
    res = K.change_test(dev, d_f, d_r, "welch")
    p, n1, n2 = res["pvals"].get(), res["n_fut"].get(), res["n_ref"].get()
    with np.errstate(invalid="ignore"):
        changed = dev.to_device((p < 0.05).astype(np.uint8))
    valid = dev.to_device(((n1 == fut.shape[1]) & (n2 == ref.shape[1])).astype(np.uint8))
    out = K.robust_fractions(dev, res["delta"], [1, 0.1, 3.5, 5], changed=changed, valid=valid).get()
    for name, k in _capi.RF_ROWS.items():
        assert np.array_equal(fused[name], out[k]), name
    assert np.array_equal(fused["pvals"], p, equal_nan=True)
    # the threshold decided in the kernel against a mask made from the same delta on the host
    mom = K.change_test(dev, d_f, d_r, "moments")
    delta = mom["delta"].get()
    a = K.robust_fractions(dev, mom["delta"], np.ones(4), valid=valid, abs_thresh=0.4).get()
    b = K.robust_fractions(dev, mom["delta"], np.ones(4), valid=valid, changed=dev.to_device((np.abs(delta) > 0.4).astype(np.uint8))).get()
    assert np.array_equal(a, b)


def test_refusals(dev):
    f, r = dev.to_device(np.zeros((2, 513, 3))), dev.to_device(np.zeros((2, 10, 3)))
    with pytest.raises(_capi.XclimHipError, match="at most 512 values per series, got 513 and 10"):
        K.change_test(dev, f, r, "ttest")
    f = dev.to_device(np.zeros((2, 8, 3)))
    with pytest.raises(_capi.XclimHipError):   # the exact table is needed and missing
        K.change_test(dev, f, r, "mwu")
    with pytest.raises(_capi.XclimHipError):   # ... or has another length
        K.change_test(dev, f, r, "mwu", np.ones(80))
    with pytest.raises(_capi.XclimHipError):   # a table where no length is at most 8
        K.change_test(dev, dev.to_device(np.zeros((2, 9, 3))), r, "mwu", np.ones(91))
