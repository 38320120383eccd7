"""The distribution-fit unit without a device: the conditions of the recorded reference results (tests/golden/distfit_vectors.npz),
the reference's known answer through scipy as the generator computes it, the mirrors of the header's ``#define``s, and the
argument validation of xclim_amd/stats.py — every NotServed and ValueError path is taken before a device is asked for."""
import os
import re

import numpy as np
import pytest

import distfitcases as D
from xclim_amd import _capi as capi
from xclim_amd import stats as S

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "units", "xclim_hip_distfit.h")


class NoDevice:
    """Handed in as ``device=``: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


# ---- the golden's conditions -------------------------------------------------------------------------------------------
def test_no_reference_nelder_mead_fit_stopped_at_its_budget():
    assert len(D.NM_CASES) >= 8
    for case in D.NM_CASES:
        warnflag, nfev, status = D.get(case, "warnflag"), D.get(case, "nfev"), D.get(case, "status")
        assert not warnflag.any(), case
        assert (nfev < D.budget(case)).all(), case
        assert not (status == capi.DISTFIT_STATUS["budget"]).any(), case
        fitted = status == capi.DISTFIT_STATUS["fitted"]
        assert (nfev[fitted] > 0).all() and np.isfinite(D.get(case, "params")[:, fitted]).all(), case
        # no Nelder-Mead family has fewer than 30 values in a fitted cell
        assert (np.isfinite(D.field(case))[:, fitted].sum(axis=0) >= 30).all(), case


def test_the_shapes_and_dtypes_reach_every_staging_decision():
    shapes = {(m["T"], m["dtype"]) for m in D.META.values()}
    assert {t for t, _ in shapes} == {30, 32, 33, 150}          # 32: the last LDS slot, 33: the first work-buffer one
    assert {m["C"] for m in D.META.values()} == {1, 65, 130}
    for T in (30, 32, 33, 150):
        assert any(m["nm"] and m["T"] == T for m in D.META.values()), T
    assert {m["dtype"] for m in D.META.values()} == {"f4", "f8"}
    for case, m in D.META.items():
        assert D.field(case).dtype == (np.float64 if m["dtype"] == "f8" else np.float32)
        assert D.field(case).shape == (m["T"], m["C"])


def test_every_decision_has_its_family():
    served = {(m["dist"], m["method"], m["floc"] is not None) for m in D.META.values()}
    assert served == {("norm", "ML", False), ("gumbel_r", "ML", False), ("genextreme", "ML", False), ("genextreme", "APP", False),
                      ("gamma", "ML", False), ("gamma", "ML", True), ("gamma", "APP", False), ("gamma", "APP", True),
                      ("fisk", "ML", False), ("fisk", "ML", True), ("fisk", "APP", False), ("fisk", "APP", True),
                      ("lognorm", "ML", True), ("lognorm", "APP", False), ("lognorm", "APP", True)}
    assert {m["floc"] for m in D.META.values() if m["floc"] is not None} >= {0.0, -5.0, -2.5, -40.0}   # floc at 0 and negative
    for case, m in D.META.items():
        x, status = D.field(case), D.get(case, "status")
        if m["C"] < 65:
            continue
        n = np.isfinite(x).sum(axis=0)
        assert n[0] == 0 and n[1] == 1 and status[0] == status[1] == capi.DISTFIT_STATUS["nan"], case   # all NaN; one value
        assert np.isnan(D.get(case, "params")[:, :2]).all()
        if not m["nm"]:
            assert n[2] == 2, case                                                                    # two values
        assert (0 < (~np.isfinite(x[:, 3])).sum() < m["T"]) or (m["nm"] and m["T"] == 30), case        # NaNs scattered
        if m["dist"] == "norm" and m["T"] <= 128:
            # a constant cell: its scale is 0 or the rounding of the mean (both sides add the same 30 or 33 terms in the same order)
            assert np.ptp(x[:, 4]) == 0 and 0.0 <= D.get(case, "params")[1, 4] < 1e-13 * abs(x[0, 4]), case
        if m["dist"] == "lognorm" and m["method"] == "ML":
            assert np.nanmin(x[:, 5]) == m["floc"] and status[5] == capi.DISTFIT_STATUS["support"], case
            assert D.get(case, "raised")[5]
    # gumbel_r: the first bracket (0.5, 2) holds no root
    wide = [c for c, m in D.META.items() if m["kind"] == "gumbel_wide"]
    assert wide and all(np.nanmin(D.get(c, "params")[1]) > 2.0 for c in wide)
    narrow = [c for c, m in D.META.items() if m["kind"] == "gumbel" and m["C"] >= 65]
    assert narrow and all(((D.get(c, "params")[1] > 0.5) & (D.get(c, "params")[1] < 2.0)).sum() > 50 for c in narrow)
    # genextreme: shapes on both sides of 0 and near it, and a value outside the support of the start values (the penalty)
    c = np.concatenate([D.get(k, "params")[0] for k in D.NM_CASES if D.META[k]["dist"] == "genextreme"])
    c = c[np.isfinite(c)]
    assert c.min() < -0.2 and c.max() > 0.2 and (np.abs(c) < 0.02).any()
    assert any(D.get(k, "penalty_at_start").any() for k in D.NM_CASES if D.META[k]["dist"] == "genextreme")


def test_levels_are_recorded_through_the_switch_of_parametric_quantile():
    import scipy.stats as scipy_stats
    assert S.quantile_route(1 - 1.0 / np.array(D.T_RETURN, float))[0] == "ppf"      # q = 0.5 is not above 0.5
    assert S.quantile_route(1.0 / np.array(D.T_RETURN, float))[0] == "ppf"
    assert S.quantile_route(1 - 1.0 / np.array(D.T_RETURN_ISF, float))[0] == "isf"
    case = "gumbel_ml_33x65f4"
    p = D.get(case, "params")
    func, arg = S.quantile_route(1 - 1.0 / np.array(D.T_RETURN_ISF, float))
    np.testing.assert_array_equal(D.get(case, "levels_isf"), scipy_stats.gumbel_r.isf(arg[:, None], p[0][None], p[1][None]))
    np.testing.assert_array_equal(D.get(case, "levels_min"), scipy_stats.gumbel_r.ppf(1.0 / np.array(D.T_RETURN, float)[:, None], p[0][None], p[1][None]))


def test_known_answer_through_scipy():
    """test_genextreme_fit of the reference: the 20 values, from the start values of _fit_start."""
    import scipy.stats as scipy_stats
    k = D.KNOWN["test_genextreme_fit"]
    x = np.asarray(k["values"], float)
    assert len(x) == 20 and k["rtol"] == 1e-5 and k["expected"] == [0.20949, 297.954091, 75.7911863]
    s = np.sqrt(6 * x.var()) / np.pi
    p = scipy_stats.genextreme.fit(x, 0.1, loc=x.mean() - 0.57722 * s, scale=s)
    np.testing.assert_allclose(p, k["expected"], rtol=k["rtol"])
    np.testing.assert_allclose(p, k["scipy"], rtol=1e-12)


# ---- the mirrors of the #defines ---------------------------------------------------------------------------------------------
def test_the_mirrors_of_the_defines():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    d = {k: int(v) for k, v in re.findall(r"^#define\s+(XH_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    assert {k[len("XH_DIST_"):].lower(): d[k] for k in ("XH_DIST_NORM", "XH_DIST_GUMBEL_R", "XH_DIST_GENEXTREME", "XH_DIST_GAMMA",
                                                         "XH_DIST_FISK", "XH_DIST_LOGNORM")} == capi.DIST_CODES
    assert sorted(capi.DIST_CODES.values()) == list(range(d["XH_DIST_NDISTS"])) and d["XH_DIST_NDISTS"] == capi.DIST_NDISTS
    assert set(capi.DIST_CODES) == set(S.FIT_DISTS)
    assert {"APP": d["XH_DIST_APP"], "ML": d["XH_DIST_ML"]} == capi.DIST_METHODS
    assert {k: d[f"XH_DIST_{k.upper()}"] for k in ("ppf", "isf", "cdf", "pdf")} == capi.DIST_FUNCS
    assert d["XH_DISTFIT_MAX_Q"] == capi.DISTFIT_MAX_Q == 16
    assert {k: d[f"XH_DISTFIT_{k.upper()}"] for k in ("fitted", "nan", "budget", "support")} == capi.DISTFIT_STATUS
    assert len(d) == 18 and d == capi.UNIT_DEFINES["xclim_hip_distfit.h"]   # every #define of the header has a mirror above


# ---- argument validation, without a device ---------------------------------------------------------------------------------
X = np.linspace(1.0, 40.0, 40).reshape(20, 2)


@pytest.mark.parametrize("dist, method, kw", [
    ("weibull_min", "ML", {}), ("genpareto", "APP", {}),                       # other distributions
    ("norm", "MM", {}), ("gamma", "PWM", {}), ("genextreme", "MSE", {}), ("genextreme", "MPS", {}),
    ("lognorm", "ML", {}), ("lognorm", "MLE", {}),                             # scipy's profile-likelihood route
    ("gamma", "ML", {"fscale": 2.0}), ("genextreme", "ML", {"optimizer": None}), ("gamma", "ML", {"bounds": {}}),
    ("norm", "ML", {"floc": 0.0}), ("gumbel_r", "ML", {"floc": 0.0}), ("genextreme", "ML", {"floc": 0.0}),
    ("norm", "APP", {}), ("gumbel_r", "APP", {}),                              # the reference itself raises KeyError here
])
def test_unserved_fits(dist, method, kw):
    with pytest.raises(S.NotServed):
        S.fit(X, dist, method, device=NoDevice(), **kw)


def test_rv_continuous_objects():
    import scipy.stats as scipy_stats
    for name in S.FIT_DISTS:
        assert S.dist_name(getattr(scipy_stats, name)) == name and S.dist_name(name) == name
    with pytest.raises(S.NotServed):
        S.dist_name(scipy_stats.weibull_min)
    with pytest.raises(S.NotServed):
        S.dist_name(scipy_stats.gamma(2.0))       # a frozen distribution is not the singleton

    class Lmom:                                   # an lmoments3-like object with a served name
        name = "gamma"

    with pytest.raises(S.NotServed):
        S.fit(X, Lmom(), "PWM", device=NoDevice())
    with pytest.raises(S.NotServed):
        S.fit(X, Lmom(), "ML", device=NoDevice())


def test_value_errors_and_field_kinds():
    with pytest.raises(ValueError, match="Fitting method not recognized: FOO"):
        S.fit(X, "norm", "foo", device=NoDevice())
    with pytest.raises(ValueError, match="Fitting method not recognized"):
        S.fa(X, 10, "weibull_min", method="nope", device=NoDevice())   # the method is checked first, as the reference does
    with pytest.raises(S.NotServed, match="int64"):
        S.fit(X.astype(np.int64), "norm", device=NoDevice())
    with pytest.raises(S.NotServed, match="bool"):
        S.fit(X > 3, "norm", device=NoDevice())
    for mode in ("mean", "sum", ""):
        with pytest.raises(ValueError, match="should be either 'max' or 'min'"):
            S.fa(X, 10, "norm", mode, device=NoDevice())
        with pytest.raises(ValueError, match="should be either 'max' or 'min'"):
            S.frequency_analysis(X, mode, 10, "norm", time=object(), device=NoDevice())
    with pytest.raises(S.NotServed):
        S.fa(X, 10, "lognorm", device=NoDevice())
    with pytest.raises(S.NotServed):
        S.frequency_analysis(X, "max", 10, "gamma", time=object(), method="PWM", device=NoDevice())
    with pytest.raises(S.NotServed):
        S.frequency_analysis(X, "high", 10, "norm", time=object(), device=NoDevice())   # no resampling operator of that name
    with pytest.raises(TypeError, match="TimeAxis"):
        S.frequency_analysis(X, "max", 10, "norm", device=NoDevice())
    with pytest.raises(ValueError, match="need `dist`"):
        S.parametric_quantile(np.ones((2, 3)), 0.5, device=NoDevice())
    with pytest.raises(ValueError, match="3 parameters"):
        S.parametric_cdf(np.ones((2, 3)), 0.5, "gamma", device=NoDevice())
    with pytest.raises(S.NotServed):
        S.parametric_pdf(np.ones((2, 3)), 0.5, "beta", device=NoDevice())
    with pytest.raises(S.NotServed):
        S.parametric_pdf(np.ones((2, 3), np.int32), 0.5, "norm", device=NoDevice())


def test_attributes_and_helpers():
    a = S.fit_attrs("genextreme", "MLE", {"units": "mm", "standard_name": "pr", "long_name": "x", "description": "y", "cell_methods": "z"})
    assert a == {"original_units": "mm", "original_standard_name": "pr", "original_long_name": "x", "original_description": "y",
                 "cell_methods": "z", "long_name": "genextreme parameters", "description": "Parameters of the genextreme distribution",
                 "method": "MLE", "estimator": "Maximum likelihood", "scipy_dist": "genextreme", "units": ""}
    assert S.fit_attrs("norm", "APP")["estimator"] == "Approximative method"
    from xclim_amd import generic as G

    assert G.default_freq() == "YS-JAN" and G.default_freq(season="DJF") == "YS-DEC" and G.default_freq(month=[7, 8]) == "YS-JUL"
    assert G.default_freq(doy_bounds=(60, 90)) == "YS-FEB" and G.default_freq(date_bounds=("03-15", "05-01")) == "YS-MAR"
    with pytest.raises(ValueError, match="Unknown group"):
        G.default_freq(week=3)
    from xclim_amd import kernels as K

    assert [K.dist_nparams(d) for d in S.FIT_DISTS] == [len(v) for v in S.FIT_DISTS.values()] == [2, 2, 3, 3, 3, 3]
