"""The distribution-fit unit on the device (xclim_amd/stats.py: fit, parametric_*, fa, frequency_analysis; xclim_amd/csrc/distfit.hip)
against the reference's recorded results (tests/golden/distfit_vectors.npz, made by tests/golden/make_distfit_golden.py).

Tolerances.  Closed-form and root-found fits, every APP and the closed-form ppf / isf / cdf / pdf: rtol 1e-9, the project's
tolerance for this class (tests/test_gpu_stdidx.py).  Converged Nelder–Mead fits: rtol 1e-3 on the parameters, the project's
tolerance for the same optimizer; the share that agrees to 1e-8 is printed.  Two tolerances are ten times the largest relative
deviation from the recorded reference values measured on an MI355X, within the caps the unit's issue sets:

* gamma's ppf / isf (Newton steps on gammainc): measured 6.66e-14 (gamma_flocneg_ml_150x65f8; 4.9e-16 to 9.7e-15 in the other
  twelve gamma cases); asserted 6.66e-13, far below the cap of 1e-6;
* the return levels of Nelder–Mead fits: measured 5.93e-13 (fisk_ml_32x65f4; gamma 1.9e-13, genextreme 2.3e-16 to 7.1e-14);
  asserted 5.93e-12, far below the cap of 1e-2.  Every one of the 508 recorded Nelder–Mead fits ran with scipy's own number of
  evaluations on the device, so what is left is the last bits of log, pow, log1p and lgamma.
"""
import numpy as np
import pytest

import distfitcases as D
from poisoned import POISON, pattern, poisoned_outputs, unwritten  # noqa: F401  (autouse: every test runs on poisoned output buffers)
from xclim_amd import _capi as capi
from xclim_amd import kernels as K
from xclim_amd import stats as S

pytestmark = pytest.mark.gpu

MEASURED_GAMMA_INVERSE = 6.66e-14   # the largest relative deviations measured on the device (module text)
MEASURED_NM_LEVELS = 5.93e-13
TOL_GAMMA_INVERSE = min(10 * MEASURED_GAMMA_INVERSE, 1e-6)
TOL_NM_LEVELS = min(10 * MEASURED_NM_LEVELS, 1e-2)


def device_fit(dev, case, **kw):
    m = D.META[case]
    return K.dist_fit(dev, dev.to_device(D.field(case)), m["dist"], m["method"], m["floc"], **kw)


def check_pattern(case, params, status, nfev):
    exp, est = D.get(case, "params"), D.get(case, "status")
    assert params.shape == exp.shape and params.dtype == np.float64
    assert not unwritten(params).any() and not unwritten(status).any() and not unwritten(nfev).any()
    np.testing.assert_array_equal(np.isnan(params), np.isnan(exp), err_msg=f"{case}: NaN pattern")
    np.testing.assert_array_equal(status, est, err_msg=f"{case}: status bytes")
    # all of a cell's parameters are NaN, or none
    assert (np.isnan(params).all(axis=0) | ~np.isnan(params).any(axis=0)).all()


def rel_dev(got, exp):
    """The largest |got - exp| / |exp| over the finite recorded values (0 where there is none)."""
    ok = np.isfinite(exp)
    assert np.isfinite(got[ok]).all()
    with np.errstate(all="ignore"):
        d = np.abs(got[ok] - exp[ok]) / np.abs(exp[ok])
    return float(np.nanmax(d)) if d.size else 0.0


@pytest.mark.parametrize("case", D.DIRECT_CASES)
def test_closed_form_and_root_found_fits(dev, case):
    params, nfev, status, _ = device_fit(dev, case)
    params, nfev, status = params.get(), nfev.get(), status.get()
    check_pattern(case, params, status, nfev)
    assert (nfev == 0).all()
    np.testing.assert_allclose(params, D.get(case, "params"), rtol=1e-9, atol=0, err_msg=case)


@pytest.mark.parametrize("case", D.NM_CASES)
def test_nelder_mead_fits(dev, case):
    params, nfev, status, _ = device_fit(dev, case)
    params, nfev, status = params.get(), nfev.get(), status.get()
    check_pattern(case, params, status, nfev)
    assert (nfev <= D.budget(case)).all() and (nfev >= 0).all()
    exp = D.get(case, "params")
    fitted = D.get(case, "status") == capi.DISTFIT_STATUS["fitted"]
    assert (nfev[fitted] > 0).all() and (nfev[~fitted] == 0).all()
    with np.errstate(all="ignore"):
        close = (np.abs(params - exp) <= 1e-8 * np.abs(exp)).all(axis=0)
    same_path = nfev == D.get(case, "nfev")
    print(f"{case}: {int(close[fitted].sum())} of {int(fitted.sum())} fits agree with scipy to 1e-8, "
          f"{int(same_path[fitted].sum())} with its evaluation count; worst relative deviation {rel_dev(params, exp):.3g}")
    np.testing.assert_allclose(params, exp, rtol=1e-3, atol=0, err_msg=case)


def route(mode, t):
    t = np.asarray(t, float)
    return S.quantile_route(1 - 1.0 / t if mode == "max" else 1.0 / t)


@pytest.mark.parametrize("case", D.CASES)
def test_fused_levels_equal_eval_on_the_same_parameters(dev, case):
    m = D.META[case]
    for mode, t in (("max", D.T_RETURN), ("min", D.T_RETURN), ("max", D.T_RETURN_ISF)):
        func, q = route(mode, t)
        params, _, _, levels = device_fit(dev, case, q=q, qfunc=func)
        again = K.dist_eval(dev, params, m["dist"], func, q).get()
        levels = levels.get()
        assert not unwritten(levels).any() and not unwritten(again).any()
        np.testing.assert_array_equal(levels.view(np.uint64), again.view(np.uint64), err_msg=f"{case} {mode} {t}")
    assert route("max", D.T_RETURN_ISF)[0] == "isf" and route("max", D.T_RETURN)[0] == "ppf"


def recorded_functions(case):
    """(func, argument, recorded values) of a case: the three level sets, cdf and pdf."""
    v = D.get(case, "v")
    return [(*route("max", D.T_RETURN), D.get(case, "levels_max")), (*route("min", D.T_RETURN), D.get(case, "levels_min")),
            (*route("max", D.T_RETURN_ISF), D.get(case, "levels_isf")), ("cdf", v, D.get(case, "cdf")), ("pdf", v, D.get(case, "pdf"))]


@pytest.mark.parametrize("case", D.CASES)
def test_eval_against_scipy_on_the_recorded_parameters(dev, case):
    m = D.META[case]
    params = dev.to_device(D.get(case, "params"))
    worst = 0.0
    for func, arg, exp in recorded_functions(case):
        got = K.dist_eval(dev, params, m["dist"], func, arg).get()
        assert not unwritten(got).any()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{case} {func}")
        if m["dist"] == "gamma" and func in ("ppf", "isf"):
            worst = max(worst, rel_dev(got, exp))
            continue
        np.testing.assert_allclose(got, exp, rtol=1e-9, atol=0, err_msg=f"{case} {func}")
    if m["dist"] == "gamma":
        print(f"{case}: gamma ppf / isf, largest relative deviation from scipy {worst:.3g} (asserted {TOL_GAMMA_INVERSE:.3g})")
        assert worst <= TOL_GAMMA_INVERSE


@pytest.mark.parametrize("case", D.NM_CASES)
def test_return_levels_of_nelder_mead_fits(dev, case):
    worst = 0.0
    for (func, q), key in ((route("max", D.T_RETURN), "levels_max"), (route("min", D.T_RETURN), "levels_min"),
                           (route("max", D.T_RETURN_ISF), "levels_isf")):
        _, _, _, levels = device_fit(dev, case, q=q, qfunc=func)
        got, exp = levels.get(), D.get(case, key)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{case} {key}")
        worst = max(worst, rel_dev(got, exp))
    print(f"{case}: return levels, largest relative deviation from the reference {worst:.3g} (asserted {TOL_NM_LEVELS:.3g})")
    assert worst <= TOL_NM_LEVELS


def test_known_answer(dev):
    k = D.KNOWN["test_genextreme_fit"]
    p, attrs = S.fit(np.asarray(k["values"], np.float64), k["dist"], k["method"], device=dev)
    np.testing.assert_allclose(p, k["expected"], rtol=1e-5)
    assert attrs["scipy_dist"] == "genextreme" and attrs["estimator"] == "Maximum likelihood"


@pytest.mark.parametrize("case", ["gev_ml_33x65f8", "gumbelwide_ml_33x65f4", "lognorm_floc0_app_33x65f8"])
def test_padded_row_views(dev, case):
    """Pitch larger than C on the field and on every output: the padding and the outputs hold poison before the call, every
    element (k, c < C) is written and the padding of every output row keeps its poison."""
    m = D.META[case]
    x = D.field(case)
    T, C = x.shape
    ld, ldp, ldl = C + 7, C + 3, C + 5
    wide = np.full((T, ld), pattern(x.dtype), x.dtype)
    wide[:, :C] = x
    nparams = K.dist_nparams(m["dist"])
    func, q = route("min", D.T_RETURN)
    outs = {"params": dev.empty((nparams, ldp), np.float64), "nfev": dev.empty((C,), np.int32), "status": dev.empty((C,), np.uint8),
            "levels": dev.empty((len(q), ldl), np.float64)}
    K.dist_fit(dev, dev.to_device(wide), m["dist"], m["method"], m["floc"], q=q, qfunc=func, C_=C, ld=ld, outs=outs,
               pitches={"params": ldp, "levels": ldl})
    dense = device_fit(dev, case, q=q, qfunc=func)
    for key, d in zip(("params", "nfev", "status", "levels"), dense):
        got, exp = outs[key].get(), d.get()
        assert not unwritten(exp).any()
        if got.ndim == 2:
            assert unwritten(got[:, C:]).all(), f"{key}: the padding was written"
            got = got[:, :C]
        assert not unwritten(got).any(), f"{key}: an element was not written"
        np.testing.assert_array_equal(got.view(f"u{got.dtype.itemsize}"), exp.view(f"u{exp.dtype.itemsize}"), err_msg=key)
    # xh_dist_eval on the padded parameters into a padded output
    out = dev.empty((len(q), ldl), np.float64)
    K.dist_eval(dev, outs["params"], m["dist"], func, q, C_=C, ld=ldp, out=out, ld_out=ldl)
    got = out.get()
    assert unwritten(got[:, C:]).all() and not unwritten(got[:, :C]).any()
    np.testing.assert_array_equal(got[:, :C].view(np.uint64), dense[3].get().view(np.uint64))


@pytest.mark.parametrize("window", [1, 3])
def test_frequency_analysis_is_the_composed_calls(dev, window):
    """Three years x 65 cells of daily data; three values per cell are too few for the Nelder-Mead paths: gumbel_r."""
    from xclim_amd import generic as G
    from xclim_amd.timeaxis import TimeAxis

    rng = np.random.default_rng(7)
    T = 3 * 365
    time = TimeAxis.daily("2001-01-01", T, "noleap")
    da = (10 + 4 * rng.standard_normal((T, 5, 13))).astype(np.float32)
    da[200:230, 0, 0] = np.nan
    for mode in ("max", "min"):
        out = S.frequency_analysis(da, mode, [2, 10], "gumbel_r", time=time, window=window, device=dev)
        if window > 1:
            sel = G.select_rolling_resample_op(da, mode, window, time, window_center=False, window_op="mean", freq="YS-JAN", device=dev)
        else:
            sel = G.select_resample_op(da, mode, time, "YS-JAN", device=dev)
        assert sel.shape == (3, 5, 13)
        p = S.fit(sel, "gumbel_r", device=dev)
        t = np.array([2, 10])
        exp = S.parametric_quantile(p, 1 - 1.0 / t if mode == "max" else 1.0 / t, device=dev)
        assert out.shape == (2, 5, 13) and np.isfinite(out[:, 1:]).all()
        np.testing.assert_array_equal(out.view(np.uint64), exp.view(np.uint64))
        np.testing.assert_array_equal(out, S.fa(sel, [2, 10], "gumbel_r", mode, device=dev))
    with pytest.raises(ValueError, match="should be either 'max' or 'min'"):
        S.frequency_analysis(da, "mean", 2, "gumbel_r", time=time, device=dev)


def test_lognorm_support_error_and_limits(dev):
    case = "lognorm_floc0_ml_33x65f4"
    with pytest.raises(ValueError, match="lognorm"):   # the cell whose minimum equals floc: the reference's error for the call
        S.fit(D.field(case), "lognorm", floc=0.0, device=dev)
    x = dev.to_device(D.field(case))
    with pytest.raises(capi.XclimHipError) as err:
        K.dist_fit(dev, x, "lognorm", "ML", 0.0, q=np.linspace(0.1, 0.9, capi.DISTFIT_MAX_Q + 1))
    assert err.value.code == capi.XH_ERR_LIMIT
    _, _, _, levels = K.dist_fit(dev, x, "lognorm", "ML", 0.0, q=np.linspace(0.1, 0.9, capi.DISTFIT_MAX_Q))
    assert not unwritten(levels.get()).any()
    many = S.fa(D.field("norm_ml_33x65f4"), np.arange(2, 22), "norm", device=dev)   # 20 periods: fit, then eval
    assert many.shape == (20, 65) and not unwritten(many).any()
