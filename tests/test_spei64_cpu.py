"""CPU checks of the float64 standardized indices: the numpy restatement of the float64 chain (tests/spei64cpu.py) against
the reference's own fits on float64 samples (tests/golden/spei_vectors.npz), the fixture's coverage, and the
XCLIM_AMD_FLOAT64 policies of the host mirror (xclim_amd.stats), raised or passed before any device work."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spei64cpu  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spei_vectors.npz")
Z = np.load(GOLD)
META = json.loads(str(Z["meta"]))
FAST = [n for n in META if META[n]["method"] == "APP" or (META[n]["dist"] == "gamma" and META[n]["floc"] is not None)]
LDS_MAX_F64 = 32  # values per group the float64 instance of xh_si_fit stages in LDS


def case(name):
    return {k.split("__", 1)[1]: Z[k] for k in Z.files if k.startswith(name + "__")}, META[name]


def field(c, m):
    """The float64 input of a case, NaN runs included (as tests/golden/make_spei_golden.py writes them)."""
    x = c["codes"].astype(np.float64) * np.float64(c["scale"])
    C = x.shape[1]
    if m["monthly_input"]:
        x[30:42, C - 1] = np.nan
    else:
        x[100:160, C - 1] = np.nan
        if m["freq"] == "D":
            x[400:403, 0] = np.nan
    return x


def test_golden_covers_the_issue():
    kinds = {(m["dist"], m["method"], m["floc"] is not None, m["zero_inflated"]) for m in META.values()}
    assert {("gamma", "ML", False, False), ("fisk", "ML", False, False), ("gamma", "APP", True, False),
            ("fisk", "APP", True, False), ("gamma", "ML", True, False)} <= kinds      # SPEI forms
    assert {("gamma", "ML", False, True), ("gamma", "APP", True, True), ("gamma", "ML", True, True)} <= kinds  # SPI
    assert all(m["floc"] < 0 for m in META.values() if m["floc"] is not None and not m["zero_inflated"])
    assert {m["window"] for m in META.values()} >= {1, 3, 12}
    assert {m["freq"] for m in META.values()} == {"MS", "D"}
    assert {m["cal"] for m in META.values() if not isinstance(m["cal"], list)} == {None, "reuse"}
    assert any(isinstance(m["cal"], list) for m in META.values())
    leap = case("spei_gamma_app_daily_leap")[0]
    assert 365 in leap["gidx"]  # day 366
    groups = [np.bincount(case(n)[0]["fit_g"][case(n)[0]["fit_g"] >= 0]).max() for n in META]
    assert max(groups) > LDS_MAX_F64 and min(groups) <= LDS_MAX_F64
    for name, m in META.items():
        c, _ = case(name)
        x = field(c, m)
        v = x[np.isfinite(x) & (x != 0)]
        assert np.mean(v.astype(np.float32).astype(np.float64) != v) > 0.999  # values float32 cannot hold
        if m["kind"] != "pr":
            assert (x < 0).any()  # a water budget
        else:
            assert (x == 0).any()
        xp = c["xp"]
        assert (np.isnan(xp[:, -1]) & np.isfinite(xp[:, 0])).any()  # a NaN month (or day, or year) in one cell only
    assert os.path.getsize(GOLD) < 300_000


@pytest.mark.parametrize("name", sorted(META))
def test_restatement_preprocessing_is_bitwise(name):
    c, m = case(name)
    xp = spei64cpu.preprocess(field(c, m), c["year"], c["month"], m["freq"], m["window"], m["monthly_input"])
    np.testing.assert_array_equal(xp, c["xp"])
    if m["cal"] == "reuse":
        Ta = int(c["reuse_T"])
        xa = spei64cpu.preprocess(field(c, m)[:Ta], c["year"][:Ta], c["month"][:Ta], m["freq"], m["window"])
        np.testing.assert_array_equal(xa, c["xp_fit"])


def _fit(name):
    c, m = case(name)
    x = c["xp_fit"] if m["cal"] == "reuse" else c["xp"]
    assert x.dtype == np.float64
    return c, m, spei64cpu.fit(x, c["fit_g"], m["G"], m["dist"], m["method"], m["zero_inflated"], m["floc"])


@pytest.mark.parametrize("name", sorted(META))
def test_restatement_matches_reference_fits(name):
    c, m, (p, nz, nn, nfev) = _fit(name)
    ref = c["params"]
    assert not c["failed"].any()
    np.testing.assert_array_equal(np.isnan(p), np.isnan(ref))
    np.testing.assert_array_equal(nz, c["nz"])
    np.testing.assert_array_equal(nn, c["nn"])
    if name in FAST:
        np.testing.assert_allclose(p, ref, rtol=1e-9, atol=0, equal_nan=True)
        return
    # Nelder-Mead: the converged fits to 1e-3; a fit stopped at the 600-evaluation budget is wherever its walk was (a
    # 3-parameter gamma fit of 5 values can run off towards scale -> inf), so it is compared through its index
    conv = np.broadcast_to((nfev < 600)[:, None, :], p.shape)
    np.testing.assert_allclose(p[conv], ref[conv], rtol=1e-3, atol=0, equal_nan=True)
    same = np.all(np.isclose(p, ref, rtol=1e-8, atol=0, equal_nan=True), axis=1)[nfev < 600].mean()
    # a 3-parameter fit of 5 or 6 values is loosely determined: a last-bit difference of log / lgamma can send its walk
    # down another path to the same optimum within 1e-3 (4 of the 22 converged fits of the reuse case)
    assert same >= 0.8, f"only {same:.3f} of the converged Nelder-Mead fits follow scipy's trajectory"
    assert nfev.max() <= 600
    if (nfev >= 600).any():
        zi = m["zero_inflated"]
        own = spei64cpu.index(c["xp"], c["gidx"], p, m["dist"], nz if zi else None, nn if zi else None)
        exp = spei64cpu.index(c["xp"], c["gidx"], ref, m["dist"], nz if zi else None, nn if zi else None)
        bad = (nfev >= 600)[c["gidx"]]
        np.testing.assert_array_equal(np.isnan(own[bad]), np.isnan(exp[bad]))
        assert np.isclose(own[bad], exp[bad], rtol=0, atol=2e-2, equal_nan=True).mean() >= 0.99


@pytest.mark.parametrize("name", sorted(META))
def test_restatement_index(name):
    c, m, _ = _fit(name)
    interp = {"center": 0.5, "upper": 1.0}.get(m["interp"], m["interp"]) if isinstance(m["interp"], str) else m["interp"]
    ab = {"ecdf": (0, 1), "weibull": (0, 0)}[m["plotting"]] if isinstance(m["plotting"], str) else m["plotting"]
    zi = m["zero_inflated"]
    si = spei64cpu.index(c["xp"], c["gidx"], c["params"], m["dist"], c["nz"] if zi else None, c["nn"] if zi else None,
                         float(interp), float(ab[0]), float(ab[1]))
    np.testing.assert_array_equal(np.isnan(si), np.isnan(c["spi"]))
    np.testing.assert_allclose(si, c["spi"], rtol=0, atol=1e-9, equal_nan=True)


# ---- the XCLIM_AMD_FLOAT64 policies of the host mirror -------------------------------------------------------------------
def test_native_served_names_the_standardized_indices():
    from xclim_amd import _capi

    assert "standardized_index" in _capi.NATIVE_SERVED and "standardized_index_fit_params" in _capi.NATIVE_SERVED
    assert "SPEI" in _capi.NATIVE_SERVED and "SPI" in _capi.NATIVE_SERVED


def test_the_float64_twins_are_declared():
    from xclim_amd import _capi

    for name in ("xh_si_fit_f64", "xh_si_apply_f64"):
        assert _capi.SIGNATURES[name] == _capi.SIGNATURES[name[:-4]]


class _NoDevice(Exception):
    pass


def _wb():
    from xclim_amd.timeaxis import TimeAxis

    rng = np.random.default_rng(0)
    return rng.normal(0.5, 2.0, (730, 2)), TimeAxis.daily("2000-01-01", 730, "noleap")


@pytest.fixture()
def no_device(monkeypatch):
    """get_device raises _NoDevice: a call that reaches it has passed every host-side refusal."""
    from xclim_amd import stats as xs

    def refuse(*a, **k):
        raise _NoDevice

    monkeypatch.setattr(xs, "get_device", refuse)


def test_native_takes_float64_fields_to_the_device(monkeypatch, no_device):
    from xclim_amd import indices as xi
    from xclim_amd import stats as xs

    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "native")
    wb, t = _wb()
    with pytest.raises(_NoDevice):
        xi.standardized_precipitation_evapotranspiration_index(wb, t, window=3)
    with pytest.raises(_NoDevice):
        xi.standardized_precipitation_index(np.abs(wb), t)
    with pytest.raises(_NoDevice):
        xs.standardized_index_fit_params(wb, t, "MS", 3, "fisk", "ML")
    xs._refuse_float64(wb)  # the adapter's check in front of a params DataArray lets it through


def test_the_other_policies_are_unchanged(monkeypatch, no_device):
    from xclim_amd import indices as xi
    from xclim_amd import stats as xs
    from xclim_amd._capi import Float64FieldError

    wb, t = _wb()
    monkeypatch.delenv("XCLIM_AMD_FLOAT64", raising=False)
    with pytest.raises(Float64FieldError, match=r"standardized_index: float64 fields are only served by threshold_count"):
        xi.standardized_precipitation_evapotranspiration_index(wb, t)
    with pytest.raises(Float64FieldError):
        xs.standardized_index_fit_params(wb, t, "MS", 1, "gamma", "ML")
    with pytest.raises(Float64FieldError):
        xs._refuse_float64(wb)
    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "round")
    with pytest.raises(_NoDevice):  # rounded later, in _flatten, with its PrecisionWarning
        xi.standardized_precipitation_evapotranspiration_index(wb, t)
    xs._refuse_float64(wb)

