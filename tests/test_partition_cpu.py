"""The uncertainty-partitioning unit without a GPU: the numpy restatement (tests/partitioncpu.py) against the recorded EXACT fits
(tests/golden/partition_vectors.npz: the rational solution of the normal equations, rounded) and against the properties the
reference's own tests ask for (tests/test_partitioning.py, with seeded standard-normal noise of the same shapes and its
tolerances); the error messages and the NotServed rules of the mirror, which answer before the device is touched; the component
names; the mirrors of the header's #defines; fractional_uncertainty and hawkins_sutton_09_weighting against hand-computed values."""
import os
import re

import numpy as np
import pytest

import partitioncpu as P
from xclim_amd import _capi, ensembles, partitioning
from xclim_amd.fields import NotServed
from xclim_amd.timeaxis import TimeAxis


def annual(years, calendar="standard"):
    years = np.asarray(years)
    return TimeAxis(years, np.full(len(years), 12), np.full(len(years), 31), calendar)


@pytest.mark.parametrize("name", P.FAMILIES)
def test_the_restatement_against_the_exact_fits(name):
    v, fam = P.vectors(), P.family(name)
    cells = list(P.EXACT_CELLS)
    da = fam["da"][..., cells]
    T = da.shape[0]
    degs = range(5) if name == P.DEG_FAMILY else [fam["deg_given"] if fam["deg_given"] is not None else 4]
    for deg in degs:
        sm, mag = (a.reshape(T, -1, len(cells)) for a in P.fit(da, P.stamps_ns(fam["years"]), deg))
        ex = v[f"{name}/deg{deg}/exact"]
        n, status = P.status_of(da.reshape(T, -1, len(cells)), deg)
        fitted = np.broadcast_to(status == P.FITTED, sm.shape)
        assert np.array_equal(np.isnan(sm[fitted]), np.isnan(ex[fitted]))
        assert np.isnan(ex[~fitted]).all()   # (an ill-posed series has no exact answer; the restatement's lstsq gives a minimum norm one)
        ok = fitted & ~np.isnan(ex)
        dist = (np.abs(sm[ok] - ex[ok]) / mag[ok]).max()
        print(f"{name} deg {deg}: the restatement is within {dist:.2e} of the scale (recorded {v[f'{name}/deg{deg}/restated_dist'][0]:.2e})")
        assert dist <= 0.1 * P.RTOL   # a tenth of the device's bound (the generator asserts the same)
    if name in P.VALUE_FAMILIES:   # the recorded g and u: the restatement is the same on this machine, within its own bounds
        g, u, bg, bu = P.restate(fam, cells)
        for got, want, bound in ((g, v[f"{name}/g"], bg), (u, v[f"{name}/u"], bu)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert (np.abs(got[ok] - want[ok]) <= bound[ok]).all()


def test_the_fixture_families_hold_what_they_are_for():
    v = P.vectors()
    assert v["ls_nan/bunched_cond"] < 1e3 and v["worst_cond"] < 1e3
    fam = P.family("ls_nan")
    assert np.flatnonzero(~np.isnan(fam["da"][:, 1, 0, 1, 2])).tolist() == list(P.BUNCHED_ROWS)
    assert np.isnan(fam["da"][..., 9]).all() and np.isnan(fam["da"][:, 0, 1, 0, 5]).all()
    g, u, _, _ = P.restate(fam, [5, 9])
    assert np.isnan(g[:, 1]).all() and np.isnan(u[:, :, 1]).all() and not np.isnan(g[:, 0]).any()
    n, status = P.status_of(P.family("ls_illposed")["da"][:, 1, 2, 0, 3])
    assert n == 4 and status == P.ILLPOSED
    g, u, _, _ = P.restate(P.family("ls_T10"), [0])   # window 11 on 10 rows: no variability, no total
    assert np.isnan(u[3]).all() and np.isnan(u[4]).all() and not np.isnan(u[:3]).any()
    g, u, _, _ = P.restate(P.family("ls_T12"), [0])   # two complete windows of 11 rows: rows 5 and 6
    assert np.flatnonzero(~np.isnan(u[3, :, 0])).tolist() == [5, 6]
    g, u, _, _ = P.restate(P.family("hs_T10"), [0])   # one complete window of 10 rows, row 5, from t0 = 2000 (row 5) on
    assert not np.isnan(u).any()
    hs = P.family("hs_nan")["da"]
    res = P.rolling(hs[:, 0, 0, :1].astype(np.float64), 10, "mean")[:, 0]   # NaN at rows 0, 20, 59: windows i - 5 .. i + 4
    assert np.flatnonzero(np.isnan(res[5:55])).tolist() == [0] + [k - 5 for k in range(16, 26)]   # rows 5 and 16 .. 25


def test_hawkins_sutton_properties_of_the_reference_tests():
    rng = np.random.default_rng(3487612)
    mean = np.arange(-6, 7, 1)[None, :] + np.arange(10, 41, 10)[:, None]
    x = rng.standard_normal((4, 13, 60)) + mean[:, :, None]
    da = np.moveaxis(x, -1, 0)[..., None]
    g, u, _, _ = P.hawkins_sutton(da, P.Y60)
    vm = dict(zip(partitioning.HS_COMPONENTS, u.mean(axis=1)[:, 0]))
    np.testing.assert_array_almost_equal(g.mean(axis=0), 0, decimal=1)
    np.testing.assert_array_almost_equal(vm["scenario"], 0, decimal=1)
    assert vm["model"] > vm["variability"]
    P.hawkins_sutton(da, P.Y60, sm=P.fit(da, P.stamps_ns(P.Y60), 2)[0])
    x = rng.standard_normal((4, 13, 60)) + np.arange(60) + mean[:, :, None]
    g, u, _, _ = P.hawkins_sutton(np.moveaxis(x, -1, 0)[..., None], P.Y60, kind="*")
    su = u[partitioning.HS_COMPONENTS.index("scenario"), :, 0]
    assert su[P.Y60 >= 2020].mean() > su[(P.Y60 >= 2000) & (P.Y60 <= 2010)].mean()


def test_lafferty_sriver_properties_of_the_reference_tests():
    rng = np.random.default_rng(3487613)
    mean = np.arange(-2, 3)[None, None, :] + np.arange(-6, 7)[None, :, None] + np.arange(10, 41, 10)[:, None, None]
    da = np.moveaxis(rng.standard_normal((4, 13, 5, 60)) + mean[..., None], -1, 0)[..., None]
    g, u, _, _ = P.lafferty_sriver(da, P.Y60)
    with np.errstate(all="ignore"):
        vm = dict(zip(partitioning.LS_COMPONENTS, np.nanmean(u, axis=1)[:, 0]))
    np.testing.assert_array_almost_equal(g.mean(axis=0), 25, decimal=1)
    assert vm["model"] > vm["variability"]
    P.lafferty_sriver(da, P.Y60, sm=P.fit(da, P.stamps_ns(P.Y60), 2)[0])
    g2, u2, _, _ = P.general_partition(da, P.Y60, ["scenario", "model", "downscaling"], var_first=["model", "downscaling"],
                                       mean_first=["scenario"], weights=["model", "downscaling"])
    names = partitioning.general_components(["model", "downscaling"], ["scenario"])
    np.testing.assert_allclose(g, g2, rtol=1e-14)   # (the two take their nested means in another order)
    for k, name in enumerate(partitioning.LS_COMPONENTS):
        assert np.array_equal(u[k], u2[names.index(name)], equal_nan=True), name


def test_component_names():
    assert partitioning.HS_COMPONENTS == ("variability", "model", "scenario", "total")
    assert partitioning.LS_COMPONENTS == ("model", "scenario", "downscaling", "variability", "total")
    assert partitioning.general_components() == ("scenario", "model", "reference", "adjustment", "variability", "total")
    assert partitioning.general_components(["a"], ["b", "c"]) == ("b", "c", "a", "variability", "total")
    for name in ("hawkins_sutton", "lafferty_sriver", "general_partition", "fractional_uncertainty", "hawkins_sutton_09_weighting",
                 "poly_smooth", "ensemble_mean_std_max_min", "HS_COMPONENTS", "LS_COMPONENTS", "general_components"):
        assert getattr(ensembles, name) is getattr(partitioning, name)


def test_the_mirrors_of_the_defines():
    header = os.path.join(os.path.dirname(P.HERE), "include", "units", "xclim_hip_partition.h")
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(XH_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    assert defines == _capi.UNIT_DEFINES["xclim_hip_partition.h"] and len(defines) == 26
    assert (P.FITTED, P.ALLNAN, P.ILLPOSED) == tuple(_capi.PT_STATUS[k] for k in ("fitted", "allnan", "illposed"))
    assert _capi.PT_MAX_T == 512 and _capi.PT_MAX_AXES == 4 and _capi.PT_MAX_AXIS == 64 and _capi.PT_MAX_MEMBERS == 4096
    assert {"xh_partition_smooth", "xh_partition_components", "xh_ensemble_stats"} <= set(_capi.UNIT_SIGNATURES)


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was asked for {name} before the arguments were checked")


def test_the_reference_s_errors_answer_before_the_device():
    dev = _NoDevice()
    t60 = annual(P.Y60)
    hs, ls = np.zeros((60, 2, 3, 4)), np.zeros((60, 2, 3, 2, 4))
    every_other = annual(np.arange(1970, 2090, 2))
    monthly = TimeAxis(np.repeat(np.arange(1970, 1975), 12), np.tile(np.arange(1, 13), 5), np.ones(60, int), "standard")
    for axis in (every_other, monthly):
        for call in (lambda a: partitioning.hawkins_sutton(hs, time=a, device=dev), lambda a: partitioning.lafferty_sriver(ls, time=a, device=dev),
                     lambda a: partitioning.general_partition(ls, time=a, dims=("scenario", "model", "reference"), device=dev),
                     lambda a: partitioning.poly_smooth(hs, a, device=_Upload())):
            with pytest.raises(ValueError, match=r"This algorithm expects annual time series\."):
                call(axis)
    with pytest.raises(ValueError, match="DataArray dimensions should include 'time', 'scenario' and 'model'."):
        partitioning.hawkins_sutton(hs, time=t60, dims=("scenario", "member"), device=dev)
    with pytest.raises(ValueError, match="DataArray dimensions should include 'time', 'scenario', 'downscaling' and 'model'."):
        partitioning.lafferty_sriver(ls, time=t60, dims=("scenario", "model", "method"), device=dev)
    with pytest.raises(ValueError, match=re.escape("DataArray dimensions should include ['scenario', 'model', 'reference', 'adjustment'] and time.")):
        partitioning.general_partition(ls, time=t60, dims=("scenario", "model", "reference"), device=dev)
    for sm in ("loess", None, 3.0):
        with pytest.raises(ValueError, match="sm should be 'poly' or a DataArray."):
            partitioning.general_partition(ls, sm, ["model", "downscaling"], ["scenario"], ["model"], time=t60,
                                           dims=("scenario", "model", "downscaling"), device=dev)


class _Upload:   # to_device hands the array back: the limits are checked on the shapes before any launch
    def to_device(self, a):
        return a


def test_what_is_not_served():
    dev = _NoDevice()
    t60 = annual(P.Y60)
    hs, ls = np.zeros((60, 2, 3, 4)), np.zeros((60, 2, 3, 2, 4))

    class Chunked:
        chunks, shape, dtype = ((1,),), (60, 2, 3, 4), np.dtype(np.float64)

    with pytest.raises(NotServed, match="integer"):
        partitioning.hawkins_sutton(hs.astype(np.int32), time=t60, device=dev)
    with pytest.raises(NotServed, match="chunked"):
        partitioning.hawkins_sutton(Chunked(), time=t60, device=dev)
    with pytest.raises(NotServed, match="da is float64 and sm float32"):
        partitioning.lafferty_sriver(ls, ls.astype(np.float32), time=t60, device=dev)
    with pytest.raises(NotServed, match="da is float32 and sm float64"):
        partitioning.hawkins_sutton(hs.astype(np.float32), hs, time=t60, device=dev)
    with pytest.raises(NotServed, match="up to 512"):
        partitioning.lafferty_sriver(np.zeros((513, 2, 3, 2, 1)), time=annual(np.arange(1500, 2013)), device=dev)
    with pytest.raises(NotServed, match="up to 4"):
        partitioning.general_partition(np.zeros((60, 2, 2, 2, 2, 2, 1)), var_first=["a", "b", "c", "d"], mean_first=["e"], weights=["a"],
                                       time=t60, dims=("a", "b", "c", "d", "e"), device=dev)
    with pytest.raises(NotServed, match="up to 64 entries each and 4096 members"):
        partitioning.hawkins_sutton(np.zeros((60, 2, 65, 1)), time=t60, device=dev)
    with pytest.raises(NotServed, match="up to 64 entries each and 4096 members"):
        partitioning.lafferty_sriver(np.zeros((60, 20, 20, 20, 1), np.float32), time=t60, device=dev)
    with pytest.raises(NotServed, match="mean_first dimension that is weighted"):
        partitioning.general_partition(ls, var_first=["model", "downscaling"], mean_first=["scenario"], weights=["scenario", "model"], time=t60,
                                       dims=("scenario", "model", "downscaling"), device=dev)
    with pytest.raises(NotServed, match="beyond"):   # a member axis the function does not partition belongs among the cells
        partitioning.hawkins_sutton(ls, time=t60, dims=("scenario", "model", "downscaling"), device=dev)
    with pytest.raises(NotServed, match="degree 5"):
        partitioning.poly_smooth(hs, t60, 5, device=dev)
    with pytest.raises(NotServed, match="float32 and float64"):
        partitioning.ensemble_mean_std_max_min(np.zeros((3, 4), np.int16), device=dev)


def test_fractional_uncertainty_and_the_hs09_weights_by_hand():
    u = np.array([[1.0, 2.0], [3.0, 2.0], [4.0, 4.0]])
    fu = partitioning.fractional_uncertainty(u, ("model", "scenario", "total"))
    assert np.array_equal(fu, [[25.0, 50.0], [75.0, 50.0], [100.0, 100.0]])
    years = np.arange(1996, 2003)
    da = np.array([[1.0, 2.0, 3.0, 4.0, 6.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 2.5, 9.0, 9.0]]).T   # (time, model)
    # baseline 1996-2000: the means are 3.2 and 0.5, the year 2000 is 6 and 2.5, so x = 2.8 and 2; obs = 2: 1 / (2 + 0.8), 1 / (2 + 0)
    w = partitioning.hawkins_sutton_09_weighting(da, 2.0, ("1996", "2000"), time=annual(years))
    np.testing.assert_allclose(w, [1 / 2.8, 0.5], rtol=1e-15)


def test_the_basis_is_orthonormal_for_every_calendar():
    for cal in ("standard", "noleap", "360_day"):
        for deg in range(5):
            q = partitioning.poly_basis(annual(P.Y151, cal) if cal != "360_day" else TimeAxis(P.Y151, np.full(151, 12), np.full(151, 30), cal), deg)
            assert q.shape == (151, deg + 1) and np.abs(q.T @ q - np.eye(deg + 1)).max() < 1e-14


def test_ensemble_stats_restatement_by_hand():
    ens = np.array([[1.0, np.nan], [3.0, np.nan], [np.nan, 5.0]])
    s = P.ensemble_stats(ens)
    assert np.array_equal(s["mean"], [2.0, 5.0]) and np.array_equal(s["stdev"], [1.0, 0.0])
    assert np.array_equal(s["max"], [3.0, 5.0]) and np.array_equal(s["min"], [1.0, 5.0])
    assert np.isnan(P.ensemble_stats(ens, None)["mean"]).all()
    assert np.array_equal(np.isnan(P.ensemble_stats(ens, 2)["max"]), [False, True])
    s = P.ensemble_stats(ens, 1, [3.0, 1.0, 1.0])
    assert np.array_equal(s["mean"], [1.5, 5.0]) and np.array_equal(s["stdev"], [np.sqrt(0.75), 0.0])
