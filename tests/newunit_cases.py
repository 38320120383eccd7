"""Edge-shape checks of the entry points of fire.hip, ffdi.hip, pet.hip, stdidx.hip, f64red.hip and f64run.hip, written once
and run on two devices: the MI355X (tests/test_gpu_edges_new_units.py) and the stand-alone sanitizer driver of the host
simulation (tests/test_hostsim_sanitize_cpu.py, where every call of these entry points runs in a fresh sanitized process on
heap blocks of exactly the fields' sizes).  Every check compares with the restatement the GPU test of that entry point uses
(ffdicpu, petcpu, spicpu / spei64cpu, firecpu, oracle) at that test's tolerance, and float outputs must have the
restatement's NaN pattern exactly (np.isnan equality, never equal_nan alone).

Fields: 2 % NaN, and — where the grid has at least two cells — cell 0 all-NaN next to valid ones.  The float64 functions need
XCLIM_AMD_FLOAT64=native in the environment (the callers set it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffdicpu  # noqa: E402
import firecpu  # noqa: E402
import petcpu  # noqa: E402
import spicpu  # noqa: E402
from oracle import calendar as ocal  # noqa: E402
from oracle import generic as ogen  # noqa: E402
from oracle import indices as oidx  # noqa: E402
from oracle.timeutil import OTime  # noqa: E402
from test_ffdi_cpu import check as ffdi_check  # noqa: E402
from test_fire_cpu import check_outputs as fire_check  # noqa: E402
from xclim_amd import calendar as hcal  # noqa: E402
from xclim_amd import converters as xc  # noqa: E402
from xclim_amd import ffdi, fire  # noqa: E402
from xclim_amd import generic as hgen  # noqa: E402
from xclim_amd import indices as xi  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import stats as xs  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

def ncells(shape):
    return int(np.prod(shape, dtype=np.int64))


def spoil(rng, a, nan_frac=0.02, nan_cell=True):
    """2 % NaN; cell 0 all-NaN when there is a valid cell next to it."""
    a[rng.random(a.shape) < nan_frac] = np.nan
    flat = a.reshape(a.shape[0], -1)
    if nan_cell and flat.shape[1] >= 2:
        flat[:, 0] = np.nan
    return a


def same_nan(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"NaN pattern {what}")


# ---- xh_mcarthur -----------------------------------------------------------------------------------------------------
def mcarthur_fields(rng, T, shape, dtype, all_nan=False):
    pr = np.where(rng.random((T,) + shape) < 0.3, rng.gamma(0.8, 8.0, (T,) + shape), 0.0)
    tas = rng.normal(27, 6, (T,) + shape)
    hurs = rng.uniform(8, 95, (T,) + shape)
    wind = np.abs(rng.normal(15, 8, (T,) + shape))
    out = [spoil(rng, a).astype(dtype) for a in (pr, tas, hurs, wind)]
    if all_nan:
        for a in out:
            a[...] = np.nan
    return out, rng.uniform(300, 1500, shape), rng.uniform(0, 200, shape)


def check_mcarthur(dev, T, shape, dtype, lim="xlim", all_nan=False):
    """KBDI, DF and FFDI of the one-launch chain against ffdicpu.chain with `check` of tests/test_ffdi_cpu.py; the drought factor
    is NaN on the first 19 days (its 20-day window) and defined from day 20 on."""
    rng = np.random.default_rng(1000 * T + ncells(shape) + (dtype == np.float64))
    (pr, tas, hurs, wind), pa, k0 = mcarthur_fields(rng, T, shape, dtype, all_nan)
    if T >= ffdi.DF_WINDOW:
        got = ffdi.mcarthur_indices(pr, tas, hurs, wind, pa, k0, lim, device=dev)
    else:   # the public function raises like the reference's isel(time=19); the launch itself serves any T: DF all NaN
        import pytest

        with pytest.raises(IndexError, match="out of bounds"):
            ffdi.mcarthur_indices(pr, tas, hurs, wind, pa, k0, lim, device=dev)
        out = ffdi._run({"pr": pr, "tasmax": tas, "hurs": hurs, "sfcWind": wind}, ["KBDI", "DF", "FFDI"], pa, k0,
                        lim=K.MCARTHUR_LIMITS[lim], device=dev)
        got = ffdi.McArthurIndices(out["KBDI"], out["DF"], out["FFDI"])
    C = ncells(shape)
    for g in (got.KBDI, got.DF, got.FFDI):
        assert g.shape == (T,) + shape and g.dtype == np.float64
    if C == 0 or T == 0:
        return
    flat = lambda a: a.reshape(T, C)  # noqa: E731
    k, d, f = ffdicpu.chain(flat(pr), flat(tas), flat(hurs), flat(wind), pa.reshape(C), k0.reshape(C), K.MCARTHUR_LIMITS[lim])
    ffdi_check("kbdi", flat(got.KBDI), k)
    ffdi_check("df", flat(got.DF), d)
    ffdi_check("ffdi", flat(got.FFDI), f, dtype == np.float64)
    assert np.isnan(flat(got.DF)[:19]).all()
    if T >= 20 and not all_nan:
        ok = ~np.isnan(flat(pr)[:20]).any(axis=0) & ~np.isnan(k[19])
        assert np.isfinite(flat(got.DF)[19][ok]).all()


# ---- xh_solar_table, xh_pet_month_table, xh_pet_daily, xh_pet_monthly ------------------------------------------------------
PET_METHODS = ("BR65", "HG85", "MB05", "FAO_PM98", "TW48", "DA02")


def pet_fields(rng, T, shape, dtype, start, all_nan=False):
    full = (T,) + shape
    t = TimeAxis.daily(start, T, "standard")
    lat = np.linspace(-80, 80, max(ncells(shape), 1))[:ncells(shape)].reshape(shape)
    base = 288 - 0.3 * np.abs(lat) + rng.normal(0, 3, full)
    spread = rng.uniform(2, 14, full)
    f = {"tasmin": base - spread / 2, "tasmax": base + spread / 2, "tas": base + rng.normal(0, 0.5, full),
         "hurs": rng.uniform(5, 100, full), "rsds": rng.uniform(0, 350, full), "rlds": rng.uniform(230, 380, full),
         "sfcWind": rng.uniform(0, 12, full), "pr": np.where(rng.random(full) < 0.4, rng.gamma(0.7, 8, full), 0) / 86400}
    f["rsus"] = 0.2 * f["rsds"]
    f["rlus"] = f["rlds"] + rng.uniform(10, 80, full)
    for k in f:
        spoil(rng, f[k])
        if all_nan:
            f[k][...] = np.nan
    return t, lat, {k: v.astype(dtype) for k, v in f.items()}


def check_pet(dev, method, dtype, shape, T=75, start="2001-03-14", all_nan=False):
    """PET and the water budget against petcpu (the tolerances of tests/test_gpu_pet.py's restatement test): 75 days from
    mid-March reach three calendar months, the first and the last one cut."""
    rng = np.random.default_rng(7 * PET_METHODS.index(method) + ncells(shape) + T + (dtype == np.float64))
    t, lat, f = pet_fields(rng, T, shape, dtype, start, all_nan)
    C = ncells(shape)
    use_tas = method in ("HG85", "MB05", "TW48")
    monthly = method in ("TW48", "DA02")
    fld = {k: v for k, v in f.items() if (k != "tas" or use_tas) and k != "pr"}
    if method == "DA02":
        fld["pr"] = f["pr"]
    got = xc.potential_evapotranspiration(**fld, lat=lat, time=t, method=method, time_of_day=12.0, device=dev)
    # (water_budget with DA02 is not served: the reference does not hand pr to its PET call)
    wb = None if method == "DA02" else xc.water_budget(f["pr"], **fld, lat=lat, time=t, method=method, time_of_day=12.0, device=dev)
    if monthly:
        got, months = got
        wb = None if wb is None else wb[0]
        seg, _ = t.segments("MS")
        assert len(months) == len(seg) - 1
        rows = len(months)
    else:
        rows = T
    for g in (got, wb):
        assert g is None or (g.shape == (rows,) + shape and g.dtype == np.float64)
    if C == 0:
        return
    flat = {k: v.reshape(T, C) for k, v in f.items()}
    if monthly:
        exp, exp_wb, em = petcpu.pet_monthly(method, t, lat.reshape(C), **{k: flat.get(k) if (k != "tas" or use_tas) else None
                                                                         for k in ("tasmin", "tasmax", "tas", "pr")})
        np.testing.assert_array_equal(months.month, em.month)
    else:
        exp, exp_wb = petcpu.pet_daily(method, t, lat.reshape(C), **{k: v for k, v in flat.items() if k != "tas" or use_tas},
                                       time_of_day=12.0)
    rtol = 1e-10 if method == "TW48" else 1e-12
    for g, e, what in ((got, exp, "pet"), (wb, exp_wb, "wb")):
        if g is None:
            continue
        g = g.reshape(e.shape)
        same_nan(g, e, f"{method} {what}")
        if np.isfinite(e).any():
            # (the water budget pr - PET cancels: its error is the PET's, measured on the PET's scale)
            np.testing.assert_allclose(g, e, rtol=rtol, atol=max(1e-12, rtol) * np.nanmax(np.abs(exp)), equal_nan=True, err_msg=what)


# ---- xh_si_fit / xh_si_apply and their float64 twins ---------------------------------------------------------------------
def assert_si_close(got, exp, atol=1e-6):
    """tests/test_gpu_stdidx.py's assert_si_close itself (imported on use: that module loads its golden vectors on import)."""
    import test_gpu_stdidx

    test_gpu_stdidx.assert_si_close(got, exp, atol=atol)


def si_field(rng, T, C, dtype, all_nan=False):
    """Monthly precipitation-like values with zeros; cell 0 all-NaN; cell 1: group 3 keeps ONE valid value (no fit: NaN
    parameters); cell 2: group 5 all zeros (under zero_inflated no value is left to fit)."""
    x = np.where(rng.random((T, C)) < 0.15, 0.0, rng.gamma(2.0, 1.5, (T, C)))
    spoil(rng, x)
    if C >= 2:
        x[3::12, 1] = np.nan
        if T > 3:
            x[3, 1] = 1.25
    if C >= 3:
        x[5::12, 2] = 0.0
    if all_nan:
        x[...] = np.nan
    return x.astype(dtype)


def check_si_public(dev, dtype, shape, months=36, all_nan=False):
    """stats.standardized_index (gamma, ML with floc = 0, zero-inflated) on `months` monthly steps against spicpu: the parameters
    to 1e-9 (a closed-form fit: the FAST class of assert_params_close), the index with assert_si_close."""
    rng = np.random.default_rng(31 * months + ncells(shape) + (dtype == np.float64))
    C = ncells(shape)
    x = si_field(rng, months, C, dtype, all_nan).reshape((months,) + shape)
    k = np.arange(months)
    t = TimeAxis(2000 + k // 12, 1 + k % 12, np.ones(months, np.int64), "noleap")
    kw = dict(dist="gamma", method="ML", zero_inflated=True, fitkwargs={"floc": 0.0})
    si = xs.standardized_index(x, t, "MS", 1, device=dev, **kw)
    assert si.shape == (months,) + shape and si.dtype == np.float64
    if C == 0:
        return
    p = xs.standardized_index_fit_params(x, t, "MS", 1, "gamma", "ML", zero_inflated=True, fitkwargs={"floc": 0.0}, device=dev)
    gidx = (t.month - 1).astype(int)
    xp = x.reshape(months, C)
    ep, nz, nn, _ = spicpu.fit(xp, gidx, 12, "gamma", "ML", True, 0.0)
    # (groups beyond the series' last month have no rows: absent, NaN after the reference's reindexing)
    vals = np.asarray(p.values).reshape(-1, 3, C)
    same_nan(vals, ep[:vals.shape[0]], "parameters")
    np.testing.assert_allclose(vals, ep[:vals.shape[0]], rtol=1e-9, atol=0, equal_nan=True)
    exp = spicpu.index(xp, gidx, ep, "gamma", nz, nn)
    assert_si_close(si.reshape(months, C), exp)
    if C >= 3 and months >= 36 and not all_nan:
        assert np.isnan(vals[3, :, 1]).all() and np.isnan(vals[5, :, 2]).all() and np.isfinite(vals[4, :, 2]).all()


def check_si_kernels(dev, dtype, C, T, G, dist, method, floc, zero_inflated, staging, all_nan=False):
    """K.si_fit + K.si_apply against spicpu.fit / index.  Closed-form fits (APP; gamma ML with floc) to 1e-9; Nelder-Mead
    fits as assert_params_close of tests/test_gpu_stdidx.py: the converged ones (nfev < 600) to 1e-3; the index from the
    restatement's parameters with assert_si_close."""
    rng = np.random.default_rng(T * 131 + C * 7 + G + (dtype == np.float64) + 2 * (dist == "fisk"))
    x = si_field(rng, T, C, dtype, all_nan)
    if dist == "fisk":   # continuous values (repeated zeros would make samples of identical values: no spread to start a fit from)
        x = np.where(np.isnan(x), np.nan, rng.gamma(2.0, 1.5, x.shape) + 0.5).astype(dtype)
    group = (np.arange(T) % G).astype(np.int32)
    group[T - 1] = -1   # a row outside every group: NaN out
    d = dev.to_device(x)
    params, nz, nn, nfev = K.si_fit(dev, d, group, G, dist, method, floc=floc, zero_inflated=zero_inflated, staging=staging,
                                    want_nfev=True)
    ep, enz, enn, _ = spicpu.fit(x, np.where(group < 0, -1, group), G, dist, method, zero_inflated, floc)
    got, nf = params.get(), nfev.get()
    same_nan(got, ep, "parameters")
    if method == "APP" or (dist == "gamma" and floc is not None):
        np.testing.assert_allclose(got, ep, rtol=1e-9, atol=0, equal_nan=True)
    else:
        # as tests/test_gpu_stdidx.py::test_random_grid_against_scipy: a walk stopped at the budget, or fisk run off towards its
        # c -> inf limit (a flat likelihood: the parameters are arbitrary there), is compared through the distribution on its
        # own sample (norm.ppf of the cdf, 2e-2); every other fit to 1e-3
        import scipy.stats

        assert nf.max() <= 600
        for g in range(G):
            for c in range(C):
                if np.isnan(ep[g, :, c]).all():
                    continue
                if nf[g, c] >= 600 or ep[g, 0, c] > 1e3 or got[g, 0, c] > 1e3:
                    v = x[group == g, c].astype(np.float64)
                    v = v[~np.isnan(v)]
                    q = lambda p: scipy.stats.norm.ppf(getattr(scipy.stats, dist).cdf(v, *p))  # noqa: E731
                    np.testing.assert_allclose(q(got[g, :, c]), q(ep[g, :, c]), rtol=0, atol=2e-2, err_msg=f"group {g} cell {c}")
                else:
                    np.testing.assert_allclose(got[g, :, c], ep[g, :, c], rtol=1e-3, atol=0, err_msg=f"group {g} cell {c}")
    if zero_inflated:
        np.testing.assert_array_equal(nz.get(), enz)
        np.testing.assert_array_equal(nn.get(), enn)
    si = K.si_apply(dev, d, group, dev.to_device(ep), dist, dev.to_device(enz) if zero_inflated else None,
                    dev.to_device(enn) if zero_inflated else None).get()
    exp = spicpu.index(x, group, ep, dist, enz if zero_inflated else None, enn if zero_inflated else None)
    exp[group < 0] = np.nan
    assert_si_close(si, exp)
    if all_nan:
        assert np.isnan(got).all() and np.isnan(si).all()


# ---- xh_fire_weather, xh_overwintering_dc -----------------------------------------------------------------------------------
FIRE_MODES = {"none": {}, "wf93_ow": dict(season_method="WF93", overwintering=True, dry_start="CFS"),
              "la08_ow": dict(season_method="LA08", overwintering=True), "gfwed_ow": dict(season_method="GFWED", overwintering=True,
                                                                                         temp_condition_days=2, snow_condition_days=4),
              "mask_ow": dict(overwintering=True)}


def check_fire(dev, T, C, mode, all_nan=False):
    """fire_weather_ufunc in every season mode (none, WF93, LA08, GFWED, a given mask), with overwintering, against firecpu with
    check_outputs of tests/test_fire_cpu.py; then xh_overwintering_dc on the last DC and the winter precipitation."""
    import test_gpu_fire as tf

    rng = np.random.default_rng(T * 1000 + C + len(mode))
    inp = tf._weather(rng, T, C, nan_frac=0.02)
    if C >= 2:
        for a in inp[:4]:
            a[:, 0] = np.nan
    if all_nan:
        for a in inp:
            a[...] = np.nan
    time = TimeAxis.daily("2001-03-01", T, "noleap")
    lat = rng.uniform(-90, 90, C)
    kw = dict(FIRE_MODES[mode])
    ckw = dict(kw)
    if mode == "mask_ow":
        kw["season_mask"] = rng.random((T, C)) < 0.7
        ckw = dict(kw, season_method="mask")
    snd = inp[4] if mode in ("la08_ow", "gfwed_ow") else None
    wpr = rng.uniform(0, 200, C).astype(np.float32) if kw.get("overwintering") else None
    exp = firecpu.fire_weather(*inp, time.month, lat, winter_pr=wpr, **ckw)
    got = fire.fire_weather_ufunc(tas=inp[0], pr=inp[1], hurs=inp[2], sfcWind=inp[3], snd=snd, lat=lat, time=time, winter_pr=wpr,
                                  device=dev, **kw)
    fire_check(got, exp)
    for k, e in exp.items():
        if k != "season_mask":
            same_nan(got[k], e, k)
    if "winter_pr" in exp:
        last = np.ascontiguousarray(exp["DC"][-1], dtype=np.float32)
        w = np.ascontiguousarray(exp["winter_pr"], dtype=np.float32)
        ow = K.overwintering_dc(dev, dev.to_device(last), dev.to_device(w), 0.75, 0.75, 15.0).get()
        e = firecpu.overwintering_dc(last, w, 0.75, 0.75, 15.0).astype(np.float32)   # (as tests/test_gpu_fire.py compares it)
        same_nan(ow, e, "overwintering")
        np.testing.assert_allclose(ow, e, rtol=1e-6, equal_nan=True)
        if all_nan:
            assert np.isnan(ow).all()


# ---- f64red.hip / f64run.hip (XCLIM_AMD_FLOAT64=native) -----------------------------------------------------------------
def near(rng, T, shape, thr, spread, p_close=0.5, nan_frac=0.02):
    """tests/test_gpu_f64_native.py's field: about half the days within a float32 ulp of `thr`; NaN days; cell 0 all-NaN."""
    u32 = float(np.spacing(np.float32(thr)))
    close = np.array([np.nextafter(thr, -np.inf), thr, np.nextafter(thr, np.inf), thr + 0.25 * u32, thr - 0.25 * u32,
                      thr + 0.45 * u32, thr - 0.45 * u32])
    x = thr + rng.normal(0, spread, (T,) + shape)
    pick = rng.random(x.shape) < p_close
    x[pick] = rng.choice(close, int(pick.sum()))
    return spoil(rng, x, nan_frac)


def axes(T, calendar="noleap", start=2001):
    if calendar == "noleap":
        return TimeAxis.daily(f"{start}-01-01", T, "noleap"), OTime.noleap(start, T)
    return TimeAxis.daily(f"{start}-01-01", T, "standard"), OTime.standard(f"{start}-01-01", T)


def bits(got, exp, what="", summed=0):
    """Bit for bit.  `summed` = the most terms a value adds, for sums and means on a grid of ONE cell: the kernels add a period in
    row order, which is numpy's order for the axis-0 sum of a (rows, C) group only when C > 1 — a single column is contiguous
    along the axis and numpy adds it pairwise.  Two orders of adding n same-sign terms differ by at most (n - 1) roundings of
    the running sum: rtol = n * 2^-52 there, nothing anywhere else."""
    got = np.asarray(got)
    assert got.dtype == np.float64, what
    same_nan(got, exp, what)
    if summed and got.size == got.shape[0]:
        np.testing.assert_allclose(got, exp, rtol=summed * 2.0 ** -52, atol=0, equal_nan=True, err_msg=what)
    else:
        np.testing.assert_array_equal(got, exp, err_msg=what)


def check_f64_reductions(dev, shape, T, freq="MS", all_nan=False, mixed=True):
    """xh_thresholded_reduce_f64, xh_domain_count_f64, xh_bivariate_count_f64, xh_range_reduce_f64 through the public functions,
    bit for bit against the oracle on the float64 arrays (counts and row-order sums)."""
    rng = np.random.default_rng(17 * T + ncells(shape))
    ta, ot = axes(T)
    thr = 283.15
    n = 31 if freq == "MS" else 366   # (the most days a period adds: bits)
    x = near(rng, T, shape, thr, 3.0)
    hi = x + 8.0 + rng.normal(0, 2.0, x.shape)
    if all_nan:
        x[...] = np.nan
    P = len(ta.segments(freq)[0]) - 1
    got = hgen.cumulative_difference(x, thr, ">", ta, freq, device=dev)
    assert got.shape == (P,) + shape
    if ncells(shape) == 0:
        for g in (hgen.domain_count(x, 280.0, 286.0, ta, freq, device=dev), hgen.diurnal_temperature_range(x, hi, "mean", ta, freq, device=dev)):
            assert g.shape == (P,) + shape
        return
    bits(got, ogen.cumulative_difference(x, thr, ">", ot, freq), "degree days", summed=n)
    for red in ("sum", "mean", "min", "max"):
        bits(hgen.thresholded_statistics(x, "<=", thr, red, ta, freq, device=dev), ogen.thresholded_statistics(x, "<=", thr, red, ot, freq), red, summed=n if red in ("sum", "mean") else 0)
    _, val = hgen.cumulative_difference(x, thr, ">", ta, freq, device=dev, with_valid=True)
    np.testing.assert_array_equal(val, ogen.select_resample_op(x, "count", ot, freq))
    np.testing.assert_array_equal(hgen.domain_count(x, 280.0, thr, ta, freq, device=dev), ogen.domain_count(x, 280.0, thr, ot, freq))
    for a, b in ((x, hi), (x.astype(np.float32), hi), (x, hi.astype(np.float32)))[:3 if mixed else 1]:
        got = hgen.bivariate_count_occurrences(data_var1=a, data_var2=b, threshold_var1=thr, threshold_var2=thr + 8, time=ta, freq=freq,
                                               op_var1=">", op_var2="<=", var_reducer="all", device=dev)
        np.testing.assert_array_equal(got, ogen.bivariate_count_occurrences(a, b, thr, thr + 8, ot, freq, ">", "<=", "all"))
        for red in ("max", "mean"):
            bits(hgen.diurnal_temperature_range(a, b, red, ta, freq, device=dev), ogen.diurnal_temperature_range(a, b, red, ot, freq), red, summed=n if red == "mean" else 0)
        bits(hgen.interday_diurnal_temperature_range(a, b, ta, freq, device=dev), ogen.interday_diurnal_temperature_range(a, b, ot, freq), "interday", summed=n)
        bits(hgen.extreme_temperature_range(a, b, ta, freq, device=dev), ogen.extreme_temperature_range(a, b, ot, freq), "extreme")


def check_f64_rolling(dev, C, T, windows=(1, 8, 9, 31), reducers=("sum", "mean", "min", "max", "std", "var"), all_nan=False):
    """xh_rolling_reduce_f64: sums, means, extremes bit for bit (the window added first row to last), std / var to 1e-13."""
    rng = np.random.default_rng(5 * T + C)
    x = near(rng, T, (C,), 285.0, 1.0, nan_frac=0.02)
    if all_nan:
        x[...] = np.nan
    d = dev.to_device(x, dtype=np.float64)
    for window in windows:
        for center in (True, False):
            for red in reducers:
                got = K.rolling_reduce(dev, d, window, red, center).get()
                exp = ogen.rolling(x, window, red, center)
                assert got.dtype == np.float64
                same_nan(got, exp, f"rolling {red} {window}")
                if red in ("std", "var"):
                    np.testing.assert_allclose(got, exp, rtol=1e-13, atol=0, equal_nan=True)
                elif C == 1 and red in ("sum", "mean"):   # (one column: numpy adds the window pairwise, see bits)
                    np.testing.assert_allclose(got, exp, rtol=window * 2.0 ** -52, atol=0, equal_nan=True)
                else:
                    np.testing.assert_array_equal(got, exp)


def check_f64_runs(dev, shape, T, freq="MS", all_nan=False):
    """xh_compare_map_f64, xh_spell_mask_f64, xh_spell_run_stats_f64, xh_run_stats_f64 (both resample orders): bitwise the oracle's
    masks, counts and run lengths."""
    rng = np.random.default_rng(23 * T + ncells(shape))
    ta, ot = axes(T)
    x = near(rng, T, shape, 285.0, 1.0, p_close=0.7)
    if all_nan:
        x[...] = np.nan
    got = hgen.compare(x, ">", 285.0, device=dev)
    assert got.shape == x.shape
    if ncells(shape) == 0:
        assert hgen.spell_mask(x, 3, "mean", ">", 285.0, device=dev).shape == x.shape
        P = len(ta.segments(freq)[0]) - 1
        assert hgen.spell_length_statistics(x, 285.0, 1, "sum", ">", "max", ta, freq, device=dev).shape == (P,) + shape
        return
    np.testing.assert_array_equal(got, ogen.compare(x, ">", 285.0))
    th = near(rng, T, shape, 285.0, 1.0, nan_frac=0.0)
    np.testing.assert_array_equal(hgen.compare(x.astype(np.float32), "<=", th, device=dev), ogen.compare(x.astype(np.float32), "<=", th))
    np.testing.assert_array_equal(hgen.get_daily_events(x, 285.0, ">", device=dev), ogen.get_daily_events(x, 285.0, ">"))
    for window, red, thr in ((3, "mean", 285.0), (12, "sum", 285.0 * 12), (12, "max", 285.0)):   # ring form, memory form
        np.testing.assert_array_equal(hgen.spell_mask(x, window, red, ">", thr, device=dev), ogen.spell_mask(x, window, red, ">", thr))
    for window, before in ((1, True), (1, False), (3, True), (8, True)):
        for stat in ("max", "sum"):
            got = hgen.spell_length_statistics(x, 285.0 * window, window, "sum", ">", stat, ta, freq, resample_before_rl=before, device=dev)
            exp = ogen.spell_length_statistics(x, 285.0 * window, window, "sum", ">", stat, ot, freq, resample_before_rl=before)
            np.testing.assert_array_equal(got, exp)
    for before in (True, False):
        got = xi.maximum_consecutive_tx_days(x, 285.0, ta, freq=freq, resample_before_rl=before, device=dev)
        raw = ogen.spell_length_statistics(x, 285.0, 1, None, ">", "max", ot, freq, resample_before_rl=before)
        np.testing.assert_array_equal(got, oidx.apply_missing(raw, x, ot, freq))


def check_f64_percentile_doy(dev, shape, years, window, wsdi=True, table_dev=None, all_nan=False):
    """xh_percentile_doy_f64 bit for bit against the oracle; xh_run_stats_doy_f64 through warm_spell_duration_index."""
    T = 365 * years
    rng = np.random.default_rng(years * 100 + window + ncells(shape))
    ta, ot = axes(T)
    t = np.arange(T).reshape((T,) + (1,) * len(shape))
    x = spoil(rng, 288.0 + 12 * np.sin(2 * np.pi * (t - 100) / 365) + rng.normal(0, 3, (T,) + shape))
    if all_nan:
        x[...] = np.nan
    p = hcal.percentile_doy(x, ta, window=window, per=[10.0, 90.0], alpha=1.0 / 3.0, beta=1.0 / 3.0, device=dev)
    p_o, doys = ocal.percentile_doy(x, ot, window, [10.0, 90.0], 1.0 / 3.0, 1.0 / 3.0)
    assert p.data.dtype == np.float64 and np.array_equal(p.dayofyear, doys)
    same_nan(p.values(), p_o, "percentile_doy")
    np.testing.assert_array_equal(p.values(), p_o)
    if all_nan:
        assert np.isnan(p.values()).all()
    if wsdi:
        p90 = hcal.percentile_doy(x, ta, window=window, per=90.0, device=table_dev or dev)
        p90_o, doys = ocal.percentile_doy(x, ot, window, 90.0)
        got = xi.warm_spell_duration_index(x, p90, ta, window=3, freq="YS", device=dev)
        raw = oidx.warm_spell_duration_index(x, p90_o[..., 0], doys, ot, 3, "YS")
        exp = oidx.apply_missing(raw, x, ot, "YS")
        same_nan(got, exp, "warm spells")
        np.testing.assert_array_equal(got, exp)


def check_f64_percentile_doy_days(dev, C, years, window, days=(0, 1, 58, 180, 363, 364), all_nan=False):
    """xh_percentile_doy_f64 at the kernel level on a few days of the year only (a workgroup per day: the whole year is the GPU
    test's) — the first and last days, whose windows reach past the ends of the series — bit for bit the oracle's rows."""
    T = 365 * years
    rng = np.random.default_rng(years * 100 + window + C)
    _, ot = axes(T)
    t = np.arange(T)[:, None]
    x = spoil(rng, 288.0 + 12 * np.sin(2 * np.pi * (t - 100) / 365) + rng.normal(0, 3, (T, C)))
    if all_nan:
        x[...] = np.nan
    per = [10.0, 50.0, 90.0]
    p_o, _ = ocal.percentile_doy(x, ot, window, per, 1.0 / 3.0, 1.0 / 3.0)   # (365, C, nper)
    days = np.asarray(days)
    tb = (np.arange(years)[:, None] * 365 + days[None, :]).astype(np.int32)
    got = K.percentile_doy(dev, dev.to_device(x, dtype=np.float64), tb, window, per, 1.0 / 3.0, 1.0 / 3.0).get()   # (nper, days, C)
    exp = np.moveaxis(p_o[days], -1, 0)
    same_nan(got, exp, "percentile_doy")
    np.testing.assert_array_equal(got, exp)


# ---- the checks every pitched (ctx, T, C, ld, ..., ld_out) entry point shares (hostargs.h) --------------------------------------
def shared_refusals(call, T, C, tables=(), expect=None):
    """One fault at a time, each answered with its code.  `call(**kw)` is the entry point on a valid call of T rows and C cells
    with the given keywords changed: ctx (None = NULL), T, C, ld, ld_out, and for every host offset table of `tables` =
    [(key, offsets, rows, too_many)] the table under `key` (None = NULL); `too_many` holds the keywords of the call with 65536
    periods, or None where the table has no such limit.  `expect` = {fault: code} where an entry point answers otherwise.
    The callers check afterwards that their outputs still hold the fill value."""
    from xclim_amd._capi import XH_ERR_ARG as ARG, XH_ERR_LAYOUT as LAYOUT, XH_ERR_LIMIT as LIMIT

    cases = [("NULL context", dict(ctx=None), ARG), ("T = -1", dict(T=-1), ARG), ("C = -1", dict(C=-1), ARG),
             ("ld = C - 1", dict(ld=C - 1), LAYOUT), ("ld_out = C - 1", dict(ld_out=C - 1), LAYOUT),
             ("T * ld + C >= 2^40", dict(ld=(1 << 40) // T + 1), LIMIT)]   # (needs no memory: the call refuses first)
    for key, good, rows, too_many in tables:
        assert good[0] == 0 and good[-1] <= rows and good[0] < good[-1]
        low, high, back = good.copy(), good.copy(), good[::-1].copy()     # (back: inside [0, rows], and it goes down)
        low[0], high[-1] = -1, rows + 1
        cases += [(f"{key} NULL", {key: None}, ARG), (f"{key}[0] < 0", {key: low}, ARG), (f"{key}[-1] > rows", {key: high}, ARG),
                  (f"{key} decreasing", {key: back}, ARG)]
        if too_many is not None:
            cases.append((f"{key}: 65536 periods", too_many, LIMIT))
    for what, kw, code in cases:
        got = call(**kw)
        assert got == (expect or {}).get(what, code), (what, got)
