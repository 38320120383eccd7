"""One bad sample stays inside its window, period or cell (tests/footprint.py says what is asserted).

An unmasked ``_FillValue`` (-9999, 1e20, the netCDF default 9.96921e36) or a NaN is put into ONE sample of an otherwise ordinary
field, and the outputs that move are compared with the outputs a float64 reference moves.  The positions come from each
kernel's decomposition: the wave seam and the ragged tail (70 cells: 0, 63, 64, 69; 72 cells: inside a lane's quad of the
four-cells-per-lane paths), the first and last row of the series, the last row of one chunk of the kernel and the first of
the next, and for k_doy_stats_sets the first day-set a chunk gathers.

Every case names the parity test its tolerance is taken from (``tol_from``) and the simulation library that holds its entry
point (``lib``): tests/test_hostsim_cpu.py and tests/test_hostsim_units_cpu.py re-run this module without a GPU, selected by
library through the test id ``<lib>-<case>-<field>-<dtype>``.

What this module found when it was written (the kernels of that day on the host simulation): k_doy_stats_sets kept running
window sums of samples shifted by a pivot sample, k_window_nanmean a running sum over a stretch of 128 rows, and both carried
the rounding loss of one huge sample to outputs whose window never held it, e.g.
  doy_mean_std_5y[flux] -9999 at row 0, cell 0: 21 days of year outside the footprint, std 0.0 for 1.0173251e-05
  doy_mean_std_2y[kelvin] 1e20 at row 0, cell 0: 21 days outside the footprint, mean 278.92706 for 281.6305
  window_nanmean_w5[kelvin] 1e20 at row 0, cell 0: 125 rows outside the footprint, 0.0 for 283.83063
(every doy_mean_std case of 2, 5 and 40 years and every window_nanmean case failed; the one-year and the window-9 cases and all
other entry points passed).  doystats.hip and detrend.hip say how each kernel contains the sample now."""
import warnings

import numpy as np
import pytest

import footprint as fp
from footprint import Case
from oracle import calendar as ocal
from oracle import generic as ogen
from oracle import quantile as oq
from oracle import sdba as osdba
from oracle.timeutil import OTime
from poisoned import poisoned_outputs  # noqa: F401  (autouse: every output buffer of this module starts as poison)
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
R6 = dict(rtol=1e-6, atol=0)
CASES = []


THRESHOLD = {"kelvin": 283.0, "flux": 1e-5}   # about the median of either field


def _x(T, on_threshold=()):
    """One field ``x`` of T rows (and the threshold that goes with its kind, for the cases that count).  ``on_threshold``: rows
    whose samples ARE the threshold, neither above nor below it, so that every bad sample put there changes a count."""
    def make(rng, kind, dtype, C):
        x = fp.FIELDS[kind](rng, T, C, dtype)
        x[list(on_threshold)] = THRESHOLD[kind]
        return {"x": x, "thr": float(x.dtype.type(THRESHOLD[kind]))}

    return make


def add(name, lib, make, device, ref, rows, tol, tol_from, *, quad=False, **kw):
    """The case on 70 cells; ``quad``: also on 72 cells (rows of 4-aligned length: the four-cells-per-lane paths), with the
    perturbed cell inside a lane's quad."""
    target = kw.pop("target", "x")
    CASES.append(Case(name, lib, lambda rng, kind, dtype: make(rng, kind, dtype, 70), device, ref, target, tuple(rows), tuple(tol),
                      tol_from, **kw))
    if quad:
        CASES.append(Case(name + "_c72", lib, lambda rng, kind, dtype: make(rng, kind, dtype, 72), device, ref, target, tuple(rows),
                          tuple(tol), tol_from, **{**kw, "cells": (1, 34, 67, 70), "C": 72}))


# ---------------------------------------------------------------------------------------------------------------- windows
# xh_rolling_reduce / xh_rolling_reduce_f64.  window <= 8: k_rolling_ring (window.hip; 3 is a compile-time window on 72 cells),
# above: k_rolling_reduce (reduce.hip).  Both cut the 160 rows into chunks of 32 (window_grid: at least 32 rows per chunk).
ROLL_REDUCERS = ("sum", "mean", "std", "var", "min", "max")
# float32: tests/test_gpu_kernels.py::test_rolling_reduce (rtol 1e-6; std atol 2e-6; var is not in that test: std's bound on
# s^2, d(s^2) = 2 s ds, relative 2e-6).  float64: tests/test_gpu_f64_native_reductions.py::test_rolling_statistics_in_float64
# (sum, mean, min, max bit for bit; std and var rtol 1e-13).
ROLL_TOL = {F32: (R6, R6, dict(rtol=1e-6, atol=2e-6), dict(rtol=2e-6, atol=2e-6), R6, R6),
            F64: (None, None, dict(rtol=1e-13, atol=0), dict(rtol=1e-13, atol=0), None, None)}


def _rolling(window):
    def device(dev, f):
        d = dev.to_device(f["x"], dtype=f["x"].dtype)
        return [K.rolling_reduce(dev, d, window, r, True).get() for r in ROLL_REDUCERS]

    def ref(f):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return [ogen.rolling(f["x"], window, r, True) for r in ROLL_REDUCERS]

    return device, ref


for _w in (3, 8, 9, 31):
    for _dt in (F32, F64):
        add(f"rolling_w{_w}_{np.dtype(_dt).name}", "shared", _x(160), *_rolling(_w), (0, 159, 31, 32), ROLL_TOL[_dt],
            "test_gpu_kernels.py::test_rolling_reduce / test_gpu_f64_native_reductions.py::test_rolling_statistics_in_float64",
            quad=_w in (3, 8), dtypes=(_dt,))


# xh_doy_mean_std through climatological_mean_doy.  One year: k_doy_stats_year; 2 to 64 years and windows 3, 5, 7:
# k_doy_stats_sets in chunks of 24 days of year, so day-of-year index 23 ends a chunk, 24 starts the next and 22 (= 24 - window
# / 2) is the first day-set that chunk gathers; window 9: the generic two-pass k_doy_mean_std (reduce2.hip); a leap day: the
# irregular days of year go to the generic kernel too.  Tolerance: tests/test_gpu_ladders.py::test_climatological_mean_doy_year_ladder.
DOY_TOL = (dict(rtol=1e-6, atol=0), dict(rtol=2e-6, atol=1e-6))


def _doy(nyears, window, calendar="noleap"):
    T = 365 * nyears + (1 if calendar == "standard" else 0)   # (standard: from 2000-01-01, a leap year)
    if calendar == "standard":
        ta, ot = TimeAxis.daily("2000-01-01", T), OTime.standard("2000-01-01", T)
    else:
        ta, ot = TimeAxis.daily("2000-01-01", T, "noleap"), OTime.noleap(2000, T, "noleap")

    def device(dev, f):
        from xclim_amd.calendar import climatological_mean_doy

        m, s, _ = climatological_mean_doy(f["x"], ta, window=window, device=dev)
        return [m, s]

    def ref(f):
        m, s, _ = ocal.climatological_mean_doy(f["x"], ot, window)
        return [m, s]

    mid = 365 * (nyears // 2)   # (a middle year: the sample is one of several of its day-set)
    rows = (0, T - 1, mid + 23, mid + 24, 22, mid + 22, 365 * (nyears - 1) + 47)
    return (_x(T), device, ref, rows if nyears <= 5 else rows[:5], DOY_TOL,
            "test_gpu_ladders.py::test_climatological_mean_doy_year_ladder")


add("doy_mean_std_1y", "shared", *_doy(1, 5), quad=True)
add("doy_mean_std_2y", "shared", *_doy(2, 5))
add("doy_mean_std_5y", "shared", *_doy(5, 5), quad=True)
add("doy_mean_std_5y_w3", "shared", *_doy(5, 3))
add("doy_mean_std_5y_w7", "shared", *_doy(5, 7))
add("doy_mean_std_40y", "shared", *_doy(40, 5))
add("doy_mean_std_5y_w9", "shared", *_doy(5, 9))
add("doy_mean_std_5y_leap", "shared", *_doy(5, 5, "standard"))


# xh_window_nanmean: a thread = one column and a stretch of 128 output rows (k_window_nanmean, detrend.hip).  600 rows, so that
# the widest window (129 rows, wider than a stretch) stays below a quarter of the series.
# Tolerance: tests/test_gpu_api.py::test_dqm_windowed_sub_grouping_matches_oracle (rtol 3e-7, atol 1e-7).
WM_WAIVER = ("k_window_nanmean (detrend.hip) keeps a running sum and sums the window again from its rows when the sample that leaves "
             "is more than WM_RESUM times what remains: after the bad sample has left, the sum has another rounding history than "
             "in the clean run (last bits of a float64 sum, within A1's tolerance)")


def _wmean(window):
    def device(dev, f):
        return [K.window_nanmean(dev, dev.to_device(f["x"]), window).get()]

    return _x(600), device, lambda f: [osdba.window_nanmean(f["x"], window)]


for _w in (5, 31, 129):
    add(f"window_nanmean_w{_w}", "shared", *_wmean(_w), (0, 599, 127, 128, 383, 384, 200), (dict(rtol=3e-7, atol=1e-7),),
        "test_gpu_api.py::test_dqm_windowed_sub_grouping_matches_oracle", waive_a2=WM_WAIVER, quad=_w == 31)


# xh_percentile_doy, float32, three years, window 5 (the multi-year register kernels in chunks of days of year).
# Tolerance: tests/test_gpu_kernels.py::test_percentile_doy.
def _pdoy():
    nyears, window, per = 3, 5, [10.0, 50.0, 90.0]
    T = 365 * nyears
    ta, ot = TimeAxis.daily("2000-01-01", T, "noleap"), OTime.noleap(2000, T, "noleap")
    tb, years, doys = ta.doy_table()

    def device(dev, f):
        return [K.percentile_doy(dev, dev.to_device(f["x"]), tb, window, per).get()]

    def ref(f):
        x = f["x"]
        rr = ocal.rolling_construct_center(x, window)
        stack = np.full((len(doys), len(years), x.shape[1], window), np.nan, dtype=np.float32)
        stack[np.searchsorted(doys, ot.doy), np.searchsorted(years, ot.year)] = rr
        stack = np.moveaxis(stack, 1, -2).reshape(len(doys), x.shape[1], len(years) * window)
        return [np.moveaxis(oq.calc_perc(stack, per, 1 / 3, 1 / 3), -1, 0)]

    return _x(T), device, ref, (0, T - 1, 365 + 23, 365 + 24, 365 + 22)


add("percentile_doy_3y", "shared", *_pdoy(), (dict(rtol=1e-12, atol=0),), "test_gpu_kernels.py::test_percentile_doy")


# The streamflow unit (hydro.hip; its own simulation library).  Its restatement (tests/hydrocpu.py) returns, with every output,
# the sum of magnitudes behind it; the bound is tests/test_hydro_cpu.py::check_run's: 1e-12 of that scale, integers exactly.
def _scaled(k):
    return dict(scale=k, rtol=1e-12)


def _api(window, p_exp):
    import hydrocpu as H

    w = H.api_weights(window, p_exp)

    def device(dev, f):
        return [K.antecedent_precip(dev, dev.to_device(f["x"], dtype=f["x"].dtype), w, per_day=H.DAY).get()]

    def ref(f):
        r = H.antecedent_precip(f["x"], H.DAY, w)
        return [r["out"], r["out_scale"]]

    return _x(300), device, ref, (0, 299, 127, 128, 255, 256), (_scaled(1),)


for _w, _p in ((7, 0.935), (31, 0.9)):
    add(f"antecedent_precip_w{_w}", "hydro", *_api(_w, _p), "test_gpu_hydro.py::test_cell_counts_against_restatement", dtypes=(F32, F64))


def _flow():
    import hydrocpu as H

    def device(dev, f):
        o = K.flow_period_stats(dev, dev.to_device(f["x"], dtype=f["x"].dtype), _SEG_MS, outputs=K.FLOW_OUTPUTS)
        return [o[k].get() for k in K.FLOW_OUTPUTS]

    def ref(f):
        r = H.flow_period_stats(f["x"], _SEG_MS)
        return [r[k] for k in K.FLOW_OUTPUTS] + [r[k + "_scale"] for k in K.FLOW_OUTPUTS[:4]]

    return _x(730), device, ref, (0, 729, 30, 31, 400), (_scaled(5), _scaled(6), _scaled(7), _scaled(8), None)


def _melt(window):
    import hydrocpu as H

    rows = (0, 729, 30, 31, 400)

    def make(rng, kind, dtype, C):   # (snow amount: the field itself; the precipitation that goes with it: always the flux field)
        x = fp.FIELDS[kind](rng, 730, C, dtype)
        # the output is a period MAXIMUM, which a sample moves only where it is behind the largest window: the samples to be
        # replaced stand out, so that the melt of the next day (of the last row: its own day) is the largest of its month
        bump = x.dtype.type(1000.0)
        x[list(rows)] += bump
        x[729] -= 2 * bump
        return {"x": x, "pr": fp.flux(rng, 730, C, dtype)}

    def device(dev, f):
        return [K.melt_period_max(dev, dev.to_device(f["x"], dtype=f["x"].dtype), _SEG_MS, dev.to_device(f["pr"], dtype=f["x"].dtype),
                                  window=window, per_day=H.DAY).get()]

    def ref(f):
        r = H.melt_period_max(f["x"], f["pr"], H.DAY, window, _SEG_MS)
        return [r["out"], r["out_scale"]]

    return make, device, ref, rows, (_scaled(1),)


# xh_rolling_zones (rainseason.hip): the zone of the mean of the last 8 rows, the window read again for every row.  Fourteen edges
# around either field's values, so that every clean mean falls into a zone.  Exact, as in tests/test_gpu_rain.py (the zones are whole numbers).
def _zones():
    import raincpu as R

    edges = {"kelvin": np.linspace(270.0, 296.0, 14), "flux": np.linspace(0.0, 1.3e-4, 14)}

    def make(rng, kind, dtype, C):
        return {"x": fp.FIELDS[kind](rng, 160, C, dtype), "edges": edges[kind]}

    return (make, lambda dev, f: [K.rolling_zones(dev, dev.to_device(f["x"], dtype=f["x"].dtype), 8, f["edges"]).get()],
            lambda f: [R.rolling_zones(f["x"], 8, f["edges"])], (0, 159, 31, 32, 127, 128), (None,))


add("rolling_zones", "rain", *_zones(), "test_gpu_rain.py::test_zones_cell_counts_and_a_window_longer_than_the_series", dtypes=(F32, F64))


# xh_doy_bounds (dataflags.hip: mean -+ 3 deviations of the day-of-year climatology, the two passes of k_doy_mean_std) and the
# "outside_n_standard_deviations_of_climatology" check of xh_data_flags on these tables, one flag per sample.  Bounds:
# tests/test_gpu_flags.py::test_doy_bounds allows 4 ulp of the dtype at max(|lo|, |hi|); an ulp is at least eps / 2 of the
# value, so 2 eps of that scale is never more.  Flags: exact (tests/test_gpu_flags.py::test_climatology).
def _clim(dtype):
    import flagscpu as R

    T = 365 * 5
    ta, ot = TimeAxis.daily("2000-01-01", T, "noleap"), OTime.noleap(2000, T, "noleap")
    tb, _, doys = ta.doy_table()
    tidx = np.searchsorted(doys, ta.doy).astype(np.int32)
    rows_seg = np.arange(T + 1)

    def device(dev, f):
        dx = dev.to_device(f["x"], dtype=f["x"].dtype)
        lo, hi = K.doy_bounds(dev, dx, tb, 5, 3.0)
        flags = K.data_flags(dev, dx, [K.flag_check("clim")], rows_seg, tidx=tidx, lo=lo, hi=hi).get()[0]
        return [lo.get(), hi.get(), flags]

    def ref(f):
        lo, hi, d = R.doy_bounds(f["x"], ot, 5, 3.0)
        with np.errstate(all="ignore"):
            scale = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
        return [lo, hi, R.clim_mask(f["x"], ot, 5, 3.0, (lo, hi, d)).astype(np.uint8), np.nan_to_num(scale, posinf=0.0)]

    eps = float(np.finfo(dtype).eps)
    return _x(T), device, ref, (0, T - 1, 365 * 2 + 23, 365 * 2 + 24, 365 + 200), (dict(scale=3, rtol=2 * eps), dict(scale=3, rtol=2 * eps), None)


for _dt in (F32, F64):
    add(f"doy_bounds_and_flags_{np.dtype(_dt).name}", "flags", *_clim(_dt), "test_gpu_flags.py::test_doy_bounds / test_climatology", dtypes=(_dt,))


# ---------------------------------------------------------------------------------------------------------------- periods
# xh_resample_reduce / xh_resample_reduce_f64 on the 24 months of two years: row 30 ends January, row 31 starts February.
# float32: tests/test_gpu_kernels.py::test_resample_reduce.  float64: no parity test at this level; both sides add at most 31
# float64 terms per period (31 * 2^-53 = 3.4e-15 of the sum of magnitudes) and take the two-pass variance: rtol 1e-12.
RES_REDUCERS = ("sum", "mean", "std", "var")
RES_TOL = {F32: (dict(rtol=1e-6, atol=1e-30), dict(rtol=1e-6, atol=1e-30), dict(rtol=1e-6, atol=1e-6), dict(rtol=1e-6, atol=1e-6)),
           F64: (dict(rtol=1e-12, atol=0),) * 4}
_TA2, _OT2 = TimeAxis.daily("2001-01-01", 730, "noleap"), OTime.noleap(2001, 730, "noleap")
_SEG_MS = _TA2.segments("MS")[0]


def _resample():
    def device(dev, f):
        d = dev.to_device(f["x"], dtype=f["x"].dtype)
        return [K.resample_reduce(dev, d, r, _SEG_MS)[0].get() for r in RES_REDUCERS]

    return _x(730), device, lambda f: [ogen.select_resample_op(f["x"], r, _OT2, "MS") for r in RES_REDUCERS]


for _dt in (F32, F64):
    add(f"resample_reduce_{np.dtype(_dt).name}", "shared", *_resample(), (0, 729, 30, 31), RES_TOL[_dt],
        "test_gpu_kernels.py::test_resample_reduce", quad=True, dtypes=(_dt,))


# xh_threshold_count: the days above and the days below a threshold per month, and the valid days.  Whatever the bad sample is,
# it moves one of the three.  Exact: tests/test_gpu_kernels.py::test_threshold_count_scalar.
def _tcount():
    def device(dev, f):
        d = dev.to_device(f["x"])
        gt, val = K.threshold_count(dev, d, ">", _SEG_MS, scalar=f["thr"])
        lt, _ = K.threshold_count(dev, d, "<", _SEG_MS, scalar=f["thr"])
        return [gt.get(), lt.get(), val.get()]

    def ref(f):
        t = f["thr"]
        return [ogen.count_occurrences(f["x"], t, ">", _OT2, "MS"), ogen.count_occurrences(f["x"], t, "<", _OT2, "MS"),
                ogen.select_resample_op(f["x"], "count", _OT2, "MS")]

    return _x(730, (0, 729, 30, 31)), device, ref


add("threshold_count", "shared", *_tcount(), (0, 729, 30, 31), (None, None, None), "test_gpu_kernels.py::test_threshold_count_scalar", quad=True)


# xh_flow_period_stats (the 7-day mean behind the base-flow index reaches 3 rows into the next month) and xh_melt_period_max
# (windows 3 and 31) on the same 24 months.
add("flow_period_stats", "hydro", *_flow(), "test_gpu_hydro.py::test_cell_counts_against_restatement", dtypes=(F32, F64))
for _w in (3, 31):
    add(f"melt_period_max_w{_w}", "hydro", *_melt(_w), "test_gpu_hydro.py::test_cell_counts_against_restatement", dtypes=(F32, F64),
        may_be_empty="a period maximum (k_melt_period_max, hydro.hip): a sample that is not behind the largest window of its month changes nothing (row 0 reaches "
                     "the output through one difference only, which a NaN removes from windows that were not the largest)")


# xh_qian_wma (agro.hip): the five-day binomial mean.  tests/test_gpu_agro.py::test_cell_counts_and_lengths_against_restatement
# bounds the error by 1e-12 of the largest magnitude of the FIELD, which one fill value would make 1e8; here by 1e-12 of the
# weighted magnitudes of the five samples behind each element, which is never more.
def _qian():
    import agrocpu as A

    def ref(f):
        a = np.abs(A.widen(f["x"]))
        scale = np.full(a.shape, 0.0)
        scale[2:-2] = sum(a[k:len(a) - 4 + k] * A.QIAN_W[k] for k in range(5))
        return [A.qian_wma(f["x"]), scale]

    return _x(300), lambda dev, f: [K.qian_wma(dev, dev.to_device(f["x"], dtype=f["x"].dtype)).get()], ref, (0, 299, 2, 297, 127, 128)


add("qian_wma", "agro", *_qian(), (_scaled(1),), "test_gpu_agro.py::test_cell_counts_and_lengths_against_restatement", dtypes=(F32, F64), quad=True)


# xh_agro_degree_sum (agro.hip): the Huglin and the biologically effective degree-day sums of every month and their valid days,
# the bad sample in the daily maximum, which both sums read.  Temperatures only: on the flux field every day is far below
# the 10 degC base and no sum could move.  Bound: tests/test_agro_cpu.py::check_run (1e-12 of the restatement's scale).
def _degree_sum():
    import agrocpu as A

    names = ("hi", "bedd", "valid")

    def make(rng, kind, dtype, C):
        tas = fp.kelvin(rng, 730, C, np.float64) + 5.0      # 15 +- 4 degC
        spread = rng.uniform(3.0, 8.0, (730, C))
        return {"tas": tas.astype(dtype), "tasmin": (tas - spread).astype(dtype), "tasmax": (tas + spread).astype(dtype)}

    def device(dev, f):
        d = {k: dev.to_device(f[k], dtype=f[k].dtype) for k in ("tas", "tasmin", "tasmax")}
        o = K.agro_degree_sum(dev, d, _SEG_MS, outputs=names)
        return [o[k].get() for k in names]

    def ref(f):
        with np.errstate(all="ignore"):
            r = A.degree_sum(f["tas"], f["tasmin"], f["tasmax"], _SEG_MS)
        return [r["hi"], r["bedd"], r["valid"], np.nan_to_num(r["hi_scale"], posinf=0.0), np.nan_to_num(r["bedd_scale"], posinf=0.0)]

    return make, device, ref, (0, 729, 30, 31, 400), (_scaled(3), _scaled(4), None)


add("agro_degree_sum", "agro", *_degree_sum(), "test_gpu_agro.py::test_cell_counts_and_lengths_against_restatement", target="tasmax",
    kinds=("kelvin",), dtypes=(F32, F64), quad=True)


# ------------------------------------------------------------------------------------------------- whole series per cell
Q20 = osdba.equally_spaced_nodes(20)


# xh_quantile_series: 400 rows (the histogram kernels) and 365 rows (the register sort of one year).  The samples to be replaced
# are the threshold, a value in the middle of the distribution: a fill value that replaces one of the flux field's many
# zeros would leave every quantile of the reference where it was.
# Tolerance: tests/test_gpu_kernels.py::test_quantile_series.
add("quantile_series", "shared", _x(400, (0, 399, 200)), lambda dev, f: [K.quantile_series(dev, dev.to_device(f["x"]), Q20).get()],
    lambda f: [osdba.quantile(f["x"], Q20).astype(np.float32)], (0, 399, 200), (R6,), "test_gpu_kernels.py::test_quantile_series",
    whole_cell=True)
add("quantile_series_1y", "shared", _x(365, (0, 364, 200)), lambda dev, f: [K.quantile_series(dev, dev.to_device(f["x"]), Q20).get()],
    lambda f: [osdba.quantile(f["x"], Q20).astype(np.float32)], (0, 364, 200), (R6,), "test_gpu_kernels.py::test_quantile_series_one_year_register_sort",
    whole_cell=True)


# xh_poly_trend followed by xh_trend_apply.  Tolerances: the "detrend" case of tests/test_gpu_strided_abi.py.
def _trend():
    def device(dev, f):
        d = dev.to_device(f["x"])
        p0, p1 = K.poly_trend(dev, d, 1)
        return [p0.get(), p1.get(), K.trend_apply(dev, d, p0, p1, "-").get()]

    def ref(f):
        x = f["x"]
        T = x.shape[0]
        tc = np.arange(T) - (T - 1) / 2
        p0, p1 = np.full(x.shape[1], np.nan), np.full(x.shape[1], np.nan)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            for c in range(x.shape[1]):
                ok = ~np.isnan(x[:, c])
                p1[c], p0[c] = np.polyfit(tc[ok], x[ok, c].astype(np.float64), 1)
            return [p0, p1, (x - (p0 + p1 * tc[:, None])).astype(np.float32)]

    return _x(400), device, ref


add("poly_trend_apply", "shared", *_trend(), (0, 399, 200), (dict(rtol=1e-9, atol=1e-9), dict(rtol=1e-7, atol=1e-9), dict(rtol=1e-6, atol=1e-5)),
    "test_gpu_strided_abi.py case detrend", whole_cell=True, quad=True)


# xh_qdm_adjust (the exact-rank kernel, "linear"): the percentage rank of every sample of the cell moves with one sample.
# Tolerance: tests/test_gpu_api.py::test_qdm_adjust_matches_oracle.
def _qdm():
    def make(rng, kind, dtype, C):
        return {"x": fp.FIELDS[kind](rng, 400, C, dtype), "af": rng.normal(1.0, 0.1, (20, C)).astype(np.float32)}

    def device(dev, f):
        return [K.qdm_adjust(dev, dev.to_device(f["x"]), dev.to_device(f["af"]), Q20, "*", "linear", "constant").get()]

    return make, device, lambda f: [osdba.qdm_adjust(f["x"], f["af"], Q20, "*", "linear", "constant").astype(np.float32)]


add("qdm_adjust", "shared", *_qdm(), (0, 399, 200), (R6,), "test_gpu_api.py::test_qdm_adjust_matches_oracle", whole_cell=True)


# xh_eqm_train followed by xh_eqm_adjust ("linear"), the bad sample in the historical field: its cell's nodes and factors move,
# and with them every adjusted step of the cell.  Tolerances: tests/test_gpu_kernels.py::test_eqm_train_adjust; the adjusted
# series adds the factors, so it takes their bound.
def _eqm():
    def make(rng, kind, dtype, C):
        f = fp.FIELDS[kind]
        hist = (f(rng, 400, C, dtype) * np.float32(1.01)).astype(np.float32)
        hist[[0, 399, 200]] = THRESHOLD[kind]   # (mid-distribution samples: see quantile_series)
        return {"ref": f(rng, 400, C, dtype), "hist": hist, "sim": f(rng, 400, C, dtype)}

    def device(dev, f):
        af, hq = K.eqm_train(dev, dev.to_device(f["ref"]), dev.to_device(f["hist"]), Q20, "+")
        return [af.get(), hq.get(), K.eqm_adjust(dev, dev.to_device(f["sim"]), af, hq, "+", "linear", "constant").get()]

    def ref(f):
        af, hq = osdba.eqm_train(f["ref"], f["hist"], 20, "+")
        af, hq = af.astype(np.float32), hq.astype(np.float32)
        return [af, hq, osdba.eqm_adjust(f["sim"], af, hq, "+", "linear", "constant").astype(np.float32)]

    return make, device, ref


add("eqm_train_adjust", "shared", *_eqm(), (0, 399, 200), (dict(rtol=1e-5, atol=1e-5), R6, dict(rtol=1e-5, atol=1e-5)),
    "test_gpu_kernels.py::test_eqm_train_adjust", whole_cell=True, target="hist")


# xh_si_fit followed by xh_si_apply through standardized_index: monthly means, a trailing 3-month window, a gamma fit with the
# location fixed at 0 per calendar month (five values each; the closed-form shape root, no optimizer walk) and the index of
# every month.  A daily sample reaches three months, hence three of the twelve fits, and through them every year's index of
# those calendar months.  The reference: the monthly means and the window in float64 numpy, rounded to the float32 the fit reads
# (as tests/test_gpu_stdidx.py::test_full_grid_monthly_spi3 builds them), then tests/spicpu.py.  Tolerance:
# tests/test_gpu_stdidx.py::test_golden_host_mirror for the closed-form fits (atol 1e-4 on the index).
def _spi():
    import spicpu
    from xclim_amd import stats as xs

    T = 365 * 5
    ta, ot = TimeAxis.daily("2001-01-01", T, "noleap"), OTime.noleap(2001, T, "noleap")
    gidx = np.arange(60) % 12

    def device(dev, f):
        return [np.asarray(xs.standardized_index(f["x"], ta, "MS", 3, dist="gamma", method="ML", zero_inflated=False, fitkwargs={"floc": 0.0},
                                                 device=dev))]

    def ref(f):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            w = np.asarray(ogen.select_resample_op(f["x"], "mean", ot, "MS")).astype(np.float32).astype(np.float64)
            xp = np.full(w.shape, np.nan, np.float32)
            xp[2:] = ((w[:-2] + w[1:-1]) + w[2:]) / 3.0
            p, _, _, _ = spicpu.fit(xp, gidx, 12, "gamma", "ML", False, 0.0)
            return [spicpu.index(xp, gidx, p, "gamma", None, None)]

    return _x(T), device, ref, (0, T - 1, 30, 31, 400), (dict(rtol=0, atol=1e-4),)


add("si_fit_apply_w3", "shared", *_spi(), "test_gpu_stdidx.py::test_golden_host_mirror", whole_cell=True)


# DetrendedQuantileMapping through its public train / adjust with group="time.dayofyear", window=31: the consumer of
# xh_window_nanmean.  Trained once on clean fields; the bad sample sits in the series that is adjusted, whose window mean
# (rows t - 15 .. t + 15) feeds the trend of 31 days of year in every year of the cell.  Additive, on the temperature field (with a
# seasonal cycle, so that the days of the year differ).  Tolerance: tests/test_gpu_api.py::test_dqm_windowed_sub_grouping_matches_oracle
# (rtol 2e-5, atol 2e-5).  Row 127 ends a stretch of k_window_nanmean, row 128 starts the next.
def _dqm():
    from xclim_amd import sdba as xsdba

    T = 365 * 4
    ta, ot = TimeAxis.daily("2001-01-01", T, "noleap"), OTime.noleap(2001, T, "noleap")
    trained = {}

    def make(rng, kind, dtype, C):
        t = np.arange(T)[:, None]
        seas = 8 * np.sin(2 * np.pi * (t - 100) / 365)
        return {"ref": (fp.kelvin(rng, T, C, np.float64) + seas).astype(np.float32),
                "hist": (fp.kelvin(rng, T, C, np.float64) + 1.5 + 1.2 * seas).astype(np.float32),
                "sim": (fp.kelvin(rng, T, C, np.float64) + 2.0 + 1.2 * seas + 3.0 * t / T).astype(np.float32)}

    def device(dev, f):
        key = (id(dev), f["sim"].shape)
        if key not in trained:
            trained[key] = xsdba.DetrendedQuantileMapping.train(f["ref"], f["hist"], nquantiles=15, kind="+", group="time.dayofyear", window=31,
                                                                time=ta, device=dev)
        return [np.asarray(trained[key].adjust(f["sim"], detrend=1, time=ta, grouped_nearest="group"))]

    def ref(f):
        key = ("oracle", f["sim"].shape)
        if key not in trained:
            trained[key] = osdba.dqm_train_grouped(f["ref"], f["hist"], ot, "dayofyear", 15, "+", window=31)
        labels, af, hq, scal = trained[key]

        def adjust(cols):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                return osdba.dqm_adjust_grouped(f["sim"][:, cols], ot, "dayofyear", labels, af[..., cols], hq[..., cols], scal[..., cols], "+",
                                                "constant", 1, mode="group", window=31)

        # (the oracle works column by column and takes 3 s for the 70 of them: the columns whose series is the clean one keep the
        # clean result, computed once; only the others are computed again)
        ckey = ("clean", f["sim"].shape)
        if ckey not in trained:
            trained[ckey] = (f["sim"].copy(), adjust(slice(None)))
        sim0, out0 = trained[ckey]
        cols = np.flatnonzero(~fp.same_bits(f["sim"], sim0).all(axis=0))
        out = out0.copy()
        if cols.size:
            out[:, cols] = adjust(cols)
        return [out]

    return make, device, ref, (0, T - 1, 127, 128, 500), (dict(rtol=2e-5, atol=2e-5),)


add("dqm_dayofyear_w31", "shared", *_dqm(), "test_gpu_api.py::test_dqm_windowed_sub_grouping_matches_oracle", target="sim", kinds=("kelvin",))


# ------------------------------------------------------------------------------------------------------------ recurrences
# spell_length_statistics (xh_spell_run_stats / xh_run_stats: a run is carried from row to row): spells above and below a
# threshold, windows 1 and 3, the longest spell, the days in spells and the number of spells per year.  With window 1 the days
# in spells are the days that meet the condition; the samples to be replaced ARE the threshold, so a fill value changes them
# for ">" or for "<" and a NaN for ">=".  Exact:
# tests/test_gpu_spells.py::test_spell_length_statistics_general.
def _spells():
    from xclim_amd import generic as xgen

    ta, ot = TimeAxis.daily("2001-01-01", 730, "noleap"), OTime.noleap(2001, 730, "noleap")
    combos = [(w, op, red) for w in (1, 3) for op in (">", "<", ">=") for red in ("max", "sum", "count")]

    def device(dev, f):
        t = f["thr"]
        return [np.asarray(xgen.spell_length_statistics(f["x"], t, w, "min", op, red, ta, "YS", device=dev)) for w, op, red in combos]

    def ref(f):
        t = f["thr"]
        return [np.asarray(ogen.spell_length_statistics(f["x"], t, w, "min", op, red, ot, "YS")) for w, op, red in combos]

    rows = (0, 729, 364, 365, 500)
    return _x(730, rows), device, ref, rows, (None,) * len(combos)


add("spell_length_statistics", "shared", *_spells(), "test_gpu_spells.py::test_spell_length_statistics_general", whole_cell=True)


# xh_mcarthur (ffdi.hip).  The drought factor alone reads the last 20 days of precipitation (and the day's soil moisture
# deficit, here a clean field): a window case.  The Keetch-Byram index carries its state from day to day: a bad precipitation
# amount or temperature may reach the rest of the cell's series, and no other cell.  Tolerances: tests/test_ffdi_cpu.py (RTOL /
# ATOL of "df" and "kbdi"), used by tests/test_gpu_ffdi.py::test_device_other_dtype.
def _mcarthur(outputs, T=300):
    import ffdicpu

    def make(rng, kind, dtype, C):
        pr = fp.flux(rng, T, C, np.float64) * 86400.0          # mm per day, events above 2 mm among them
        pr[[0, T - 1, 127, 128, 19, 20]] = 10.0                # the days to be replaced are rain events
        return {"pr": pr.astype(dtype),
                "tasmax": (fp.kelvin(rng, T, C, np.float64) - 263.0).astype(dtype),     # degC, 20 +- 4
                "smd": rng.uniform(0.0, 100.0, (T, C)).astype(dtype), "pr_annual": rng.uniform(200.0, 1600.0, C)}

    def device(dev, f):
        d = {k: dev.to_device(f[k], dtype=f[k].dtype) for k in ("pr", "tasmax", "smd")}
        outs = K.mcarthur(dev, d, dev.to_device(f["pr_annual"], dtype=np.float64), outputs=outputs)
        return [outs[o].get() for o in outputs]

    def ref(f):
        if outputs == ("DF",):
            return [ffdicpu.drought_factor(f["pr"], f["smd"])]
        return [ffdicpu.kbdi(f["pr"], f["tasmax"], f["pr_annual"])]

    return make, device, ref, (0, T - 1, 127, 128, 19, 20)


add("mcarthur_drought_factor", "shared", *_mcarthur(("DF",)), (dict(rtol=1e-12, atol=1e-12),), "test_gpu_ffdi.py::test_device_other_dtype",
    target="pr", kinds=("flux",), dtypes=(F32, F64),
    may_be_empty="ffdi.hip takes a day as a rain event where pr > 2: the comparison is false for a NaN as for a dry day, and the event "
                 "of row 0 counts only in the window of row 19")
add("mcarthur_kbdi_pr", "shared", *_mcarthur(("KBDI",)), (dict(rtol=1e-12, atol=1e-9),), "test_gpu_ffdi.py::test_device_other_dtype",
    target="pr", kinds=("flux",), dtypes=(F32, F64), whole_cell=True,
    may_be_empty="the index is clamped to [0, 203.2] (ffdi.hip): on a day whose index is 0 before and after, the rain changes nothing")
add("mcarthur_kbdi_tasmax", "shared", *_mcarthur(("KBDI",)), (dict(rtol=1e-12, atol=1e-9),), "test_gpu_ffdi.py::test_device_other_dtype",
    target="tasmax", kinds=("kelvin",), dtypes=(F32, F64), whole_cell=True,
    may_be_empty="the index is clamped to [0, 203.2] (ffdi.hip): on the rain day of row 0 it is 0 whatever the temperature says")


# xh_fire_weather (fire.hip) through fire_weather_ufunc, no season: the drought code, the duff and the fine fuel moisture codes
# carry their state from day to day, so a bad precipitation amount or temperature may reach the rest of its cell's series.
# float32 fields only.  Tolerance: tests/test_fire_cpu.py::check_outputs (rtol 1e-6, atol 1e-5), used by
# tests/test_gpu_fire.py::test_partial_waves_odd_cells_short_series.
def _fire(T=300):
    import firecpu
    from xclim_amd import fire

    time = TimeAxis.daily("2001-03-01", T, "noleap")

    def make(rng, kind, dtype, C):
        pr = fp.flux(rng, T, C, np.float64) * 86400.0                                           # mm per day
        pr[[0, T - 1, 150]] = 10.0                                                              # the days to be replaced are rain events
        return {"pr": pr.astype(np.float32),
                "tas": (fp.kelvin(rng, T, C, np.float64) - 263.0).astype(np.float32),           # degC, 20 +- 4
                "hurs": np.clip(rng.normal(65.0, 18.0, (T, C)), 5.0, 100.0).astype(np.float32),
                "ws": np.abs(rng.normal(12.0, 7.0, (T, C))).astype(np.float32), "lat": rng.uniform(-60.0, 60.0, C)}

    def device(dev, f):
        o = fire.fire_weather_ufunc(tas=f["tas"], pr=f["pr"], hurs=f["hurs"], sfcWind=f["ws"], lat=f["lat"], time=time, device=dev)
        return [np.asarray(o[k]) for k in firecpu.INDEXES]

    def ref(f):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            o = firecpu.fire_weather(f["tas"], f["pr"], f["hurs"], f["ws"], None, time.month, f["lat"])
        return [o[k] for k in firecpu.INDEXES]

    return make, device, ref, (0, T - 1, 150), (dict(rtol=1e-6, atol=1e-5),) * len(firecpu.INDEXES)


add("fire_weather_pr", "shared", *_fire(), "test_gpu_fire.py::test_partial_waves_odd_cells_short_series", target="pr", kinds=("flux",),
    whole_cell=True)
add("fire_weather_tas", "shared", *_fire(), "test_gpu_fire.py::test_partial_waves_odd_cells_short_series", target="tas", kinds=("kelvin",),
    whole_cell=True)


# xh_chill_daily (chill.hip): Linvill's hourly profile of every day (the night reads the next day's minimum) and the Dynamic
# Model's march through the hours of a period, which restarts with every period: a bad daily minimum may reach the rest of its
# 30-day period (and the night before), no other period and no other cell.  Temperatures around the release threshold (278 +- 4 K).
# Tolerances: tests/test_gpu_chill.py::test_daily_shapes_against_restatement (RTOL = 1e-12 on the portions and the hourly field,
# the chill units and the counts exactly).
def _chill(D=120):
    import chillcpu
    from test_chill_cpu import K2C, RTOL

    seg = np.array([0, 30, 60, 90, D])
    names = ("cp", "cu", "valid", "hourly")

    def make(rng, kind, dtype, C):
        base = fp.kelvin(rng, D, C, np.float64) - 5.0
        spread = rng.uniform(2.0, 12.0, (D, C))
        return {"tasmin": (base - spread / 2).astype(dtype), "tasmax": (base + spread / 2).astype(dtype),
                "dl": rng.uniform(8.0, 16.0, (D, 3)), "li": (np.arange(C) % 3).astype(np.int32)}

    def device(dev, f):
        dt = f["tasmin"].dtype
        o = K.chill_daily(dev, dev.to_device(f["tasmin"], dtype=dt), dev.to_device(f["tasmax"], dtype=dt),
                          dev.to_device(f["dl"], dtype=np.float64), f["li"], seg, outputs=names)
        return [o[k].get() for k in names]

    def ref(f):
        with np.errstate(all="ignore"):
            hourly = chillcpu.hourly_temperature(f["tasmin"], f["tasmax"], f["dl"][:, f["li"]])
            cp, _, valid = chillcpu.portions(hourly, 24 * seg)
            return [cp, chillcpu.units(hourly - K2C, 24 * seg), valid, hourly]

    return make, device, ref, (0, D - 1, 29, 30, 75), (dict(rtol=RTOL, atol=0), None, None, dict(rtol=RTOL, atol=0))


add("chill_daily", "chill", *_chill(), "test_gpu_chill.py::test_daily_shapes_against_restatement", target="tasmin", kinds=("kelvin",),
    dtypes=(F32, F64), whole_cell=True, quad=True)


# xh_bioclim (bioclim.hip) on 20 quarters of five years ("QS"), daily fields in 7-day steps: the quarter windows of 13 steps run
# across the period ends, so a bad sample reaches the quarters of its own period and of the next, two of twenty.  Row 89 ends
# the first quarter of a year, row 90 starts the second.  Tolerances: tests/test_anuclim_cpu.py::check, used by
# tests/test_gpu_bioclim.py::test_midyear_start_against_restatement (the standing bound of the dtype, BIO4 / BIO15 the
# measured bound of the single-pass formula, step indices and counts exactly).
def _bioclim(dtype):
    import anuclimcpu as A
    from test_anuclim_cpu import CV_BOUND, RTOL32, RTOL64

    T, DAY = 365 * 5, 86400.0
    ta = TimeAxis.daily("2001-01-01", T, "noleap")
    so, sr, ss, W = A.tables(ta.year, ta.month, "D", "QS")
    factor = np.full(T, DAY)
    names = K.BIOCLIM_VARS + K.BIOCLIM_WHICH + K.BIOCLIM_COUNTS
    kw = dict(kelvin_offset=0.0, cv_scale=DAY, thresh=1.5e-5)

    def make(rng, kind, dtype, C):
        tas = fp.kelvin(rng, T, C, np.float64)
        lo, hi = rng.uniform(2.0, 6.0, (T, C)), rng.uniform(2.0, 6.0, (T, C))
        return {"tas": tas.astype(dtype), "tasmin": (tas - lo).astype(dtype), "tasmax": (tas + hi).astype(dtype),
                "pr": fp.flux(rng, T, C, dtype)}

    def device(dev, f):
        d = {k: dev.to_device(f[k], dtype=f[k].dtype) for k in ("tas", "tasmin", "tasmax", "pr")}
        o = K.bioclim(dev, d, so, factor, sr, ss, W, binned=True, outputs=names, **kw)
        return [o[k].get() for k in names]

    def ref(f):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            o = A.bioclim({k: f[k] for k in ("tas", "tasmin", "tasmax", "pr")}, so, factor, sr, ss, W, True, kw["kelvin_offset"],
                          kw["cv_scale"], kw["thresh"])
        return [o[k] for k in names]

    std = RTOL32 if dtype == F32 else RTOL64
    tol = tuple(dict(rtol=CV_BOUND if n in ("bio4", "bio15") else std, atol=0) if n.startswith("bio") else None for n in names)
    return make, device, ref, (0, T - 1, 365 + 89, 365 + 90, 365 * 2 + 200), tol


for _dt in (F32, F64):
    add(f"bioclim_tas_{np.dtype(_dt).name}", "bioclim", *_bioclim(_dt), "test_gpu_bioclim.py::test_midyear_start_against_restatement",
        target="tas", kinds=("kelvin",), dtypes=(_dt,))
    add(f"bioclim_pr_{np.dtype(_dt).name}", "bioclim", *_bioclim(_dt), "test_gpu_bioclim.py::test_midyear_start_against_restatement",
        target="pr", kinds=("flux",), dtypes=(_dt,))


# xh_rain_season (rainseason.hip) on five years, one period each, every row inside all three date windows.  Every year is built
# the same way on a 0.25 mm grid (every window sum is exact): three days of 10 mm (the wet start: 30 mm in 3 days), then 2 to
# 2.75 mm a day (never a dry day) up to day 345, then exactly 20 dry days (the end).  A bad sample moves the season of its
# own year, one period of five.  Exact, as tests/test_gpu_rain.py::test_cell_counts.
def _rain_season():
    import raincpu as R

    T = 365 * 5
    seg = np.arange(0, T + 1, 365)
    flags = np.full(T, 7, np.uint8)
    doy = (np.arange(T) % 365 + 1).astype(np.int32)
    names = ("start", "end", "length")

    def make(rng, kind, dtype, C):
        d = np.arange(T)[:, None] % 365
        pr = 2.0 + 0.25 * ((np.arange(T)[:, None] + np.arange(C)[None, :]) % 4)
        pr = np.where(d < 3, 10.0, np.where(d >= 345, 0.0, pr))
        return {"pr": pr.astype(dtype)}

    def device(dev, f):
        o = K.rain_season(dev, dev.to_device(f["pr"], dtype=f["pr"].dtype), seg, flags, doy, per_day=1.0, outputs=names)
        return [o[k].get() for k in names]

    def ref(f):
        with np.errstate(all="ignore"):
            return list(R.rain_season_flags(f["pr"], seg, flags, doy, "mm/d"))

    return make, device, ref, (0, T - 1, 365 * 2 - 1, 365 * 2), (None, None, None)


add("rain_season", "rain", *_rain_season(), "test_gpu_rain.py::test_cell_counts", target="pr", kinds=("flux",), dtypes=(F32, F64),
    may_be_empty="rainseason.hip compares amounts with thresholds: -9999 on a dry day of the end (rows 729 and 1824) is still dry, and "
                 "1e20 on the first wet day of a year (rows 0 and 730) leaves the three-day sum above its threshold")


# xh_precip_phase_period (phase.hip), the binary partition at 0 degC, all fourteen outputs of the 24 months of two years, the
# bad sample in the precipitation and, in a case of its own, in the temperature (273 +- 4 K: both phases every month).  Rain on
# frozen ground looks back 7 rows, across the month's first row.  Exact, as the binary cases of
# tests/test_gpu_phase.py::test_golden_cases (compare: assert_array_equal).
def _phase():
    import phasecpu as R
    from xclim_amd import phase

    ot = R.otime("2001-01-01", 730, "noleap")
    pd = 86400.0

    def make(rng, kind, dtype, C):
        pr, tas = fp.flux(rng, 730, C, dtype), (fp.kelvin(rng, 730, C, np.float64) - 10.0).astype(dtype)
        pr[[0, 729, 30, 31, 400]] = 2e-5           # the days to be replaced are wet (1.7 mm), thawing ...
        tas[[0, 30, 400]], tas[[729, 31]] = 276.0, 270.0   # ... or freezing
        return {"pr": pr, "tas": tas}

    def device(dev, f):
        dt = f["pr"].dtype
        rnd =(lambda v: float(np.float32(v))) if dt == np.float32 else float
        part = phase.partition("binary", None, units="K", dtype=dt, time=_TA2, clip_temp=None, landmask=True, cell_shape=(f["pr"].shape[1],),
                               device=dev)
        o = K.precip_phase_period(dev, dev.to_device(f["pr"], dtype=dt), dev.to_device(f["tas"], dtype=dt), _SEG_MS, part, R.OUTPUTS,
                                  per_day=pd, doy=_TA2.doy, snow_low=0.0, snow_high=R.SNOW_HIGH, snow_thresh=1.0, hplt_pr=rnd(0.4 / pd),
                                  hplt_tas=rnd(-0.2 + R.K2C), rofg_pr=rnd(1.0 / pd), rofg_frz=rnd(R.K2C))
        return [o[k].get() for k in R.OUTPUTS]

    def ref(f):
        with np.errstate(all="ignore"):
            o = R.period_outputs(f["pr"], f["tas"], ot, "MS", given=False, per_day=pd, method="binary", landmask=True)
        return [o[k] for k in R.OUTPUTS]

    return make, device, ref, (0, 729, 30, 31, 400), (None,) * len(R.OUTPUTS)


add("precip_phase_period_pr", "phase", *_phase(), "test_gpu_phase.py::test_golden_cases", target="pr", kinds=("flux",), dtypes=(F32, F64),
    quad=True)
add("precip_phase_period_tas", "phase", *_phase(), "test_gpu_phase.py::test_golden_cases", target="tas", kinds=("kelvin",), dtypes=(F32, F64),
    may_be_empty="the binary partition of phase.hip compares the temperature with a threshold: -9999 on a freezing day (rows 31 and 729) "
                 "and 1e20 on a thawing day (rows 0, 30 and 400) leave every output as it was")


# xh_dist_fit (distfit.hip), the normal distribution by maximum likelihood on 30 values per cell: the mean and the deviation
# about it (ddof 0) of the values that are not NaN, written here in numpy as scipy's norm.fit computes them; the status byte is
# "fitted" throughout.  Tolerance: tests/test_gpu_distfit.py::test_closed_form_and_root_found_fits (rtol 1e-9).
def _dist_fit():
    def device(dev, f):
        params, _, status, _ = K.dist_fit(dev, dev.to_device(f["x"], dtype=f["x"].dtype), "norm", "ML")
        return [params.get(), status.get()]

    def ref(f):
        x = f["x"].astype(np.float64)
        p = np.empty((2, x.shape[1]))
        with np.errstate(all="ignore"):
            for c in range(x.shape[1]):
                v = x[~np.isnan(x[:, c]), c]
                p[0, c] = v.mean()
                p[1, c] = np.sqrt(((v - p[0, c]) ** 2).mean())
        return [p, np.zeros(x.shape[1], np.uint8)]

    return _x(30), device, ref, (0, 29, 15), (dict(rtol=1e-9, atol=0), None)


add("dist_fit_norm", "distfit", *_dist_fit(), "test_gpu_distfit.py::test_closed_form_and_root_found_fits", dtypes=(F32, F64), whole_cell=True,
    quad=True)


# ----------------------------------------------------------------------------------------------------------------- the tests
PARAMS =[pytest.param(c, kind, dt, id=f"{c.lib}-{c.name}-{kind}-{np.dtype(dt).name}") for c in CASES for kind in c.kinds for dt in c.dtypes]
WAIVED = sorted({(c.name, c.waive_a2) for c in CASES if c.waive_a2})
DROPPED = sorted((c.name, p, why) for c in CASES for p, why in c.dropped.items())
MAY_BE_EMPTY = sorted((c.name, c.may_be_empty) for c in CASES if c.may_be_empty)


@pytest.mark.parametrize("case,kind,dtype", PARAMS)
def test_one_bad_sample_stays_in_its_footprint(dev, case, kind, dtype):
    report = []
    try:
        fp.check(dev, case, kind, dtype, report=report)
    finally:
        print("\n".join(report))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_flags_a_fill_value_is_flagged_and_no_other_flag_of_the_field_moves(dev, dtype):
    """The climatology check on the bound tables of the field itself: whichever of the four values replaces a sample, that sample
    is flagged; the flags of the other cells do not move at all, and those of its own cell move only where the reference's do."""
    case = next(c for c in CASES if c.name == f"doy_bounds_and_flags_{np.dtype(dtype).name}")
    fields = case.make(np.random.default_rng(case.seed), "kelvin", dtype)
    clean, ref_clean = case.device(dev, fields)[2], case.ref(fields)[2]
    t, c = 365 * 2 + 24, 64
    for name, v in fp.PERTURBATIONS.items():
        pert = dict(fields, x=fields["x"].copy())
        pert["x"][t, c] = v
        got, exp = case.device(dev, pert)[2], case.ref(pert)[2]
        assert got[t, c] == 1, name
        moved, may = got != clean, exp != ref_clean
        assert not np.delete(moved, c, axis=1).any(), name
        assert not (moved[:, c] & ~may[:, c]).any(), name


def test_the_waivers_and_dropped_cases_are_listed(dev):
    """Prints the cases that waive A2 (bit-identity outside the footprint), the perturbations a case leaves out and the cases in
    which the reference may stay as it is at some positions, each with its reason; a waiver without a reason that names code,
    or a dropped perturbation without one, fails."""
    print(f"{len(CASES)} cases, {len(PARAMS)} tests; A2 waived for {len(WAIVED)}:")
    for name, why in WAIVED:
        print(f"  {name}: {why}")
        assert ".hip" in why or ".py" in why, name
    print(f"perturbations left out: {len(DROPPED)}")
    for name, p, why in DROPPED:
        print(f"  {name} / {p}: {why}")
        assert why and p in fp.PERTURBATIONS, name
    print(f"positions at which the reference may stay as it is (then nothing at all may move there): {len(MAY_BE_EMPTY)} cases")
    for name, why in MAY_BE_EMPTY:
        print(f"  {name}: {why}")
        assert ".hip" in why, name
    assert len({c.name for c in CASES}) == len(CASES)
