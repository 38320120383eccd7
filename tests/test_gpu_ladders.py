"""The size-dispatched kernel ladders at their switch points.

Each hot kernel is a ladder of template instances picked by the series length T, the number of quantile nodes nq or the
number of years; every instance has its own keys per lane, threads per column and LDS sizes.  For every ladder the tests
below run both sides of every switch point (s and s + 1) and one size inside every range, against the oracle with the
exactness the rest of the suite asks of that operation.  The split tables are read by the CPU guard at the end of the
module, which checks them against the dispatch constants in the .hip sources: an instance added or moved without
extending these tables fails that guard on any machine.  The grouped sdba kernels (rows per group, window rows, nodes)
have their tables and their tests in tests/test_gpu_sdba_edges.py; the guard here reads those tables too.
"""

import os
import re
import warnings

import numpy as np
import pytest

from oracle import calendar as ocal
from oracle import generic as ogen
from oracle import sdba as osdba
from oracle.timeutil import OTime
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

import test_gpu_sdba_edges as edges   # (the split tables of the grouped sdba kernels)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xclim_amd", "csrc")

# switch points: the instance for sizes <= s differs from the one for s + 1
COL_SPLITS = (384, 512, 1024, 2048, 3072, 4096, 6144, 8192, 10240, 11264, 12288, 14336, 16384, 32768)   # xh_select_columns (+ lean)
TM_SPLITS = (384, 512, 1024, 32768, 65535)       # time-major: short-series kernels (6 | 8 keys per lane) | select4.hip | its counter limits
QDM_SPLITS = (512, 2048, 4096, 8192, 12288, 16384, 32768)                                           # xh_qdm_columns | sorted
EQM_SPLITS = (10, 20, 32)                        # xh_eqm_adjust (nearest / linear / cubic), xh_eqm_adjust_g2d
PLANE_SPLITS = (20, 32)                          # plane_run: row kernel instances, linear pair path, nearest limit
PDOY_SPLITS = (32, 64)                           # percentile_doy: top-16 / quad / walk kernels
DOYSTATS_SPLITS = (1, 2, 8, 32, 64)              # climatological_mean_doy: k_doy_stats_year / k_doy_stats_sets<NY> | fallback

# one size inside every range (and beyond the last split)
COL_INNER = (300, 800, 1500, 2600, 3500, 5000, 7000, 9000, 10950, 11800, 13000, 15000, 20000, 40000)
QDM_INNER = (300, 1000, 3000, 6000, 10000, 14000, 20000, 40000)


def _both_sides(splits, inner=()):
    return sorted(set(splits) | {s + 1 for s in splits} | set(inner))


def _qnodes(nq):
    if nq == 1:
        return np.array([0.37])
    if nq == 20:
        return osdba.equally_spaced_nodes(20)
    return np.linspace(0.0, 1.0, nq)   # (the end points 0 and 1 included)


def _prev_split(splits, T):
    lower = [s for s in splits if s < T]
    return lower[-1] if lower else max(1, T // 3)


def _series(rng, T, C, splits):
    """(T, C) float32: clean normal columns, 3 % NaN, all-NaN, constant, heavily tied, tied + NaN, and two columns whose
    VALID count lies in a lower range than T (the instance is picked by T, the selection runs on the valid samples)."""
    x = (288 + rng.normal(0, 3, (T, C))).astype(np.float32)
    x[rng.random(T) < 0.03, 1] = np.nan
    x[:, 2] = np.nan
    x[:, 3] = np.float32(7.25)
    x[:, 4] = np.round(x[:, 4])
    x[:, 5] = np.round(x[:, 5] * 2) / 2
    x[rng.random(T) < 0.03, 5] = np.nan
    for c, keep in ((6, _prev_split(splits, T)), (7, max(1, T // 2))):
        drop = rng.permutation(T)[: T - keep]
        x[drop, c] = np.nan
    return x


# ---------------------------------------------------------------- quantile selection, column layout (time_axis=1)
@pytest.mark.gpu
@pytest.mark.parametrize("T", _both_sides(COL_SPLITS, COL_INNER))
def test_quantile_series_column_ladder(dev, rng, T):
    """xh_select_columns: grouped kernel (T <= 512), one wave per column (<= 1024), the ten lean instances (<= 16384), the
    LDS kernel (<= 32768), the radix select beyond.  Bitwise against the oracle (same fp64 lerp)."""
    from xclim_amd import kernels as K

    C = 67 if T <= 1025 else 9
    x = _series(rng, T, C, COL_SPLITS)
    xd = dev.to_device(np.ascontiguousarray(x.T))
    for nq in (1, 20, 64):
        q = _qnodes(nq)
        out = K.quantile_series(dev, xd, q, time_axis=1).get()
        np.testing.assert_array_equal(out, osdba.quantile(x, q).astype(np.float32), err_msg=f"T={T} nq={nq}")


# ---------------------------------------------------------------- quantile selection, time-major layout (time_axis=0)
@pytest.mark.gpu
@pytest.mark.parametrize("T", _both_sides(TM_SPLITS))
def test_quantile_series_time_major_ladder(dev, rng, T):
    """Time-major views: the short-series kernels up to 512 steps, the transposed pipeline at 513 .. 1024, the two-pass
    select4.hip from 1025 to 65535 (u16 counters; beyond 32768 the flagged columns take the radix select), the transposed
    pipeline again at 65536.  Bitwise against the oracle and against the column layout."""
    from xclim_amd import kernels as K

    C = 67
    x = _series(rng, T, C, TM_SPLITS)
    xd, xcd = dev.to_device(x), dev.to_device(np.ascontiguousarray(x.T))
    for nq in (1, 20, 64):
        q = _qnodes(nq)
        out = K.quantile_series(dev, xd, q).get()
        np.testing.assert_array_equal(out, osdba.quantile(x, q).astype(np.float32), err_msg=f"T={T} nq={nq}")
        np.testing.assert_array_equal(out, K.quantile_series(dev, xcd, q, time_axis=1).get(), err_msg=f"T={T} nq={nq}")


# ---------------------------------------------------------------- QDM exact-rank ranks (time_axis=1)
@pytest.mark.gpu
@pytest.mark.parametrize("T", _both_sides(QDM_SPLITS, QDM_INNER))
def test_qdm_adjust_column_ladder(dev, rng, T, monkeypatch):
    """xh_qdm_columns (seven instances up to 32768 steps) and the sorted path beyond, on time-minor columns: average ranks
    of tied rows and tied values, NaN samples, a column whose valid count lies in a lower range.  rtol 1e-6 against the
    oracle (scipy rankdata + interp1d), bitwise against the sorted path of qdm3.hip (diagnostic switch)."""
    from xclim_amd import kernels as K

    C, nq = 5, 20
    q = osdba.equally_spaced_nodes(nq)
    sim = (13 + 4 * rng.standard_normal((T, C))).astype(np.float32)
    sim = np.abs(sim) + 1
    sim[rng.random((T, C)) < 0.03] = np.nan
    if T > 10:
        sim[T // 3] = sim[T // 2]                      # a whole row repeated
    sim[:, 0] = np.round(sim[:, 0])                    # a heavily tied column
    drop = rng.permutation(T)[: T - _prev_split(QDM_SPLITS, T)]
    sim[drop, 4] = np.nan
    afs = {"+": rng.normal(0, 1, (nq, C)).astype(np.float32), "*": (1 + 0.1 * rng.normal(0, 1, (nq, C))).astype(np.float32)}
    sd = dev.to_device(np.ascontiguousarray(sim.T))
    got = {}
    for kind in ("+", "*"):
        afd = dev.to_device(afs[kind])
        for interp in ("nearest", "linear"):
            for extrap in ("constant", "nan"):
                out = K.qdm_adjust(dev, sd, afd, q, kind, interp, extrap, time_axis=1).get().T
                exp = osdba.qdm_adjust(sim, afs[kind], q, kind, interp, extrap)
                np.testing.assert_allclose(out, exp, rtol=1e-6, atol=0, equal_nan=True, err_msg=f"T={T} {kind} {interp} {extrap}")
                got[kind, interp, extrap] = out
    monkeypatch.setenv("XH_DIAGNOSTICS", "1")
    monkeypatch.setenv("XH_QDM_FORCE_SORTED", "1")
    for (kind, interp, extrap), out in got.items():
        srt = K.qdm_adjust(dev, sd, dev.to_device(afs[kind]), q, kind, interp, extrap, time_axis=1).get().T
        np.testing.assert_array_equal(srt, out, err_msg=f"T={T} {kind} {interp} {extrap}")


# ---------------------------------------------------------------- node-count instances
def _eqm_nodes(rng, nq, C):
    ref = (288 + rng.normal(0, 3, (413, C))).astype(np.float32)
    hist = (289.5 + rng.normal(0, 3, (413, C))).astype(np.float32)
    eaf, ehq = osdba.eqm_train(ref, hist, nq, "+")
    eaf, ehq = eaf.astype(np.float32), ehq.astype(np.float32)
    eaf[1, 3] = np.nan             # an invalid node in one cell
    ehq[nq - 2, 5] = np.nan
    eaf[1:, 9] = np.nan            # one valid node
    return eaf, ehq


@pytest.mark.gpu
@pytest.mark.parametrize("nq", _both_sides(EQM_SPLITS))
@pytest.mark.parametrize("interp", ["nearest", "linear", "cubic"])
def test_eqm_adjust_node_ladder(dev, rng, nq, interp):
    """xh_eqm_adjust: register node arrays of 10 / 20 / 32 / 64 (nearest, linear) and 20 / 32 (cubic, at most 32 nodes)."""
    from xclim_amd import kernels as K
    from xclim_amd._capi import XclimHipError

    T, C = 413, 67
    sim = (290 + rng.normal(0, 4, (T, C))).astype(np.float32)
    sim[rng.random((T, C)) < 0.01] = np.nan
    eaf, ehq = _eqm_nodes(rng, nq, C)
    sd, ad, hd = dev.to_device(sim), dev.to_device(eaf), dev.to_device(ehq)
    if interp == "cubic" and nq > 32:
        with pytest.raises(XclimHipError, match="at most 32 quantile nodes"):
            K.eqm_adjust(dev, sd, ad, hd, "+", "cubic", "constant")
        return
    for kind in ("+", "*"):
        for extrap in ("constant", "nan"):
            out = K.eqm_adjust(dev, sd, ad, hd, kind, interp, extrap).get()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                exp = osdba.eqm_adjust(sim, eaf, ehq, kind, interp, extrap)
            np.testing.assert_allclose(out, exp, rtol=2e-6 if interp == "cubic" else 1e-6, atol=0, equal_nan=True,
                                       err_msg=f"{kind} {extrap}")


def _group_nodes(rng, G, nq, C):
    cyc = np.sin(2 * np.pi * np.arange(G) / G)[:, None, None]
    hq = (np.sort(rng.normal(0, 3, (G, nq, C)), axis=1) + 5 * cyc + 288).astype(np.float32)
    af = (rng.normal(0, 1, (G, nq, C)) + cyc).astype(np.float32)
    return hq, af


@pytest.mark.gpu
@pytest.mark.parametrize("nq", _both_sides(EQM_SPLITS))
def test_eqm_grouped_nearest_node_ladder(dev, rng, nq):
    """Grouped "nearest" (xsdba's 2-D interp_on_quantiles over the (value, group) plane): the whole series through the row
    kernel of xh_plane_nearest (instances 20 / 32) and one group at a time through xh_eqm_adjust_g2d (20 / 32); both refuse
    more than 32 nodes."""
    from xclim_amd import kernels as K
    from xclim_amd._capi import XclimHipError

    G, C, T = 12, 67, 300
    hq, af = _group_nodes(rng, G, nq, C)
    x = (288 + rng.normal(0, 8, (T, C))).astype(np.float32)
    x[rng.random((T, C)) < 0.03] = np.nan
    g = rng.integers(1, G + 1, T).astype(np.float64)
    g[:2] = [1.0, float(G)]                               # the cyclic ends
    xd, hd, ad = dev.to_device(x), dev.to_device(hq), dev.to_device(af)
    labels = np.arange(1, G + 1)
    if nq > 32:
        with pytest.raises(XclimHipError, match="at most 32 nodes"):
            K.plane_nearest(dev, xd, g, ad, hd, "+", "constant")
        with pytest.raises(XclimHipError, match="nq <= 32"):
            K.eqm_adjust_g2d(dev, xd, ad, hd, 1, "+", "constant")
        return
    for extrap in ("constant", "nan"):
        fac = osdba.interp_on_quantiles_2d(x, g, labels, hq, af, "nearest", extrap)
        for kind in ("+", "*"):
            exp = (x + fac if kind == "+" else x * fac).astype(np.float32)
            got = K.plane_nearest(dev, xd, g, ad, hd, kind, extrap).get()
            np.testing.assert_allclose(got, exp, rtol=1e-6, atol=0, equal_nan=True, err_msg=f"plane {kind} {extrap}")
        for gc in (1, 5, G):                              # one group's rows through the per-group kernel
            rows = x[g == gc]
            fac = osdba.interp_on_quantiles_2d(rows, np.full(len(rows), float(gc)), labels, hq, af, "nearest", extrap)
            got = K.eqm_adjust_g2d(dev, dev.to_device(rows), ad, hd, gc, "+", extrap).get()
            np.testing.assert_allclose(got, rows + fac, rtol=1e-6, atol=0, equal_nan=True, err_msg=f"g2d group {gc} {extrap}")


@pytest.mark.gpu
@pytest.mark.parametrize("nq", _both_sides(PLANE_SPLITS[:1]))
def test_plane_linear_node_ladder(dev, rng, nq):
    """The linear plane's pair path serves nq <= 20; 21 nodes take the general path.  Same acceptance as the plane tests
    (griddata, only verified exact degeneracies may differ)."""
    from tests.test_gpu_plane import _check, _nodes

    G, C, T = 12, 7, 300
    xq, yq = _nodes(rng, G, nq, C, 1.5, "t")
    lo, hi = xq.min(), xq.max()
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (T, C)).astype(np.float32)
    x[rng.random((T, C)) < 0.03] = np.nan
    _check(dev, x, rng.uniform(0.5, G + 0.5, T), xq, yq)


# ---------------------------------------------------------------- year-count instances
def _axes(nyears, calendar):
    if calendar == "standard":
        T = 365 * nyears + sum(1 for y in range(1981, 1981 + nyears) if y % 4 == 0)
        return TimeAxis.daily("1981-01-01", T), OTime.standard("1981-01-01", T)
    T = 365 * nyears
    return TimeAxis.daily("1981-01-01", T, calendar), OTime.noleap(1981, T, calendar)


def _doy_field(rng, T, C):
    t = np.arange(T)[:, None]
    x = (288 + 12 * np.sin(2 * np.pi * (t - 100) / 365) + rng.normal(0, 3, (T, C))).astype(np.float32)
    x[rng.random((T, C)) < 0.01] = np.nan
    x[:, 0] = np.nan                       # no valid day at all
    x[:, 1] = np.float32(280.0)            # constant
    x[: T // 3, 2] = np.nan                # fewer valid years than the instance was picked for
    x[:, 3] = np.round(x[:, 3])            # ties
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("nyears", _both_sides(PDOY_SPLITS))
@pytest.mark.parametrize("calendar", ["standard", "noleap"])
def test_percentile_doy_year_ladder(dev, rng, nyears, calendar):
    """percentile_doy on 32 / 33 and 64 / 65 years, windows 3, 5, 7: the top-16 register kernel (both ends), the quad
    kernel (window 5), the split walk (up to 32 years), the LDS ring beyond; the day-366 step included."""
    from xclim_amd.calendar import percentile_doy

    C = 67
    ta, ot = _axes(nyears, calendar)
    x = _doy_field(rng, len(ot.doy), C)
    per = [1.0, 10.0, 50.0, 90.0, 99.0]
    for window in (3, 5, 7):
        p = percentile_doy(x, ta, window=window, per=per, device=dev)
        exp, doys = ocal.percentile_doy(x, ot, window, per)
        np.testing.assert_array_equal(p.dayofyear, doys)
        np.testing.assert_allclose(p.values(), exp, rtol=1e-12, atol=0, equal_nan=True, err_msg=f"window {window}")


@pytest.mark.gpu
@pytest.mark.parametrize("nyears", _both_sides(DOYSTATS_SPLITS))
@pytest.mark.parametrize("calendar", ["standard", "noleap"])
def test_climatological_mean_doy_year_ladder(dev, rng, nyears, calendar):
    """climatological_mean_doy: the one-year rolling kernel, k_doy_stats_sets for 1 / 2 / 8 / 32 / 64 years, the generic
    kernel above 64 years and for a window other than 3, 5, 7."""
    from xclim_amd.calendar import climatological_mean_doy

    C = 67
    ta, ot = _axes(nyears, calendar)
    x = _doy_field(rng, len(ot.doy), C)
    for window in (3, 5, 7, 9):
        m, s, doys = climatological_mean_doy(x, ta, window=window, device=dev)
        em, es, edoys = ocal.climatological_mean_doy(x, ot, window)
        np.testing.assert_array_equal(doys, edoys)
        np.testing.assert_allclose(m, em, rtol=1e-6, equal_nan=True, err_msg=f"window {window}")
        np.testing.assert_allclose(s, es, rtol=2e-6, atol=1e-6, equal_nan=True, err_msg=f"window {window}")


# ---------------------------------------------------------------- weighted windows with per-cell thresholds
@pytest.mark.gpu
@pytest.mark.parametrize("window", [2, 7])
def test_spell_mask_weights_per_cell_threshold(dev, rng, window):
    """gen:523-524: weights and a threshold per cell -> xh_rolling_dot (float64 sum of the trailing window, NaN until it is
    full or when a sample is NaN), then the per-cell compare; also the dot product itself against float64 numpy."""
    from xclim_amd import generic as xgen
    from xclim_amd import kernels as K

    T, C = 400, 67
    x = rng.normal(0, 1, (T, C)).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.nan
    w = rng.random(window) + 0.1
    dot = K.rolling_dot(dev, dev.to_device(x), w).get()
    exp = np.full((T, C), np.nan)
    for t in range(window - 1, T):
        exp[t] = w @ x[t - window + 1: t + 1].astype(np.float64)
    np.testing.assert_array_equal(dot, exp.astype(np.float32))
    thr = rng.normal(0.0, 0.5, C)
    for op in (">", "<="):
        got = xgen.spell_mask(x, window, "mean", op, thr, weights=list(w), device=dev)
        np.testing.assert_array_equal(got, ogen.spell_mask(x, window, "mean", op, thr, weights=list(w)))
        assert 0 < got.mean() < 1


# ---------------------------------------------------------------- the guard (CPU)
# (source, function, size variable, split table): every comparison of the variable with an integer literal or a named
# `constexpr int` of the file in the function body, outside its XH_REQUIRE argument checks, must be a listed switch point.
# A function that dispatches on several sizes lists a tuple of variables and a tuple of tables, in the same order.
DISPATCH = [
    ("select.hip", "xh_select_columns", "T", COL_SPLITS),
    ("select2.hip", "xh_select_columns_lean", "T", COL_SPLITS),
    ("select.hip", "xh_select_time_major", "T", TM_SPLITS),
    ("select4.hip", "hs_run", "T", TM_SPLITS),
    ("qdm.hip", "xh_qdm_columns", "T", QDM_SPLITS),
    ("qdm.hip", "xh_qdm_adjust", "T", QDM_SPLITS),
    ("eqm.hip", "xh_eqm_adjust", "nq", EQM_SPLITS),
    ("eqm.hip", "xh_eqm_adjust_g2d", "nq", EQM_SPLITS),
    ("plane.hip", "plane_run", "nq", PLANE_SPLITS),
    ("pdoy_top.hip", "xh_launch_pdoy_top16", "nyears", PDOY_SPLITS),
    ("pdoy_top.hip", "xh_launch_pdoy_top16_count", "nyears", PDOY_SPLITS),
    ("pdoy_quad.hip", "xh_launch_pdoy_quad", "nyears", PDOY_SPLITS),
    ("pdoy_walk.hip", "xh_launch_pdoy_walk", "nyears", PDOY_SPLITS),
    ("doystats.hip", "xh_launch_doy_stats_sets", "nyears", DOYSTATS_SPLITS),
    # the grouped sdba kernels: their tables and their tests are tests/test_gpu_sdba_edges.py.  ws_train's `most` (a window
    # that GROWS past 1024 rows after a first window that fits) is a shape the schedules of xclim_amd/sdba.py never have: it runs
    # in test_sliding_window_that_grows_past_its_capacity_is_declined alone, on a hand-made schedule (1024 | 1026 rows)
    ("winsel.hip", "ws_train", ("n0", "most", "per", "nq"), (edges.WINDOW_ROW_SPLITS, edges.WINDOW_ROW_SPLITS, edges.GROUP_SPLITS, edges.NODE_SPLITS)),
    ("winsel.hip", "gq_train", ("most", "nq"), (edges.GROUP_SPLITS, edges.GQ_NODE_SPLITS)),
    ("qdm.hip", "xh_qdm_adjust_groups", ("most", "nq"), (edges.GROUP_SPLITS, edges.NODE_SPLITS)),
    ("select.hip", "launch_select_grp_g", "T", COL_SPLITS),
]


def _close(text, i, op, cl):
    """Index just past the bracket that closes the one at text[i]."""
    depth = 0
    for j in range(i, len(text)):
        depth += text[j] == op
        depth -= text[j] == cl
        if depth == 0:
            return j + 1
    raise ValueError("unbalanced brackets")


def _function_body(src, name):
    text = re.sub(r"/\*.*?\*/", " ", re.sub(r"//[^\n]*", "", src), flags=re.S)
    for m in re.finditer(r"^(?:static\s+)?int\s+" + re.escape(name) + r"\s*\(", text, flags=re.M):
        end = _close(text, m.end() - 1, "(", ")")
        rest = text[end:].lstrip()
        if rest.startswith("{"):
            start = text.index("{", end)
            return text[start:_close(text, start, "{", "}")]
    raise AssertionError(f"no definition of {name}")


def dispatch_points(csrc, fname, func, var):
    """The switch points of `var` in `func`: `var <= N` / `var > N` / `var == N` split at N, `var < N` / `var >= N` at N - 1.
    N is an integer literal or a named constant of the file (`constexpr int WS_CAP = 1024;`)."""
    src = open(os.path.join(csrc, fname)).read()
    consts = {n: int(v) for n, v in re.findall(r"\bconstexpr\s+int\s+([A-Za-z_]\w*)\s*=\s*(\d+)\s*;", src)}
    body = _function_body(src, func)
    while True:   # argument checks are limits, not switch points
        m = re.search(r"\bXH_REQUIRE\s*\(", body)
        if not m:
            break
        body = body[: m.start()] + body[_close(body, m.end() - 1, "(", ")"):]
    pts = set()
    for op, n in re.findall(r"(?<![\w.>])" + var + r"\s*(<=|>=|==|<|>)\s*(\d+|[A-Z][A-Z0-9_]*)\b", body):
        if not n.isdigit():
            assert n in consts, f"{fname}:{func}: `{var} {op} {n}` compares with a name that is no `constexpr int` of the file"
            n = consts[n]
        pts.add(int(n) - 1 if op in ("<", ">=") else int(n))
    return pts


@pytest.mark.parametrize("fname,func,var,splits", DISPATCH, ids=[f"{f}:{fn}" for f, fn, _, _ in DISPATCH])
def test_dispatch_points_are_tested(fname, func, var, splits):
    """`var` / `splits`: one size variable and its table, or a tuple of variables with a tuple of tables (a function that
    dispatches on several sizes: rows per group, window rows, nodes) — every variable is held to its own table."""
    pairs = [(var, splits)] if isinstance(var, str) else list(zip(var, splits, strict=True))
    for v, table in pairs:
        pts = dispatch_points(CSRC, fname, func, v)
        assert pts, f"{fname}:{func}: no `{v}` comparison found (was the dispatch renamed?)"
        missing = sorted(pts - set(table))
        assert not missing, f"{fname}:{func} switches at {v} = {missing}, which the ladder tests do not run"


def test_the_group_size_tables_are_what_the_edge_module_runs():
    """The tables of the grouped sdba kernels live next to their tests (tests/test_gpu_sdba_edges.py): both sides of every
    split must be among that module's parametrizations."""
    assert {s + d for s in edges.GROUP_SPLITS for d in (0, 1)} <= set(edges.LADDER_YEARS)
    assert {y for y, w, c in edges.WINDOW_CASES} >= {s + 1 for s in edges.GROUP_SPLITS}          # per | per group: 33, 65 years
    assert {s + d for s in edges.NODE_SPLITS for d in (0, 1)} <= set(edges.LADDER_NQ)       # k_qdm_groups
    assert {s + d for s in edges.NODE_SPLITS for d in (0, 1)} <= set(edges.WINDOW_NQ)       # the window kernel's own ladder
    assert {s + d for s in edges.GQ_NODE_SPLITS for d in (0, 1)} <= set(edges.GQ_LADDER_NQ)
    for s in edges.WINDOW_ROW_SPLITS:   # rows of the first window and of the largest: a case just inside, one just beyond
        assert any(s - 64 <= r <= s for r in edges.WINDOW_ROWS) and any(s < r <= s + 64 for r in edges.WINDOW_ROWS)
    assert {s + d for s in edges.SELECT_GRP_SPLITS for d in (0, 1)} <= set(_both_sides(COL_SPLITS)) & set(_both_sides(TM_SPLITS))
