"""The data-quality-flag unit on the device (xclim_amd/csrc/dataflags.hip, xclim_amd.dataflags) against the numpy restatement
tests/flagscpu.py: three years of a standard calendar from 1971-01-01 (T = 1096, three "YS" periods, 1972 with its day 366), 1, 65
and 130 cells (one lane, one wave plus a lane, two waves plus two lanes), float32 and float64.  One family of cases per decision
of the kernel; the same flags from the entry points that existed before (float32); the mirror against the reference's known
answers; the refusals.  Every test runs on poisoned output buffers.

Every flag is a boolean and every comparison is ``assert_array_equal``.  The climatology fields keep every sample at least half
a deviation away from either bound, which is asserted on the restatement where they are built: the rounding difference between
two correct tables cannot move a flag."""
import numpy as np
import pytest

import flagscpu as R
import stridedabi as S
from stridedabi import FLAGS_TABLE
from test_flags_cpu import DEFAULTS, check_known_answers, mirror_api, refusals
from xclim_amd import _capi, dataflags
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
CELLS = (1, 65, 130)
DTYPES = (np.float32, np.float64)
T = 1096
TIME = TimeAxis.daily("1971-01-01", T)
YEARS = np.asarray(TIME.segments("YS")[0], np.int64)          # [0, 365, 731, 1096]
ROWS = np.arange(T + 1, dtype=np.int64)                        # P = T: the element-wise masks
OPS = (">", "<", ">=", "<=", "==", "!=")
A = 285.5                                                      # an operand that is a float32 value: a sample can sit exactly on it


def launch(dev, x, specs, seg, reduce_cells=False, tables=None, tidx=None):
    """One launch of xh_data_flags on specs in the restatement's form; a "pair" names its companion by the array itself."""
    ys = []
    for s in specs:
        if s[0] == "pair" and not any(s[2] is y for y in ys):
            ys.append(s[2])
    checks = []
    for s in specs:
        if s[0] == "cmp":
            checks.append(K.flag_check("cmp", s[1], s[2]))
        elif s[0] == "outside":
            checks.append(K.flag_check("outside", None, s[1], s[2]))
        elif s[0] == "pair":
            checks.append(K.flag_check("pair", s[1], other=[i for i, y in enumerate(ys) if y is s[2]][0]))
        elif s[0] == "repeat":
            checks.append(K.flag_check("repeat", s[1], s[2], n=s[3]))
        else:
            checks.append(K.flag_check("clim"))
    d = [dev.to_device(np.ascontiguousarray(y)) for y in ys]
    lo, hi = tables if tables is not None else (None, None)
    return K.data_flags(dev, dev.to_device(np.ascontiguousarray(x)), checks, seg, y0=d[0] if d else None, y1=d[1] if len(d) > 1 else None,
                        tidx=tidx, lo=lo, hi=hi, reduce_cells=reduce_cells).get()


def check(dev, x, specs, segs=(YEARS, ROWS), reduces=(False, True), what=""):
    for seg in segs:
        for red in reduces:
            got = launch(dev, x, specs, seg, red)
            want = R.flags(x, specs, seg, red)
            assert got.dtype == np.uint8 and got.shape == want.shape
            np.testing.assert_array_equal(got, want, err_msg=f"{what} P={len(seg) - 1} reduce_cells={red}")


# ---- 1. CMP, OUTSIDE, PAIR ---------------------------------------------------------------------------------------------------
def compare_field(C, dtype, seed=1):
    """Samples around A with, in every column, the operand itself, one ulp of the dtype on either side of it and NaN."""
    rng = np.random.default_rng(seed)
    a = dtype(A)
    x = (A + rng.normal(0, 2.0, (T, C))).astype(dtype)
    special = np.array([a, np.nextafter(a, dtype(np.inf)), np.nextafter(a, dtype(-np.inf)), np.nan], dtype)
    for c in range(C):
        rows = rng.choice(T, 24, replace=False)
        x[rows, c] = np.tile(special, 6)
    x[[0, 364, 365, T - 1], C - 1] = special                   # the corners of the periods, in the last cell
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("C", CELLS)
def test_compare_outside_and_pair(dev, C, dtype):
    x = compare_field(C, dtype)
    b = dtype(A + 1.0)
    x[5:9, 0] = [b, np.nextafter(b, dtype(np.inf)), np.nextafter(b, dtype(-np.inf)), np.nan]
    rng = np.random.default_rng(2)
    y0, y1 = x.copy(), x.copy()                                # companions equal to the sample, one ulp beside it, NaN on either side
    pick = rng.integers(0, 5, x.shape)
    y0[pick == 1] = np.nextafter(x, dtype(np.inf))[pick == 1]
    y0[pick == 2] = np.nextafter(x, dtype(-np.inf))[pick == 2]
    y0[pick == 3] = np.nan
    y1[pick == 0] = np.nextafter(x, dtype(np.inf))[pick == 0]
    y1[pick == 4] = np.nan
    specs = [("cmp", op, A) for op in OPS] + [("outside", A, float(b))] + [("pair", op, y0 if i % 2 == 0 else y1) for i, op in enumerate(OPS)]
    want = R.flags(x, specs, ROWS, False)
    assert all(0 < w.sum() < w.size for w in want)            # every check decides both ways
    nan = np.isnan(x) | np.isnan(y0)
    assert not want[7][nan].any() and want[5][np.isnan(x)].all() and want[12][np.isnan(x) | np.isnan(y1)].all()   # NaN: only != is true
    check(dev, x, specs, what="compare")
    # an operand that is not a float32 value: the sample is widened, never the operand narrowed
    thr = 285.1
    x[3, 0] = dtype(thr)
    check(dev, x, [("cmp", op, thr) for op in OPS], segs=(ROWS,), reduces=(False,), what="widened")


# ---- 2. REPEAT ---------------------------------------------------------------------------------------------------------------
def repeat_field(C, dtype):
    """Distinct values everywhere (t + a fraction per cell), and in every cell its own planted runs; n = 5 is the length looked
    for.  Cell c (mod 8): 0 runs of 4 and of 5 rows; 1 a run on row 0 and one that ends on row T - 1; 2 a run that begins in 1971
    and reaches 5 rows in 1972; 3 a run from 1971 into 1973; 4 a run split by a NaN; 5 zeros of both signs; 6 runs whose value is
    A; 7 a run of NaN."""
    x = (np.arange(T)[:, None] * 0.25 + 300.0 + np.arange(C)[None, :] * 1000.0).astype(dtype)
    assert len(np.unique(x)) == x.size
    for c in range(C):
        k = c % 8
        if k == 0:
            x[10:14, c] = 7.0
            x[20:25, c] = 8.0
        elif k == 1:
            x[0:5, c] = 7.0
            x[T - 5:T, c] = 8.0
        elif k == 2:
            x[362:367, c] = 7.0
        elif k == 3:
            x[363:733, c] = 7.0
        elif k == 4:
            x[100:105, c] = 7.0
            x[102, c] = np.nan
        elif k == 5:
            x[200:205, c] = [0.0, -0.0, 0.0, -0.0, 0.0]
        elif k == 6:
            x[300:305, c] = A
            x[400:404, c] = A
            x[363:368, c] = np.nextafter(dtype(A), dtype(np.inf))
        else:
            x[500:506, c] = np.nan
    return x


REPEATS = [("repeat", None, 0.0, 5), ("repeat", None, 0.0, 4), ("repeat", None, 0.0, 2), ("repeat", None, 0.0, 1), ("repeat", None, 0.0, 369),
           ("repeat", None, 0.0, 371)] + [("repeat", op, A, 5) for op in OPS] + [("repeat", "==", 0.0, 5), ("repeat", "!=", A, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("C", CELLS)
def test_repeating_values(dev, C, dtype):
    x = repeat_field(C, dtype)
    want = R.flags(x, REPEATS, ROWS, False)
    n5, n4, n2, n1 = want[:4]
    assert not n5[10:14, 0].any() and n4[10:14, 0].all() and n5[20:25, 0].all() and not n5[25, 0]       # n - 1 and n rows
    assert n1.all()                                                                                    # n = 1: every row, NaN included
    if C > 7:
        assert n5[0:5, 1].all() and n5[T - 5:, 1].all()
        assert n5[362:367, 2].all() and R.flags(x, REPEATS[:1], YEARS, False)[0, :2, 2].all()           # the earlier year is flagged
        assert want[4][363:733, 3].all() and not want[5][:, 3].any()                                    # 370 rows: 369 yes, 371 no
        assert not n5[:, 4].any() and n2[[100, 101, 103, 104], 4].all() and not n2[102, 4]              # a NaN splits the run
        assert n5[200:205, 5].all() and want[12][200:205, 5].all()                                      # -0.0 == 0.0, and == 0.0 as a threshold
        assert not n2[500:506, 7].any()                                                                 # every NaN is a run of one
        for i, op in enumerate(OPS):                                                                    # the run value at the threshold
            assert want[6 + i][300:305, 6].all() == (op in (">=", "<=", "==")) and want[6 + i][363:368, 6].all() == (op in (">", ">=", "!="))
            assert not want[6 + i][400:404, 6].any()
    check(dev, x, REPEATS, what="repeat")


# ---- 3. CLIM and 4. xh_doy_bounds --------------------------------------------------------------------------------------------
WINDOW, NDEV, FLAT_DOY = 15, 5.0, 120


def clim_field(C, dtype, seed):
    """A seasonal cycle plus Gaussian noise; an outlier of 12 deviations in exactly one (cell, year): the last cell, 1972, day 200;
    a NaN sample; a day of year (FLAT_DOY) whose samples, and those of its whole window, are all equal; 1972 has day 366."""
    rng = np.random.default_rng(seed)
    x = 283.0 + 10.0 * np.sin(2 * np.pi * (TIME.doy[:, None] - 110) / 365.25) + rng.normal(0, 2.0, (T, C))
    x[np.abs(TIME.doy - FLAT_DOY) <= WINDOW // 2] = 280.0
    x[365 + 199, C - 1] += 24.0
    x[40, 0] = np.nan
    return x.astype(dtype)


def clim_margin(x, lo, hi, doys):
    """The least distance of a sample from either of its bounds, in deviations; inf for NaN samples and days without deviation."""
    idx = np.searchsorted(doys, TIME.doy)
    lo, hi = lo[idx].astype(np.float64), hi[idx].astype(np.float64)
    sig = (hi - lo) / (2 * NDEV)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.minimum(np.abs(x - lo), np.abs(x - hi)) / sig
    return np.where(np.isnan(x) | (sig == 0), np.inf, m)


_CLIM = {}


def clim_case(C, dtype):
    """(field, restated tables, restated mask), built once per shape; the seed is the first that keeps the margin."""
    key = (C, np.dtype(dtype).name)
    if key not in _CLIM:
        for seed in range(11, 41):
            x = clim_field(C, dtype, seed)
            lo, hi, doys = R.doy_bounds(x, TIME, WINDOW, NDEV)
            if clim_margin(x, lo, hi, doys).min() >= 0.5:
                break
        _CLIM[key] = (x, (lo, hi, doys), R.clim_mask(x, TIME, WINDOW, NDEV, (lo, hi, doys)))
    return _CLIM[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("C", CELLS)
def test_climatology(dev, C, dtype):
    x, (lo, hi, doys), want = clim_case(C, dtype)
    assert clim_margin(x, lo, hi, doys).min() >= 0.5          # the condition on the field, on the restatement
    assert len(doys) == 366 and not np.isnan(lo[365]).any()
    flat = TIME.doy == FLAT_DOY
    assert want[flat].all() and want[40, 0] and want[365 + 199, C - 1] and want.sum() == 3 * C + 2       # no deviation; NaN; the outlier
    tb, _, _ = TIME.doy_table()
    tidx = np.searchsorted(doys, TIME.doy).astype(np.int32)
    dx = dev.to_device(x)
    dlo, dhi = K.doy_bounds(dev, dx, tb, WINDOW, NDEV)
    for seg in (YEARS, ROWS):
        for red in (False, True):
            got = K.data_flags(dev, dx, [K.flag_check("clim")], seg, tidx=tidx, lo=dlo, hi=dhi, reduce_cells=red).get()
            np.testing.assert_array_equal(got[0], R.aggregate(want, seg, red), err_msg=f"P={len(seg) - 1} reduce_cells={red}")
    # a NaN bound flags: the tables of a field with a day that has no sample at all
    holed = x.copy()
    holed[np.abs(TIME.doy - 300) <= WINDOW // 2, 0] = np.nan
    hlo, hhi = K.doy_bounds(dev, dev.to_device(holed), tb, WINDOW, NDEV)
    assert np.isnan(hlo.get()[299, 0]) and np.isnan(hhi.get()[299, 0])
    got = K.data_flags(dev, dev.to_device(holed), [K.flag_check("clim")], ROWS, tidx=tidx, lo=hlo, hi=hhi).get()[0]
    assert got[TIME.doy == 300][:, 0].all()
    np.testing.assert_array_equal(got.astype(bool), R.clim_mask(holed, TIME, WINDOW, NDEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("window", [1, 3, 4, 5, 7, 15])
def test_doy_bounds(dev, window, dtype):
    """Both sides add in float64 and round four times (mean, deviation, product, sum): 4 ulp of the dtype at |mu| + n * sig.  NaN
    patterns are equal.  Windows 3, 5 and 7 have kernels of their own; the windows of days 1 and 2 reach before row 0, those of
    the last days past row T - 1."""
    C = 65
    x = clim_case(C, dtype)[0].copy()
    x[np.abs(TIME.doy - 300) <= window // 2, 1] = np.nan      # a day without any sample
    x[:, 2] = np.nan
    tb, _, doys = TIME.doy_table()
    lo, hi = (a.get() for a in K.doy_bounds(dev, dev.to_device(x), tb, window, NDEV))
    elo, ehi, edoys = R.doy_bounds(x, TIME, window, NDEV)
    assert lo.dtype == hi.dtype == np.dtype(dtype) and lo.shape == elo.shape == (366, C) and np.array_equal(doys, edoys)
    np.testing.assert_array_equal(np.isnan(lo), np.isnan(elo))
    np.testing.assert_array_equal(np.isnan(hi), np.isnan(ehi))
    assert np.isnan(lo[:, 2]).all() and np.isnan(lo[299, 1]) and not np.isnan(lo[:, 0]).any()
    scale = np.maximum(np.abs(elo), np.abs(ehi)).astype(np.float64)
    tol = 4 * np.spacing(scale.astype(dtype)).astype(np.float64)
    for got, exp in ((lo, elo), (hi, ehi)):
        ok = ~np.isnan(exp)
        assert (np.abs(got.astype(np.float64) - exp.astype(np.float64))[ok] <= tol[ok]).all()


# ---- 5. programs and shapes --------------------------------------------------------------------------------------------------
def mixed_program(C, dtype):
    """All five kinds in one program of 16 checks, on the climatology field with planted runs and companions."""
    x, (lo, hi, doys), _ = clim_case(C, dtype)
    x = x.copy()
    x[362:367, C - 1] = 291.0
    y0, y1 = (x + dtype(0.5)).astype(dtype), (x - dtype(0.5)).astype(dtype)
    y0[700:703, C - 1] = x[700:703, C - 1] - dtype(1.0)
    y1[20, 0] = np.nan
    specs = ([("cmp", op, 291.0) for op in OPS] + [("outside", 270.0, 295.0), ("pair", ">", y0), ("pair", "<", y1), ("pair", "!=", y1),
             ("repeat", None, 0.0, 5), ("repeat", "==", 291.0, 3), ("repeat", ">", 0.0, 1), ("clim", NDEV, WINDOW), ("clim", NDEV, WINDOW),
             ("outside", 280.0, 280.0)])
    assert len(specs) == _capi.FLAGS_MAX_CHECKS
    return x, specs


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("C", CELLS)
def test_sixteen_checks_in_one_program_equal_each_alone(dev, C, dtype):
    x, specs = mixed_program(C, dtype)
    tb, _, doys = TIME.doy_table()
    tidx = np.searchsorted(doys, TIME.doy).astype(np.int32)
    tabs = K.doy_bounds(dev, dev.to_device(x), tb, WINDOW, NDEV)
    for seg in (YEARS, ROWS):
        for red in (False, True):
            full = launch(dev, x, specs, seg, red, tabs, tidx)
            assert full.shape[0] == 16
            for k, s in enumerate(specs):                      # K = 1
                alone = launch(dev, x, [s], seg, red, tabs, tidx)
                np.testing.assert_array_equal(alone[0], full[k], err_msg=f"check {k} {s[:2]} P={len(seg) - 1} reduce_cells={red}")
            rest = [k for k, s in enumerate(specs) if s[0] != "clim"]
            np.testing.assert_array_equal(full[rest], R.flags(x, [specs[k] for k in rest], seg, red))
    assert 0 < full.sum() < full.size


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("C", CELLS)
def test_the_only_flagged_cell_is_the_last_one(dev, C, dtype):
    x = np.full((T, C), 280.0, dtype) + np.arange(T, dtype=dtype)[:, None] * dtype(0.001)
    x[400, C - 1] = 400.0
    x[900:905, C - 1] = 1.0
    specs = [("cmp", ">", 350.0), ("repeat", None, 0.0, 5), ("cmp", ">", 500.0)]
    got = launch(dev, x, specs, YEARS, True)
    np.testing.assert_array_equal(got, [[0, 1, 0], [0, 0, 1], [0, 0, 0]])
    cells = launch(dev, x, specs, YEARS, False)
    assert cells[:, :, :C - 1].sum() == 0 and cells[0, 1, C - 1] == 1 and cells[1, 2, C - 1] == 1 and cells.sum() == 2
    check(dev, x, specs, what="last cell")


def test_empty_periods_and_empty_shapes(dev):
    x = repeat_field(65, np.float64)
    seg = np.array([0, 0, 365, 365, 365, 731, T, T], np.int64)
    specs = REPEATS[:4] + [("cmp", ">", 400.0)]
    for red in (False, True):
        got = launch(dev, x, specs, seg, red)
        np.testing.assert_array_equal(got, R.flags(x, specs, seg, red))
        assert got[:, [0, 2, 3, 6]].sum() == 0 and got[3, [1, 4, 5]].all()
    for T0, C0, seg0 in ((0, 65, [0]), (0, 65, [0, 0, 0]), (T, 0, YEARS), (T, 65, None)):
        xs = np.zeros((T0, C0))
        if seg0 is None:      # P = 0 with rows does not cover [0, T]; K = 0 does nothing
            out = K.data_flags(dev, dev.to_device(xs), [], YEARS)
            assert out.shape == (0, 3, 65)
            continue
        out = K.data_flags(dev, dev.to_device(xs), [K.flag_check("cmp", ">", 1.0)], seg0, reduce_cells=False)
        assert out.shape == (1, len(seg0) - 1, C0)
        lo, hi = K.doy_bounds(dev, dev.to_device(xs), np.full((1, 4), -1, np.int32), 5, 5.0)
        assert lo.shape == hi.shape == (4, C0)
    lo, _ = K.doy_bounds(dev, dev.to_device(np.ones((3, 2))), np.zeros((1, 0), np.int32), 5, 5.0)
    assert lo.shape == (0, 2)


@pytest.mark.parametrize("dtype,C,pitch", [(np.float32, 65, 80), (np.float64, 130, 144), (np.float64, 1, 7)])
def test_padded_views_give_the_same_bits(dev, monkeypatch, dtype, C, pitch):
    """Every pitched operand of the two entry points (x, y0, y1, lo, hi, out; x and the tables of xh_doy_bounds) in rows of `pitch`
    elements, NaN / 1e30 in the extra columns of the inputs and in front of their first row, 0xA5 bytes in those of the outputs
    (tests/stridedabi.py: padded, which asserts that they stay)."""
    x, specs = mixed_program(C, dtype)
    tb, _, doys = TIME.doy_table()
    tidx = np.searchsorted(doys, TIME.doy).astype(np.int32)

    def run():
        tabs = K.doy_bounds(dev, dev.to_device(x), tb, WINDOW, NDEV)
        return [launch(dev, x, specs, YEARS, False, tabs, tidx), launch(dev, x, specs, ROWS, False, tabs, tidx), tabs[0].get(), tabs[1].get()]

    plain = run()
    with S.padded(dev, monkeypatch, pads=(pitch - C, pitch - C), shift=5) as log:
        got = run()
    for g, e in zip(got, plain):
        np.testing.assert_array_equal(g, e)
    assert [n for n, _ in log] == ["xh_doy_bounds", "xh_data_flags", "xh_data_flags"]
    assert log[0][1] == {"ld": (pitch, C), "ld_out": (pitch, C)}
    assert all(used == {k: (pitch, C) for k in ("ld", "ld_y0", "ld_y1", "ld_tab", "ld_out")} for _, used in log[1:]), log


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    refusals(dev)


def test_kernels_py_refuses_before_the_call(dev):
    x = dev.to_device(np.ones((10, 3)))
    one = [K.flag_check("cmp", ">", 1.0)]
    with pytest.raises(ValueError, match="at most 16 checks"):
        K.data_flags(dev, x, one * 17, [0, 10])
    with pytest.raises(ValueError, match="cover"):
        K.data_flags(dev, x, one, [0, 9])
    with pytest.raises(ValueError, match="needs tidx"):
        K.data_flags(dev, x, [K.flag_check("clim")], [0, 10])
    with pytest.raises(TypeError, match="all float32 or all float64"):
        K.data_flags(dev, x, [K.flag_check("pair", ">")], [0, 10], y0=dev.to_device(np.ones((10, 3), np.float32)))
    with pytest.raises(ValueError, match="unknown check kind"):
        K.flag_check("between")
    with pytest.raises(ValueError, match="at least 1"):
        K.flag_check("repeat", None, n=0)
    with pytest.raises(ValueError, match="not recognized"):
        K.flag_check("cmp", "~", 1.0)
    with pytest.raises(_capi.XclimHipError) as err:      # the entry point's own refusal surfaces with its code
        K.data_flags(dev, x, [K.flag_check("pair", ">")], [0, 10])
    assert err.value.code == _capi.XH_ERR_ARG and "companion" in err.value.msg


# ---- 7. the same flags from the entry points that existed before ------------------------------------------------------------
@pytest.mark.parametrize("C", CELLS)
def test_cross_check_with_the_existing_entry_points(dev, C):
    """float32: the flags equal the ``any`` per period of the masks of xh_suspicious_run, xh_within_bnds_doy (given the same
    tables) and xh_compare_map (float64 compare of the widened sample)."""
    x, specs = mixed_program(C, np.float32)
    tb, _, doys = TIME.doy_table()
    tidx = np.searchsorted(doys, TIME.doy).astype(np.int32)
    dx = dev.to_device(x)
    lo, hi = K.doy_bounds(dev, dx, tb, WINDOW, NDEV)
    masks, kept = [], []
    for s in specs:
        if s[0] == "cmp":
            m = K.compare_map(dev, dx, s[1], np.float64(s[2])).get()
        elif s[0] == "pair":
            m = K.compare_map(dev, dx, s[1], dev.to_device(s[2])).get()
        elif s[0] == "repeat":
            m = K.suspicious_run(dev, dx, s[3], s[1], s[2] if s[1] is not None else None).get()
        elif s[0] == "clim":
            m = 1 - K.within_bnds_doy(dev, dx, dev.to_device(lo.get().astype(np.float64)), dev.to_device(hi.get().astype(np.float64)), tidx).get()
        else:
            continue
        masks.append(m.astype(bool))
        kept.append(s)
    assert len(kept) == 14
    for seg in (YEARS, ROWS):
        for red in (False, True):
            got = launch(dev, x, kept, seg, red, (lo, hi), tidx)
            want = np.array([R.aggregate(m, seg, red) for m in masks], np.uint8).reshape(got.shape)
            np.testing.assert_array_equal(got, want, err_msg=f"P={len(seg) - 1} reduce_cells={red}")


# ---- 8. the mirror -----------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_device(dev):
    check_known_answers(mirror_api(dev))


def mirror_fields(dtype):
    rng = np.random.default_rng(8)
    shape = (T, 5, 13)
    tas = (283.0 + 10.0 * np.sin(2 * np.pi * (TIME.doy[:, None, None] - 110) / 365.25) + rng.normal(0, 2.0, shape)).astype(dtype)
    ds = {"tas": tas, "tasmax": (tas + dtype(4.0)).astype(dtype), "tasmin": (tas - dtype(4.0)).astype(dtype)}
    tas[800, 4, 12] = 340.0                      # extremely high, above tasmax
    tas[30, 0, 0] = 150.0                        # extremely low, below tasmin
    tas[500:506, 2, 3] = 285.0                   # a run
    tas[901, 1, 1] = np.nan                      # outside the climatology (15 samples a day cannot hold one five deviations out)
    ds["tasmax"][900, 1, 1] = np.nan
    return ds


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_dims_and_freq_of_the_mirror(dev, dtype):
    """The recorded defaults of tas on a (T, 5, 13) grid in every served combination of ``dims`` and ``freq``: the restatement's
    shapes and values; one launch of xh_doy_bounds and one of xh_data_flags each."""
    ds = mirror_fields(dtype)
    flags = DEFAULTS["tas"]["data_flags"]
    seen = set()
    for freq in (None, "YS", "MS"):
        for dims in ("all", None, "time", "cells"):
            trace = dev.start_trace()
            try:
                got = dataflags.data_flags(ds["tas"], ds, flags, dims, freq, name="tas", time=TIME, units="K", device=dev)
            finally:
                dev.stop_trace()
            assert [n for n, _ in trace if n in FLAGS_TABLE] == ["xh_doy_bounds", "xh_data_flags"]
            want = R.data_flags(ds["tas"], ds, flags, dims, freq, name="tas", time=TIME, units="K")
            assert list(got) == list(want) and len(got) == 6
            for k in got:
                assert got[k].dtype == bool and got[k].shape == want[k].shape, (k, dims, freq)
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} dims={dims} freq={freq}")
                seen.add(got[k].shape)
            assert all(v.any() for k, v in got.items())
    assert seen == {(), (T,), (T, 5, 13), (5, 13), (3,), (3, 5, 13), (36,), (36, 5, 13)}
    # the swapped pair role: the variable under test is the right-hand operand of tas_exceeds_tasmax
    pair = {"tas_exceeds_tasmax": None}
    got = dataflags.data_flags(ds["tasmax"], ds, pair, None, name="tasmax", device=dev)["tas_exceeds_tasmax"]
    np.testing.assert_array_equal(got, ds["tas"] > ds["tasmax"])
    np.testing.assert_array_equal(got, dataflags.tas_exceeds_tasmax(ds["tas"], ds["tasmax"], device=dev))
    assert got.sum() == 1 and got[800, 4, 12]
    assert dataflags.data_flags(ds["tas"], {}, pair, name="tas", device=dev) == {"tas_exceeds_tasmax": None}


def test_the_defaults_of_pr_sfcwind_and_hurs(dev):
    rng = np.random.default_rng(9)
    pr = np.where(rng.random((T, 4, 5)) < 0.5, rng.gamma(1.0, 8.0, (T, 4, 5)), 0.0) / 86400
    pr[100:106, 1, 1] = 5 / 3600 / 24
    pr[200:211, 2, 2] = 1 / 3600 / 24
    pr[300, 3, 4] = 301 / 86400
    wind = np.abs(rng.normal(5, 3, (T, 4, 5))).astype(np.float32)
    wind[50:57, 0, 0] = 3.5
    wind[60:66, 0, 1] = 1.5
    wind[700, 3, 3] = 47.0
    hurs = rng.uniform(5, 100, (T, 4, 5))
    hurs[5, 0, 0] = 100.0000001
    for name, x, units in (("pr", pr, "kg m-2 s-1"), ("sfcWind", wind, "m s-1"), ("hurs", hurs, "%")):
        flags = DEFAULTS[name]["data_flags"]
        for dims, freq in (("all", None), (None, None), ("time", "YS")):
            got = dataflags.data_flags(x, None, flags, dims, freq, name=name, time=TIME, units=units, device=dev)
            want = R.data_flags(x, None, flags, dims, freq, name=name, time=TIME, units=units)
            assert list(got) == list(want)
            for k in got:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} {k} dims={dims} freq={freq}")
    got = dataflags.data_flags(pr, None, DEFAULTS["pr"]["data_flags"], None, name="pr", units="kg m-2 s-1", device=dev)
    assert [int(v.sum()) for v in got.values()] == [0, 1, 6, 11]
    got = dataflags.data_flags(wind, None, DEFAULTS["sfcWind"]["data_flags"], None, name="sfcWind", units="m s-1", device=dev)
    assert got["wind_values_outside_of_bounds"].sum() == 1 and got["values_gt_2_repeating_for_6_or_more_days"].sum() == 7


def test_raise_flags_and_more_than_sixteen_checks(dev):
    ds = mirror_fields(np.float64)
    with pytest.raises(dataflags.DataQualityException) as err:
        dataflags.data_flags(ds["tas"], ds, DEFAULTS["tas"]["data_flags"], raise_flags=True, name="tas", time=TIME, units="K", device=dev)
    assert str(err.value) == ("Data quality flags indicate suspicious values. Flags raised are:\n  - " + "\n  - ".join([
        "Temperatures found in excess of 60 degC in tas.", "Temperatures found below -90 degC in tas.",
        "Mean temperature values found above maximum temperatures.", "Mean temperature values found below minimum temperatures.",
        "Runs of repetitive values for 5 or more days found for tas.",
        "Values outside of 5 standard deviations from climatology found for tas with moving window of 5 days."]))
    clean = {k: v[:, :1, :1] for k, v in mirror_fields(np.float64).items()}
    clean["tas"][30] = clean["tasmax"][30] - 4.0
    kept = [f for f in DEFAULTS["tas"]["data_flags"] if "outside_n_standard_deviations_of_climatology" not in f]
    got = dataflags.data_flags(clean["tas"], clean, kept, raise_flags=True, name="tas", units="K", device=dev)
    assert len(got) == 5 and not any(v.any() for v in got.values())
    # 20 checks, two climatology settings: three launches of xh_data_flags, two of xh_doy_bounds
    many = [{"values_repeating_for_n_or_more_days": {"n": n}} for n in range(2, 20)]
    many += [{"outside_n_standard_deviations_of_climatology": {"n": n, "window": w}} for n, w in ((5, 5), (4, 7))]
    trace = dev.start_trace()
    try:
        got = dataflags.data_flags(ds["tas"], ds, many, "cells", "YS", name="tas", time=TIME, units="K", device=dev)
    finally:
        dev.stop_trace()
    assert sorted(n for n, _ in trace if n in FLAGS_TABLE) == ["xh_data_flags"] * 3 + ["xh_doy_bounds"] * 2
    want = R.data_flags(ds["tas"], ds, many, "cells", "YS", name="tas", time=TIME, units="K")
    assert list(got) == list(want) and len(got) == 20
    for k in got:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
