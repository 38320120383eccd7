"""GPU parity of the one-year sliding percentile_doy kernel (k_pdoy_slide) where its doy chunks MEET.  The kernel cuts the year
into chunks, each with a prologue of W - 1 halo rows; nothing else in the suite moves the chunk boundaries.  Here: series of 1 to
365 days against forced chunk lengths (partial last chunk, a single chunk, a series shorter than a chunk, a chunk shorter than
the halo), cell counts that leave partial waves and workgroups and the 1-cell-per-lane fallback, windows 3 / 5 / 7, both fast
modes and the sorting path, NaN and infinite samples placed ON the chunk boundaries, misaligned buffers, and the fused count,
whose chunks cross the period boundaries.  Everything bitwise.

Written with the round-27 geometry (four consecutive chunks per workgroup, every other wave marching backwards, the rows around
a boundary shared through LDS: DESIGN.md §7), which passed it and was not kept because it was slower; a later attempt at the
chunk boundaries has these cases to pass: groups of four chunks (partial last group, a group of one chunk) are among them."""

import numpy as np
import pytest

from oracle import calendar as ocal
from oracle import quantile as oq
from oracle.timeutil import OTime
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK = (10, 32)    # pdoy_impl (quantile.hip): 10 days where no window is sorted, else 32
DEFAULT_COUNT_CHUNK = 61    # pdoy_count_impl
LENGTHS = [1, 2, 4, 5, 8, 9, 31, 32, 33, 127, 128, 129, 365]
CHUNKS = [None, 1, 2, 3, 5, 8]
CELLS = [1, 2, 3, 255, 256, 257, 258, 511, 513, 1026]
PERS8 = [1.0, 5.0, 10.0, 25.0, 50.0, 75.0, 90.0, 99.0]


def _force_chunk(monkeypatch, chunk):
    """Both instances read their chunk length from the environment under XH_DIAGNOSTICS=1, at every call."""
    if chunk is None:
        monkeypatch.delenv("XH_PDOY_SLIDE_CHUNK", raising=False)
        monkeypatch.delenv("XH_PDOY_SLIDE_COUNT_CHUNK", raising=False)
        return
    monkeypatch.setenv("XH_DIAGNOSTICS", "1")
    monkeypatch.setenv("XH_PDOY_SLIDE_CHUNK", str(chunk))
    monkeypatch.setenv("XH_PDOY_SLIDE_COUNT_CHUNK", str(chunk))


def _axes(T):
    return TimeAxis.daily("2001-01-01", T, "noleap"), OTime.noleap(2001, T, "noleap")


def _put(x, row, col, value):
    if 0 <= row < x.shape[0]:
        x[row, col] = value


def _field(rng, T, C, chunk, nan_frac=0.01):
    """A year of temperatures with the special samples ON every chunk boundary b (columns rotate with the boundary, so a
    short chunk does not fill a column): a NaN run over rows b-3 .. b+2, a single NaN at b-1, one at b, -inf at b, +inf at
    b-1; one all-NaN column.  (Fewer than 16 cells: the random NaNs only.)"""
    t = np.arange(T)[:, None]
    x = (288 + 12 * np.sin(2 * np.pi * (t - 100) / 365) + rng.normal(0, 3, (T, C))).astype(np.float32)
    x[rng.random((T, C)) < nan_frac] = np.nan
    if C < 16:
        return x
    n = C - 1                      # column C - 1 is the all-NaN one
    chunks = chunk if isinstance(chunk, tuple) else (chunk,)
    for i, b in enumerate(sorted({b for c in chunks for b in range(c, T + 1, c)})):
        c = 5 * i
        for r in range(b - 3, b + 3):
            _put(x, r, c % n, np.nan)
        _put(x, b - 1, (c + 1) % n, np.nan)
        _put(x, b, (c + 2) % n, np.nan)
        _put(x, b, (c + 3) % n, -np.inf)
        _put(x, b - 1, (c + 4) % n, np.inf)
    x[:, C - 1] = np.nan
    return x


def _oracle(x, window, per):
    T = x.shape[0]
    ta, ot = _axes(T)
    tb, years, doys = ta.doy_table()
    C = x.shape[1]
    rr = ocal.rolling_construct_center(x, window)
    stack = np.full((len(doys), len(years), C, window), np.nan, dtype=np.float32)
    stack[np.searchsorted(doys, ot.doy), np.searchsorted(years, ot.year)] = rr
    stack = np.moveaxis(stack, 1, -2).reshape(len(doys), C, len(years) * window)
    return np.moveaxis(oq.calc_perc(stack, per, 1 / 3, 1 / 3), -1, 0)  # (nper, ndoy, C)


def _pdoy(dev, xd, T, window, per, out=None):
    tb, _, _ = _axes(T)[0].doy_table()
    return K.percentile_doy(dev, xd, tb, window, per, out=out).get()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("T", LENGTHS)
def test_series_length_against_chunk(dev, rng, monkeypatch, T, chunk):
    """Partial last chunk, one chunk, up to 365 chunks, a series shorter than a chunk, a chunk shorter than the W - 1 = 4 halo
    rows; per 90 / 5 clip to the window maximum / minimum (fast modes 1 / 2: the -inf on a boundary sends the minimum through
    the nanmax rule), per 50 sorts.  258 cells: two waves, the second one a single cell pair."""
    _force_chunk(monkeypatch, chunk)
    x = _field(rng, T, 258, chunk or DEFAULT_CHUNK)
    xd = dev.to_device(x)
    for per in ([90.0], [5.0], [50.0]):
        np.testing.assert_array_equal(_pdoy(dev, xd, T, 5, per), _oracle(x, 5, per), err_msg=str(per))


@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("C", CELLS)
def test_cells_against_workgroups(dev, rng, monkeypatch, C, chunk):
    """A wave past C, the last pair of a row, odd C (one cell per lane)."""
    _force_chunk(monkeypatch, chunk)
    x = _field(rng, 365, C, chunk or DEFAULT_CHUNK)
    np.testing.assert_array_equal(_pdoy(dev, dev.to_device(x), 365, 5, [90.0]), _oracle(x, 5, [90.0]))


@pytest.mark.parametrize("chunk", [None, 2, 5])
@pytest.mark.parametrize("per", [[90.0], [5.0], [50.0], PERS8])
@pytest.mark.parametrize("window", [3, 5, 7])
def test_windows_and_percentiles(dev, rng, monkeypatch, window, per, chunk):
    """(chunk 2 is shorter than the halo of every window, chunk 5 than that of window 7)"""
    _force_chunk(monkeypatch, chunk)
    T, C = 129, 258
    x = _field(rng, T, C, chunk or DEFAULT_CHUNK, nan_frac=0.02)
    np.testing.assert_array_equal(_pdoy(dev, dev.to_device(x), T, window, per), _oracle(x, window, per))


@pytest.mark.parametrize("chunk", [None, 3])
def test_nan_free_block_and_all_nan_block(dev, rng, monkeypatch, chunk):
    """The 256 cells of a wave without a NaN take the wave-uniform paths across every boundary; a block of all-NaN cells and
    the blocks with the NaN runs across the boundaries take the per-lane path."""
    _force_chunk(monkeypatch, chunk)
    T, C = 365, 1024 + 2
    x = _field(rng, T, C, chunk or DEFAULT_CHUNK, nan_frac=0.0)
    t = np.arange(T)[:, None]
    x[:, 256:512] = (288 + 12 * np.sin(2 * np.pi * (t - 100) / 365) + rng.normal(0, 3, (T, 256))).astype(np.float32)
    x[:, 512:768] = np.nan
    xd = dev.to_device(x)
    for per in ([90.0], [5.0], [50.0]):
        np.testing.assert_array_equal(_pdoy(dev, xd, T, 5, per), _oracle(x, 5, per), err_msg=str(per))


@pytest.mark.parametrize("chunk", [None, 5])
@pytest.mark.parametrize("x_off,out_off", [(4, 0), (0, 8), (4, 8)])
def test_misaligned_buffers(dev, rng, monkeypatch, x_off, out_off, chunk):
    """The field 4 bytes off, the output 8 bytes off: one cell per lane, bit-identical to the aligned call and to the oracle."""
    _force_chunk(monkeypatch, chunk)
    T, C, per = 365, 1026, [5.0, 50.0, 90.0]
    x = _field(rng, T, C, chunk or DEFAULT_CHUNK)
    ref = _pdoy(dev, dev.to_device(x), T, 5, per)
    np.testing.assert_array_equal(ref, _oracle(x, 5, per))
    pad = x_off // 4
    big = np.zeros(T * C + 4, np.float32)
    big[pad: pad + T * C] = x.reshape(-1)
    dbig = dev.to_device(big)
    xv = dev.wrap(dbig.ptr + x_off, (T, C), np.float32)
    obig = dev.empty((len(per) * T * C + 2,), np.float64)
    ov = dev.wrap(obig.ptr + out_off, (len(per), T, C), np.float64)
    np.testing.assert_array_equal(_pdoy(dev, xv, T, 5, per, out=ov), ref)


@pytest.mark.parametrize("chunk", [None, 1, 3, 8])
@pytest.mark.parametrize("freq", ["YS", "MS"])
@pytest.mark.parametrize("per,op", [(90.0, ">"), (5.0, "<"), (50.0, ">=")])
def test_count_instance(dev, rng, monkeypatch, per, op, freq, chunk):
    """xh_percentile_doy_count (k_pdoy_slide<.., COUNT>) = percentile_doy -> threshold_count on the same field.  Months change
    inside a chunk, whose partial counts are flushed with atomics at every change: the counts are integers, so they are exact.
    258 cells in pairs, 257 one per lane."""
    _force_chunk(monkeypatch, chunk)
    T = 365
    ta, _ = _axes(T)
    tb, _, doys = ta.doy_table()
    seg, _ = ta.segments(freq)
    P = len(seg) - 1
    tidx = np.searchsorted(doys, ta.doy).astype(np.int32)
    period = (np.searchsorted(seg, tb, side="right") - 1).astype(np.int32)
    for C in (258, 257):
        x = _field(rng, T, C, chunk or DEFAULT_COUNT_CHUNK)
        xd = dev.to_device(x)
        p = K.percentile_doy(dev, xd, tb, 5, [per])
        cnt, val = K.threshold_count(dev, xd, op, seg, doy_table=p.reshape(len(doys), C), tidx=tidx)
        fused = K.percentile_doy_count(dev, xd, tb, 5, per, op, period, P)
        assert fused is not None
        np.testing.assert_array_equal(fused[0].get(), cnt.get())
        np.testing.assert_array_equal(fused[1].get(), val.get())
