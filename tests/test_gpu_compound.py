"""The compound-extreme unit on the device (xclim_amd/csrc/compound.hip, xclim_amd.compound) against
tests/golden/compound_vectors.npz, the values of the numpy restatement tests/compoundcpu.py: every family of decisions at ``MS``,
``YS``, ``YS-JUL`` and ``QS-DEC``, float32 and float64 fields, 3 years x 1, 65 and 130 cells (one lane, one wave plus one, and the
16-byte tail), padded and offset row views, the fused four-output launch against the four single launches, absent outputs, kept
results, the missing mask and the refusals.  Every test runs on poisoned output buffers (tests/poisoned.py).

Every result is an integer, a day of year, an exact sum or NaN, and every comparison is ``assert_array_equal``: the built families
lie on grids on which every sum is exact in any order and precision, and the random float32 families keep 1e-6 relative between
every sum (or sample) and its threshold, which tests/test_compound_cpu.py asserts."""
import numpy as np
import pytest

import compoundcpu as CC
from poisoned import poisoned_outputs, unwritten  # noqa: F401  (autouse: the tests of this module run on poisoned output buffers)
from test_compound_cpu import (CASES, COUNTS, META, TABLES, TABLE_ARGS, check_known_answers, get, golden_otime, golden_time, mirror_api,
                               refusals, same, tile)
from xclim_amd import compound
from xclim_amd import kernels as K
from xclim_amd._capi import DeviceArray
from xclim_amd.calendar import DoyPercentile

pytestmark = pytest.mark.gpu
CELLS = (1, 65, 130)
DTYPES = [np.float32, np.float64]
IDS = ["float32", "float64"]
FREQS = ("MS", "YS", "YS-JUL", "QS-DEC")
OUT = {n: compound.COMPOUND_OUTPUTS[n] for n in COUNTS}   # the reference's name -> the kernel's


# ---- views: a (R, C) block inside a larger poisoned or 1e30-filled buffer -----------------------------------------------------------
def _view(dev, flat, off, R, ld):
    v = DeviceArray(dev, flat.ptr + off * flat.dtype.itemsize, (R, ld), flat.dtype, owner=False)
    v._owner = flat
    return v


def _padded(dev, a, ld, off):
    """The (R, C) host array as a (R, ld) device view that begins ``off`` elements into its buffer; every element of the buffer
    outside the (R, C) block is 1e30."""
    R, C = a.shape
    host = np.full(R * ld + off + 4, 1e30, a.dtype)
    host[off:off + R * ld].reshape(R, ld)[:, :C] = a
    return _view(dev, dev.to_device(host), off, R, ld)


def _output(dev, R, ld, off):
    flat = dev.empty((R * ld + off + 4,), np.float64)   # (poisoned by the module's fixture)
    return flat, _view(dev, flat, off, R, ld)


def _written(flat, off, R, C, ld):
    """The (R, C) block of a downloaded output buffer, after asserting that nothing outside it was written and all of it was."""
    host = flat.get()
    block = host[off:off + R * ld].reshape(R, ld)
    mask = np.zeros(host.shape, bool)
    mask[off:off + R * ld].reshape(R, ld)[:, :C] = True
    assert unwritten(host[~mask]).all(), "an element outside the (R, C) block was written"
    assert not unwritten(block[:, :C]).any(), "an element of the (R, C) block was not written"
    return block[:, :C].copy()


# ---- xh_compound_doy_days ---------------------------------------------------------------------------------------------------------
def compound_inputs(name, cells, dtype):
    m = META[name]
    use = m["use"]
    tas, pr = tile(get(name, "tas"), cells, use).astype(dtype), tile(get(name, "pr"), cells, use).astype(dtype)
    tabs = {k: tile(get(name, k), cells, use) for k in K.CD_TABLES}
    return m, tas, pr, tabs, golden_time(m["axis"])


def expected(name, key, cells):
    return tile(get(name, key), cells, META[name]["use"])


@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES["compound"])
def test_compound_days_golden(dev, name, dtype, cells):
    """The mirror on every case: 366-row tables, 365-row tables re-gridded on the device, a noleap axis, random float32 fields;
    the fused launch at every frequency, and each of the four functions alone at one."""
    m, tas, pr, tabs, t = compound_inputs(name, cells, dtype)
    pers = {TABLE_ARGS[k]: v for k, v in tabs.items()}
    for freq in FREQS:
        got = compound.compound_days(tas, pr, **pers, freq=freq, time=t, device=dev)
        assert list(got) == list(COUNTS)
        for n in COUNTS:
            same(got[n], expected(name, f"{freq}/{n}", cells), f"{name} {freq} {n}")
    for n in COUNTS:
        a, b = TABLES[n]
        same(getattr(compound, n)(tas, pr, tabs[a], tabs[b], "YS-JUL", time=t, device=dev), expected(name, f"YS-JUL/{n}", cells), f"{name} {n} alone")


def _kernel_case(dev, name, cells, dtype, freq="MS"):
    m, tas, pr, tabs, t = compound_inputs(name, cells, dtype)
    assert m["ndoy"] == 366 and m["axis"] == "std"
    seg = t.segments(freq)[0]
    tidx = (t.doy - 1).astype(np.int32)
    return tas, pr, tabs, tidx, seg


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["compound.tab366", "compound.random"])
def test_the_fused_launch_equals_every_subset_bit_for_bit(dev, name, dtype):
    tas, pr, tabs, tidx, seg = _kernel_case(dev, name, 130, dtype)
    d = {k: dev.to_device(v) for k, v in dict(tabs, tas=tas, pr=pr).items()}
    dt = {k: d[k] for k in K.CD_TABLES}
    full = {o: v.get() for o, v in K.compound_doy_days(dev, d["tas"], d["pr"], dt, tidx, seg, list(OUT.values())).items()}
    assert list(full) == list(OUT.values())
    for n, o in OUT.items():
        same(full[o], expected(name, f"MS/{n}", 130), f"{name} fused {n}")
    for mask in range(1, 16):
        names = [o for i, o in enumerate(OUT.values()) if mask >> i & 1]
        need = {t for o in names for t in K.CD_NEEDS[o]}
        got = K.compound_doy_days(dev, d["tas"], d["pr"], {k: dt[k] for k in need}, tidx, seg, names)   # only what they need is passed
        assert list(got) == names
        for o in names:
            same(got[o].get(), full[o], f"{name} {names}: {o}")


@pytest.mark.parametrize("cells", [1, 3, 4, 5, 65, 130])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_compound_days_on_padded_and_offset_views(dev, dtype, cells):
    """Row pitches that keep and that break the 16-byte lanes, a base pointer off the 16-byte grid, outputs in rows of another
    pitch: the same bits, the padding and everything around the blocks untouched; absent outputs are NULL and nothing but the
    requested blocks is written."""
    tas, pr, tabs, tidx, seg = _kernel_case(dev, "compound.tab366", cells, dtype, "QS-DEC")
    P, lane = len(seg) - 1, 16 // np.dtype(dtype).itemsize
    dense = K.compound_doy_days(dev, dev.to_device(tas), dev.to_device(pr), {k: dev.to_device(v) for k, v in tabs.items()}, tidx, seg, list(OUT.values()))
    dense = {o: v.get() for o, v in dense.items()}
    for n, o in OUT.items():
        same(dense[o], expected("compound.tab366", f"QS-DEC/{n}", cells), f"dense {n}")
    for ld, ldt, ldo, off in ((cells + 3, cells + 1, cells + 3, 0), (cells + lane, cells + 2, cells + 2 * lane, 0), (cells + lane, cells + 2, cells + lane, 1)):
        f = {k: _padded(dev, v, ld, off) for k, v in (("tas", tas), ("pr", pr))}
        tb = {k: _padded(dev, v, ldt, 2 * off) for k, v in tabs.items()}
        bufs = {o: _output(dev, P, ldo, off) for o in OUT.values()}
        K.compound_doy_days(dev, f["tas"], f["pr"], tb, tidx, seg, list(OUT.values()), C_=cells, ld=ld, ld_tab=ldt,
                            outs={o: v for o, (_, v) in bufs.items()}, ld_out=ldo)
        for o in OUT.values():
            same(_written(bufs[o][0], off, P, cells, ldo), dense[o], f"{o} ld={ld} off={off}")
        for o in OUT.values():   # alone: the other three pointers are NULL, the tables it does not need as well
            flat, view = _output(dev, P, ldo, off)
            K.compound_doy_days(dev, f["tas"], f["pr"], {k: tb[k] for k in K.CD_NEEDS[o]}, tidx, seg, [o], C_=cells, ld=ld, ld_tab=ldt,
                                outs={o: view}, ld_out=ldo)
            same(_written(flat, off, P, cells, ldo), dense[o], f"{o} alone ld={ld} off={off}")


def test_compound_days_argument_errors_leave_the_outputs_untouched(dev):
    tas, pr, tabs, tidx, seg = _kernel_case(dev, "compound.tab366", 5, np.float32)
    d = {k: dev.to_device(v) for k, v in dict(tabs, tas=tas, pr=pr).items()}
    dt = {k: d[k] for k in K.CD_TABLES}
    out = dev.empty((len(seg) - 1, 5), np.float64)
    bad = tidx.copy()
    bad[700] = 366
    with pytest.raises(Exception, match="outside the table"):
        K.compound_doy_days(dev, d["tas"], d["pr"], dt, bad, seg, ["cold_dry"], outs={"cold_dry": out})
    with pytest.raises(Exception, match="needs time-major rows"):
        K.compound_doy_days(dev, d["tas"], d["pr"], dt, tidx, seg, ["cold_dry"], outs={"cold_dry": out}, C_=5, ld=4)
    with pytest.raises(Exception, match="ld_tab"):
        K.compound_doy_days(dev, d["tas"], d["pr"], dt, tidx, seg, ["cold_dry"], outs={"cold_dry": out}, ld_tab=4)
    assert unwritten(out.get()).all()
    # empty periods count nothing; no period and no cell launch nothing
    seg2 = np.array([0, 0, seg[1], seg[1], seg[2]])
    got = K.compound_doy_days(dev, d["tas"], d["pr"], dt, tidx, seg2, ["warm_wet"])["warm_wet"].get()
    same(got[[0, 2]], np.zeros((2, 5)), "empty periods")
    same(got[[1, 3]], expected("compound.tab366", "MS/warm_and_wet_days", 5)[:2], "between empty periods")


# ---- xh_degree_exceedance_date ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES["dded"])
def test_exceedance_date_golden(dev, name, dtype, cells):
    m, t = META[name], golden_time("std")
    tas = tile(get(name, "tas"), cells).astype(dtype)
    for s, p in m["sets"].items():
        for freq in p["freqs"]:
            got = compound.degree_days_exceedance_date(tas, m["thresh"], m["sum_thresh"], p["op"], p["after_date"], p["never_reached"], freq,
                                                       time=t, device=dev)
            same(got, tile(get(name, f"{s}/{freq}"), cells), f"{name} {s} {freq}")


def test_exceedance_date_in_celsius_negative_and_nan_thresholds(dev):
    """The same field in degC with the threshold in degC (the grid is exact in both); a negative ``sum_thresh`` is exceeded by the
    0 of the period's first row, which is the reference's all-rows-marked NaN; a NaN ``sum_thresh`` is never exceeded and never
    "never reached"."""
    m, t, ot = META["dded.built"], golden_time("std"), golden_otime("std")
    tas = tile(get("dded.built", "tas"), 65)
    got = compound.degree_days_exceedance_date(tas - 273.0, m["thresh"] - 273.0, m["sum_thresh"], after_date="04-15", time=t, units="degC", device=dev)
    same(got, tile(get("dded.built", "apr15/YS"), 65), "degC")
    default = compound.degree_days_exceedance_date(tas - 273.15, time=t, units="degC", device=dev)
    same(default, CC.degree_days_exceedance_date(tas - 273.15, ot, 0.0, 25.0), "the default threshold, 0 degC")
    for st in (-1.0, np.nan):
        for never in (None, 300):
            got = compound.degree_days_exceedance_date(tas, m["thresh"], st, never_reached=never, time=t, device=dev)
            same(got, CC.degree_days_exceedance_date(tas, ot, m["thresh"], st, never_reached=never), f"sum_thresh={st} never={never}")
            assert np.isnan(got).all()


# ---- xh_blowing_snow_days ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES["snow"])
def test_blowing_snow_golden(dev, name, dtype, cells):
    m, t = META[name], golden_time("std")
    snd, wind = tile(get(name, "snd"), cells).astype(dtype), tile(get(name, "sfcWind"), cells).astype(dtype)
    for i, indexer in m["indexers"].items():
        for freq in FREQS:
            got = compound.blowing_snow(snd, wind, m["snd_thresh"], m["sfcWind_thresh"], m["window"], freq, time=t, device=dev, **indexer)
            same(got, tile(get(name, f"{i}/{freq}"), cells), f"{name} {i} {freq}")


def test_blowing_snow_drops_the_period_of_the_lone_first_row(dev):
    """``diff`` drops row 0: a series that begins on the last day of a period has no such period in the result."""
    m = META["snow.w3"]
    snd, wind = get("snow.w3", "snd")[21:], get("snow.w3", "sfcWind")[21:]        # 1999-03-31: alone in March
    t, ot = golden_time("std").subset(slice(21, None)), golden_otime("std").isel(slice(21, None))
    assert (t.month[0], t.day[0]) == (3, 31)
    for freq, first in (("MS", 1), ("YS", 0)):
        want = CC.blowing_snow(snd, wind, ot, m["snd_thresh"], m["sfcWind_thresh"], 3, freq)
        assert len(want) == len(t.segments(freq)[0]) - 1 - first
        same(compound.blowing_snow(snd, wind, m["snd_thresh"], m["sfcWind_thresh"], 3, freq, time=t, device=dev), want, freq)
        same(compound.blowing_snow(snd, wind, m["snd_thresh"], m["sfcWind_thresh"], 3, freq, time=t, device=dev, keep=True).get(), want, f"{freq} kept")


# ---- xh_pair_period_sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", CASES["wci"])
def test_water_cycle_intensity_golden(dev, name, dtype, cells):
    t = golden_time("std")
    pr, ev = tile(get(name, "pr"), cells).astype(dtype), tile(get(name, "evspsbl"), cells).astype(dtype)
    for freq in FREQS:
        same(compound.water_cycle_intensity(pr, ev, freq, time=t, device=dev), tile(get(name, freq), cells), f"{name} {freq}")
    per_day = compound.water_cycle_intensity(pr * dtype(64.0), ev * dtype(64.0), "YS", time=t, flux_units="mm/d", device=dev)
    same(per_day, CC.water_cycle_intensity(pr * dtype(64.0), ev * dtype(64.0), golden_otime("std"), "YS", "mm/d"), "mm/d")


# ---- the three period kernels on padded and offset views --------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [1, 65, 130])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_period_kernels_on_padded_and_offset_views(dev, dtype, cells):
    t = golden_time("std")
    seg = t.segments("YS-JUL")[0]
    P = len(seg) - 1
    tas = tile(get("dded.built", "tas"), cells).astype(dtype)
    snd, wind = tile(get("snow.w32", "snd"), cells).astype(dtype), tile(get("snow.w32", "sfcWind"), cells).astype(dtype)
    pr, ev = tile(get("wci.built", "pr"), cells).astype(dtype), tile(get("wci.built", "evspsbl"), cells).astype(dtype)
    start, never = compound.exceedance_tables(t, seg, "04-15", 300)
    flags = compound.select_time_mask(t, month=[12, 1, 2])
    calls = {
        "dded": lambda f, **kw: K.degree_exceedance_date(dev, f(tas), seg, start, never, t.doy, thresh=278.0, sum_thresh=200.0, **kw),
        "snow": lambda f, **kw: K.blowing_snow_days(dev, f(snd), f(wind), seg, flags, snd_thresh=0.5, wind_thresh=4.0, window=32, **kw),
        "wci": lambda f, **kw: K.pair_period_sum(dev, f(pr), f(ev), seg, 86400.0, **kw),
    }
    want = {"dded": tile(CC.degree_days_exceedance_date(get("dded.built", "tas"), golden_otime("std"), 278.0, 200.0, after_date="04-15", never_reached=300, freq="YS-JUL"), cells),
            "snow": tile(get("snow.w32", "winter/YS-JUL"), cells), "wci": tile(get("wci.built", "YS-JUL"), cells)}
    for k, call in calls.items():
        dense = call(dev.to_device).get()
        same(dense, want[k], f"{k} dense")
        for ld, ldo, off in ((cells + 3, cells + 5, 0), (cells + 4, cells + 4, 1)):
            flat, view = _output(dev, P, ldo, off)
            call(lambda a: _padded(dev, a, ld, off), C_=cells, ld=ld, out=view, ld_out=ldo)
            same(_written(flat, off, P, cells, ldo), dense, f"{k} ld={ld} off={off}")


def test_period_kernels_argument_errors(dev):
    t = golden_time("std")
    seg = t.segments("YS")[0]
    x = dev.to_device(np.full((len(t), 4), 280.0, np.float32))
    out = dev.empty((len(seg) - 1, 4), np.float64)
    start, never = compound.exceedance_tables(t, seg, None, None)
    with pytest.raises(Exception, match="neither -1 nor a row of its period"):
        K.degree_exceedance_date(dev, x, seg, start + 400, never, t.doy, thresh=0.0, sum_thresh=1.0, out=out)
    with pytest.raises(Exception, match="outside 1 .. 366"):
        K.degree_exceedance_date(dev, x, seg, start, never, np.zeros(len(t)), thresh=0.0, sum_thresh=1.0, out=out)
    with pytest.raises(Exception, match="needs time-major rows"):
        K.blowing_snow_days(dev, x, x, seg, snd_thresh=0.5, wind_thresh=4.0, out=out, C_=4, ld=3)
    with pytest.raises(Exception, match="needs time-major rows"):
        K.pair_period_sum(dev, x, x, seg, out=out, ld_out=3)
    assert unwritten(out.get()).all()
    nothing = K.degree_exceedance_date(dev, x, seg, np.full(len(seg) - 1, -1), never, t.doy, thresh=0.0, sum_thresh=1.0).get()
    assert np.isnan(nothing).all()          # no period holds the date


# ---- the reference's known answers, kept results, the missing mask, the refusals -----------------------------------------------------
def test_known_answers_on_the_device(dev):
    check_known_answers(mirror_api(dev))


def test_kept_results_feed_the_next_call_without_a_host_copy(dev):
    """Fields and tables on the device, ``keep=True``: the results are device arrays, and a call on them uploads nothing but its
    small host tables."""
    m, tas, pr, tabs, t = compound_inputs("compound.tab366", 130, np.float32)
    d = {k: dev.to_device(v) for k, v in dict(tabs, tas=tas, pr=pr).items()}
    pers = {TABLE_ARGS[k]: DoyPercentile(d[k].reshape(1, 366, 130), np.arange(1, 367), [25.0], (130,), {}) for k in K.CD_TABLES}
    trace = dev.start_trace()
    try:
        kept = compound.compound_days(d["tas"], d["pr"], **pers, freq="MS", time=t, device=dev, keep=True)
        wci = compound.water_cycle_intensity(d["pr"], d["pr"], "MS", time=t, device=dev, keep=True)
        total = K.pair_period_sum(dev, kept["cold_and_dry_days"], kept["warm_and_wet_days"], [0, 12, 24, 37])     # a kept result as a field
    finally:
        dev.stop_trace()
    assert [n for n, _ in trace if n.startswith("xh_")] == ["xh_compound_doy_days", "xh_pair_period_sum", "xh_pair_period_sum"]
    assert not [a for n, a in trace if n == "h2d" and a[0] >= tas.nbytes // 4], "a field or a table was uploaded again"
    assert all(isinstance(v, DeviceArray) and v.shape == (37, 130) for v in kept.values()) and isinstance(wci, DeviceArray)
    for n in COUNTS:
        same(kept[n].get(), expected("compound.tab366", f"MS/{n}", 130), f"kept {n}")
    both = expected("compound.tab366", "MS/cold_and_dry_days", 130) + expected("compound.tab366", "MS/warm_and_wet_days", 130)
    same(total.get(), np.stack([both[0:12].sum(0), both[12:24].sum(0), both[24:37].sum(0)]), "the sum of two kept counts")


def test_missing_mask(dev):
    """MissingAny on the downloaded results: a period with a NaN row in either field, and the two periods the series cuts."""
    m, tas, pr, tabs, t = compound_inputs("compound.tab366", 65, np.float64)
    full_t, full_p = np.where(np.isnan(tas), 280.0, tas), np.where(np.isnan(pr), 0.0, pr)
    full_t[400, 1] = np.nan
    full_p[800, 2] = np.nan
    pers = {TABLE_ARGS[k]: v for k, v in tabs.items()}
    plain = compound.compound_days(full_t, full_p, **pers, freq="YS", time=t, device=dev)
    masked = compound.compound_days(full_t, full_p, **pers, freq="YS", time=t, device=dev, mask_missing=True)
    for n in COUNTS:
        assert np.isnan(masked[n][[0, 3]]).all() and np.isnan(masked[n][1, 1]) and np.isnan(masked[n][2, 2])
        keep = np.ones((4, 65), bool)
        keep[[0, 3]] = False
        keep[1, 1] = keep[2, 2] = False
        same(masked[n][keep], plain[n][keep], f"{n}: complete periods are kept")
    d = compound.degree_days_exceedance_date(full_t, 278.0, 200.0, time=t, device=dev, mask_missing=True)
    w = compound.water_cycle_intensity(full_p, full_p, "YS", time=t, device=dev, mask_missing=True)
    s = compound.blowing_snow(full_t, full_p, 0.5, 0.0, 3, "YS", time=t, device=dev, mask_missing=True)
    assert np.isnan(d[1, 1]) and not np.isnan(d[1, 0]) and np.isnan(w[2, 2]) and not np.isnan(w[1, 2])
    assert np.isnan(s[[0, 3]]).all() and np.isnan(s[1, 1]) and np.isnan(s[2, 2]) and not np.isnan(s[1:3, 5:]).any()


def test_refusals(dev):
    refusals(dev)
    x = np.zeros((10, 2), np.float32)
    with pytest.raises(TypeError, match="share one dtype"):
        compound.water_cycle_intensity(dev.to_device(x), dev.to_device(x.astype(np.float64)), time=golden_time("std").subset(slice(0, 10)), device=dev)
