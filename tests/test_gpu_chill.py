"""The winter-chill indices on the device (xh_chill_hourly, xh_chill_daily, xclim_amd.chill) against the reference's own
outputs (tests/golden/chill_vectors.npz) and, where no golden output exists, against the numpy restatement tests/chillcpu.py;
both entry points on padded, poisoned row views (tests/stridedabi.py); the adapter (patch.install) through a stand-in
``xclim.indices._agro`` module.

Tolerances.  float64 marches against the reference's float64 run: RTOL = 1e-12 relative and the same release pattern
``delta > 0`` (tests/test_chill_cpu.py: the golden file guarantees min |E - 1| >= 1e-9, so a 1-ulp exp cannot flip a release).
float32 fields: the same against the reference's run on the widened values; against its own float32 run the device may be
at most twice as far from it, per period sum, as the reference's float64 run is (the device result is one rounding of
the float64 one).  Chill units are sums of halves: exact.  The fused path against the hourly path on its own hourly
temperatures: bit for bit."""

import ctypes
import types

import numpy as np
import pytest

import chillcpu
import fakexr
import stridedabi as S
from stridedabi import CHILL_TABLE
from test_chill_cpu import DAILY, HOURLY, K2C, RTOL, check_delta, check_sums, golden_case, nan_empty
from xclim_amd import chill, converters, patch
from xclim_amd import kernels as K
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
_vp = ctypes.c_void_p


def _host(outs):
    return {k: v.get() for k, v in outs.items()}


# ---- the golden cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOURLY)
def test_hourly_matches_reference(dev, name):
    c = golden_case(name)
    seg = 24 * c.seg
    d = dev.to_device(c.tas)
    got = _host(K.chill_hourly(dev, d, seg, c.rows_sel(), add_K=c.add_K, sub_C=c.sub_C, outputs=("cp", "cu", "valid", "delta")))
    check_delta(got["delta"][:, c.cells], c.g["delta"])
    check_sums(nan_empty(got["cp"], c), c.g["cp"])
    _, _, valid = chillcpu.portions(c.kelvin(c.tas), seg, c.rows_sel())
    np.testing.assert_array_equal(got["valid"], valid)
    if "cu" in c.g:
        np.testing.assert_array_equal(got["cu"], c.g["cu"])
        pos = _host(K.chill_hourly(dev, d, seg, add_K=c.add_K, sub_C=c.sub_C, positive_only=True, outputs=("cu",)))["cu"]
        np.testing.assert_array_equal(pos, c.g["cu_pos"])
    if c.dtype == np.float32:
        # against the reference's own float32 run: at most twice as far from it as its float64 run is, plus the float64 bar
        cp32, gap = c.g["cp32"].astype(np.float64), c.g["gap32"]
        far = np.abs(got["cp"] - cp32)
        print(f"{name}: |dev - ref32| max {far.max():.3e}, |ref64 - ref32| max {gap.max():.3e}, relative {(gap / np.maximum(np.abs(c.g['cp']), 1e-300)).max():.3e}")
        assert (far <= 2 * gap + RTOL * np.abs(c.g["cp"])).all()
    # the host mirror: the same numbers on the periods of the daily axis, NaN where no hour is selected
    cp = chill.chill_portions(c.tas, c.time, c.freq, units=c.units, device=dev, **c.indexer)
    np.testing.assert_array_equal(cp, nan_empty(got["cp"], c))
    if "cu" in c.g:
        np.testing.assert_array_equal(chill.chill_units(c.tas, c.time, False, c.freq, units=c.units, device=dev), c.g["cu"])
        np.testing.assert_array_equal(chill.chill_units(c.tas, c.time, True, c.freq, units=c.units, device=dev), c.g["cu_pos"])


def _daily_device(dev, c, dl, li, positive_only=False, sel=None, seg=None):
    outs = K.chill_daily(dev, dev.to_device(c.tasmin), dev.to_device(c.tasmax), dev.to_device(np.ascontiguousarray(dl)), li,
                         c.seg if seg is None else seg, sel, add_K=c.add_K, sub_C=c.sub_C, positive_only=positive_only,
                         outputs=("cp", "cu", "valid", "hourly"))
    return outs


@pytest.mark.parametrize("name", DAILY)
def test_daily_matches_reference_and_the_hourly_path_bitwise(dev, name):
    """xh_chill_daily on the reference's own day lengths: make_hourly_temperature and the two indices of its result; then
    xh_chill_hourly on the fused path's own hourly_out: cp, cu and valid bit for bit."""
    c = golden_case(name)
    li = np.arange(c.tasmin.shape[1], dtype=np.int32)
    for positive_only in (False, True):
        outs = _daily_device(dev, c, c.dl, li, positive_only)
        got = _host(outs)
        if not positive_only:
            np.testing.assert_array_equal(np.isnan(got["hourly"]), np.isnan(c.hourly))
            np.testing.assert_allclose(got["hourly"], c.hourly, rtol=RTOL, atol=0, equal_nan=True)
            check_sums(got["cp"], c.g["cp"])
            _, delta, valid = chillcpu.portions(c.kelvin(c.hourly), 24 * c.seg)
            np.testing.assert_array_equal(got["valid"], valid)
        np.testing.assert_array_equal(got["cu"], c.g["cu_pos" if positive_only else "cu"])
        again = _host(K.chill_hourly(dev, outs["hourly"], 24 * c.seg, add_K=c.add_K, sub_C=c.sub_C, positive_only=positive_only,
                                     outputs=("cp", "cu", "valid", "delta")))
        for k in ("cp", "cu", "valid"):
            np.testing.assert_array_equal(again[k].view(np.int64 if k != "valid" else np.int32),
                                          got[k].view(np.int64 if k != "valid" else np.int32), err_msg=k)
        if not positive_only:
            check_delta(again["delta"], c.g["delta"])


@pytest.mark.parametrize("name", ["daily_f64", "daily_f32"])
def test_daily_host_mirror(dev, name):
    """xclim_amd.chill on the device's own day-length table (xh_solar_table).  That table meets the reference's to 1e-12
    relative (tests/test_gpu_pet.py); near the polar boundary the night's slope 1 / log(25 - dl) amplifies it by up to 1e4 K
    per hour of day length, hence 1e-6 K here.  The exact check of the arithmetic is the test above."""
    c = golden_case(name)
    h = chill.make_hourly_temperature(c.tasmin, c.tasmax, c.lat, c.time, device=dev)
    assert h.shape == c.hourly.shape and h.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(h), np.isnan(c.hourly))
    np.testing.assert_allclose(h, c.hourly, rtol=0, atol=1e-6, equal_nan=True)
    both = chill.chill_from_daily(c.tasmin, c.tasmax, c.lat, c.time, False, c.freq, units=c.units, device=dev)
    cp = chill.chill_portions_from_daily(c.tasmin, c.tasmax, c.lat, c.time, c.freq, units=c.units, device=dev)
    cu = chill.chill_units_from_daily(c.tasmin, c.tasmax, c.lat, c.time, False, c.freq, units=c.units, device=dev)
    np.testing.assert_array_equal(both.chill_portions, cp)
    np.testing.assert_array_equal(both.chill_units, cu)
    # the chain the reference's docstrings recommend, on the mirror's own hourly field: bit for bit
    np.testing.assert_array_equal(cp, chill.chill_portions(h, c.time, c.freq, units=c.units, device=dev))
    np.testing.assert_array_equal(cu, chill.chill_units(h, c.time, False, c.freq, units=c.units, device=dev))
    np.testing.assert_allclose(cp, c.g["cp"], rtol=1e-6, atol=1e-6)
    # MissingAny on hours: every period with a NaN hour (or an incomplete month) is NaN
    masked = chill.chill_portions_from_daily(c.tasmin, c.tasmax, c.lat, c.time, c.freq, units=c.units, device=dev, mask_missing=True)
    full = np.array([(~np.isnan(c.hourly[24 * a:24 * b])).sum(axis=0) for a, b in zip(c.seg[:-1], c.seg[1:])])
    np.testing.assert_array_equal(np.isnan(masked), full != chill.hourly_expected_count(c.time, c.freq)[:, None])


def test_known_answers_on_device(dev):
    """tests/test_indices.py:375-399 and tests/test_helpers.py:302-338 of the reference through the public functions."""
    t = TimeAxis.daily("2000-01-01", 120)
    cp = chill.chill_portions(np.linspace(0, 15, 120 * 24) + K2C, t, device=dev)
    np.testing.assert_array_almost_equal(cp, [72.2441765], decimal=7)
    v = np.array(10 * [1.1] + 15 * [2.0] + 20 * [5.6] + 10 * [16.0] + 5 * [20.0] + 12 * [np.nan]) + K2C
    t3 = TimeAxis.daily("2000-01-01", 3)
    assert chill.chill_units(v, t3, units="K", device=dev)[0] == 0.5 * 15 + 20 - 0.5 * 10 - 5
    assert chill.chill_units(v, t3, positive_only=True, units="K", device=dev)[0] == 0.5 * 15 + 20 - 0.5 * 3
    c = golden_case("known_equator")
    h = chill.make_hourly_temperature(c.tasmin, c.tasmax, 0.0, c.time, device=dev)
    np.testing.assert_allclose(h[:, 0], c.hourly[:, 0])   # (assert_allclose's defaults, as the reference's test)


def test_periods_without_a_selected_hour_and_missing_mask(dev):
    """month=[12, 1, 2] with monthly periods: the months outside the selection are NaN (see xclim_amd.chill), chill units
    of an all-NaN period are 0; MissingAny keeps only complete, NaN-free periods."""
    t = TimeAxis.daily("2001-11-20", 80)
    rng = np.random.default_rng(5)
    x = (278 + rng.normal(0, 4, (80 * 24, 3))).astype(np.float32)
    x[24 * 50 + 3, 1] = np.nan   # one hour of January at cell 1
    cp = chill.chill_portions(x, t, "MS", device=dev, month=[12, 1, 2])
    assert cp.shape == (4, 3)
    assert np.isnan(cp[0]).all() and not np.isnan(cp[1:]).any()       # November is not selected
    masked = chill.chill_portions(x, t, "MS", device=dev, month=[12, 1, 2], mask_missing=True)
    np.testing.assert_array_equal(np.isnan(masked), [[True] * 3, [False] * 3, [False, True, False], [True] * 3])
    np.testing.assert_array_equal(masked[1], cp[1])
    x[:24 * 11] = np.nan
    cu = chill.chill_units(x, t, False, "MS", units="K", device=dev)
    assert (cu[0] == 0).all()


# ---- the smallest shapes that can still go wrong ---------------------------------------------------------------------
def _field(rng, D, C, dtype):
    """Hourly temperatures in K around the release threshold, with a NaN sprinkle."""
    hour = np.arange(24 * D)[:, None]
    x = 279 + 5 * np.sin(2 * np.pi * (hour - 9) / 24.0) + rng.normal(0, 2.5, (24 * D, C)) + np.linspace(-5, 5, C)[None, :]
    x = x.astype(dtype)
    x[rng.random(x.shape) < 0.002] = np.nan
    return x


def _periods(D):
    """(day offsets, per-day selection or None) for P = 1 and, from 3 days on, P = 3 with a period of a single day; with 40 days
    also a period without a selected day."""
    forms = [(np.array([0, D]), None)]
    if D >= 3:
        seg = np.array([0, 1, D // 2, D])
        forms.append((seg, None))
        sel = np.ones(D, bool)
        sel[seg[1]:seg[2]] = False      # a period of zero selected hours
        sel[seg[2] + 1] = False
        forms.append((seg, sel))
    return forms


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C", [1, 63, 65, 257])
@pytest.mark.parametrize("D", [1, 2, 40])
def test_hourly_shapes_against_restatement(dev, C, D, dtype):
    rng = np.random.default_rng(1000 * D + C)
    x = _field(rng, D, C, dtype)
    d = dev.to_device(x)
    for seg, sel in _periods(D):
        rows = None if sel is None else np.repeat(sel, 24)
        if rows is None and D >= 2:   # a row_sel of its own: the first and the last hour of every period dropped
            rows = np.ones(24 * D, bool)
            rows[24 * seg[:-1]] = False
            rows[24 * seg[1:] - 1] = False
        for positive_only in (False, True):
            got = _host(K.chill_hourly(dev, d, 24 * seg, rows, positive_only=positive_only, outputs=("cp", "cu", "valid", "delta")))
            delta, margin = chillcpu.delta_rows(x, 24 * seg, rows)
            assert margin >= 1e-9, "the seeded field puts a release on the last bit of exp: change the seed"
            cp, _, valid = chillcpu.portions(x, 24 * seg, rows)
            check_delta(got["delta"], delta)
            check_sums(got["cp"], cp)
            np.testing.assert_array_equal(got["valid"], valid)
            np.testing.assert_array_equal(got["cu"], chillcpu.units(x - x.dtype.type(K2C), 24 * seg, positive_only, rows))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C", [1, 63, 65, 257])
@pytest.mark.parametrize("D", [1, 2, 40])
def test_daily_shapes_against_restatement(dev, C, D, dtype):
    rng = np.random.default_rng(2000 * D + C)
    base = 278 + rng.normal(0, 3, (D, C)) + np.linspace(-4, 4, C)[None, :]
    spread = rng.uniform(2, 12, (D, C))
    tn, tx = (base - spread / 2).astype(dtype), (base + spread / 2).astype(dtype)
    tn[rng.random(tn.shape) < 0.01] = np.nan
    L = 3
    dl = rng.uniform(5.0, 19.5, (D, L))
    dl[D // 2, 2] = np.nan            # a polar day
    dl[0, 1] = 12.0                   # sunset on the hour
    li = rng.integers(0, L, C).astype(np.int32)
    hourly = chillcpu.hourly_temperature(tn, tx, dl[:, li])
    dn, dx, ddl = dev.to_device(tn), dev.to_device(tx), dev.to_device(dl)
    for seg, sel in _periods(D):
        rows = None if sel is None else np.repeat(sel, 24)
        for positive_only in (False, True):
            got = _host(K.chill_daily(dev, dn, dx, ddl, li, seg, sel, positive_only=positive_only, outputs=("cp", "cu", "valid", "hourly")))
            np.testing.assert_array_equal(np.isnan(got["hourly"]), np.isnan(hourly))
            np.testing.assert_allclose(got["hourly"], hourly, rtol=RTOL, atol=0, equal_nan=True)
            _, margin = chillcpu.delta_rows(hourly, 24 * seg, rows)
            assert margin >= 1e-9, "the seeded field puts a release on the last bit of exp: change the seed"
            cp, _, valid = chillcpu.portions(hourly, 24 * seg, rows)
            check_sums(got["cp"], cp)
            np.testing.assert_array_equal(got["valid"], valid)
            np.testing.assert_array_equal(got["cu"], chillcpu.units(hourly - K2C, 24 * seg, positive_only, rows))


# ---- padded, poisoned row views --------------------------------------------------------------------------------------
# (the operands of the two entry points: stridedabi.CHILL_TABLE)


def _same_bits(a, b):
    if a.dtype.kind == "f":
        return bool(((a.view(f"u{a.itemsize}") == b.view(f"u{b.itemsize}")) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C,pads", [(67, (1, 3)), (260, (2, 6)), (260, (4, 12))])
def test_padded_views_give_the_same_bits(dev, monkeypatch, C, pads, dtype):
    """Both entry points with every strided operand in rows longer than the field is wide, NaN / 1e30 in the extra columns of
    the inputs and 0xA5 bytes in those of the outputs (tests/stridedabi.py: padded): the same bits, untouched padding."""
    for name, ops in CHILL_TABLE.items():
        for op in ops:   # the table names parameters of the prototypes
            assert {op.ptr, op.stride} <= set(S.PROTOS[name]), (name, op)
    rng = np.random.default_rng(C)
    D = 5
    seg = np.array([0, 2, 5])
    sel = np.array([1, 1, 0, 1, 1], bool)
    x = _field(rng, D, C, dtype)
    tn = (276 + rng.normal(0, 3, (D, C))).astype(dtype)
    tx = (tn + rng.uniform(2, 10, (D, C))).astype(dtype)
    dl = rng.uniform(6, 18, (D, 2))
    li = rng.integers(0, 2, C).astype(np.int32)

    def run():
        h = K.chill_hourly(dev, dev.to_device(x), 24 * seg, np.repeat(sel, 24), positive_only=True, outputs=("cp", "cu", "valid", "delta"))
        d = K.chill_daily(dev, dev.to_device(tn), dev.to_device(tx), dev.to_device(dl), li, seg, sel, outputs=("cp", "cu", "valid", "hourly"))
        return [v.get() for v in h.values()] + [v.get() for v in d.values()]

    plain = run()
    with S.padded(dev, monkeypatch, pads=pads) as log:
        got = run()
    assert len(got) == len(plain) == 8
    for i, (g, p) in enumerate(zip(got, plain)):
        assert g.shape == p.shape and g.dtype == p.dtype and _same_bits(g, p), f"output {i} differs under strides {log}"
    for entry in CHILL_TABLE:
        used = [u for n, u in log if n == entry]
        assert used and all(s != w for s, w in used[0].values()) and set(used[0]) == {"ld", "ld_out"}, log


def test_a_stride_below_the_width_is_refused(dev):
    from xclim_amd._capi import XH_ERR_LAYOUT

    C, D = 8, 2
    x = dev.to_device(np.full((24 * D, C), 280.0))
    tn = dev.to_device(np.full((D, C), 275.0))
    seg = dev.to_device(np.array([0, 24 * D], np.int64))
    dseg = dev.to_device(np.array([0, D], np.int64))
    dl = dev.to_device(np.full((D, 1), 12.0))
    li = dev.to_device(np.zeros(C, np.int32))
    out = dev.empty((24 * D, C), np.float64)
    for ld, ld_out in ((C - 1, C), (C, C - 1)):
        assert dev.lib.xh_chill_hourly(dev.ctx, 24 * D, C, ld, 1, _vp(x.ptr), 24, 1, _vp(seg.ptr), _vp(0), 0.0, K2C, 0, _vp(0), _vp(0),
                                       _vp(0), _vp(out.ptr), ld_out) == XH_ERR_LAYOUT
        assert dev.lib.xh_chill_daily(dev.ctx, D, C, ld, 1, _vp(tn.ptr), _vp(tn.ptr), _vp(dl.ptr), 1, _vp(li.ptr), 1, _vp(dseg.ptr),
                                      _vp(0), 0.0, K2C, 0, _vp(0), _vp(0), _vp(0), _vp(out.ptr), ld_out) == XH_ERR_LAYOUT


def test_refusals_answer_before_any_launch(dev):
    """The faults every pitched entry point answers (tests/newunit_cases.py: shared_refusals), one at a time; seg is a device
    pointer here, so of a table's faults only NULL and the 65535 limit apply.  The sentinel is intact afterwards, and the same
    calls with nothing wrong then run."""
    from newunit_cases import shared_refusals
    from xclim_amd._capi import XH_ERR_ARG, XH_ERR_LIMIT

    C, D, P = 8, 2, 2
    x = dev.to_device(np.full((24 * D, C), 280.0))
    tn = dev.to_device(np.full((D, C), 275.0))
    seg = dev.to_device(np.array([0, 24, 24 * D], np.int64))
    dseg = dev.to_device(np.array([0, 1, D], np.int64))
    dl = dev.to_device(np.full((D, 1), 12.0))
    li = dev.to_device(np.zeros(C, np.int32))
    out = dev.to_device(np.full((24 * D, C), -7.0))

    def hourly(ctx=dev.ctx, T=24 * D, C=C, ld=C, ld_out=C, P=P, seg=_vp(seg.ptr)):
        return dev.lib.xh_chill_hourly(ctx, T, C, ld, 1, _vp(x.ptr), 24, P, seg, _vp(0), 0.0, K2C, 0, _vp(0), _vp(0), _vp(0), _vp(out.ptr),
                                       ld_out)

    def daily(ctx=dev.ctx, T=D, C=C, ld=C, ld_out=C, P=P, seg=_vp(dseg.ptr)):
        return dev.lib.xh_chill_daily(ctx, T, C, ld, 1, _vp(tn.ptr), _vp(tn.ptr), _vp(dl.ptr), 1, _vp(li.ptr), P, seg, _vp(0), 0.0, K2C, 0,
                                      _vp(0), _vp(0), _vp(0), _vp(out.ptr), ld_out)

    shared_refusals(hourly, 24 * D, C)
    shared_refusals(daily, D, C)
    for call in (hourly, daily):
        assert call(seg=_vp(0)) == XH_ERR_ARG and call(P=-1) == XH_ERR_ARG and call(P=65536) == XH_ERR_LIMIT
    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((24 * D, C), -7.0))
    assert hourly() == 0
    dev.sync()
    assert (out.get() != -7.0).all()
    out = dev.to_device(np.full((24 * D, C), -7.0))
    assert daily() == 0
    dev.sync()
    assert (out.get() != -7.0).all()


# ---- the adapter ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def agromod(dev):
    """A stand-in xclim.indices._agro whose original asserts if it is reached (unless allowed)."""
    import xclim_amd._capi as capi

    calls = []

    def orig(tas_K):
        calls.append(np.asarray(tas_K).dtype)
        assert mod.allow_forward, "the original _chill_portion_one_season was reached"
        return "forwarded"

    mod = types.SimpleNamespace(_chill_portion_one_season=orig, allow_forward=False, calls=calls, orig=orig)
    old = capi._default_device
    capi._default_device = dev
    done = patch.install(env=fakexr.make_env(), modules={"xclim.indices._agro": mod})
    assert "xclim.indices._agro._chill_portion_one_season" in done
    yield mod
    patch.uninstall()
    capi._default_device = old


@pytest.mark.parametrize("name", ["seasonal_f64", "seasonal_f32", "nan_hours"])
def test_adapter_serves_time_last_views(dev, agromod, name):
    """What xr.apply_ufunc hands over inside resample_map: one period of the field in K, time moved last."""
    c = golden_case(name)
    a, b = 24 * c.seg[0], 24 * c.seg[1]
    tas_K = (c.tas[a:b] + c.tas.dtype.type(c.add_K))      # convert_units_to in the field's dtype
    view = np.moveaxis(tas_K, 0, -1)
    assert not view.flags.c_contiguous or view.shape[0] == 1
    trace = dev.start_trace()
    try:
        got = agromod._chill_portion_one_season(view)
    finally:
        dev.stop_trace()
    assert [n for n, _ in trace if n.startswith("xh_")] == ["xh_chill_hourly"]
    assert got.shape == view.shape and got.dtype == view.dtype and agromod.calls == []
    exp, _ = chillcpu.delta_rows(tas_K, np.array([0, b - a]))
    if c.dtype == np.float32:   # the float64 delta rounded once
        np.testing.assert_array_equal(got > 0, np.moveaxis(exp, 0, -1) > 0)
        np.testing.assert_allclose(got, np.moveaxis(exp, 0, -1).astype(np.float32), rtol=2.0 ** -23, atol=0)
    else:
        check_delta(np.moveaxis(got, -1, 0), exp)


def test_adapter_loop_shapes_and_forwards(dev, agromod):
    rng = np.random.default_rng(11)
    x = _field(rng, 3, 6, np.float64)                              # (72, 6)
    cube = np.moveaxis(x, 0, -1).reshape(2, 3, 72)                 # a 3-D loop shape (lat, lon, time)
    got = agromod._chill_portion_one_season(cube)
    exp, _ = chillcpu.delta_rows(x, np.array([0, 72]))
    assert got.shape == cube.shape and got.dtype == np.float64
    check_delta(np.moveaxis(got.reshape(6, 72), -1, 0), exp)
    one = agromod._chill_portion_one_season(np.ascontiguousarray(x[:, 2]))      # a single series, no loop dimension
    check_delta(one[:, None], exp[:, 2:3])
    assert agromod.calls == []
    agromod.allow_forward = True
    assert agromod._chill_portion_one_season(cube.astype(np.float16)) == "forwarded"
    assert agromod._chill_portion_one_season(cube.astype(np.int32)) == "forwarded"
    assert agromod._chill_portion_one_season(np.ones((4, 0))) == "forwarded"
    assert agromod._chill_portion_one_season(np.ones((0, 5), np.float32)) == "forwarded"
    assert len(agromod.calls) == 4


def test_uninstall_restores_the_original(dev):
    def orig(tas_K):
        return "original"

    mod = types.SimpleNamespace(_chill_portion_one_season=orig)
    patch.install(env=fakexr.make_env(), modules={"xclim.indices._agro": mod})
    try:
        assert mod._chill_portion_one_season is not orig and mod._chill_portion_one_season.__wrapped__ is orig
    finally:
        patch.uninstall()
    assert mod._chill_portion_one_season is orig


# ---- one realistic size ----------------------------------------------------------------------------------------------
def test_30_years_1440x8_fused_against_restatement(dev):
    """30 noleap years x 1440 x 8 cells of float32 tasmin / tasmax through the fused path in one launch (30 periods per cell);
    24 seeded cells against the restatement over every hour of every year."""
    ny, T, C = 30, 365 * 30, 1440 * 8
    time = TimeAxis.daily("1981-01-01", T, "noleap")
    t = np.arange(T)
    season = (9 * np.cos(2 * np.pi * (t - 200) / 365.0)).astype(np.float32)

    def fields(n, cell0=0):
        tn = K.fill_synthetic(dev, T, n, 0, 71, 274 - season, 3.0, cell0=cell0)
        tx = K.fill_synthetic(dev, T, n, 0, 72, 283 - season, 3.0, cell0=cell0)
        return tn, tx

    lat = np.repeat(np.array([-60.0, -45.0, -20.0, 0.0, 15.0, 40.0, 52.0, 63.0]), 1440)
    tn, tx = fields(C)
    out = chill.chill_from_daily(tn, tx, lat, time, True, "YS", units="K", device=dev, keep=True)
    cp, cu = out.chill_portions.get(), out.chill_units.get()
    assert cp.shape == cu.shape == (ny, C)
    rng = np.random.default_rng(30)
    cells = np.sort(rng.choice(C, 24, replace=False))
    one = [np.concatenate([f.get() for f in col], axis=1) for col in zip(*[fields(1, cell0=int(c)) for c in cells])]
    lat_u, li = converters._lat_table(lat[cells], (len(cells),))
    dl = converters.day_lengths(time, lat_u, device=dev)[:, li]       # the table the fused path reads
    hourly = chillcpu.hourly_temperature(one[0], one[1], dl)
    # the years are independent and equally long: every (year, cell) as one column of a single year
    cols = hourly.reshape(ny, 8760, len(cells)).transpose(1, 0, 2).reshape(8760, ny * len(cells))
    seg = np.array([0, 8760])
    ecp, _, _ = chillcpu.portions(cols, seg)
    ecu = chillcpu.units(cols - K2C, seg, positive_only=True)
    check_sums(cp[:, cells], ecp.reshape(ny, len(cells)))
    np.testing.assert_array_equal(cu[:, cells], ecu.reshape(ny, len(cells)))
    assert (cp[:, cells] > 0).all()
