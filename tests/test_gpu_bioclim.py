"""The ANUCLIM variables BIO1-BIO19 on the device (xh_bioclim, xclim_amd.anuclim) against tests/golden/anuclim_vectors.npz —
which holds the known answers of the reference's own tests — and, at the cell counts no golden value exists for, against the
numpy restatement tests/anuclimcpu.py; against the project's own period reductions bit for bit; on padded, poisoned row
views (tests/stridedabi.py); the refusals of the entry point.  The xarray adapter has a module of its own
(tests/test_gpu_anuclim_adapter.py).

Tolerances (tests/test_anuclim_cpu.py: check).  float64 fields 1e-12 relative, float32 fields 1e-6 relative, the step indices
and counts exactly, the same NaN pattern.  BIO4 / BIO15: four times the largest relative distance of the single-pass formula
(Welford, numpy float64) from the two-pass value over every golden case, as stored in the golden file (1.4e-13 measured, so
5.7e-13; the formula would have been rejected above 1e-10)."""

import ctypes

import numpy as np
import pytest

import anuclimcpu as A
import stridedabi as S
from stridedabi import BIOCLIM_TABLE
from test_anuclim_cpu import CV_BOUND, KNOWN, SEEDED, check, golden_case
from xclim_amd import anuclim, indices
from xclim_amd import kernels as K
from xclim_amd._capi import XH_ERR_ARG, XH_ERR_LAYOUT
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
_vp = ctypes.c_void_p
DAY = 86400.0
ALL = K.BIOCLIM_VARS + K.BIOCLIM_WHICH + K.BIOCLIM_COUNTS


def _host(outs):
    return {k: v.get() for k, v in outs.items()}


def _names(fields):
    """The outputs that the given fields can serve."""
    have = set(fields)
    names = [f"bio{k}" for k, reads in anuclim._READS.items() if set(reads) <= have]
    names += [w for w, reads in anuclim._WHICH_READS.items() if set(reads) <= have]
    return names + ["n_" + f for f in fields]


# ---- the golden cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEEDED + KNOWN)
def test_golden_cases(dev, name):
    c = golden_case(name)
    d = {k: dev.to_device(v) for k, v in c.fields.items()}
    for freq, exp in c.expected.items():
        so, sr, ss, W = c.tables(freq)
        names = _names(c.fields)
        assert set(names) == set(exp)
        got = _host(K.bioclim(dev, d, so, c.factor, sr, ss, W, binned=c.kind == "D", kelvin_offset=c.kelvin, cv_scale=c.cv_scale,
                              thresh=c.thresh, outputs=names))
        for k in names:
            check(got[k], exp[k], k, c.dtype, f"{name} {freq}")
        for key, want in c.answers.items():       # the reference's known answers, to the decimals it asserts them with
            np.testing.assert_array_almost_equal(got[key][:, 0], want, decimal=6)
        # the host mirror: the same bits on the axis' own tables
        f = c.fields
        ks = [k for k in names if k.startswith("bio")]
        mirror = anuclim.bioclim(f.get("tas"), f.get("tasmin"), f.get("tasmax"), f.get("pr"), c.time, freq, ks, units=c.units,
                                 which=[w for w in names if w in K.BIOCLIM_WHICH], pr_units=c.pr_units, thresh=c.thresh, device=dev)
        for k in mirror:
            np.testing.assert_array_equal(mirror[k], got[k], err_msg=f"{name} {freq} {k}")


# ---- one, several and more than a workgroup of cells ----------------------------------------------------------------
def _synth(seed, t, C, dtype):
    rng = np.random.default_rng(seed)
    T = len(t)
    doy = t.doy[:, None].astype(np.float64)
    tas = 283 + 10 * np.sin(2 * np.pi * (doy - 100) / 365) + rng.normal(0, 3, (T, C)) + np.linspace(-3, 3, C)[None, :]
    tn, tx = tas - rng.uniform(2, 6, (T, C)), tas + rng.uniform(2, 6, (T, C))
    pr = np.maximum(rng.normal(2 + np.cos(2 * np.pi * doy / 365), 4, (T, C)), 0) / DAY
    f = {k: v.astype(dtype) for k, v in dict(tas=tas, tasmin=tn, tasmax=tx, pr=pr).items()}
    for k in f:                                    # a NaN sprinkle, a week without a value in one cell
        f[k][rng.random((T, C)) < 0.003] = np.nan
    f["tas"][21:28, C // 2] = f["pr"][21:28, C // 2] = np.nan
    return f


_MIDYEAR = {}


def _midyear(C, dtype):
    """1999-03-15 + 1002 days (a last bin of one day), the fields and the restatement's values for YS and YS-JUL: once."""
    key = (C, np.dtype(dtype).name)
    if key not in _MIDYEAR:
        t = TimeAxis.daily("1999-03-15", 1002)
        f = _synth(100 + C, t, C, dtype)
        exp = {}
        for freq in ("YS", "YS-JUL"):
            so, sr, ss, W = A.tables(t.year, t.month, "D", freq)
            exp[freq] = A.bioclim(f, so, np.full(1002, DAY), sr, ss, W, True, 0.0, DAY, 1.5 / DAY, want_gap=True)
            assert exp[freq].pop("min_gap") > 1e-9, "the seeded field puts two quarters within 1e-9: change the seed"
        _MIDYEAR[key] = (t, f, exp)
    return _MIDYEAR[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C", [1, 67, 260])
def test_midyear_start_against_restatement(dev, C, dtype):
    t, f, exp = _midyear(C, dtype)
    for freq in ("YS", "YS-JUL"):
        got = anuclim.bioclim(f["tas"], f["tasmin"], f["tasmax"], f["pr"], t, freq, which=K.BIOCLIM_WHICH, thresh=1.5 / DAY, device=dev)
        assert set(got) == set(K.BIOCLIM_VARS + K.BIOCLIM_WHICH)
        for k, v in got.items():
            check(v, exp[freq][k], k, dtype, f"C={C} {freq}")


def test_all_nineteen_are_one_launch(dev):
    t, f, _ = _midyear(67, np.float32)
    d = {k: dev.to_device(v) for k, v in f.items()}
    trace = dev.start_trace()
    try:
        out = anuclim.bioclim(d["tas"], d["tasmin"], d["tasmax"], d["pr"], t, "YS", keep=True, device=dev)
    finally:
        dev.stop_trace()
    assert sorted(out) == sorted(K.BIOCLIM_VARS) and all(v.shape == (3, 67) for v in out.values())
    assert [n for n, _ in trace if n.startswith("xh_")] == ["xh_bioclim"], [n for n, _ in trace]
    assert not [n for n, _ in trace if n in ("h2d", "d2h")], "device-resident fields: nothing moves but the host tables"


# ---- against the project's own reductions, and the single-variable functions ---------------------------------------
def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def test_period_reductions_bit_for_bit(dev, monkeypatch):
    """BIO1, BIO2, BIO5, BIO6 and BIO7 of float64 fields are what the project's own float64 reductions give (XCLIM_AMD_FLOAT64=native)."""
    monkeypatch.setenv("XCLIM_AMD_FLOAT64", "native")
    t, f, _ = _midyear(67, np.float64)
    b = anuclim.bioclim(f["tas"], f["tasmin"], f["tasmax"], f["pr"], t, "YS", [1, 2, 5, 6, 7], device=dev)
    kw = dict(device=dev, mask_missing=False)
    other = {"bio1": indices.tg_mean(f["tas"], t, "YS", **kw),
             "bio2": indices.daily_temperature_range(f["tasmin"], f["tasmax"], t, "YS", **kw),
             "bio5": indices.tg_max(f["tasmax"], t, "YS", **kw), "bio6": indices.tg_min(f["tasmin"], t, "YS", **kw),
             "bio7": indices.extreme_temperature_range(f["tasmin"], f["tasmax"], t, "YS", **kw)}
    for k, v in other.items():
        assert v.dtype == np.float64
        np.testing.assert_array_equal(_bits(b[k]), _bits(v), err_msg=k)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_single_variable_functions_equal_the_entries(dev, dtype):
    t, f, _ = _midyear(67, dtype)
    tas, tn, tx, pr = f["tas"], f["tasmin"], f["tasmax"], f["pr"]
    b = anuclim.bioclim(tas, tn, tx, pr, t, "YS-JUL", thresh=1.5 / DAY, device=dev)
    kw = dict(device=dev)
    one = {3: anuclim.isothermality(tn, tx, t, "YS-JUL", **kw), 4: anuclim.temperature_seasonality(tas, t, "YS-JUL", **kw),
           15: anuclim.precip_seasonality(pr, t, "YS-JUL", **kw),
           10: anuclim.tg_mean_warmcold_quarter(tas, t, "warmest", "YS-JUL", **kw),
           11: anuclim.tg_mean_warmcold_quarter(tas, t, "coldest", "YS-JUL", **kw),
           8: anuclim.tg_mean_wetdry_quarter(tas, pr, t, "wettest", "YS-JUL", **kw),
           9: anuclim.tg_mean_wetdry_quarter(tas, pr, t, "dryest", "YS-JUL", **kw),
           16: anuclim.prcptot_wetdry_quarter(pr, t, "wettest", "YS-JUL", **kw),
           17: anuclim.prcptot_wetdry_quarter(pr, t, "driest", "YS-JUL", **kw),
           18: anuclim.prcptot_warmcold_quarter(pr, tas, t, "warmest", "YS-JUL", **kw),
           19: anuclim.prcptot_warmcold_quarter(pr, tas, t, "coldest", "YS-JUL", **kw),
           12: anuclim.prcptot(pr, t, 1.5 / DAY, "YS-JUL", **kw), 13: anuclim.prcptot_wetdry_period(pr, t, op="wettest", freq="YS-JUL", **kw),
           14: anuclim.prcptot_wetdry_period(pr, t, op="driest", freq="YS-JUL", **kw)}
    for k, v in one.items():
        np.testing.assert_array_equal(_bits(v), _bits(b[f"bio{k}"]), err_msg=f"bio{k}")
    with pytest.raises(NotImplementedError):
        anuclim.tg_mean_warmcold_quarter(tas, t, "wettest", device=dev)


def test_only_the_needed_fields_are_read(dev):
    """A launch for BIO1 with the other three field pointers NULL, and BIO12 with pr alone: the host mirror hands over only
    what the outputs read."""
    t, f, exp = _midyear(67, np.float32)
    trace = dev.start_trace()
    try:
        b1 = anuclim.bioclim(tas=f["tas"], time=t, variables=[1], device=dev)["bio1"]
    finally:
        dev.stop_trace()
    (args,) = [a for n, a in trace if n == "xh_bioclim"]
    assert args[4].value and not args[5].value and not args[6].value and not args[7].value
    check(b1, exp["YS"]["bio1"], "bio1", np.float32)
    with pytest.raises(TypeError, match="pr is needed"):
        anuclim.bioclim(tas=f["tas"], time=t, variables=[1, 12], device=dev)


def test_missing_mask(dev):
    t, f, exp = _midyear(67, np.float32)
    m = anuclim.bioclim(f["tas"], f["tasmin"], f["tasmax"], f["pr"], t, "YS", [1, 3, 8, 12], thresh=1.5 / DAY, device=dev,
                        mask_missing=True)
    full = t.expected_count("YS")[:, None]
    e = exp["YS"]
    bad = {k: e["n_" + k] != full for k in ("tas", "tasmin", "tasmax", "pr")}
    assert bad["tas"][0].all() and not bad["tas"][1].all() and bad["tas"][1].any()     # 1999 starts in March; a NaN sprinkle in 2000
    for k, reads in ((1, ("tas",)), (3, ("tasmin", "tasmax")), (8, ("tas", "pr")), (12, ("pr",))):
        want = np.where(np.any([bad[r] for r in reads], axis=0), np.nan, e[f"bio{k}"])
        check(m[f"bio{k}"], want, f"bio{k}", np.float32, "masked")
    with pytest.raises(ValueError, match="keep=True"):
        anuclim.bioclim(tas=f["tas"], time=t, variables=[1], device=dev, keep=True, mask_missing=True)


# ---- padded, poisoned row views --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("C,pitch", [(67, 80), (260, 272)])
def test_padded_views_give_the_same_bits(dev, monkeypatch, C, pitch, dtype):
    """Every input and output in rows of `pitch` elements, NaN / 1e30 in the extra columns of the inputs and in front of their
    first row, 0xA5 bytes in those of the outputs (tests/stridedabi.py: padded, which asserts that they stay): the same bits."""
    for name, ops in BIOCLIM_TABLE.items():
        for op in ops:
            assert {op.ptr, op.stride} <= set(S.PROTOS[name]), (name, op)
    t, f, _ = _midyear(C, dtype)
    so, sr, ss, W = A.tables(t.year, t.month, "D", "YS-JUL")

    def run():
        d = {k: dev.to_device(v) for k, v in f.items()}
        return _host(K.bioclim(dev, d, so, np.full(len(t), DAY), sr, ss, W, cv_scale=DAY, thresh=1.5 / DAY, outputs=ALL))

    plain = run()
    with S.padded(dev, monkeypatch, pads=(pitch - C, pitch - C), shift=5) as log:
        got = run()
    assert set(got) == set(plain) == set(ALL)
    for k in ALL:
        g, p = got[k], plain[k]
        same = (g == p) | (np.isnan(g) & np.isnan(p)) if g.dtype.kind == "f" else g == p
        assert g.shape == p.shape and same.all(), f"{k} differs under row pitches {log}"
    (used,) = [u for n, u in log if n == "xh_bioclim"]
    assert used == {"ld": (pitch, C), "ld_out": (pitch, C)}, log


# ---- refusals: every one a code, before anything is launched --------------------------------------------------------
def test_refusals(dev):
    from newunit_cases import shared_refusals

    T, C, S_, P = 30, 8, 5, 1
    x = dev.to_device(np.full((T, C), 280.0))
    out = dev.to_device(np.full((P, C), -7.0))
    so = np.array([0, 7, 14, 21, 28, 30], np.int64)
    fa = np.ones(T)
    sr, ss = np.array([0, T], np.int64), np.array([0, S_], np.int64)
    outs = (_vp * 19)()
    outs[0] = out.ptr
    none = (_vp * 19)()
    p = lambda a: a.ctypes.data_as(_vp)  # noqa: E731

    def call(ld=C, ld_out=C, so=so, fa=fa, sr=sr, ss=ss, W=13, outputs=outs, tas=_vp(x.ptr), S=S_, P=P, T=T, C=C, ctx=dev.ctx):
        tab = [p(a) if a is not None else _vp(0) for a in (so, fa, sr, ss)]
        return dev.lib.xh_bioclim(ctx, T, C, ld, 1, tas, _vp(0), _vp(0), _vp(0), S, tab[0], tab[1], 1, P, tab[2], tab[3], W, 0.0, 1.0,
                                  0.0, outputs, _vp(0), _vp(0), ld_out)

    assert call(ld=C - 1) == XH_ERR_LAYOUT and call(ld_out=C - 1) == XH_ERR_LAYOUT
    for k in ("so", "fa", "sr", "ss"):
        assert call(**{k: None}) == XH_ERR_ARG, k                                  # NULL tables
    assert call(so=np.array([0, 7, 14, 21, 28, 31], np.int64)) == XH_ERR_ARG       # a step past the last row
    assert call(so=np.array([0, 7, 6, 21, 28, 30], np.int64)) == XH_ERR_ARG        # steps that go back
    assert call(sr=np.array([0, T + 1], np.int64)) == XH_ERR_ARG and call(sr=np.array([-1, T], np.int64)) == XH_ERR_ARG
    assert call(ss=np.array([0, S_ + 1], np.int64)) == XH_ERR_ARG and call(ss=np.array([3, 2], np.int64)) == XH_ERR_ARG
    assert call(W=5) == XH_ERR_ARG
    assert call(outputs=none) == XH_ERR_ARG and call(outputs=_vp(0)) == XH_ERR_ARG   # no output requested
    assert call(tas=_vp(0)) == XH_ERR_ARG                                          # BIO1 without tas
    quarters = (_vp * 19)()
    quarters[9] = out.ptr
    assert call(outputs=quarters, sr=np.array([0, T], np.int64), ss=np.array([0, 4], np.int64)) == XH_ERR_ARG   # steps that stop before the rows
    many = dict(sr=np.zeros(65538, np.int64), ss=np.zeros(65538, np.int64), P=65536)
    shared_refusals(call, T, C, [("sr", sr, T, many), ("ss", ss, S_, many), ("so", so, T, None)])
    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((P, C), -7.0))                # nothing was launched: the sentinel is intact
    assert call() == 0                                                             # and the same call with nothing wrong runs
    np.testing.assert_array_equal(out.get(), np.full((P, C), 280.0))


def test_unknown_units_and_shapes(dev):
    t = TimeAxis.daily("2001-01-01", 400)
    x = np.full((400, 3), 280.0, np.float32)
    with pytest.raises(ValueError, match="units"):
        anuclim.temperature_seasonality(x, t, units="F", device=dev)
    with pytest.raises(ValueError, match="pr_units"):
        anuclim.prcptot(x, t, pr_units="in/d", device=dev)
    with pytest.raises(ValueError, match="rows"):
        anuclim.prcptot(x[:-1], t, device=dev)
    assert anuclim.prcptot(x[:, :0], t, device=dev).shape == (2, 0)
    # a mixed pair is widened: the float64 values of both
    tn, tx = x - np.float32(5.1), (x + 4.9).astype(np.float64)
    got = anuclim.isothermality(tn, tx, t, device=dev)
    np.testing.assert_array_equal(got, anuclim.isothermality(tn.astype(np.float64), tx, t, device=dev))
    assert CV_BOUND > 0
