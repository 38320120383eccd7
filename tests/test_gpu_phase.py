"""The snow / rain partition unit on the device (xclim_amd/csrc/phase.hip, xclim_amd.phase) against the numpy restatement
tests/phasecpu.py and its stored values tests/golden/phase_vectors.npz: every family of decisions, every method, float32 and
float64 fields, a series of 800 days from 1999-06-10 whose "YS", "YS-JUL" and "MS" periods touch row 0 and row T - 1 and hold a
leap February and a short last period, 1 to 257 cells, every single output and all together, padded and poisoned row views; the
fused outputs against xh_precip_phase_map followed by the existing reduce and count entry points; the host mirrors bit for bit
against the kernel calls; the reference's known answers through the mirror; the refusals.  Every test runs on poisoned output
buffers, and after every call of an entry point no output element may still hold the poison (tests/unwritten.py: watch).

Tolerances.  Exact (``assert_array_equal``) for the binary and given-snow results, every count, day of year and NaN pattern, and
the exact families (amounts on a 0.25 mm grid in "mm/d").  For brown, auer and dai: ``|device - restatement| <= 1e-12 * |pr|`` per
sample and ``1e-12 *`` the sum of the absolute terms per period sum, the tolerance of the agro and hydro units (the device's tanh
and its interpolation may round the last bit differently).  The counts and dates of the fractional methods are exact because the
fields keep every snow amount more than 1e-9 relative away from every threshold (asserted in tests/test_phase_cpu.py)."""

import numpy as np
import pytest

import phasecpu as R
import stridedabi as S
from stridedabi import PHASE_TABLE
from test_phase_cpu import CASES, META, OUTPUTS, check_known_answers, golden_case, margin, mirror_api, refusals
from xclim_amd import kernels as K
from xclim_amd import phase
from xclim_amd.timeaxis import TimeAxis
from unwritten import watched  # noqa: F401  (autouse: after every call of an entry point no output element may still hold the poison)
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu
CELLS = (1, 63, 64, 65, 257)       # one lane, a wave less one, a wave, a wave and one, more than one workgroup of 256
FREQS = ("YS", "YS-JUL", "MS")
SUMS = ("pr_sum", "solid_sum", "liquid_sum", "snow_sum_over")
RTOL = 1e-12


def setup(dev, name, cells=None, freq=None):
    """(meta, pr, second, time, freq, partition, keywords of the kernel call) of a golden case tiled to ``cells`` columns."""
    m, pr, second, _ = golden_case(name)
    idx = np.arange(pr.shape[1] if cells is None else cells) % pr.shape[1]
    pr, second = np.ascontiguousarray(pr[:, idx]), np.ascontiguousarray(second[:, idx])
    time = TimeAxis.daily(m["start"], len(pr))
    kw = dict(m["params"])
    land = kw.pop("landmask", True)
    if isinstance(land, list):
        land = np.array(land, bool)[idx]
    method, thresh, units, clip = kw.pop("method", "given"), kw.pop("thresh", None), kw.pop("units", "K"), kw.pop("clip_temp", None)
    part = phase.partition(method, thresh, units=units, dtype=pr.dtype, time=time, clip_temp=clip, landmask=land, cell_shape=(len(idx),),
                           device=dev)
    lim = {"snow_low": kw.get("snow_low", 0.0), "snow_high": R.SNOW_HIGH, "snow_thresh": kw.get("snow_thresh", 1.0)}
    off = R.K2C if units == "K" else 0.0
    pd = R.PER_DAY[m["flux_units"]]
    if method != "given":
        rnd = (lambda v: float(np.float32(v))) if pr.dtype == np.float32 else float
        lim.update(hplt_pr=rnd(kw.get("pr_thresh", 0.4 / pd)), hplt_tas=rnd(kw.get("tas_thresh", -0.2 + off)),
                   rofg_pr=rnd(kw.get("rofg_thresh", 1.0 / pd)), rofg_frz=rnd(off))
    rest = dict(m["params"], landmask=land) if method != "given" else dict(m["params"])
    return m, pr, second, time, freq or m["freq"], part, dict(per_day=pd, doy=time.doy, **lim), rest


def launch(dev, name, cells=None, freq=None, outputs=None):
    m, pr, second, time, freq, part, kw, _ = setup(dev, name, cells, freq)
    seg = time.segments(freq)[0]
    outs = K.precip_phase_period(dev, dev.to_device(pr), dev.to_device(second), seg, part, outputs or m["outputs"], **kw)
    return {k: v.get() for k, v in outs.items()}


def expected(dev, name, cells=None, freq=None):
    """The restatement on the same columns: ({output: (P, C)}, {sum output: the sum of its absolute terms})."""
    m, pr, second, _, freq, _, kw, rest = setup(dev, name, cells, freq)
    time = R.otime(m["start"], len(pr))
    exp = R.period_outputs(pr, second, time, freq, given=m["given"], per_day=kw["per_day"], **rest)
    mag = R.period_outputs(np.abs(pr), second, time, freq, given=m["given"], per_day=kw["per_day"], **rest)
    return exp, {k: np.abs(mag[k]) for k in SUMS}


def compare(name, got, exp, mag, what=""):
    m = META[name]
    exact = m["given"] or m["params"]["method"] == "binary"
    for k, g in got.items():
        assert g.dtype == np.float64 and g.shape == exp[k].shape, (name, k)
        if exact or k not in SUMS:
            np.testing.assert_array_equal(g, exp[k], err_msg=f"{name} {k} {what}")
        else:
            assert (np.abs(g - exp[k]) <= RTOL * mag[k]).all(), (name, k, what, float(np.max(np.abs(g - exp[k]) / np.maximum(mag[k], 1e-300))))


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(dev, name):
    m, _, _, stored = golden_case(name)
    got = launch(dev, name)
    assert list(got) == [o for o in OUTPUTS if o in m["outputs"]]
    exp, mag = expected(dev, name)
    compare(name, got, stored, mag, "stored")
    compare(name, got, exp, mag, "restated")
    if "no_snow_day" in m["family"]:
        assert (got["solid_sum"][:, 2] == 0).all() and np.isnan(got["first_snow"][:, 2]).all() and (got["snow_n_over"][:, 2] == 0).all()
    if "all_nan_period" in m["family"]:
        p = list(TimeAxis.daily(m["start"], 800).segments(m["freq"])[1]).index((2000, 1))
        assert got["pr_sum"][p, 6] == 0 and got["pr_n"][p, 6] == 0 and got["tas_n"][p, 6] == 0 and np.isnan(got["last_snow"][p, 6])
    if "rofg_early_thaw" in m["family"]:
        ys = launch(dev, name, freq="YS", outputs=["rofg_days"])["rofg_days"]
        np.testing.assert_array_equal(ys[:, 8], [1, 0, 0])      # the thaw on row 6 never counts, the one on row 30 does
        np.testing.assert_array_equal(ys[:, 9], [2, 1, 0])      # row 7 counts; the freeze run that crosses into 2000 ends in a count there
        np.testing.assert_array_equal(ys[:, 10], [1, 2, 0])     # row 8; the first row of 2000 (warmed on 1999's rows); 5 rows after a thaw: none


@pytest.mark.parametrize("freq", FREQS)
@pytest.mark.parametrize("name", CASES)
def test_every_frequency(dev, name, freq):
    got = launch(dev, name, freq=freq)
    exp, mag = expected(dev, name, freq=freq)
    compare(name, got, exp, mag, freq)
    P = len(TimeAxis.daily("1999-06-10", 800).segments(freq)[0]) - 1
    assert got["pr_sum"].shape[0] == P == {"YS": 3, "YS-JUL": 4, "MS": 27}[freq]


@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("name", ["exact.float32", "exact.float64", "auer.float32", "dai_seasonal.float32", "given.float32"])
def test_cell_counts(dev, name, cells):
    got = launch(dev, name, cells)
    exp, mag = expected(dev, name, cells)
    compare(name, got, exp, mag, f"C={cells}")


@pytest.mark.parametrize("name", ["exact.float32", "brown.float64", "dai_clip.float64", "given.float32"])
def test_every_single_output_equals_the_full_launch(dev, name):
    """The values do not depend on the subset: each output alone, and a few pairs, against all together, bit for bit."""
    names = META[name]["outputs"]
    full = launch(dev, name, 65)
    for subset in [[o] for o in names] + [names[:3], names[3:7], names[-2:], names[::2]]:
        got = launch(dev, name, 65, outputs=subset)
        assert list(got) == [o for o in OUTPUTS if o in subset]
        for k, g in got.items():
            np.testing.assert_array_equal(g, full[k], err_msg=f"{name} {subset}: {k}")


# ---- xh_precip_phase_map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [64, 65, 260])
@pytest.mark.parametrize("name", [n for n in CASES if not META[n]["given"]])
def test_map_against_the_restatement(dev, name, cells):
    """64 and 260 columns take the 16-byte loads (4 float32 or 2 float64 cells per lane), 65 the scalar ones."""
    m, pr, tas, time, _, part, _, rest = setup(dev, name, cells)
    snow, rain = R.split(pr, tas, rest["method"], rest.get("thresh"), rest.get("units", "K"), time.month, rest.get("clip_temp"), rest["landmask"])
    x, t = dev.to_device(pr), dev.to_device(tas)
    both = {k: v.get() for k, v in K.precip_phase_map(dev, x, t, part).items()}
    binary = rest["method"] == "binary"
    for k, want in (("snow", snow), ("rain", rain)):
        g = both[k]
        assert g.dtype == (pr.dtype if binary else np.float64) and g.shape == pr.shape
        np.testing.assert_array_equal(np.isnan(g), np.isnan(want), err_msg=f"{name} {k}: NaN pattern")
        if binary:
            np.testing.assert_array_equal(g, want, err_msg=f"{name} {k}")
        else:
            ok = ~np.isnan(want)
            assert (np.abs(g - want)[ok] <= RTOL * np.abs(pr.astype(np.float64))[ok]).all(), (name, k)
        alone = K.precip_phase_map(dev, x, t, part, outputs=(k,))
        assert list(alone) == [k]
        np.testing.assert_array_equal(alone[k].get(), g, err_msg=f"{name} {k} alone")


@pytest.mark.parametrize("name", ["exact.float64", "brown.float64", "dai_clip.float64"])
def test_fused_outputs_equal_the_map_and_the_existing_entry_points(dev, name):
    """xh_precip_phase_map, then xh_resample_reduce_f64 (sum, count) and xh_threshold_count_f64 on the snow field it wrote: the
    composed path the fused kernel replaces, on the same device ("mm/d" fields: the daily amount is the field itself)."""
    m, pr, tas, time, freq, part, kw, _ = setup(dev, name, 65)
    assert m["flux_units"] == "mm/d"
    seg = time.segments(freq)[0]
    x, t = dev.to_device(pr), dev.to_device(tas)
    fused = {k: v.get() for k, v in K.precip_phase_period(dev, x, t, seg, part, ("solid_sum", "liquid_sum", "solid_n", "snow_n_over"), **kw).items()}
    field = K.precip_phase_map(dev, x, t, part)
    _, mag = expected(dev, name, 65)
    for k in ("solid", "liquid"):
        total = K.resample_reduce(dev, field["snow" if k == "solid" else "rain"], "sum", seg, want_valid=False)[0].get()
        assert (np.abs(fused[k + "_sum"] - total) <= RTOL * mag[k + "_sum"]).all(), (name, k)
    np.testing.assert_array_equal(fused["solid_n"], K.resample_reduce(dev, field["snow"], "count", seg, want_valid=False)[0].get())
    over = K.threshold_count(dev, field["snow"], ">=", seg, scalar=kw["snow_thresh"], scalar_f64=True, want_valid=False)[0].get()
    np.testing.assert_array_equal(fused["snow_n_over"], over)


# ---- the mirrors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_mirrors_equal_the_kernel_calls(dev, name):
    m, pr, second, time, freq, part, kw, rest = setup(dev, name)
    got = launch(dev, name)
    args = {k: v for k, v in rest.items() if k not in ("snow_low", "snow_thresh", "pr_thresh", "tas_thresh", "rofg_thresh")}
    lim = {k: rest[k] for k in ("snow_low", "snow_thresh", "pr_thresh", "tas_thresh", "rofg_thresh") if k in rest}
    common = dict(time=time, flux_units=m["flux_units"], device=dev, freq=freq)
    if m["given"]:
        r = phase.phase_indices(pr, prsn=second, outputs=m["outputs"], snow_high=R.SNOW_HIGH, **lim, **common)
    else:
        r = phase.phase_indices(pr, second, outputs=m["outputs"], **args, **lim, **common)
    for k in m["outputs"]:
        np.testing.assert_array_equal(r[k], got[k], err_msg=f"{name} {k}: phase_indices")
    seg = time.segments(freq)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        intensity = np.where(got["snow_n_over"] > 0, got["snow_sum_over"] / got["snow_n_over"], 0.0)
        if m["given"]:
            np.testing.assert_array_equal(phase.first_snowfall(second, lim["snow_thresh"], **common), got["first_snow"])
            np.testing.assert_array_equal(phase.snowfall_intensity(second, lim["snow_thresh"], **common), intensity)
            one = K.precip_phase_period(dev, dev.to_device(pr), dev.to_device(second), seg, part, ("pr_sum", "solid_sum"), **dict(kw, per_day=1.0))
            one = {k: v.get() for k, v in one.items()}
            np.testing.assert_array_equal(phase.liquid_precip_ratio(pr, prsn=second, **common), (one["pr_sum"] - one["solid_sum"]) / one["pr_sum"])
            return
        how = {k: v for k, v in args.items() if k != "thresh"}      # method, units, clip_temp, landmask
        thresh = args.get("thresh")
        np.testing.assert_array_equal(phase.precip_accumulation(pr, second, "solid", thresh, **how, **common), got["solid_sum"])
        np.testing.assert_array_equal(phase.precip_average(pr, second, "liquid", thresh, **how, **common), got["liquid_sum"] / got["liquid_n"])
        np.testing.assert_array_equal(phase.last_snowfall(pr=pr, tas=second, thresh=lim["snow_thresh"], phase_thresh=thresh, **how, **common),
                                      got["last_snow"])
        np.testing.assert_array_equal(phase.snowfall_intensity(pr=pr, tas=second, thresh=lim["snow_thresh"], phase_thresh=thresh, **how, **common),
                                      intensity)
        np.testing.assert_array_equal(phase.snowfall_frequency(pr=pr, tas=second, thresh=lim["snow_low"], phase_thresh=thresh, **how, **common),
                                      got["snow_days"] / got["solid_n"] * 100)
        one = K.precip_phase_period(dev, dev.to_device(pr), dev.to_device(second), seg, part, ("pr_sum", "solid_sum"), **dict(kw, per_day=1.0))
        one = {k: v.get() for k, v in one.items()}
        ratio = (one["pr_sum"] - one["solid_sum"]) / one["pr_sum"]
        np.testing.assert_array_equal(phase.liquid_precip_ratio(pr, tas=second, thresh=thresh, **how, **common), ratio)
        if freq == "YS-JUL":
            assert phase.winter_rain_ratio(pr=pr, tas=second, thresh=thresh, **how, **common).shape[0] == 0      # no period is labelled in December
        if args["method"] == "binary":
            np.testing.assert_array_equal(phase.high_precip_low_temp(pr, second, lim["pr_thresh"], lim["tas_thresh"], units=how["units"], **common),
                                          got["hplt_days"])
            np.testing.assert_array_equal(phase.rain_on_frozen_ground_days(pr, second, lim["rofg_thresh"], units=how["units"], **common), got["rofg_days"])
    snow, rain = phase.phase_approximation(pr, second, args.get("thresh"), args["method"], args.get("clip_temp"), args.get("landmask", True), time=time,
                                           units=args.get("units", "K"), device=dev)
    field = K.precip_phase_map(dev, dev.to_device(pr), dev.to_device(second), part)
    np.testing.assert_array_equal(snow, field["snow"].get())
    np.testing.assert_array_equal(rain, field["rain"].get())


def test_known_answers_on_the_device(dev):
    """The test that fails without the feature: the reference's own answers through the mirror on the device."""
    assert check_known_answers(mirror_api(dev)) == 33


def test_missing_mask_keep_and_empty_shapes(dev):
    m, pr, tas, time, freq, part, kw, rest = setup(dev, "exact.float64")
    common = dict(time=time, flux_units="mm/d", device=dev, freq="YS", units="K", thresh=rest["thresh"])
    plain = phase.phase_indices(pr, tas, outputs=("solid_sum", "rofg_days"), **common)
    masked = phase.phase_indices(pr, tas, outputs=("solid_sum", "rofg_days"), mask_missing=True, **common)
    for k in plain:
        assert np.isnan(masked[k][0]).all() and np.isnan(masked[k][2]).all()          # the partial first and last years
        ok = ~np.isnan(pr[205:571]).any(axis=0) & ~np.isnan(tas[205:571]).any(axis=0)     # the rows of the year 2000
        np.testing.assert_array_equal(masked[k][1, ok], plain[k][1, ok])
        assert np.isnan(masked[k][1, ~ok]).all() and ok.sum() >= 5
    kept = phase.phase_indices(pr, tas, outputs=("solid_sum",), keep=True, **common)
    np.testing.assert_array_equal(kept["solid_sum"].get(), plain["solid_sum"])
    with pytest.raises(ValueError, match="keep=True"):
        phase.phase_indices(pr, tas, outputs=("solid_sum",), keep=True, mask_missing=True, **common)
    assert phase.phase_indices(pr[:, :0], tas[:, :0], outputs=("solid_sum",), **common)["solid_sum"].shape == (3, 0)
    assert phase.snowfall_approximation(pr[:, :0], tas[:, :0], device=dev).shape == (800, 0)
    seg = np.array([0, 0, 300, 300, 800])      # empty periods: sums and counts 0, dates NaN
    outs = K.precip_phase_period(dev, dev.to_device(pr), dev.to_device(tas), seg, part, OUTPUTS, **kw)
    for k, v in outs.items():
        g = v.get()
        assert (np.isnan(g[[0, 2]]) if k in ("first_snow", "last_snow") else g[[0, 2]] == 0).all(), k
    with pytest.raises(ValueError, match="need a temperature"):
        K.precip_phase_period(dev, dev.to_device(pr), dev.to_device(tas), seg, phase.partition("given"), ("hplt_days",))


# ---- padded, poisoned row views --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,pitch", [("exact.float32", 65, 80), ("auer.float64", 64, 72), ("dai_seasonal.float32", 130, 144)])
def test_padded_views_give_the_same_bits(dev, monkeypatch, name, C, pitch):
    """Every strided operand of the two entry points in rows of `pitch` elements, NaN / 1e30 in the extra columns of the inputs and
    in front of their first row, 0xA5 bytes in those of the outputs (tests/stridedabi.py: padded, which asserts that they stay)."""
    for entry, ops in PHASE_TABLE.items():
        for op in ops:
            assert {op.ptr, op.stride} <= set(S.parameters(entry)), (entry, op)
    m, pr, tas, time, freq, part, kw, _ = setup(dev, name, C)

    def run():
        out = launch(dev, name, C)
        out.update({k: v.get() for k, v in K.precip_phase_map(dev, dev.to_device(pr), dev.to_device(tas), part).items()})
        return out

    plain = run()
    with S.padded(dev, monkeypatch, pads=(pitch - C, pitch - C), shift=5) as log:
        got = run()
    assert set(got) == set(plain) and len(got) == 16
    for k, g in got.items():
        np.testing.assert_array_equal(g, plain[k], err_msg=f"{k} differs under row pitches {log}")
    assert [n for n, _ in log] == ["xh_precip_phase_period", "xh_precip_phase_map"]
    assert all(used == {"ld": (pitch, C), "ld_out": (pitch, C)} for _, used in log), log


def test_every_output_operand_was_armed_and_checked(dev, watched):
    launch(dev, "exact.float32", 65)
    m, pr, tas, _, _, part, _, _ = setup(dev, "brown.float64", 64)
    K.precip_phase_map(dev, dev.to_device(pr), dev.to_device(tas), part)
    seen = {n: armed for n, armed in watched if n in PHASE_TABLE}
    assert set(seen) == set(PHASE_TABLE)
    assert set(seen["xh_precip_phase_map"]) == {"snow_out", "rain_out"} and all(seen["xh_precip_phase_map"].values())
    assert set(seen["xh_precip_phase_period"]) == {f"outs[{k}]" for k in range(len(OUTPUTS))} and all(seen["xh_precip_phase_period"].values())


def test_the_fractional_cases_keep_their_margin():
    for name in CASES:
        if META[name]["params"].get("method") not in ("binary", None):
            assert margin(name) > 1e-9, name


def test_refusals(dev):
    refusals(dev)
