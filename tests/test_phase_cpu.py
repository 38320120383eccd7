"""The snow / rain partition unit without a GPU: the numpy restatement tests/phasecpu.py reproduces the known answers of the
reference's own tests (tests/golden/phase_known_answers.json: 13 of the two approximations, 20 of the period indices) to the
tolerances those tests use, and the golden file tests/golden/phase_vectors.npz; the host logic of the mirror (season bytes, the
fmin / fmax swap of the dai methods, the auer table, the float32 rounding of ``thresh``, the winter periods); what the mirror
does not serve; the mirrors of the header's #defines (tests/test_abi_cpu.py checks header, ctypes table and library).  ``check_known_answers`` and ``refusals`` are shared with
tests/test_gpu_phase.py (the device) and tests/test_hostsim_phase_cpu.py (the host simulation).

None of the listed tests of the reference needs a data file, so none is left out; the three unit variants of the snowfall tests
(mm/day, m s-1, kg m-2 s-1) are one case in mm/d, thresholds being plain numbers here."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import phasecpu as R
import stridedabi as S
from stridedabi import PHASE_TABLE
from xclim_amd import _capi, phase
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "xclim_hip_phase.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "phase_vectors.npz")
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "phase_known_answers.json")))
_vp = ctypes.c_void_p
OUTPUTS = _capi.PHASE_OUTPUTS


def build(spec, start):
    """A (rows, 1) float64 series of the known-answer file: values, a base with spans, or a rule on the row / the year."""
    if "values" in spec:
        return np.asarray(spec["values"], np.float64)[:, None]
    rows = spec["rows"]
    if spec.get("value") == "year":
        return TimeAxis.daily(start, rows).year.astype(np.float64)[:, None]
    if "value" in spec:
        return np.array([eval(spec["value"], {"abs": abs}, {"row": r}) for r in range(rows)], np.float64)[:, None]  # noqa: S307
    a = np.full((rows, 1), float(spec["base"]))
    for lo, hi, v in spec["spans"]:
        a[lo:hi] = v
    return a


# ---- the two ways to an answer: the restatement, and the mirror on a device ---------------------------------------------
class Restated:
    @staticmethod
    def approximation(fn, pr, tas, start, units, method, thresh, clip_temp, landmask):
        month = R.otime(start, len(pr)).month
        return R.split(pr, tas, method, thresh, units, month, clip_temp, landmask)[fn == "rain_approximation"]

    @staticmethod
    def period(fn, pr, second, given, start, freq, flux_units, units, args):
        time = R.otime(start, len(pr))
        pd = R.PER_DAY[flux_units]
        kw = {"units": units, **{k: v for k, v in args.items() if k in ("pr_thresh", "tas_thresh")}}
        if fn in ("precip_accumulation", "precip_average"):
            return getattr(R, fn)(pr, second, args.get("phase"), time, freq, pd, thresh=args.get("thresh"), units=units)
        if fn in ("liquid_precip_ratio", "winter_rain_ratio"):
            out = R.liquid_precip_ratio(pr, second, time, freq, given=given, units=units)
            return out[R.winter(time, freq)] if fn == "winter_rain_ratio" else out
        if fn == "rain_on_frozen_ground_days":
            kw.update(rofg_thresh=args.get("thresh"))
        elif fn != "high_precip_low_temp":   # the four snowfall indices: "1 mm/day" by default
            kw.update(snow_thresh=args.get("thresh", 1.0), snow_low=args.get("thresh", 1.0))
        o = R.period_outputs(pr, second, time, freq, given=given, per_day=pd, **kw)
        if fn == "snowfall_frequency":
            return R.snowfall_frequency(o)
        if fn == "snowfall_intensity":
            return R.snowfall_intensity(o)
        return o[{"rain_on_frozen_ground_days": "rofg_days", "high_precip_low_temp": "hplt_days", "first_snowfall": "first_snow",
                  "last_snowfall": "last_snow"}[fn]]


def mirror_api(dev):
    """xclim_amd.phase on ``dev`` behind the same two signatures."""

    class Mirror:
        @staticmethod
        def approximation(fn, pr, tas, start, units, method, thresh, clip_temp, landmask):
            time = TimeAxis.daily(start, len(pr))
            return getattr(phase, fn)(pr, tas, thresh, method, clip_temp, landmask, time=time, units=units, device=dev)

        @staticmethod
        def period(fn, pr, second, given, start, freq, flux_units, units, args):
            kw = {"time": TimeAxis.daily(start, len(pr)), "flux_units": flux_units, "units": units, "device": dev, "freq": freq}
            f = getattr(phase, fn)
            if fn in ("precip_accumulation", "precip_average"):
                return f(pr, second, args.get("phase"), args.get("thresh"), **kw)
            if fn == "liquid_precip_ratio":
                return f(pr, prsn=second if given else None, tas=None if given else second, **kw)
            if fn == "winter_rain_ratio":
                return f(pr=pr, prsn=second if given else None, tas=None if given else second, **kw)
            if fn in ("high_precip_low_temp", "rain_on_frozen_ground_days"):
                return f(pr, second, **args, **kw)
            return f(second, **args, **kw) if given else f(pr=pr, tas=second, **args, **kw)

    return Mirror


def check_known_answers(f=Restated):
    for k in KNOWN["approximation"]:
        cells = k.get("cells", 1)
        pr, tas = (np.repeat(np.asarray(k[n], np.float64)[:, None], cells, axis=1) for n in ("pr", "tas"))
        land = k["landmask"] if isinstance(k["landmask"], bool) else np.array(k["landmask"], bool)
        got = f.approximation(k["function"], pr, tas, k["start"], k["units"], k["method"], k["thresh"], k["clip_temp"], land)
        want = np.asarray(k["expected"], np.float64).reshape(cells, -1).T
        np.testing.assert_allclose(got, want, atol=k["atol"], rtol=k["rtol"], err_msg=k["name"])
    for k in KNOWN["period"]:
        pr = build(k["pr"], k["start"])
        given = k["second"] == "prsn" or k["second"] is None
        second = (pr if k["second"] == "prsn" else None) if given else build(k["second"]["tas"], k["start"])
        got = f.period(k["function"], pr, second, k["second"] == "prsn", k["start"], k["freq"], k["flux_units"], k["units"], dict(k["arguments"]))
        got = np.asarray(got)[:, 0]
        want = np.asarray(k["expected"], np.float64)
        got = got[:len(want)] if k["check"] == "first" else got
        if k["tolerance"] == "equal":
            np.testing.assert_array_equal(got, want, err_msg=k["name"])
        elif k["tolerance"] == "decimal7":
            np.testing.assert_almost_equal(got, want, err_msg=k["name"])
        else:
            np.testing.assert_allclose(got, want, err_msg=k["name"])
    return len(KNOWN["approximation"]) + len(KNOWN["period"])


def test_restatement_reproduces_the_known_answers():
    assert check_known_answers() == 33
    names = {k["name"] for k in KNOWN["approximation"] + KNOWN["period"]}
    assert len(names) == 33


# ---- the host logic of the mirror -------------------------------------------------------------------------------------------
def test_season_bytes_follow_the_months():
    t = TimeAxis.daily("2000-11-29", 400)
    s = phase.season_bytes(t)
    assert s.dtype == np.uint8 and s.shape == (400,)
    for month, season in ((12, 0), (1, 0), (2, 0), (3, 1), (5, 1), (6, 2), (8, 2), (9, 3), (11, 3)):
        assert (s[t.month == month] == season).all(), month
    np.testing.assert_array_equal(s, R.seasons(t.month))


def test_auer_table_of_the_mirror_and_of_the_restatement():
    nodes, vals = phase.auer_table()
    rn, rv = R.auer_nodes()
    np.testing.assert_array_equal(nodes, rn)
    np.testing.assert_allclose(vals, rv, rtol=0, atol=1e-15)
    assert len(nodes) == 103 and (np.diff(nodes) > 0).all() and vals[0] == 1 and (vals[-2:] == 0).all() and nodes[1] == 0 and nodes[-2] == 6
    assert (vals >= 0).all() and (vals <= 1).all()


@pytest.mark.parametrize("method", ["dai_annual", "dai_seasonal"])
def test_fmin_and_fmax_swap_between_snow_and_rain(method):
    tab = phase.dai_table(method, 5.0)
    assert tab.shape == (2, 2, 4, 6) and tab.size == _capi.PHASE_DAI_NTAB
    a, b, c, d, fmin, den = np.moveaxis(tab, -1, 0)

    def f(t):
        return a * (np.tanh(b * (t - c)) - d) / 100

    np.testing.assert_array_equal(fmin[0], f(5.0)[0])              # snow: fmin at +clip, fmax at -clip
    np.testing.assert_array_equal(den[0], (f(-5.0) - f(5.0))[0])
    np.testing.assert_array_equal(fmin[1], f(-5.0)[1])             # rain: the other way round
    np.testing.assert_array_equal(den[1], (f(5.0) - f(-5.0))[1])
    assert (den > 0).all()                                         # both rescaled fractions run from 0 to 1
    assert np.isnan(phase.dai_table(method)[..., 4:]).all()
    if method == "dai_annual":
        assert (tab == tab[:, :, :1]).all()


def test_thresh_is_rounded_to_float32_on_a_float32_field():
    t = 273.16                                    # float32 rounds it UP, to 273.160003662109375
    p32, p64 = phase.partition("binary", t, dtype=np.float32), phase.partition("binary", t, dtype=np.float64)
    assert p32["par"][0] == float(np.float32(t)) > t and p64["par"][0] == t
    tas = np.array([np.float32(t)], np.float32)   # equals the rounded threshold, lies above the float64 one
    assert (tas <= t).all() and not (tas.astype(np.float64) <= t).any()   # numpy >= 2 rounds the Python scalar; float64 would not
    assert (tas.astype(np.float64) <= p32["par"][0]).all()
    t = 273.15
    assert phase.partition("binary", None, units="degC")["par"][0] == 0.0 and phase.partition("binary", None, units="K")["par"][0] == t
    b = phase.partition("brown", 274.15, units="K")["par"]
    assert b[0] == 274.15 and b[1] == ((274.15 - 273.15) + 2) + 273.15
    a = phase.partition("auer", 1.0, units="degC")["par"]
    assert a[0] == 274.15 and a[2] == 273.15 and phase.partition("auer", 274.15, units="K")["par"][2] == 0.0


def test_winter_periods():
    t = TimeAxis.daily("2000-12-01", 450)
    np.testing.assert_array_equal(phase.winter_periods(t, "QS-DEC"), [True, False, False, False, True])
    np.testing.assert_array_equal(phase.winter_periods(t, "QS-DEC"), R.winter(R.otime("2000-12-01", 450), "QS-DEC"))


def test_axes_and_arguments_that_are_not_served():
    t = TimeAxis.daily("2000-01-01", 400)
    pr, tas = np.ones((400, 2)), np.full((400, 2), 270.0)
    gappy = t.subset(np.r_[0:10, 11:400])
    with pytest.raises(phase.NotServed):
        phase.precip_accumulation(pr[:399], tas[:399], "solid", time=gappy)
    with pytest.raises(phase.NotServed):
        phase.precip_accumulation(pr[::30], tas[::30], "solid", time=t.subset(slice(None, None, 30)))
    with pytest.raises(phase.NotServed, match="integer"):
        phase.precip_accumulation(pr.astype(np.int32), tas, "solid", time=t)
    with pytest.raises(phase.NotServed, match="scalar"):
        phase.precip_accumulation(pr, tas, "solid", np.full(2, 270.0), time=t)
    with pytest.raises(phase.NotServed, match="window = 7"):
        phase.rain_on_frozen_ground_days(pr, tas, window=5, time=t)
    with pytest.raises(ValueError, match="not one of 'binary', 'brown', 'auer', 'dai_annual' or 'dai_seasonal'"):
        phase.snowfall_approximation(pr, tas, method="linear")
    with pytest.raises(ValueError, match="Unknown method dai_monthly for rain approximation"):
        phase.rain_approximation(pr, tas, method="dai_monthly")
    with pytest.raises(ValueError, match="Non-scalar `thresh` are not allowed with method `brown`"):
        phase.snowfall_approximation(pr, tas, np.full(2, 270.0), method="brown")
    with pytest.raises(ValueError, match="units"):
        phase.snowfall_approximation(pr, tas, units="degF")
    with pytest.raises(ValueError, match="flux_units"):
        phase.precip_accumulation(pr, tas, "solid", time=t, flux_units="in/d")
    with pytest.raises(KeyError):
        phase.liquid_precip_ratio(pr, time=t)
    with pytest.raises(TypeError, match="Freq must be a string"):
        phase.precip_accumulation(pr, tas, "solid", freq=3, time=t)
    assert phase.converters.ADAPTED == ("snowfall_approximation", "rain_approximation")
    assert len(phase.multivariate.ADAPTED) == 6 and len(phase.threshold.ADAPTED) == 4


# ---- the golden file ------------------------------------------------------------------------------------------------------
_Z = np.load(GOLDEN, allow_pickle=False)
META = json.loads(str(_Z["meta"]))
CASES = sorted(META)
FAMILIES = ("at_thresh", "brown_upper", "auer_nodes", "dai_clip", "season_change", "land_ocean", "nan_pr", "no_snow_day", "all_nan_period",
            "rofg_early_thaw", "rofg_boundary", "rofg_first_row", "random")


def golden_case(name):
    """(meta, pr, second, expected {output: (P, C)}) of one case."""
    m = META[name]
    return m, _Z[f"{name}/pr"], _Z[f"{name}/second"], {o: _Z[f"{name}/{o}"] for o in m["outputs"]}


def restated(name):
    m, pr, second, _ = golden_case(name)
    time = R.otime(m["start"], pr.shape[0])
    kw = dict(m["params"])
    if isinstance(kw.get("landmask"), list):
        kw["landmask"] = np.array(kw["landmask"], bool)
    return R.period_outputs(pr, second, time, m["freq"], given=m["given"], per_day=R.PER_DAY[m["flux_units"]], **kw)


def test_the_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    assert {f for m in META.values() for f in m["family"]} == set(FAMILIES)
    assert {m["params"].get("method", "given") for m in META.values()} == set(phase.METHODS) | {"given"}
    assert {m["dtype"] for m in META.values()} == {"float32", "float64"}


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden_file(name):
    m, _, _, exp = golden_case(name)
    got = restated(name)
    exact = m["given"] or m["params"]["method"] == "binary"
    for o in m["outputs"]:
        if exact or not o.endswith(("_sum", "_sum_over")):
            np.testing.assert_array_equal(got[o], exp[o], err_msg=f"{name} {o}")
        else:   # (tanh and the interpolation may round differently from one numpy build to the next)
            np.testing.assert_allclose(got[o], exp[o], rtol=1e-12, atol=0, err_msg=f"{name} {o}")


def margin(name):
    """The smallest relative distance of a day's snow amount from the thresholds it is compared with."""
    m, pr, second, _ = golden_case(name)
    kw = dict(m["params"])
    if m["given"]:
        snow = second.astype(np.float64)
    else:
        land = np.array(kw["landmask"], bool) if isinstance(kw.get("landmask"), list) else kw.get("landmask", True)
        snow = R.split(pr, second, kw["method"], kw.get("thresh"), kw.get("units", "K"), R.otime(m["start"], len(pr)).month, kw.get("clip_temp"), land)[0]
    sm = np.asarray(snow, np.float64) * R.PER_DAY[m["flux_units"]]
    lims = [kw.get("snow_low", 0.0), kw.get("snow_thresh", 1.0)]
    sm = sm[np.isfinite(sm)]
    return min(np.min(np.abs(sm - v) / max(abs(v), 1e-300)) if v else np.min(np.where(sm == 0, 1.0, np.abs(sm))) for v in lims)


@pytest.mark.parametrize("name", [n for n in CASES if "random" in META[n]["family"] and META[n]["params"].get("method") not in ("binary", None)])
def test_fractional_fields_keep_their_distance_from_the_thresholds(name):
    """A condition of the exact comparison of counts and dates on the fractional methods, not a tolerance."""
    assert margin(name) > 1e-9


# ---- the C ABI (tests/test_abi_cpu.py checks the header against the ctypes table, the library and the registry) ---------
def test_the_operand_table_is_the_header_s():
    assert set(S.prototypes(HEADER)) == set(PHASE_TABLE)
    assert PHASE_TABLE["xh_precip_phase_period"][-1].ptrs == len(OUTPUTS)


def test_the_methods_outputs_and_sizes_mirror_the_header():
    txt = open(HEADER).read()
    for k, o in enumerate(OUTPUTS):
        assert re.search(rf"#define XH_PHASE_{o.upper()} {k}\b", txt), o
    for m, k in _capi.PHASE_METHODS.items():
        assert re.search(rf"#define XH_PHASE_{m.upper()} {k}\b", txt), m
    assert f"#define XH_PHASE_NOUT {len(OUTPUTS)}" in txt and f"#define XH_PHASE_NPAR {_capi.PHASE_NPAR}" in txt
    assert f"#define XH_PHASE_DAI_NTAB {_capi.PHASE_DAI_NTAB}" in txt and f"#define XH_PHASE_NLIM {_capi.PHASE_NLIM}" in txt


def test_entry_points_reject_a_null_context():
    lib = _capi.load_library()
    null, some = _vp(0), _vp(64)   # never dereferenced: the check fails first
    assert lib.xh_precip_phase_map(null, 10, 4, 4, 0, some, some, 0, some, null, 0, null, null, some, some, 4) == _capi.XH_ERR_ARG
    assert lib.xh_precip_phase_period(null, 10, 4, 4, 0, some, some, 1.0, 1, some, null, 0, some, null, 0, null, null, some, 7, 1, some,
                                      4) == _capi.XH_ERR_ARG


def refusals(dev):
    """Every refusal is a code that answers before anything is launched: the sentinel in the outputs is intact afterwards, and the
    same call with nothing wrong then runs.  On the device (tests/test_gpu_phase.py) and, through it, on the host simulation."""
    ARG, LAYOUT, LIMIT = _capi.XH_ERR_ARG, _capi.XH_ERR_LAYOUT, _capi.XH_ERR_LIMIT
    T, C, P = 40, 8, 2
    x = dev.to_device(np.ones((T, C)))
    sentinel = np.full((P, C), 7.5)
    out, full = dev.to_device(sentinel), dev.to_device(np.full((T, C), 7.5))
    seg, doy = np.array([0, 20, 40], np.int64), np.arange(1, T + 1, dtype=np.int32)
    par, lim = np.zeros(6), np.zeros(7)
    nodes = np.concatenate(phase.auer_table())
    dai = phase.dai_table("dai_annual", 2.0).reshape(-1)
    p = _capi.np_ptr
    fmap, fper = (getattr(dev.lib, n) for n in PHASE_TABLE)

    def per(ld=C, ld_out=C, seg=seg, P=P, doy=doy, method=0, par=par, tab=None, ntab=0, season=None, window=7, mask=1 | 1 << 10, o=out, T=T):
        outs = np.array([o.ptr] * len(OUTPUTS), np.uint64)
        return fper(dev.ctx, T, C, ld, 1, _vp(x.ptr), _vp(x.ptr), 1.0, P, p(seg), p(doy) if doy is not None else _vp(0), method, p(par),
                    p(tab) if tab is not None else _vp(0), ntab, p(season) if season is not None else _vp(0), _vp(0), p(lim), window, mask,
                    p(outs), ld_out)

    def mp(ld=C, ld_out=C, method=0, tab=None, ntab=0, snow=full, par=par):
        return fmap(dev.ctx, T, C, ld, 1, _vp(x.ptr), _vp(x.ptr), method, p(par), p(tab) if tab is not None else _vp(0), ntab, _vp(0), _vp(0),
                    _vp(snow.ptr) if snow is not None else _vp(0), _vp(0), ld_out)

    assert per(ld=C - 1) == LAYOUT and per(ld_out=C - 1) == LAYOUT and mp(ld=C - 1) == LAYOUT and mp(ld_out=C - 1) == LAYOUT
    assert per(mask=0) == ARG and per(mask=1 << 14) == ARG                         # no output, an output that does not exist
    assert per(doy=None) == ARG                                                     # dates without days of year
    assert per(doy=np.zeros(T, np.int32)) == ARG
    assert per(seg=np.array([0, 30, 20], np.int64)) == ARG and per(seg=np.array([0, 20, 41], np.int64)) == ARG
    assert per(window=0) == ARG
    assert per(method=6) == ARG and per(method=-1) == ARG and mp(method=5) == ARG   # the given-snow method has no map
    assert per(method=5, mask=1 << 12) == ARG and per(method=5, mask=1 << 13) == ARG
    assert per(method=2) == ARG and per(method=2, tab=nodes[::-1].copy(), ntab=103) == ARG    # no table, nodes that decrease
    assert per(method=2, tab=np.zeros(2 * 5000), ntab=5000) == LIMIT
    assert per(method=3, tab=dai, ntab=95) == ARG
    clip = par.copy()
    clip[4] = 1
    assert per(method=3, tab=phase.dai_table("dai_annual").reshape(-1), ntab=96, par=clip) == ARG   # clip without fmin / fmax
    brown = par.copy()
    brown[:2] = 2.0, 2.0
    assert per(method=1, par=brown) == ARG and mp(method=1, par=brown) == ARG
    assert per(season=np.full(T, 4, np.uint8)) == ARG
    assert mp(snow=None) == ARG
    assert per(P=70000, seg=np.zeros(70001, np.int64)) == LIMIT
    np.testing.assert_array_equal(out.get(), sentinel)                                # nothing was launched
    assert (full.get() == 7.5).all()
    assert per() == 0 and per(method=2, tab=nodes, ntab=103) == 0 and per(method=3, tab=dai, ntab=96, par=clip) == 0 and mp() == 0
    assert per(T=0, P=0, seg=np.zeros(1, np.int64)) == 0
    dev.sync()
    assert not (out.get() == sentinel).any() and (full.get() == 0.0).all()   # (tas = 1 lies above thresh = 0: no snow)
