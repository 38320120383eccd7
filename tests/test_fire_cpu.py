"""CPU checks of the fire weather system: the numpy restatement (tests/firecpu.py) against the reference's own outputs
(tests/golden/fire_vectors.npz, tests/golden/make_fire_golden.py), the reference's known answers, the C ABI of the two
new entry points and the argument errors of xclim_amd.fire (raised before any device is touched)."""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import firecpu  # noqa: E402
import stridedabi as S  # noqa: E402

from xclim_amd import _capi  # noqa: E402
from xclim_amd import fire  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "fire_vectors.npz"))
CASES = [str(c) for c in GOLD["cases"]]


def golden_case(name):
    """Inputs of a golden case with TIME FIRST, its parameters and its expected outputs (time first)."""
    g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
    P = json.loads(str(g["params"]))
    inp = {}
    for k in ("tas", "pr", "hurs", "sfcWind", "snd"):
        if k in g:  # int16 multiples of 1 / scale, NaN = -32768 (tests/golden/make_fire_golden.py: decode)
            q, scale = g[k], float(GOLD[f"input_scale/{k}"])
            inp[k] = np.ascontiguousarray(np.where(q == -32768, np.nan, q / scale).astype(np.float32).T)
        else:  # the snow depth of a case whose season never reads it
            inp[k] = np.zeros_like(inp["tas"])
    if "season_mask_in" in g:
        inp["season_mask"] = np.ascontiguousarray(g["season_mask_in"].T)
    inp["month"] = g["month"].astype(np.int64)
    for k in ("lat", "dc0", "dmc0", "ffmc0", "winter_pr_in"):
        inp[k] = g[k]
    exp = {k[4:]: (np.ascontiguousarray(v.T) if v.ndim == 2 else v) for k, v in g.items() if k.startswith("out_")}
    return inp, P, exp


def check_outputs(got, exp, rtol=1e-6, atol=1e-5):
    """Codes and indexes to rtol 1e-6 (the reference's own bar against cffdrs) with a small atol for values near 0 and
    for the float32 exp / log / pow of numpy (not correctly rounded); masks bit-exact; NaN where the reference has NaN."""
    assert set(got) == set(exp), (sorted(got), sorted(exp))
    for k, e in exp.items():
        g = np.asarray(got[k])
        assert g.shape == e.shape, (k, g.shape, e.shape)
        if k == "season_mask":
            np.testing.assert_array_equal(g.astype(bool), e.astype(bool), err_msg=k)
        else:
            np.testing.assert_allclose(g.astype(np.float64), e.astype(np.float64), rtol=rtol, atol=atol, equal_nan=True, err_msg=k)


def test_golden_cover_every_mode():
    modes = {json.loads(str(GOLD[f"{c}/params"]))["season_method"] for c in CASES}
    assert modes == {None, "mask", "WF93", "LA08", "GFWED"}
    dry = {json.loads(str(GOLD[f"{c}/params"]))["dry_start"] for c in CASES}
    assert dry == {None, "CFS", "GFWED"}
    lat = np.concatenate([GOLD[f"{c}/lat"] for c in CASES])
    assert set(np.unique(firecpu.band5(lat))) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name", CASES)
def test_firecpu_matches_reference(name):
    inp, P, exp = golden_case(name)
    kw = {k: P[k] for k in firecpu.DEFAULTS}
    got = firecpu.fire_weather(inp["tas"], inp["pr"], inp["hurs"], inp["sfcWind"], inp["snd"], inp["month"], inp["lat"],
                               indexes=P["indexes"], season_method=P["season_method"], season_mask=inp.get("season_mask"),
                               dc0=inp["dc0"], dmc0=inp["dmc0"], ffmc0=inp["ffmc0"], winter_pr=inp["winter_pr_in"],
                               overwintering=P["overwintering"], dry_start=P["dry_start"],
                               initial_start_up=P["initial_start_up"], **kw)
    check_outputs(got, exp)
    for k in ("DC", "DMC", "FFMC", "BUI", "winter_pr"):  # the float64 codes and the float32 BUI are exact here
        if k in exp:
            np.testing.assert_array_equal(got[k], exp[k], err_msg=k)


@pytest.mark.parametrize("inputs,exp", [([300, 110, 0.75, 0.75, 15], 109.4657), ([300, 110, 1.0, 0.9, 15], 16.35315),
                                        ([100, 50, 0.75, 0.75, 15], 105.176), ([1, 550, 0.75, 0.75, 10], 10)])
def test_overwintering_known_answers(inputs, exp):
    """The reference's test_overwintering_drought_code (tests/test_cffwis.py:124-153 of xclim)."""
    np.testing.assert_allclose(firecpu.overwintering_dc(*inputs), exp, rtol=1e-6)


def test_helper_known_answers():
    assert firecpu.day_length(44, 1) == 6.5 == float(GOLD["known/day_length_44_1"])
    assert firecpu.day_length_factor(44, 1) == -1.6 == float(GOLD["known/day_length_factor_44_1"])
    assert firecpu.bui_step(0, 0) == 0 == float(GOLD["known/bui_0_0"])
    with pytest.raises(ValueError):
        firecpu.day_length(91, 1)


@pytest.mark.parametrize("name,nargs", [("xh_fire_weather", 28), ("xh_overwintering_dc", 8)])
def test_entry_points_header_ctypes_and_exports(name, nargs):
    lib = _capi.load_library()
    assert hasattr(lib, name)
    assert len(S.header_declarations()[name]) == nargs == len(_capi.SIGNATURES[name])
    assert lib.xh_abi_version() == 1


def test_entry_points_reject_null_arguments():
    lib = _capi.load_library()
    null = ctypes.c_void_p(0)
    assert lib.xh_overwintering_dc(null, null, null, 4, 0.75, 0.75, 15.0, null) == _capi.XH_ERR_ARG
    rc = lib.xh_fire_weather(null, 10, 4, 4, *([null] * 12), 4, 0, 3, 3, 0, 0, 1, null, null, 4, null, null)
    assert rc == _capi.XH_ERR_ARG


def _series(T=100):
    one = np.ones((T, 2), np.float32)
    return one, TimeAxis.daily("2017-01-01", T, "noleap")


def test_fire_weather_ufunc_errors():
    """The reference's test_fire_weather_ufunc_errors (tests/test_cffwis.py:319-369 of xclim), in this API."""
    x, time = _series()
    lat = np.full(2, 45.0)
    nan = np.full(2, np.nan, np.float32)
    with pytest.raises(TypeError):  # ISI needs sfcWind
        fire.fire_weather_ufunc(tas=x, pr=x, hurs=x, lat=lat, dc0=nan, indexes=["DC", "ISI"], time=time)
    with pytest.raises(TypeError):  # DC needs lat
        fire.fire_weather_ufunc(tas=x, pr=x, dc0=nan, indexes=["DC"], time=time)
    with pytest.raises(TypeError):  # LA08 needs snd
        fire.fire_weather_ufunc(tas=x, pr=x, lat=lat, dc0=nan, indexes=["DC"], season_method="LA08", time=time)
    with pytest.raises(ValueError, match="dry_start"):
        fire.fire_weather_ufunc(tas=x, pr=x, lat=lat, indexes=["DC"], dry_start="US", time=time)
    with pytest.raises(ValueError, match="overwintering"):
        fire.fire_weather_ufunc(tas=x, pr=x, lat=lat, indexes=["DC"], overwintering=True, time=time)
    with pytest.raises(ValueError, match="not a valid parameter"):
        fire.drought_code(x, x, lat, time=time, dc_begin=3)
    with pytest.raises(NotImplementedError):  # GFWED dry start with snow depth: out of scope, no CPU fallback
        fire.fire_weather_ufunc(tas=x, pr=x, lat=lat, snd=x, indexes=["DC"], season_method="WF93", dry_start="GFWED", time=time)


def test_fire_season_errors():
    x, _ = _series()
    with pytest.raises(ValueError, match="Thresholds must be scalar."):
        fire.fire_season(x, temp_start_thresh=np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="method"):
        fire.fire_season(x, method="XX")
    with pytest.raises(NotImplementedError):
        fire.fire_season(x, snd=x, method="GFWED", temp_condition_days=8)
