"""What the adapters of the period-index mirrors (anuclim, agro, hydrology, rainseason) share, without a device: the forwarding shim
of xr_adapter.py, the period front end of fields.py and the install helper of patch.py (through ``patch.install`` on stand-in
modules, as the adapter tests wire them)."""

import inspect
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fakexr  # noqa: E402
from xclim_amd import anuclim, patch, rainseason  # noqa: E402
from xclim_amd import fields as F  # noqa: E402
from xclim_amd.timeaxis import TimeAxis, parse_freq  # noqa: E402
from xclim_amd.xr_adapter import forwarding_adapter  # noqa: E402


# ---- forwarding_adapter -------------------------------------------------------------------------------------------------
def _orig(da, thresh="1 mm", freq="YS", *, op=">"):
    """the original's text"""
    return ("original", da, thresh, freq, op)


def test_arguments_that_do_not_bind_go_to_the_original_as_they_came():
    seen, ran = [], []

    def orig(*args, **kwargs):   # (what a call reaches after the binding against _orig's signature failed)
        seen.append((args, kwargs))
        return "original"

    orig.__signature__ = inspect.signature(_orig)
    fn = forwarding_adapter("index", orig, lambda p: ran.append(p) or "served")
    assert fn("x", "2 mm", "MS", "one too many", op="<") == "original"
    assert fn("x", no_such_keyword=1) == "original"
    assert fn() == "original"
    assert seen == [(("x", "2 mm", "MS", "one too many"), {"op": "<"}), (("x",), {"no_such_keyword": 1}), ((), {})]
    assert ran == []


def test_a_runner_that_raises_not_served_goes_to_the_original_with_the_same_arguments():
    def runner(p):
        raise F.NotServed("not this form")

    fn = forwarding_adapter("index", _orig, runner)
    assert fn("x", freq="MS", op="<") == ("original", "x", "1 mm", "MS", "<")


@pytest.mark.parametrize("error", [NotImplementedError, ValueError, KeyError])
def test_every_other_exception_of_the_runner_is_the_caller_s(error):
    def runner(p):
        raise error("the runner's own")

    fn = forwarding_adapter("index", _orig, runner)
    with pytest.raises(error, match="the runner's own") as e:
        fn("x")
    assert type(e.value) is error   # (NotServed is a NotImplementedError: the plain one is not taken for it)


def test_the_replacement_carries_the_original_s_name_text_and_wrapped():
    fn = forwarding_adapter("public_name", _orig, lambda p: None)
    assert fn.__wrapped__ is _orig and fn.__name__ == "public_name" and fn.__doc__ == "the original's text"


def test_the_runner_sees_the_bound_arguments_with_the_defaults_applied():
    fn = forwarding_adapter("index", _orig, dict)
    assert fn("x", freq="MS") == {"da": "x", "thresh": "1 mm", "freq": "MS", "op": ">"}
    assert fn(da="x", op="<") == {"da": "x", "thresh": "1 mm", "freq": "YS", "op": "<"}


# ---- the period front end of fields.py ----------------------------------------------------------------------------------
def test_mask_incomplete_masks_exactly_the_incomplete_period_in_a_float64_copy():
    count = np.arange(6, dtype=np.int32).reshape(2, 3)
    valid = np.array([[31, 31, 31], [28, 27, 28]])
    out = F.mask_incomplete({"n": count}, valid, [31, 27])    # the second period holds 27 days where 28 rows have a value
    assert set(out) == {"n"} and out["n"].dtype == np.float64
    np.testing.assert_array_equal(out["n"][0], [0.0, 1.0, 2.0])
    np.testing.assert_array_equal(out["n"][1], [np.nan, 4.0, np.nan])
    out = F.mask_incomplete({"n": count}, np.array([[31, 31, 31], [27, 27, 27]]), [31, 28])
    np.testing.assert_array_equal(out["n"], [[0.0, 1.0, 2.0], [np.nan] * 3])
    assert count.dtype == np.int32
    np.testing.assert_array_equal(count, np.arange(6).reshape(2, 3))


def test_the_period_checks_raise_what_the_mirrors_raised():
    t = TimeAxis.daily("2001-01-01", 90)
    np.testing.assert_array_equal(F.period_segments(t, "MS"), [0, 31, 59, 90])
    assert F.period_segments(t, "MS").dtype == np.int64
    with pytest.raises(NotImplementedError) as e:
        parse_freq("17min")
    assert not isinstance(e.value, F.NotServed)
    with pytest.raises(F.NotServed, match="17min"):
        F.period_segments(t, "17min")
    assert F.check_freq("YS") is None
    with pytest.raises(TypeError, match=r"^Freq must be a string\.$"):
        F.check_freq(3)
    for keep, mask in ((False, False), (True, False), (False, True)):
        assert F.no_keep_with_mask(keep, mask) is None
    with pytest.raises(ValueError, match="^keep=True returns the device arrays as computed: pass mask_missing=False$"):
        F.no_keep_with_mask(True, True)


def test_the_precipitation_spellings_of_anuclim_are_the_table_it_had():
    assert anuclim._PR_SPELLINGS == {
        "kg m-2 s-1": "kg m-2 s-1", "kg/m2/s": "kg m-2 s-1", "mm/s": "mm/s", "mm s-1": "mm/s", "mm/d": "mm/d", "mm/day": "mm/d",
        "mm d-1": "mm/d", "mm day-1": "mm/d", "mm / d": "mm/d", "mm/week": "mm/week", "mm week-1": "mm/week",
        "mm/month": "mm/month", "mm month-1": "mm/month"}
    assert len(anuclim._PR_SPELLINGS) == 13 and set(anuclim._PR_SPELLINGS.values()) == set(anuclim._PR_UNITS)


# ---- the install helper of patch.py -------------------------------------------------------------------------------------
DEFINING, PACKAGE = "xclim.indices._agro", "xclim.indices"


def _function(name, says):
    ns = {}
    exec(f"def {name}(pr=None, tasmin=None, freq='YS'):\n    return {says!r}\n", ns)
    return ns[name]


def _modules(names=rainseason.ADAPTED, another=()):
    """The defining module and the package that re-exports its functions; the package holds a function of its own under the names
    in ``another``."""
    mod, pkg = types.ModuleType(DEFINING), types.ModuleType(PACKAGE)
    originals = {}
    for name in names:
        originals[name] = _function(name, "original " + name)
        setattr(mod, name, originals[name])
        setattr(pkg, name, _function(name, "another " + name) if name in another else originals[name])
    return {DEFINING: mod, PACKAGE: pkg}, originals


@pytest.fixture()
def installed():
    try:
        yield lambda mods: patch.install(fakexr.make_env(), mods)
    finally:
        patch.uninstall()


def test_install_patches_the_defining_module_and_a_re_export_of_the_same_object(installed):
    mods, originals = _modules()
    held = {modname: dict(vars(m)) for modname, m in mods.items()}
    names = installed(mods)
    assert names == [f"{modname}.{n}" for modname in (DEFINING, PACKAGE) for n in rainseason.ADAPTED]
    for m in mods.values():
        for n, fn in originals.items():
            assert getattr(m, n).__wrapped__ is fn and getattr(m, n).__name__ == n
    assert mods[DEFINING].rain_season is mods[PACKAGE].rain_season
    assert mods[PACKAGE].hardiness_zones(tasmin="not a DataArray") == "original hardiness_zones"    # NotServed: forwarded
    patch.uninstall()
    for modname, m in mods.items():
        assert all(getattr(m, n) is held[modname][n] for n in originals)      # restored by identity


def test_install_leaves_another_function_under_the_same_name_alone(installed):
    mods, originals = _modules(another=("hardiness_zones",))
    theirs = mods[PACKAGE].hardiness_zones
    names = installed(mods)
    assert names == [f"{DEFINING}.rain_season", f"{DEFINING}.hardiness_zones", f"{PACKAGE}.rain_season"]
    assert mods[PACKAGE].hardiness_zones is theirs and theirs("x") == "another hardiness_zones"
    assert mods[DEFINING].hardiness_zones.__wrapped__ is originals["hardiness_zones"]
    patch.uninstall()
    assert mods[PACKAGE].hardiness_zones is theirs and mods[DEFINING].hardiness_zones is originals["hardiness_zones"]


def test_install_patches_nothing_where_the_defining_module_lacks_a_name(installed):
    mods, originals = _modules(names=("rain_season",))
    assert installed(mods) == []
    assert all(m.rain_season is originals["rain_season"] for m in mods.values())
