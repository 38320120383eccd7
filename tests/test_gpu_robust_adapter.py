"""The xarray adapter of the change-robustness unit, EXECUTED: ``patch.install(env, modules)`` on stand-in modules wired like the
reference — ``xclim.ensembles._robustness`` defines ``robustness_fractions`` and ``robustness_coefficient`` next to its ``xr``,
``gen_call_string`` and ``SIGNIFICANCE_TESTS``, and ``xclim.ensembles`` re-exports both — with the DataArray stand-in of
tests/fakexr.py and a Dataset that is a dict with ``attrs``.  The stand-in originals only record that they were reached.  The
cases are the reference's own (tests/test_ensembles.py:576-768, recorded in tests/golden/robust_known_answers.json): the
eight parametrized ``test_robustness_fractions`` cases, the weighted, delta, empty, missing
and coefficient cases."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fakexr  # noqa: E402
import robustcpu as RC  # noqa: E402

from poisoned import poisoned_outputs  # noqa: E402,F401

pytestmark = pytest.mark.gpu

NAMES = ("robustness_fractions", "robustness_coefficient")
DA = fakexr.DataArray


class Dataset(dict):
    def __init__(self, data_vars, attrs=None):
        super().__init__(data_vars)
        self.attrs = dict(attrs or {})

    data_vars = property(lambda self: self)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class AtLeastNValid:
    def __init__(self, n=20):
        self.options = {"n": n}


class MissingPct:
    options = {"tolerance": 0.1}


@pytest.fixture()
def wired(dev):
    from xclim_amd import _capi as capi
    from xclim_amd import patch

    old = capi._default_device
    capi._default_device = dev
    reached = []
    rob = types.ModuleType("xclim.ensembles._robustness")

    def robustness_fractions(fut, ref=None, test=None, weights=None, invalid=None, strict_sign=True, **kwargs):
        reached.append(("robustness_fractions", test))
        return "original robustness_fractions"

    def robustness_coefficient(fut, ref):
        reached.append(("robustness_coefficient", None))
        return "original robustness_coefficient"

    rob.robustness_fractions, rob.robustness_coefficient = robustness_fractions, robustness_coefficient
    rob.xr = types.SimpleNamespace(Dataset=Dataset, DataArray=DA)
    rob.gen_call_string = lambda name, **kw: f"{name}({', '.join(f'{k}={v}' for k, v in kw.items())})"
    rob.SIGNIFICANCE_TESTS = {n: None for n in ("ttest", "welch-ttest", "mannwhitney-utest", "brownforsythe-test", "ipcc-ar6-c", "mine")}
    rob.compare = lambda *a, **k: None
    pub = types.ModuleType("xclim.ensembles")
    pub.robustness_fractions, pub.robustness_coefficient = robustness_fractions, robustness_coefficient
    mods = {"xclim.ensembles._robustness": rob, "xclim.ensembles": pub}
    names = patch.install(fakexr.make_env(), mods)
    try:
        yield mods, names, reached
    finally:
        patch.uninstall()
        capi._default_device = old


def _robust_data():
    k = RC.known()
    fut, ref = np.array(k["robust_data"]["fut"]), np.array(k["robust_data"]["ref"])   # (realization, time, lon)
    from xclim_amd.timeaxis import TimeAxis

    coords = {"lon": DA(np.arange(4.0), dims=("lon",), attrs={"axis": "X"}), "realization": np.arange(4),
              "time": fakexr.time_coord(TimeAxis(np.arange(2000, 2040), np.ones(40, int), np.ones(40, int), "noleap"))}
    # the reference's layout: (lon, realization, time)
    f = DA(np.ascontiguousarray(np.moveaxis(fut, -1, 0)), dims=("lon", "realization", "time"), coords=coords, name="tas")
    r = DA(np.ascontiguousarray(np.moveaxis(ref, -1, 0)), dims=("lon", "realization", "time"), coords=coords, name="tas")
    return k, f, r


def test_both_functions_are_replaced_in_both_modules(wired):
    mods, names, _ = wired
    for m in mods:
        for n in NAMES:
            assert f"{m}.{n}" in names
    for n in NAMES:
        assert mods["xclim.ensembles"].__dict__[n] is mods["xclim.ensembles._robustness"].__dict__[n]


def test_the_reference_s_parametrized_cases(wired):
    mods, _, reached = wired
    k, fut, ref = _robust_data()
    fn = mods["xclim.ensembles"].robustness_fractions
    for case in k["fractions"]:
        test = case["test"].split("/")[0]
        test = None if test == "None" else test
        fracs = fn(fut, ref, test=test, **case["kwargs"])
        assert isinstance(fracs, Dataset) and fracs.attrs == {"description": "Significant change and sign of change fractions."}
        assert fracs.changed.attrs["test"] == str(test) and fracs.changed.dims == ("lon",) and fracs.changed.coords["lon"].attrs == {"axis": "X"}
        np.testing.assert_array_almost_equal(fracs.positive.values, [0.5, 0.5, 1, 1])
        np.testing.assert_array_almost_equal(fracs.agree.values, [0.5, 0.5, 1, 1])
        np.testing.assert_array_almost_equal(fracs.valid.values, [1, 1, 1, 0.5])
        np.testing.assert_array_almost_equal(fracs.changed.values, case["changed"])
        np.testing.assert_array_almost_equal(fracs.changed_positive.values, case["changed_positive"])
        if case["changed_table"] is not None:
            assert fracs.pvals.dims == ("realization", "lon")
            with np.errstate(invalid="ignore"):
                np.testing.assert_array_equal((fracs.pvals.values < 0.05).T, np.array(case["changed_table"], bool))
            assert fracs.pvals.attrs["description"] == f"P-values from change significance test. Significant change was tested with test {test} and parameters p_change=0.05."
        else:
            assert "pvals" not in fracs
    assert reached == []
    assert fn(fut, ref, test="ipcc-ar6-c").changed.attrs["description"].endswith("tested with test ipcc-ar6-c and parameters ref_pi=None.")
    no_time = DA(ref.values, dims=ref.dims, coords={k: c for k, c in ref.coords.items() if k != "time"})
    assert fn(fut, no_time, test="ipcc-ar6-c") == "original robustness_fractions" and reached.pop() == ("robustness_fractions", "ipcc-ar6-c")
    t = fn(fut, ref, test="threshold", abs_thresh=2)
    assert t.changed.attrs["description"] == ("Fraction of valid members showing significant change. Significant change was tested with test "
                                              "threshold and parameters abs_thresh=2.")
    assert t.positive.attrs == {"description": "Fraction of valid members showing strictly  positive change.", "units": ""}
    assert "zero or " in fn(fut, ref, strict_sign=False).agree.attrs["description"]


def test_weighted_delta_empty_and_missing(wired):
    mods, _, reached = wired
    k, fut, ref = _robust_data()
    fn = mods["xclim.ensembles._robustness"].robustness_fractions
    w = DA(np.array(k["weighted"]["weights"]), dims=("realization",), coords={"realization": np.arange(4)})
    fracs = fn(fut, ref, test=None, weights=w)
    assert fracs.changed.attrs["test"] == "None"
    np.testing.assert_array_equal(fracs.changed.values, [1, 1, 1, 1])
    np.testing.assert_array_almost_equal(fracs.changed_positive.values, k["weighted"]["changed_positive"])
    for case in k["delta"]:
        delta = DA(np.array(case["delta"], float), dims=("realization",))
        kw = {"test": "threshold", "abs_thresh": case["abs_thresh"]} if case["abs_thresh"] is not None else {"test": None}
        if case["weights"] is not None:
            kw["weights"] = DA(np.array(case["weights"], float), dims=("realization",))
        fracs = fn(delta, strict_sign=case["strict_sign"], **kw)
        for name in ("changed", "changed_positive", "positive", "agree"):
            if name in case:
                np.testing.assert_array_almost_equal(fracs[name].values, case[name], 15)
                assert fracs[name].dims == ()
    nan = DA(np.full((20, 10), np.nan), dims=("realization", "time"))
    f = fn(nan, nan, test="ttest")
    assert f.changed.values == 0 and f.valid.values == 0
    # the second half of every future series missing: AtLeastNValid(n=20) keeps the members valid, MissingAny does not
    half = fut.values.copy()
    half[:2, :, 20:] = np.nan
    half = DA(half, dims=fut.dims, coords=fut.coords)
    np.testing.assert_array_almost_equal(fn(half, ref, test="ttest", invalid=AtLeastNValid(n=20)).valid.values, [1, 1, 1, 0.5])
    np.testing.assert_array_almost_equal(fn(half, ref, test="ttest").valid.values, [0, 0, 1, 0.5])
    assert reached == []
    # forwarded: another invalid method, a user-registered test, integer and chunked fields
    assert fn(fut, ref, test="ttest", invalid=MissingPct()) == "original robustness_fractions"
    assert fn(fut, ref, test="mine") == "original robustness_fractions"
    assert fn(DA(np.nan_to_num(fut.values).astype(np.int32), dims=fut.dims), ref) == "original robustness_fractions"
    chunked = DA(fakexr.ChunkedArray(fut.values, ((2, 2), (2, 2), (20, 20))), dims=fut.dims, coords=fut.coords)
    assert fn(chunked, ref, test="ttest") == "original robustness_fractions"
    assert len(reached) == 4
    with pytest.raises(ValueError, match="When deltas are given"):
        fn(DA(np.zeros(4), dims=("realization",)), test="ttest")
    with pytest.raises(ValueError, match="One and only one of abs_thresh or rel_thresh"):
        fn(fut, ref, test="threshold")
    with pytest.raises(ValueError, match="Statistical test nope must be one of ttest, welch-ttest, mannwhitney-utest, brownforsythe-test, ipcc-ar6-c, mine."):
        fn(fut, ref, test="nope")


def test_coefficient_cases(wired):
    mods, _, reached = wired
    k = RC.known()
    fn = mods["xclim.ensembles"].robustness_coefficient
    for case in k["coefficient"]:
        ref = DA(np.array(case["ref"], float), dims=("time",), name="tas")
        fut = DA(np.array(case["fut"], float), dims=("realization", "time"), name="tas")
        R = fn(fut, ref)
        np.testing.assert_almost_equal(R.values, case["expected"])
        assert R.dims == () and R.attrs["name"] == "R" and R.attrs["long_name"] == "Ensemble robustness coefficient"
        Rs = fn(Dataset({"tas": fut}), Dataset({"tas": ref}))
        np.testing.assert_almost_equal(Rs.tas.values, case["expected"])
    # cells on a grid, time first
    v = RC.vectors()
    f, r = v["coef/fut"][:, :, :12].reshape(6, 30, 3, 4), v["coef/ref"][:, :12].reshape(25, 3, 4)
    got = fn(DA(np.moveaxis(f, 1, 0), dims=("time", "realization", "y", "x"), coords={"y": np.arange(3.0)}), DA(r, dims=("time", "y", "x")))
    assert got.dims == ("y", "x") and list(got.coords) == ["y"]
    np.testing.assert_allclose(got.values.ravel(), v["coef/R"][:12], rtol=1e-12)
    assert reached == []
    assert fn(DA(f.astype(np.int64), dims=("realization", "time", "y", "x")), DA(r, dims=("time", "y", "x"))) == "original robustness_coefficient"
