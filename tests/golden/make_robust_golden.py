"""Generate tests/golden/robust_vectors.npz and tests/golden/robust_known_answers.json by EXECUTING the reference's
ensembles/_robustness.py.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_robust_golden.py

The module imports xarray and three xclim modules, none of which is installed here.  Its source is compiled as it stands with
stand-ins in ``sys.modules``: an ``xarray`` whose ``DataArray`` is a small labelled array and whose ``apply_ufunc`` loops over
the cells and calls the function it is given once per (realization, cell) — what ``xr.apply_ufunc(..., vectorize=True)`` does —
and empty ``xclim.core.formatting`` / ``xclim.core.missing`` / ``xclim.indices.generic``.  ``mean("time")`` of the stand-in is
``np.nanmean`` of the contiguous series.  Nothing of the reference is copied into this repository: the fixtures hold inputs and
what the reference's own closures (``_ttest_func``, ``wtt_wrapper``, ``mwu_wrapper``, the Brown-Forsythe lambda,
``_knutti_sedlacek``) and scipy 1.15 returned for them.  The module's ``spstats`` is wrapped so that the statistic and the degrees
of freedom of each scipy call are recorded next to the p-value the closure returns.

robust_vectors.npz, one group per family ``<family>/...``: ``fut`` (R, T1, C), ``ref`` (R, T2, C), and per test ``<test>/p``,
``<test>/stat``, ``<test>/df`` (R, C); NaN where the reference's guard answers before scipy is called.  NOTE: the reference's
``_mannwhitney_utest(ref, fut)`` names its parameters the other way round, so the recorded Mann-Whitney statistic is U of the
REFERENCE sample: n1 n2 - U1 of the future sample.  A ``<family>32`` group holds the float32 fields; its results are the
reference's on the widened values (scipy itself would go on in float32).  ``coef/...``: ``fut`` (R, T1, C), ``ref`` (T2, C), ``R``.

Families (R = 4 unless noted): main (130 cells, T 40 / 30, no NaN); ties (values on a 0.5 grid); mwu_8_12 and mwu_9_9 (no ties:
the exact and the asymptotic route at the switch); mwu_8_12_tie; pending (T 10 / 12 with two NaN in some series of 10: the exact
route with other counts than the table's); nan_one (NaN in fut only); allnan; one_left; const_eq (a constant series equal to the
reference mean: 0 / 0) and const_ne; identical (fut is ref) and allequal (one value everywhere: p clipped to 1); medians (T 7 / 8
and, in medians2, 16 / 15); lds63 / lds64 / lds65 (T1 + T2 around the LDS switch); t129 (129 / 129), t512 (512 / 300) and t500 (500 / 511, whose
split goes three levels deep): the pairwise split.  ``ar6_60`` / ``ar6_50`` (6 cells): annual values with a trend for ``ipcc-ar6-c``, ``x`` their days, ``gamma_lin`` and
``gamma_pi`` the thresholds without and with ``ref_pi`` — the RESTATEMENT's (tests/robustcpu.py), since xarray's resample and polyfit
cannot be executed here; the comparisons |delta| > gamma keep a 1e-6 relative gap.  The generator asserts that every recorded p keeps |p / 0.05 - 1| >= 1e-6, and that the threshold comparisons of
the known answers keep the same gap.

robust_known_answers.json: the reference's tests/test_ensembles.py:530-769 — ``robust_data`` (drawn here with its seed), the
expected ``changed`` tables and fractions of the eight parametrized cases, the weighted, delta and categories cases and the two
coefficients, each with what the reference's closure gave here."""
import json
import os
import sys
import types
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import robustcpu as RC  # noqa: E402

REF = "/root/reference/src/xclim/ensembles/_robustness.py"
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261020
P_CHANGE = 0.05
TESTS = {"ttest": "ttest", "welch": "welch-ttest", "mwu": "mannwhitney-utest", "bf": "brownforsythe-test"}


class Arr:
    """The least of a DataArray that the reference's tests and closures touch."""

    def __init__(self, data, dims):
        self.data, self.dims, self.attrs = np.asarray(data), tuple(dims), {}
        assert self.data.ndim == len(self.dims)

    def mean(self, dim):
        ax = self.dims.index(dim)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = np.nanmean(np.ascontiguousarray(np.moveaxis(self.data, ax, -1)), axis=-1)
        return Arr(m, self.dims[:ax] + self.dims[ax + 1:])

    def __lt__(self, other):
        return Arr(self.data < other, self.dims)


class Recorder:
    """scipy.stats with the last result of the four tests kept."""

    def __init__(self, stats):
        self.stats, self.last = stats, None

    def __getattr__(self, name):
        fn = getattr(self.stats, name)

        def call(*a, **kw):
            res = fn(*a, **kw)
            self.last = (float(res[0]), float(getattr(res, "df", np.nan)))
            return res

        return call


def reference_module():
    import scipy.stats

    rec = Recorder(scipy.stats)
    extras = []

    def apply_ufunc(func, *args, input_core_dims, **kw):
        loop = []
        for a, core in zip(args, input_core_dims):
            loop += [(d, n) for d, n in zip(a.dims, a.data.shape) if d not in core and (d, n) not in loop]
        out = np.empty([n for _, n in loop])
        ext = np.full(out.shape + (2,), np.nan)
        for idx in np.ndindex(*out.shape):
            pos = dict(zip([d for d, _ in loop], idx))
            pieces = []
            for a, core in zip(args, input_core_dims):
                moved = np.moveaxis(a.data, [a.dims.index(d) for d in core], range(a.data.ndim - len(core), a.data.ndim)) if core else a.data
                rest = [d for d in a.dims if d not in core]
                pieces.append(np.ascontiguousarray(moved[tuple(pos[d] for d in rest)]))
            rec.last = None
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[idx] = func(*pieces)
            if rec.last is not None:
                ext[idx] = rec.last
        extras.append(ext)
        return Arr(out, [d for d, _ in loop])

    xr = types.ModuleType("xarray")
    xr.DataArray, xr.Dataset, xr.apply_ufunc = Arr, dict, apply_ufunc
    stubs = {"xarray": xr}
    for name in ("xclim", "xclim.core", "xclim.core.formatting", "xclim.core.missing", "xclim.indices", "xclim.indices.generic"):
        stubs[name] = types.ModuleType(name)
    stubs["xclim.core.formatting"].gen_call_string = lambda *a, **k: ""
    stubs["xclim.core.formatting"].update_xclim_history = lambda f: f
    stubs["xclim.core.missing"].MissingAny = stubs["xclim.core.missing"].MissingBase = object
    stubs["xclim.indices.generic"].compare = stubs["xclim.indices.generic"].detrend = None
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        ns = {"__name__": "reference_robustness"}
        exec(compile(open(REF).read(), REF, "exec"), ns)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert list(ns["SIGNIFICANCE_TESTS"]) == ["ttest", "welch-ttest", "mannwhitney-utest", "brownforsythe-test", "ipcc-ar6-c"]
    ns["spstats"] = rec
    return ns, extras


def run_tests(ns, extras, fut, ref):
    """{test: (p, stat, df)} of the reference for fut (R, T1, C) and ref (R, T2, C), on the values widened to float64."""
    f = Arr(np.asarray(fut, np.float64), ("realization", "time", "cell"))
    r = Arr(np.asarray(ref, np.float64), ("realization", "time", "cell"))
    out = {}
    for key, name in TESTS.items():
        del extras[:]
        changed, pvals = ns["SIGNIFICANCE_TESTS"][name](f, r)
        assert len(extras) == 1 and np.array_equal(changed.data, pvals.data < P_CHANGE)
        out[key] = (pvals.data, extras[0][..., 0], extras[0][..., 1])
    return out


def coefficient(ns, extras, fut, ref):
    R = ns["robustness_coefficient"](Arr(np.asarray(fut, np.float64), ("realization", "time", "cell")), Arr(np.asarray(ref, np.float64), ("time", "cell")))
    return R.data


def families(rng):
    fam = {}

    def normal(T1, T2, C, R=4, shift=1.0):
        ref = rng.normal(274.0, 0.8, (R, T2, C))
        fut = rng.normal(274.0, 0.9, (R, T1, C)) + rng.uniform(-shift, shift, (R, 1, C))
        return fut, ref

    fam["main"] = normal(40, 30, 130)
    f, r = normal(40, 30, 16)
    fam["ties"] = (np.round(f * 2) / 2, np.round(r * 2) / 2)
    fam["mwu_8_12"] = normal(8, 12, 8)
    fam["mwu_9_9"] = normal(9, 9, 8)
    f, r = normal(8, 12, 8)
    f[:, 3, :] = r[:, 5, :]
    fam["mwu_8_12_tie"] = (f, r)
    f, r = normal(10, 12, 8)
    f[:, 2, ::2] = np.nan
    f[:, 7, ::2] = np.nan
    fam["pending"] = (f, r)
    f, r = normal(40, 30, 8)
    f[rng.random(f.shape) < 0.1] = np.nan
    fam["nan_one"] = (f, r)
    f, r = normal(40, 30, 4)
    f[0, :, 0] = np.nan
    r[1, :, 1] = np.nan
    f[2, :, 2] = np.nan
    r[2, :, 2] = np.nan
    fam["allnan"] = (f, r)
    f, r = normal(40, 30, 4)
    f[:, 1:, 0] = np.nan
    r[:, :-1, 1] = np.nan
    f[:, :20, 2] = np.nan
    f[:, 21:, 2] = np.nan
    fam["one_left"] = (f, r)
    # integers: the mean of the symmetric reference is exactly 274
    r = np.tile(274.0 + np.concatenate([np.arange(1, 16), -np.arange(1, 16)])[None, :, None], (4, 1, 3))
    fam["const_eq"] = (np.full((4, 40, 3), 274.0), r)
    fam["const_ne"] = (np.full((4, 40, 3), 275.0), r)
    f, r = normal(30, 30, 4)
    fam["identical"] = (r.copy(), r)
    fam["allequal"] = (np.full((4, 40, 2), 3.0), np.full((4, 30, 2), 3.0))
    fam["medians"] = normal(7, 8, 8)
    fam["medians2"] = normal(16, 15, 8)
    fam["lds63"] = normal(33, 30, 5)
    fam["lds64"] = normal(34, 30, 5)
    fam["lds65"] = normal(35, 30, 5)
    fam["t129"] = normal(129, 129, 4, shift=0.3)
    fam["t512"] = normal(512, 300, 3, shift=0.15)
    # 500 = 248 + (120 + (64 + 68)), 511 = 248 + (128 + (64 + 71)): three levels (a generator of its own: added later)
    r5 = np.random.default_rng(SEED + 1)
    fam["t500"] = (r5.normal(274.0, 0.9, (4, 500, 3)) + r5.uniform(-0.15, 0.15, (4, 1, 3)), r5.normal(274.0, 0.8, (4, 511, 3)))
    # a delta that is exactly 0: integer-valued series with equal means and different spreads, next to members that move
    f = np.tile(np.array([1.0, 3.0, 2.0, 2.0, 0.0, 4.0, 2.0, 2.0])[None, :, None], (4, 1, 3))
    r = np.tile(np.array([2.0, 2.0, 1.0, 3.0, 2.0, 2.0])[None, :, None], (4, 1, 3))
    f[1] += 1.0
    f[2, :, 1] -= 2.0
    fam["zero_delta"] = (f, r)
    return fam


def known_answers(ns, extras):
    from scipy.stats import norm

    random = np.random.default_rng(seed=list(map(ord, "𝕽𝔞𝖓𝔡𝖔𝔪")))
    ref = np.tile(np.array([norm.rvs(loc=274, scale=0.8, size=(40,), random_state=random) for r in range(4)]), (4, 1, 1))
    shapes = ([(274.0, 0.7), (274.0, 0.6), (274.0, 0.7), (275.6, 1.1)], [(272.5, 1.2), (272.4, 0.8), (275.5, 0.8), (275.6, 1.1)],
              [(275.6, 0.8), (275.8, 1.2), (276.5, 0.8), (277.6, 1.1)], [(np.nan, 0.3), (np.nan, 1.2), (275.5, 0.8), (275.6, 1.1)])
    with np.errstate(all="ignore"):
        fut = np.array([[norm.rvs(loc=loc, scale=sc, size=(40,), random_state=random) for loc, sc in shps] for shps in shapes])
    # (lon, realization, time) -> (realization, time, lon)
    fut, ref = np.moveaxis(fut, 0, -1), np.moveaxis(ref, 0, -1)
    expected = {
        "ttest": ([0.75, 1, 1, 1], [0.5, 0.5, 1, 1], [[0, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 1, 1]], {}),
        "welch-ttest": ([0.25, 1, 1, 1], [0.25, 0.5, 1, 1], [[0, 0, 0, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 1, 1]], {}),
        "mannwhitney-utest": ([0.5, 1, 1, 1], [0.25, 0.5, 1, 1], [[0, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 1, 1]], {}),
        "brownforsythe-test": ([0.25, 0.25, 0.25, 0], [0.25, 0.0, 0.25, 0], [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], {}),
        "ipcc-ar6-c": ([0.25, 1, 1, 1], [0.25, 0.5, 1, 1], None, {}),
        "threshold/rel": ([0.25, 1, 1, 1], [0.25, 0.5, 1, 1], None, {"rel_thresh": 0.002}),
        "threshold/abs": ([0, 0, 0.5, 0], [0, 0, 0.5, 0], None, {"abs_thresh": 2}),
        "None": ([1, 1, 1, 1], [0.5, 0.5, 1, 1], None, {}),
    }
    res = run_tests(ns, extras, fut, ref)
    # the threshold comparisons of the reference's cases keep a 1e-6 relative gap (NaN members aside)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mr = np.nanmean(ref, axis=1)
        delta = np.nanmean(fut, axis=1) - mr
    for ratio in (np.abs(delta) / 2, np.abs(delta / mr) / 0.002):
        assert np.nanmin(np.abs(ratio - 1)) >= 1e-6, "a threshold comparison within 1e-6 of its threshold"
    g_ar6, _ = RC.ar6_gamma(ref, 365.0 * np.arange(40), False)   # robust_data is stamped yearly on a noleap calendar
    assert np.nanmin(np.abs(np.abs(delta) / g_ar6 - 1)) >= 1e-6, "the ar6 comparison of the known answers within 1e-6 of its threshold"
    cases = []
    for name, (chng, pos, changed, kws) in expected.items():
        case = {"test": name, "changed": chng, "changed_positive": pos, "changed_table": changed, "kwargs": kws}
        key = {v: k for k, v in TESTS.items()}.get(name)
        if key:
            p = res[key][0]                                   # (realization, lon)
            with np.errstate(invalid="ignore"):
                got = (p < P_CHANGE).T.astype(int).tolist()   # the table is (lon, realization)
            assert got == changed, (name, got, changed)
            case["reference_pvals"] = p.tolist()
        cases.append(case)
    known = {"robust_data": {"fut": fut.tolist(), "ref": ref.tolist()}, "fractions": cases,
             "common": {"positive": [0.5, 0.5, 1, 1], "agree": [0.5, 0.5, 1, 1], "valid": [1, 1, 1, 0.5]},
             "weighted": {"weights": [1, 0.1, 3.5, 5], "changed": [1, 1, 1, 1], "changed_positive": [0.53125, 0.88541667, 1.0, 1.0]},
             "delta": [
                 {"delta": [-2, 1, -2, -1, 0, 0], "abs_thresh": 1.5, "weights": None, "strict_sign": True,
                  "changed": 2 / 6, "changed_positive": 0.0, "positive": 1 / 6, "agree": 3 / 6},
                 {"delta": [-2, 1, -2, -1], "abs_thresh": 1.5, "weights": [4, 3, 2, 1], "strict_sign": True, "changed": 0.6, "positive": 0.3,
                  "agree": 0.7},
                 {"delta": [-2, 1, -2, -1, 2, 0], "abs_thresh": None, "weights": None, "strict_sign": False, "changed": 1, "positive": 3 / 6,
                  "agree": 4 / 6}],
             "categories": {"changed": [0.5, 0.8, 1, 1], "agree": [1, 0.5, 0.5, 1], "expected": [2, 3, 3, 1], "flag_values": [1, 2, 3],
                            "flag_meanings": "robust_signal no_change_or_no_signal conflicting_signal"}}
    cref = [274, 275, 274.5, 276, 274.3, 273.3]
    coef = []
    for second, expect in (([275, 275.8, 276, 275.2, 276.2, 275.7], 0.91972477), ([274, 274.8, 273.7, 274.2, 273.9, 274.5], 0.83743842)):
        cfut = [[277, 277.1, 278, 278.4, 278.1, 276.9], second]
        got = float(coefficient(ns, extras, np.array(cfut)[:, :, None], np.array(cref)[:, None])[0])
        assert abs(got - expect) < 1.5e-7, (got, expect)
        coef.append({"fut": cfut, "ref": cref, "expected": expect, "decimals": 7, "reference": got})
    known["coefficient"] = coef
    return known


def main():
    ns, extras = reference_module()
    rng = np.random.default_rng(SEED)
    store, worst = {}, np.inf
    fams = families(rng)
    for name in ("main", "ties", "nan_one", "medians", "lds65", "t129"):
        f, r = fams[name]
        fams[name + "32"] = (f.astype(np.float32), r.astype(np.float32))
    for name, (f, r) in fams.items():
        store[f"{name}/fut"], store[f"{name}/ref"] = f, r
        for key, (p, stat, df) in run_tests(ns, extras, f, r).items():
            store[f"{name}/{key}/p"], store[f"{name}/{key}/stat"], store[f"{name}/{key}/df"] = p, stat, df
            with np.errstate(all="ignore"):
                gap = np.nanmin(np.abs(p / P_CHANGE - 1), initial=np.inf)
            assert gap >= 1e-6, f"{name}/{key}: a p-value {gap:.1e} (relative) from p_change: another seed"
            worst = min(worst, gap)
    # what each family is there for
    assert np.isnan(store["allnan/ttest/p"][0, 0]) and np.isnan(store["allnan/mwu/p"][1, 1]) and np.isnan(store["allnan/welch/p"][2, 2])
    assert np.isnan(store["one_left/ttest/p"][:, 0]).all() and np.isfinite(store["one_left/mwu/p"]).all()
    assert np.isnan(store["const_eq/ttest/p"]).all() and (store["const_ne/ttest/p"] == 0).all() and np.isinf(store["const_ne/ttest/stat"]).all()
    assert (store["allequal/mwu/p"] == 1).all() and (store["identical/mwu/p"] == 1).all()
    assert np.isnan(store["nan_one/bf/p"]).any() and np.isfinite(store["nan_one/mwu/p"]).all()
    # the coefficient: 6 members of 30 years against 25 reference years, 20 cells; a tie family on a 0.5 grid; one NaN cell
    cf, cr = rng.normal(276.0, 1.0, (6, 30, 20)) + rng.normal(0, 0.7, (6, 1, 20)), rng.normal(274.0, 0.8, (25, 20))
    cf[:, :, 10:15], cr[:, 10:15] = np.round(cf[:, :, 10:15] * 2) / 2, np.round(cr[:, 10:15] * 2) / 2
    cf[3, 4, 19] = np.nan
    for tag, (a, b) in {"coef": (cf, cr), "coef32": (cf.astype(np.float32), cr.astype(np.float32))}.items():
        store[f"{tag}/fut"], store[f"{tag}/ref"] = a, b
        with np.errstate(all="ignore"):
            store[f"{tag}/R"] = coefficient(ns, extras, a, b)
        assert np.isnan(store[f"{tag}/R"][19]) and np.isfinite(store[f"{tag}/R"][:19]).all()
    # ipcc-ar6-c: xarray's resample / polyfit cannot be executed here, so gamma is the restatement's (tests/robustcpu.py: np.polyfit
    # on days); 60 and 50 annual values (a partial last block of 10), noleap years, a NaN year in one series, with a trend
    ra = np.random.default_rng(SEED + 2)
    for years in (60, 50):
        t = np.arange(years)[None, :, None]
        aref = 274.0 + 0.02 * t + 1e-4 * t * t + ra.normal(0, 0.5, (4, years, 6))
        aref[1, 7, 2] = np.nan
        afut = aref[:, :40] + ra.uniform(-1.2, 1.2, (4, 1, 6))
        x = 365.0 * np.arange(years)
        store[f"ar6_{years}/fut"], store[f"ar6_{years}/ref"], store[f"ar6_{years}/x"] = afut, aref, x
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            delta = np.nanmean(afut, axis=1) - np.nanmean(aref, axis=1)
        for tag, with_pi in (("lin", False), ("pi", True)):
            g, _ = RC.ar6_gamma(aref, x, with_pi)
            assert np.nanmin(np.abs(np.abs(delta) / g - 1)) >= 1e-6, "an ar6 comparison within 1e-6 of its threshold"
            assert (np.abs(delta) > g).any() and (np.abs(delta) <= g).any()
            store[f"ar6_{years}/gamma_{tag}"] = g
    np.savez_compressed(os.path.join(HERE, "robust_vectors.npz"), **store)
    known = known_answers(ns, extras)
    with open(os.path.join(HERE, "robust_known_answers.json"), "w") as fh:
        json.dump(known, fh)
    print(f"{len(store)} arrays; the closest p-value is {worst:.2e} (relative) from p_change")


if __name__ == "__main__":
    main()
