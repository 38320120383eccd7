"""Host mirror of ``xclim.ensembles.ensemble_percentiles`` (reference: src/xclim/ensembles/_base.py:213-372) — the
second caller of ``calc_perc``.

The ensemble is a numpy / device array with the REALIZATION axis first: ``(realization, ...)``; the percentiles of the
members are taken per remaining element with the NaN-aware Hyndman-Fan estimate of ``core/utils.py:370-557`` — the same
kernel as ``percentile_doy`` (``xh_nan_quantile``), samples on the slow axis so the members are read coalesced.

The second half mirrors ``xclim.ensembles._robustness`` (src/xclim/ensembles/_robustness.py) on the change-robustness unit
(include/units/xclim_hip_robust.h): :func:`robustness_fractions`, :func:`robustness_coefficient`,
:func:`robustness_categories` and :func:`mwu_exact_sf`, the exact null distribution of Mann-Whitney's U.  Fields are numpy or
device arrays ``(realization, time, *cells)``.  :class:`NotServed` (the adapter forwards these to the reference): integer or
chunked fields, fields of mixed dtype, sizes beyond the unit's limits, ``invalid`` methods other than MissingAny and
AtLeastNValid, a user-registered test, and ``ipcc-ar6-c`` on an axis that is neither annual nor daily without gaps.  ASSUMPTIONS:
float32 fields are widened to float64 on load, where scipy goes on in float32; xarray's ``polyfit`` skips NaN years and fits on
the datetime coordinate, which is restated as a least-squares polynomial on days since the first stamp.
"""

from __future__ import annotations

import numpy as np

from . import _capi as capi
from . import kernels as K
from ._capi import DeviceArray, get_device, handle_float64
from .fields import NotServed
from .partitioning import (HS_COMPONENTS, LS_COMPONENTS, ensemble_mean_std_max_min, fractional_uncertainty,  # noqa: F401
                           general_components, general_partition, hawkins_sutton, hawkins_sutton_09_weighting, lafferty_sriver,
                           poly_smooth)

# _base.py:21-28
_quantile_params = {
    "interpolated_inverted_cdf": (0, 1),
    "hazen": (0.5, 0.5),
    "weibull": (0, 0),
    "linear": (1, 1),
    "median_unbiased": (1 / 3, 1 / 3),
    "normal_unbiased": (3 / 8, 3 / 8),
}


def ensemble_percentiles(ens, values=None, min_members: int | None = 1, weights=None, method: str = "linear", *,
                         device=None, keep: bool = False):
    """_base.py:213-372 for one variable.  Returns ``(..., percentiles)`` (percentile axis LAST like the reference's
    ``output_core_dims=[["percentiles"]]``) in float64, or the device array ``(nper, C)`` with ``keep=True``.
    Elements with fewer than ``min_members`` valid members are NaN (``None``: all members required)."""
    if values is None:
        values = [10, 50, 90]
    if method not in _quantile_params:
        raise KeyError(method)
    if weights is not None and method != "linear":
        raise ValueError("Only the 'linear' method is supported when using weights.")  # _base.py:347-348
    alpha, beta = _quantile_params[method]
    dev = device or get_device()
    if isinstance(ens, DeviceArray):
        x, lead = ens.reshape(ens.shape[0], -1), ens.shape[1:]
    else:
        a = np.asarray(ens)
        lead = a.shape[1:]
        if a.dtype == np.float64 and weights is None:  # float64 members: xh_nan_quantile_f64 (`diff` in float64, utl:486)
            x = dev.to_device(np.ascontiguousarray(a.reshape(a.shape[0], -1)))
        else:
            handle_float64(a, "ensemble_percentiles (weighted)")
            x = dev.to_device(np.ascontiguousarray(a.reshape(a.shape[0], -1), dtype=np.float32))
    R = x.shape[0]
    if min_members is None:
        min_members = R
    q = np.array([v / 100.0 for v in values], dtype=np.float64)
    if weights is not None:
        # _base.py:350-356: xarray's weighted quantile (parity unpinned: xarray is not available; see wquantile.hip)
        out = K.weighted_quantile(dev, x, weights, q)
    else:
        out = K.nan_quantile(dev, x, q, alpha, beta, sample_axis=0)  # (nper, C) float64
    if min_members != 1:
        seg = np.array([0, R], dtype=np.int64)
        nvalid, _ = K.resample_reduce(dev, x, "count", seg, want_valid=False)  # (1, C) int32
        enough = nvalid.get()[0] >= min_members
        o = out.get()
        o[:, ~enough] = np.nan
        if keep:
            return dev.to_device(o)
        return np.moveaxis(o.reshape((len(values),) + tuple(lead)), 0, -1)
    if keep:
        return out
    return np.moveaxis(out.get().reshape((len(values),) + tuple(lead)), 0, -1)


# ---- xclim.ensembles._robustness ------------------------------------------------------------------------------------------
# the reference's registry (_robustness.py:518-661) -> the unit's tests; "ipcc-ar6-c" has no scipy call: xh_ar6_gamma
ROBUSTNESS_TESTS = {"ttest": "ttest", "welch-ttest": "welch", "mannwhitney-utest": "mwu", "brownforsythe-test": "bf"}
FRACTIONS = tuple(capi.RF_ROWS)
_MWU_EXACT_MAX = 8   # scipy's _mwu_choose_method: the exact route needs a count of at most 8 (and no tie)


def mwu_exact_counts(n1: int, n2: int) -> list:
    """The number of arrangements of n1 + n2 untied values with U = 0 .. n1 n2, exact integers: the coefficients of the Gaussian
    binomial prod_{i=1..m} (1 - q^(n+i)) / (1 - q^i), m = min(n1, n2), built factor by factor in Python integers."""
    m, n = min(int(n1), int(n2)), max(int(n1), int(n2))
    deg = m * n
    c = [0] * (deg + 1)
    c[0] = 1
    for i in range(1, m + 1):
        for u in range(deg, n + i - 1, -1):   # times (1 - q^(n+i))
            c[u] -= c[u - n - i]
        for u in range(i, deg + 1):           # divided by (1 - q^i)
            c[u] += c[u - i]
    return c


def mwu_exact_sf(n1: int, n2: int) -> np.ndarray:
    """sf[k] = P(U >= k), k = 0 .. n1 n2, of Mann-Whitney's U for untied samples of n1 and n2 values under the null hypothesis:
    the exact count of arrangements with U >= k divided once by the total comb(n1 + n2, n1) (Python's integer division into a
    float is correctly rounded).  scipy's two-sided p is ``min(1, 2 sf[max(U1, U2)])``."""
    counts = mwu_exact_counts(n1, n2)
    total = sum(counts)
    sf, tail = np.empty(len(counts)), 0
    for k in range(len(counts) - 1, -1, -1):
        tail += counts[k]
        sf[k] = tail / total
    return sf


def _invalid_rule(invalid):
    """None / MissingAny -> ("any", None); AtLeastNValid(n) -> ("n", n); by name, as the instances come from the patched package."""
    if invalid is None or invalid == "any":
        return "any", None
    if isinstance(invalid, tuple) and len(invalid) == 2 and invalid[0] == "at_least_n":
        return "n", int(invalid[1])
    name = type(invalid).__name__
    if name == "MissingAny":
        return "any", None
    if name == "AtLeastNValid":
        return "n", int(getattr(invalid, "options", {}).get("n", 20))
    raise NotServed(f"robustness_fractions: invalid={name} is not served (MissingAny and AtLeastNValid are)")


def _field3(a, what, dev):
    """(DeviceArray (R, T, C), cells shape) of a numpy or device array (R, T, *cells) in its own float dtype."""
    if isinstance(a, DeviceArray):
        if np.dtype(a.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise NotServed(f"robustness: {what} is {np.dtype(a.dtype).name}; float32 and float64 fields are served")
        return a.reshape(a.shape[0], a.shape[1], -1), tuple(a.shape[2:])
    if hasattr(a, "chunks") and getattr(a, "chunks", None) is not None:
        raise NotServed(f"robustness: {what} is chunked")
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        raise NotServed(f"robustness: {what} is an integer field")
    if a.dtype not in (np.float32, np.float64):
        raise NotServed(f"robustness: {what} is {a.dtype.name}; float32 and float64 fields are served")
    return dev.to_device(np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1))), a.shape[2:]


def _finish_pending(res, T1, T2):
    """The XH_CT_EXACT_PENDING pairs of a Mann-Whitney launch, on the host: one null distribution per distinct (n1', n2')."""
    status = res["status"]
    todo = status == capi.CT_STATUS["exact_pending"]
    if not todo.any():
        return
    n1, n2, u1 = res["n_fut"][todo], res["n_ref"][todo], res["stat"][todo]
    p = np.empty(u1.shape)
    for a, b in sorted(set(zip(n1.tolist(), n2.tolist()))):
        sf = mwu_exact_sf(a, b)
        sel = (n1 == a) & (n2 == b)
        u = np.maximum(u1[sel], a * b - u1[sel]).astype(np.int64)
        p[sel] = np.minimum(1.0, 2.0 * sf[u])
    res["pvals"][todo] = p
    status[todo] = capi.CT_STATUS["done"]


def _ar6_axis(ref_time, T: int, blocks: bool):
    """(days of the annual stamps since the first, the offsets of the years in a daily axis or None, the 20-year block offsets or
    None) for ``ipcc-ar6-c``: ``resample(time="YS")`` labels each year with its 1 January, ``resample(time="20YS")`` counts blocks of
    20 labels from the first (the last may be partial).  Served: an annual axis (one stamp per year, on the same month and day,
    consecutive years) and a daily gap-free one."""
    from .timeaxis import TimeAxis

    who = "robustness_fractions: ipcc-ar6-c"
    if not isinstance(ref_time, TimeAxis):
        raise NotServed(f"{who} needs ref_time, the TimeAxis of ref")
    if len(ref_time) != T:
        raise ValueError(f"ref_time has {len(ref_time)} stamps, ref {T} rows")
    y, m, d = (np.asarray(v) for v in (ref_time.year, ref_time.month, ref_time.day))
    annual = T >= 1 and np.all(np.diff(y) == 1) and np.all(m == m[0]) and np.all(d == d[0])
    seg = None
    if annual:
        years = y
    else:
        o = np.asarray(ref_time.ordinal())
        if T < 2 or not np.all(np.diff(o) == 1):
            raise NotServed(f"{who}: the time axis of ref is neither annual nor daily without gaps")
        seg, starts = ref_time.segments("YS")
        years = np.array([s[0] for s in starts])
    if len(years) > capi.CT_MAX_T:
        raise NotServed(f"{who}: up to {capi.CT_MAX_T} years are served, got {len(years)}")
    labels = np.asarray(TimeAxis(years, np.ones_like(years), np.ones_like(years), ref_time.calendar).ordinal(), np.float64)
    bl = np.append(np.arange(0, len(years), 20), len(years)).astype(np.int64) if blocks else None
    return labels - labels[0], seg, bl


def _ar6_gamma(dev, ref, x_years, year_seg, blocks, with_pi: bool):
    """gamma (R, C) on the host: the annual means of a daily ``ref`` (``xh_resample_reduce``, member by member), then one launch
    of ``xh_ar6_gamma``: sqrt(2 / 20) 1.645 std of the linearly detrended years, or with ``ref_pi`` sqrt(2) 1.645 std of the
    20-year means after a quadratic fit (_robustness.py:651-657; as there, ``ref_pi`` only chooses the rule: ``ref`` is detrended)."""
    r3 = ref if isinstance(ref, DeviceArray) else np.asarray(ref)
    R, T = int(r3.shape[0]), int(r3.shape[1])
    if isinstance(r3, DeviceArray):
        r3 = r3.reshape(R, T, -1)
        host = None
    else:
        host = np.ascontiguousarray(r3.reshape(R, T, -1))
    if year_seg is None:
        y = r3 if host is None else dev.to_device(host)
    else:
        if host is None:
            host = r3.get()
        y = dev.to_device(np.stack([K.resample_reduce(dev, dev.to_device(np.ascontiguousarray(host[r])), "mean", year_seg, want_valid=False)[0].get()
                                    for r in range(R)]))
    factor = np.sqrt(2) * 1.645 if with_pi else np.sqrt(2 / 20) * 1.645
    return K.ar6_gamma(dev, y, x_years, 2 if with_pi else 1, factor, blocks).get()


def change_test(fut, ref, test: str = "moments", *, device=None) -> dict:
    """One ``xh_change_test`` launch on ``fut`` (R, T1, *cells) and ``ref`` (R, T2, *cells) or (T2, *cells), with the table of the
    exact Mann-Whitney route where it is needed and the pending pairs finished on the host.  Returns host arrays (R, C) by the
    names of ``kernels.CT_OUTPUTS``."""
    dev = device or get_device()
    f, cells = _field3(fut, "fut", dev)
    if isinstance(ref, DeviceArray):
        r = ref.reshape(*ref.shape[:-len(cells)], -1) if cells else ref.reshape(*ref.shape, 1)
    else:
        r = np.asarray(ref)
        if r.dtype.kind in "iub":
            raise NotServed("robustness: ref is an integer field")
        r = dev.to_device(np.ascontiguousarray(r.reshape(r.shape[:r.ndim - len(cells)] + (-1,))))
    if np.dtype(r.dtype) != np.dtype(f.dtype):
        raise NotServed(f"robustness: fut is {np.dtype(f.dtype).name} and ref {np.dtype(r.dtype).name}")
    T1, T2 = int(f.shape[1]), int(r.shape[-2])
    if T1 > capi.CT_MAX_T or T2 > capi.CT_MAX_T:
        raise NotServed(f"robustness: series of up to {capi.CT_MAX_T} values are served, got {T1} and {T2}")
    sf = mwu_exact_sf(T1, T2) if test == "mwu" and min(T1, T2) <= _MWU_EXACT_MAX else None
    res = {k: v.get() for k, v in K.change_test(dev, f, r, test, sf).items()}
    if test == "mwu":
        _finish_pending(res, T1, T2)
    return res


def robustness_fractions(fut, ref=None, test=None, weights=None, invalid=None, strict_sign: bool = True, *, time=None, ref_time=None,
                         device=None, keep: bool = False, **kwargs):
    """_robustness.py:74-333 on arrays: ``fut`` (R, T1, *cells) and ``ref`` (R, T2, *cells), or with ``ref=None`` the deltas
    (R, *cells); ``ref`` may also be (T2, *cells), one reference for all members.  A one-dimensional ``fut`` or ``ref`` is one series: the
    realization axis is added.  Returns a
    dict with the reference's names: the seven fractions (*cells) float64 and, for the four scipy tests, ``pvals`` (R, *cells).
    ``keep=True`` returns the fractions as one device array (7, C) under "fractions" instead.  ``ref_time`` (a :class:`TimeAxis`, annual or daily) is
    needed by ``ipcc-ar6-c`` alone; ``time`` is taken for symmetry and unused.  The outputs of the
    test launch come to the host, where the pending exact Mann-Whitney pairs are finished and the ``valid`` and ``changed`` masks
    are made, and go back for the fractions launch: on a 1440 x 720 x 20 map that is about 1 GB each way, so the call is bound by
    the host link, not by the launches that DESIGN.md times."""
    dev = device or get_device()
    if test is not None and test != "threshold" and test not in ROBUSTNESS_TESTS:
        if test != "ipcc-ar6-c":
                raise ValueError(f"Statistical test {test} must be one of {', '.join(list(ROBUSTNESS_TESTS) + ['ipcc-ar6-c'])}.")
    abs_thresh, rel_thresh = kwargs.get("abs_thresh"), kwargs.get("rel_thresh")
    if test == "threshold" and (abs_thresh is None) == (rel_thresh is None):
        raise ValueError("One and only one of abs_thresh or rel_thresh must be given if test='threshold'.")
    p_change = float(kwargs.get("p_change", 0.05))
    pvals = None
    if ref is None:
        if test not in (None, "threshold"):
            raise ValueError("When deltas are given (ref=None), 'test' must be None or 'threshold'.")
        if test == "threshold" and rel_thresh is not None:
            raise NotServed("robustness_fractions: rel_thresh needs ref")
        d = fut.get() if isinstance(fut, DeviceArray) else np.asarray(fut)
        if d.dtype.kind in "iub":
            raise NotServed("robustness_fractions: integer deltas")
        d = np.asarray(d, np.float64)
        if d.ndim == 0:
            d = d[None]
        cells = d.shape[1:]
        delta = dev.to_device(np.ascontiguousarray(d.reshape(d.shape[0], -1)))
        R = d.shape[0]
        changed = valid = mean_ref = None
    else:
        rule, n_min = _invalid_rule(invalid)
        if len(fut.shape) == 1:   # one series: no realization axis
            fut = fut.reshape(1, -1) if isinstance(fut, DeviceArray) else np.asarray(fut)[None]
        if len(ref.shape) == 1:
            ref = ref.reshape(1, -1) if isinstance(ref, DeviceArray) else np.asarray(ref)[None]
        gamma = None
        if test == "ipcc-ar6-c":   # (every refusal before the first launch)
            x_years, year_seg, blocks = _ar6_axis(ref_time, int(ref.shape[1]), kwargs.get("ref_pi") is not None)
        res = change_test(fut, ref, ROBUSTNESS_TESTS.get(test, "moments"), device=dev)
        R, cells = int(fut.shape[0]), tuple(fut.shape[2:])
        if test == "ipcc-ar6-c":
            gamma = _ar6_gamma(dev, ref, x_years, year_seg, blocks, kwargs.get("ref_pi") is not None)
        T1, T2 = int(fut.shape[1]), int(ref.shape[-1 - len(cells)])
        ok = (res["n_fut"] == T1) & (res["n_ref"] == T2) if rule == "any" else (res["n_fut"] >= n_min) & (res["n_ref"] >= n_min)
        valid = dev.to_device(ok.astype(np.uint8))
        delta = dev.to_device(res["delta"])
        mean_ref = dev.to_device(res["mean_ref"]) if rel_thresh is not None else None
        changed = None
        if gamma is not None:
            with np.errstate(invalid="ignore"):
                changed = dev.to_device((np.abs(res["delta"]) > gamma).astype(np.uint8))
        if test in ROBUSTNESS_TESTS:
            pvals = res["pvals"]
            with np.errstate(invalid="ignore"):
                changed = dev.to_device((pvals < p_change).astype(np.uint8))
    if weights is None:
        w = np.ones(R)
    else:
        w = np.asarray(weights, np.float64).reshape(-1)
        if w.size != R:
            raise ValueError(f"weights must have one value per realization ({R}), got {w.size}")
    out = K.robust_fractions(dev, delta, w, changed=changed, valid=valid, mean_ref=mean_ref, strict_sign=strict_sign,
                             abs_thresh=abs_thresh if test == "threshold" else None, rel_thresh=rel_thresh if test == "threshold" else None)
    if keep:
        res_out = {"fractions": out}
    else:
        o = out.get()
        res_out = {name: o[k].reshape(cells) for name, k in capi.RF_ROWS.items()}
    if pvals is not None:
        res_out["pvals"] = pvals.reshape((R,) + tuple(cells))
    return res_out


def robustness_coefficient(fut, ref, *, device=None, keep: bool = False):
    """_robustness.py:430-515 on arrays: ``fut`` (R, T1, *cells), ``ref`` (T2, *cells); returns float64 (*cells)."""
    dev = device or get_device()
    f, cells = _field3(fut, "fut", dev)
    if isinstance(ref, DeviceArray):
        r = ref.reshape(ref.shape[0], -1)
    else:
        r = np.asarray(ref)
        if r.dtype.kind in "iub":
            raise NotServed("robustness: ref is an integer field")
        r = dev.to_device(np.ascontiguousarray(r.reshape(r.shape[0], -1)))
    if np.dtype(r.dtype) != np.dtype(f.dtype):
        raise NotServed(f"robustness: fut is {np.dtype(f.dtype).name} and ref {np.dtype(r.dtype).name}")
    R, T1, T2 = int(f.shape[0]), int(f.shape[1]), int(r.shape[0])
    if T1 > capi.CT_MAX_T or R * T1 + R > capi.RC_MAX_POOL or T2 + R > capi.RC_MAX_POOL:
        raise NotServed(f"robustness_coefficient: pools of up to {capi.RC_MAX_POOL} values are served, got R {R}, T {T1} and {T2}")
    out = K.robust_coefficient(dev, f, r)
    return out if keep else out.get().reshape(cells)


def robustness_categories(changed_or_fractions, agree=None, valid=None, *, categories=None, ops=None, thresholds=None):
    """_robustness.py:336-426 in numpy: the categorical map (int, 99 where no category holds) and its flag attributes, as
    ``(array, attrs)``."""
    import operator

    if categories is None:
        categories = ["Robust signal", "No change or no signal", "Conflicting signal"]
    if ops is None:
        ops = [(">=", ">="), ("<", None), (">=", "<")]
    if thresholds is None:
        thresholds = [(0.66, 0.8), (0.66, None), (0.66, 0.8)]
    if isinstance(changed_or_fractions, dict):
        changed, agree, valid = (changed_or_fractions[k] for k in ("changed", "agree", "valid"))
    else:
        changed = changed_or_fractions
    changed = np.asarray(changed, np.float64)
    cmp = {">": operator.gt, "<": operator.lt, ">=": operator.ge, "<=": operator.le, "==": operator.eq, "!=": operator.ne}
    out = np.full(changed.shape, 99, dtype=np.int64)
    for i, ((chg_op, agr_op), (chg_t, agr_t)) in reversed(list(enumerate(zip(ops, thresholds), 1))):
        if not agr_op:
            cond = cmp[chg_op](changed, chg_t)
        elif not chg_op:
            cond = cmp[agr_op](np.asarray(agree), agr_t)
        else:
            cond = cmp[chg_op](changed, chg_t) & cmp[agr_op](np.asarray(agree), agr_t)
        out = np.where(cond, i, out)
    if valid is not None:
        out = np.where(np.asarray(valid) > 0, out, 99)
    attrs = {"flag_values": list(range(1, len(categories) + 1)), "_FillValue": 99, "flag_descriptions": categories,
             "flag_meanings": " ".join(c.casefold().replace(" ", "_") for c in categories)}
    return out, attrs


# ---- the xarray adapter (patch.install) ------------------------------------------------------------------------------------
ADAPTED = ("robustness_fractions", "robustness_coefficient")
_REFERENCE_TESTS = tuple(ROBUSTNESS_TESTS) + ("ipcc-ar6-c",)


def make_adapters(env, originals: dict, xr=None, gen_call_string=None, registry=None, device=None) -> dict:
    """``robustness_fractions`` and ``robustness_coefficient`` of ``xclim.ensembles._robustness`` on DataArrays: the dims and
    coordinates of the inputs without ``time`` and ``realization``, the attributes and description strings of
    _robustness.py:273-331 and :507-514, Dataset input for the coefficient.  ``xr`` (for ``Dataset``), ``gen_call_string`` and
    ``registry`` (SIGNIFICANCE_TESTS) are the defining module's own.  Whatever raises :class:`NotServed` goes to the original."""
    from .xr_adapter import forwarding_adapter

    DA = env.DataArray
    Dataset = getattr(xr, "Dataset", None)

    def values(da, *lead):
        if not isinstance(da, DA):
            raise NotServed("robustness: an input that is not a DataArray")
        if getattr(da.data, "chunks", None) is not None:
            raise NotServed("robustness: chunked fields")
        if any(d not in da.dims for d in lead):
            raise NotServed(f"robustness: a field without {lead}")
        cells = tuple(d for d in da.dims if d not in lead)
        return np.asarray(da.transpose(*lead, *cells).values), cells

    def call_string(params):
        if gen_call_string is not None:
            return gen_call_string("", **params)[1:-1]
        return ", ".join(f"{k}={v}" for k, v in params.items())

    def fractions(p):
        fut, ref, test, weights, invalid = p["fut"], p["ref"], p["test"], p["weights"], p["invalid"]
        strict_sign, kwargs = p["strict_sign"], dict(p.get("kwargs") or {})
        if Dataset is None:
            raise NotServed("robustness_fractions: no Dataset class")
        if registry is not None and test in registry and test not in _REFERENCE_TESTS:
            raise NotServed(f"robustness_fractions: the user-registered test {test}")
        if registry is not None and test is not None and test != "threshold" and test not in registry:   # the reference's message
            raise ValueError(f"Statistical test {test} must be one of {', '.join(registry.keys())}.")
        real = "realization"
        has_real = isinstance(fut, DA) and real in fut.dims
        lead = ((real,) if has_real else ()) + (("time",) if ref is not None else ())
        f, cells = values(fut, *lead)
        if not has_real:
            f = f[None]
        r = None
        if ref is not None:
            rlead = ((real,) if real in getattr(ref, "dims", ()) else ()) + ("time",)
            r, rcells = values(ref, *rlead)
            if rcells != cells:
                raise NotServed("robustness_fractions: fut and ref on different cell dimensions")
            if real not in ref.dims:
                r = r[None]
            if r.shape[0] != f.shape[0]:
                raise NotServed("robustness_fractions: fut and ref with different realizations")
        w = None
        if weights is not None:
            w, wcells = values(weights, real)
            if wcells:
                raise NotServed("robustness_fractions: weights along more than realization")
        if test == "threshold":
            params = {k: kwargs[k] for k in ("abs_thresh", "rel_thresh") if kwargs.get(k) is not None}
            if len(params) != 1:
                raise ValueError("One and only one of abs_thresh or rel_thresh must be given if test='threshold'.")
        elif test in ROBUSTNESS_TESTS:
            params = {"p_change": kwargs.get("p_change", 0.05)}
        else:
            params = {}
        extra = {}
        if test == "ipcc-ar6-c":
            from .xr_adapter import time_axis_of

            params = {"ref_pi": kwargs.get("ref_pi")}
            try:
                extra = {"ref_time": time_axis_of(ref), "ref_pi": kwargs.get("ref_pi")}
            except Exception:
                raise NotServed("robustness_fractions: ipcc-ar6-c on a time coordinate without calendar fields") from None
        res = robustness_fractions(f, r, test, w, invalid, strict_sign, device=device, **{**params, **extra})
        test_str = f"Significant change was tested with test {test} and parameters {call_string(params)}."
        strict = "strictly " if strict_sign else "zero or "
        coords = {k: c for k, c in fut.coords.items() if k in cells}
        desc = {
            "changed": (f"Fraction of valid members showing significant change. {test_str}", True),
            "positive": (f"Fraction of valid members showing {strict} positive change.", False),
            "changed_positive": (f"Fraction of valid members showing significant and {strict} positive change. {test_str}", True),
            "negative": (f"Fraction of valid members showing {strict} negative change.", False),
            "changed_negative": (f"Fraction of valid members showing significant and {strict} negative change. {test_str}", True),
            "valid": ("Fraction of valid members (No missing values along time).", False),
            "agree": ("Fraction of valid members agreeing on the sign of change. "
                      + ("Maximum between the positive, negative and no change fractions." if strict_sign
                         else "Maximum between the zero or positive and the zero or negative change fractions."), False),
        }
        out = {}
        for name in ("changed", "positive", "changed_positive", "negative", "changed_negative", "valid", "agree"):
            text, tested = desc[name]
            attrs = {"description": text, "units": ""}
            if tested:
                attrs["test"] = str(test)
            out[name] = DA(res[name], dims=cells, coords=coords, attrs=attrs)
        if "pvals" in res:
            pc = dict(coords)
            if has_real and real in fut.coords:
                pc[real] = fut.coords[real]
            pv = res["pvals"] if has_real else res["pvals"][0]
            out["pvals"] = DA(pv, dims=((real,) if has_real else ()) + cells, coords=pc,
                              attrs={"description": f"P-values from change significance test. {test_str}", "units": ""})
        return Dataset(out, attrs={"description": "Significant change and sign of change fractions."})

    COEF_ATTRS = {"name": "R", "long_name": "Ensemble robustness coefficient",
                  "description": "Ensemble robustness coefficient as defined by Knutti and Sedláček (2013).",
                  "reference": "Knutti, R. and Sedláček, J. (2013) Robustness and uncertainties in the new CMIP5 climate model projections. "
                               "Nat. Clim. Change.", "units": ""}

    def coefficient_one(fut, ref):
        f, cells = values(fut, "realization", "time")
        r, rcells = values(ref, "time")
        if rcells != cells:
            raise NotServed("robustness_coefficient: fut and ref on different cell dimensions")
        out = robustness_coefficient(f, r, device=device)
        return DA(out, dims=cells, coords={k: c for k, c in fut.coords.items() if k in cells}, name=fut.name, attrs=COEF_ATTRS)

    def coefficient(p):
        fut, ref = p["fut"], p["ref"]
        if isinstance(fut, DA) and isinstance(ref, DA):
            return coefficient_one(fut, ref)
        try:
            fvars, rvars = dict(fut.data_vars), dict(ref.data_vars)
        except AttributeError:
            raise NotServed("robustness_coefficient: inputs that are neither DataArrays nor Datasets") from None
        if Dataset is None or list(fvars) != list(rvars):
            raise NotServed("robustness_coefficient: Datasets with different variables")
        return Dataset({k: coefficient_one(fvars[k], rvars[k]) for k in fvars}, attrs=COEF_ATTRS)

    return {"robustness_fractions": forwarding_adapter("robustness_fractions", originals["robustness_fractions"], fractions),
            "robustness_coefficient": forwarding_adapter("robustness_coefficient", originals["robustness_coefficient"], coefficient)}
