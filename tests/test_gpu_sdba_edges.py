"""The grouped quantile-mapping kernels at their size edges, against the ORACLE (oracle/sdba.py) — never against another HIP path.

The one-launch kernels (winsel.hip k_group_quantiles, qdm.hip k_qdm_groups) and the sliding window (winsel.hip k_window_quantiles)
are compared with the per-group HIP route in tests/test_gpu_api.py; a change that moves the per-group route moves both sides of those
comparisons.  Here every case is the oracle's, at the group sizes where an instance changes (32 | 33, 64 | 65 rows per group, 1024 |
1025 window rows, 32 | 33 nodes), on cells that are not clean: NaN samples, groups with no or one valid sample, empty cells, ties,
infinities, a negative and a zero mean, a constant, values at both ends of the float32 exponent range.  The launch trace says which
entry point served a case, so a silent fallback cannot pass for the fast path.  The split tables below are read by the CPU guard of
tests/test_gpu_ladders.py.

Tolerances: the ones the oracle tests of tests/test_gpu_api.py use for the same quantities (EQM hist_q rtol 1e-6; af rtol 1e-6,
atol 1e-5; DQM scaling rtol 1e-6, hist_q rtol 1e-5 / atol 2e-6, af rtol 1e-5 / atol 1e-5; QDM rtol 1e-6, + atol 1e-6 for "linear";
quantile_series bit for bit); NaN and infinity patterns equal; no element is left out of a comparison.

The checks are functions of (device, sizes): tests/test_hostsim_cpu.py re-runs them at fiber sizes on the host simulation."""

import numpy as np
import pytest

from oracle import sdba as osdba
from oracle.timeutil import OTime
from xclim_amd.timeaxis import TimeAxis
from poisoned import poisoned_outputs  # noqa: F401  (autouse: the tests of this module that use the device run on poisoned output buffers)

pytestmark = pytest.mark.gpu

# switch points (tests/test_gpu_ladders.py::test_dispatch_points_are_tested reads these)
GROUP_SPLITS = (32, 64)          # rows per group: k_group_quantiles<32 | 64>, k_qdm_groups<32 | 64>, k_window_quantiles' per | per group
WINDOW_ROW_SPLITS = (1024,)      # rows of the first window (n0) and of the largest one (most): WS_CAP
NODE_SPLITS = (32,)              # nq: xh_qdm_adjust_groups, and the window kernel (WS_MAXQ: 2 nq targets on 64 lanes)
GQ_NODE_SPLITS = (1024,)         # nq: gq_train (xh_eqm_train_groups / xh_dqm_train_groups read the nodes from memory)
GQ_LADDER_NQ = (1024, 1025)
LADDER_YEARS = tuple(sorted(set(GROUP_SPLITS) | {s + 1 for s in GROUP_SPLITS}))
LADDER_NQ = tuple(sorted(set(NODE_SPLITS) | {s + 1 for s in NODE_SPLITS}))
WINDOW_NQ = LADDER_NQ             # the window kernel's own node ladder (test_sliding_window_node_limit)
# (years, window, calendar): what each case reaches is in the docstring of test_sliding_window_training
WINDOW_CASES = ((33, 15, "noleap"), (64, 15, "noleap"), (65, 15, "noleap"), (40, 25, "noleap"), (41, 25, "noleap"),
                (50, 7, "standard"), (17, 61, "standard"))
WINDOW_ROWS = tuple(y * w for y, w, cal in WINDOW_CASES if cal == "noleap")     # 1000 / 1025 on both sides of WS_CAP

CELLS = ("plain", "nan3", "nan90", "hist_nan", "ref_nan", "ties", "ref_inf", "hist_ninf", "negated", "hist_zero", "const", "big",
         "tiny") + ("plain",) * 5 + ("nan3",) * 3 + ("ties",) * 3
FEW_CELLS = ("plain", "nan90", "ties", "ref_inf", "negated", "tiny")   # (the host simulation's share)


def _axes(years, calendar, start=2001):
    if calendar == "standard":
        T = sum(366 if (y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)) else 365 for y in range(start, start + years))
        return TimeAxis.daily(f"{start}-01-01", T), OTime.standard(f"{start}-01-01", T)
    T = 365 * years
    return TimeAxis.daily(f"{start}-01-01", T, calendar), OTime.noleap(start, T, calendar)


def edge_fields(seed, T, cells=CELLS):
    """(ref, hist, sim), each (T, len(cells)) float32 on a daily axis; the cell kinds:
    plain; nan3: 3 % NaN; nan90: ~90 % NaN (groups with no or one valid sample); hist_nan / ref_nan: that field all NaN (sim: with
    hist); ties: rounded; ref_inf: a run of +inf in ref (and sim); hist_ninf: a run of -inf in hist (and sim); negated: a negative
    mean; hist_zero: hist (and sim) all zero (0 / 0 for "*"); const; big: around 1e38; tiny: on both sides of zero inside +-1e-37."""
    rng = np.random.default_rng(seed)
    C = len(cells)
    t = np.arange(T)[:, None]
    seas = np.sin(2 * np.pi * (t - 100) / 365)
    ref = (30 + 8 * seas + rng.normal(0, 3, (T, C))).astype(np.float32)
    hist = (31.5 + 9 * seas + rng.normal(0, 4, (T, C))).astype(np.float32)
    sim = (33 + 9 * seas + 3.0 * t / T + rng.normal(0, 4, (T, C))).astype(np.float32)
    a, b = T // 7, T // 7 + max(3, T // 40)
    for c, kind in enumerate(cells):
        if kind == "nan3":
            for f in (ref, hist, sim):
                f[rng.random(T) < 0.03, c] = np.nan
        elif kind == "nan90":
            for f in (ref, hist, sim):
                f[rng.random(T) < 0.9, c] = np.nan
        elif kind == "hist_nan":
            hist[:, c] = np.nan
            sim[:, c] = np.nan
        elif kind == "ref_nan":
            ref[:, c] = np.nan
        elif kind == "ties":
            ref[:, c], hist[:, c], sim[:, c] = np.round(ref[:, c]), np.round(hist[:, c] * 2) / 2, np.round(sim[:, c])
        elif kind == "ref_inf":
            ref[a:b, c] = np.inf
            sim[a:b, c] = np.inf
        elif kind == "hist_ninf":
            hist[a:b, c] = -np.inf
            sim[a:b, c] = -np.inf
        elif kind == "negated":
            ref[:, c], hist[:, c], sim[:, c] = -ref[:, c], -hist[:, c], -sim[:, c]
        elif kind == "hist_zero":
            hist[:, c] = 0.0
            sim[:, c] = 0.0
        elif kind == "const":
            ref[:, c], hist[:, c], sim[:, c] = 7.25, 6.5, 8.0
        elif kind == "big":
            for f in (ref, hist, sim):
                f[:, c] = (1e38 * (1 + 0.1 * rng.normal(0, 1, T))).astype(np.float32)
        elif kind == "tiny":
            for f in (ref, hist, sim):
                f[:, c] = (1e-37 * rng.uniform(-1, 1, T)).astype(np.float32)
    return ref, hist, sim


def close(case, what, got, exp, rtol, atol=0.0):
    """assert_allclose over every element (NaN and infinities in the same places), the worst relative deviation printed first."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, f"{case} {what}: {got.shape} against {exp.shape}"
    fin = np.isfinite(got) & np.isfinite(exp)
    atol = np.asarray(atol, dtype=np.float64)            # (a scalar, or one value per cell)
    with np.errstate(all="ignore"):   # relative to |expected|, or to atol / rtol where the absolute term is the larger allowance
        dev_ = np.where(fin, np.abs(got - exp) / np.maximum(np.maximum(np.abs(exp), atol / rtol), 1e-300), 0.0)
    worst = float(dev_.max(initial=0.0))
    print(f"[sdba-edges] {case} {what}: worst relative deviation {worst:.3g} (rtol {rtol:g}, atol {float(atol.max()):g}), "
          f"{int(np.isnan(exp).sum())} NaN, {int(np.isinf(exp).sum())} inf of {exp.size}")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=f"{case} {what}: NaN pattern")
    np.testing.assert_array_equal(np.isinf(got), np.isinf(exp), err_msg=f"{case} {what}: infinity pattern")
    np.testing.assert_array_equal(got[np.isinf(exp)], exp[np.isinf(exp)], err_msg=f"{case} {what}: sign of the infinities")
    with np.errstate(all="ignore"):   # numpy's allclose rule, |got - exp| <= atol + rtol |exp|, with a per-cell atol
        bad = fin & ~(np.abs(got - exp) <= atol + rtol * np.abs(exp))
    assert not bad.any(), (f"{case} {what}: {int(bad.sum())} of {exp.size} beyond rtol {rtol:g} / atol {float(atol.max()):g}; first at "
                           f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]!r} against {exp[bad][0]!r}; worst relative deviation {worst:.3g}")


class traced:
    """The entry points called on `dev` inside the block, as a list of names (``.names``) and of (name, args) (``.calls``)."""

    def __init__(self, dev, monkeypatch=None):
        self.dev = dev
        if monkeypatch is not None:
            monkeypatch.setenv("XH_DIAGNOSTICS", "1")

    def __enter__(self):
        self.calls = self.dev.start_trace()
        return self

    def __exit__(self, *exc):
        self.dev.stop_trace()
        self.names = [n for n, _ in self.calls]
        return False

    def count(self, name):
        return self.names.count(name)


def _q(nq):
    return osdba.equally_spaced_nodes(nq)


# ---------------------------------------------------------------- the group-size ladder: training
def check_group_training(dev, years, calendar, kind, nq, cells=CELLS, monkeypatch=None):
    """EmpiricalQuantileMapping.train / DetrendedQuantileMapping.train, group="time.dayofyear" without a window (a group = one row
    per year): xh_eqm_train_groups / xh_dqm_train_groups up to 64 rows per group, the per-group route beyond."""
    from xclim_amd import sdba as xsdba

    ta, ot = _axes(years, calendar)
    ref, hist, _ = edge_fields(1000 + years, len(ta), cells)
    G = 366 if calendar == "standard" else 365
    fast = years <= 64
    case = f"train-{years}-{calendar}-{kind}-nq{nq}"
    with traced(dev, monkeypatch) as tr:
        eqm = xsdba.EmpiricalQuantileMapping.train(ref, hist, nquantiles=nq, kind=kind, group="time.dayofyear", time=ta, device=dev)
    if fast:
        assert tr.count("xh_eqm_train_groups") == 1 and tr.count("xh_eqm_train") == 0, tr.names[:8]
    else:
        assert tr.count("xh_eqm_train_groups") == 0 and tr.count("xh_eqm_train") == G, (tr.count("xh_eqm_train"), tr.names[:8])
    eaf, ehq, labels = osdba.eqm_train_grouped(ref, hist, ot, "dayofyear", 1, nq, kind)
    np.testing.assert_array_equal(eqm.group_labels, labels)
    close(case, "eqm hist_q", eqm.hist_q, ehq, 1e-6)
    close(case, "eqm af", eqm.af, eaf, 1e-6, 1e-5)
    with traced(dev, monkeypatch) as tr:
        dqm = xsdba.DetrendedQuantileMapping.train(ref, hist, nquantiles=nq, kind=kind, group="time.dayofyear", time=ta, device=dev)
    if fast:
        assert tr.count("xh_dqm_train_groups") == 1 and tr.count("xh_eqm_train") == 0, tr.names[:8]
    else:   # the group means in one launch per field, the tables from the per-group training of the normalised series
        assert tr.count("xh_dqm_train_groups") == 0 and tr.count("xh_eqm_train_groups") == 0, tr.names[:8]
        assert tr.count("xh_poly_trend_groups") == 2 and tr.count("xh_eqm_train") == G, tr.names[:8]
    labels, daf, dhq, dsc = osdba.dqm_train_grouped(ref, hist, ot, "dayofyear", nq, kind)
    np.testing.assert_array_equal(dqm.group_labels, labels)
    close(case, "dqm scaling", dqm.scaling, dsc, 1e-6)
    close(case, "dqm hist_q", dqm.hist_q, dhq, 1e-5, 2e-6)
    close(case, "dqm af", dqm.af, daf, 1e-5, 1e-5)


@pytest.mark.parametrize("kind", ["+", "*"])
@pytest.mark.parametrize("years", LADDER_YEARS)
def test_group_size_ladder_training(dev, monkeypatch, years, kind):
    check_group_training(dev, years, "noleap", kind, 20, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kind", ["+", "*"])
def test_group_training_standard_calendar_64_years(dev, monkeypatch, kind):
    """(day 366 is a group of 16 rows among groups of 64)"""
    check_group_training(dev, 64, "standard", kind, 20, monkeypatch=monkeypatch)


@pytest.mark.parametrize("nq", LADDER_NQ)
def test_group_training_node_limit(dev, monkeypatch, nq):
    """32 | 33 nodes: the training kernel takes both (its limit is the node table, 1024)."""
    check_group_training(dev, 33, "noleap", "+", nq, monkeypatch=monkeypatch)


def check_group_kernel_node_limit(dev, nq):
    """xh_eqm_train_groups / xh_dqm_train_groups themselves at their own node limit: 1024 nodes served, 1025 declined."""
    from xclim_amd import kernels as K

    T, G = 45, 5
    ref, hist, _ = edge_fields(1500, T, FEW_CELLS)
    gid = np.arange(T) % G
    rows = np.argsort(gid, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=G))]).astype(np.int64)
    q = np.linspace(0.0, 1.0, nq)
    d_ref, d_hist = dev.to_device(ref), dev.to_device(hist)
    for normalised in (False, True):
        res = K.eqm_train_groups(dev, d_ref, d_hist, rows, offs, q, "+", normalised=normalised)
        if nq > 1024:
            assert res is None
            continue
        exp = [(osdba.dqm_train if normalised else osdba.eqm_train)(ref[gid == g], hist[gid == g], q, "+") for g in range(G)]
        tol = ((1e-5, 2e-6), (1e-5, 1e-5)) if normalised else ((1e-6, 0.0), (1e-6, 1e-5))
        close(f"group-kernel-nq{nq}", f"hist_q normalised={normalised}", res[1].get(), np.stack([e[1] for e in exp]), *tol[0])
        close(f"group-kernel-nq{nq}", f"af normalised={normalised}", res[0].get(), np.stack([e[0] for e in exp]), *tol[1])


@pytest.mark.parametrize("nq", GQ_LADDER_NQ)
def test_group_training_kernel_node_limit(dev, nq):
    check_group_kernel_node_limit(dev, nq)


# ---------------------------------------------------------------- the group-size ladder: QuantileDeltaMapping.adjust
def _qdm_case(dev, years, calendar, kind, nq, cells):
    """A trained QuantileDeltaMapping (its tables checked against the oracle's: the adjust comparisons below hand them to the
    oracle) and a sim field.  Trained per test: nothing of one test's device memory outlives it."""
    from xclim_amd import sdba as xsdba

    ta, ot = _axes(years, calendar)
    ref, hist, sim = edge_fields(2000 + years, len(ta), cells)
    qdm = xsdba.QuantileDeltaMapping.train(ref, hist, nquantiles=nq, kind=kind, group="time.dayofyear", time=ta, device=dev)
    af = qdm.af
    eaf, ehq, labels = osdba.eqm_train_grouped(ref, hist, ot, "dayofyear", 1, nq, kind)
    np.testing.assert_array_equal(qdm.group_labels, labels)
    close(f"qdm-train-{years}-{calendar}-{kind}-nq{nq}", "hist_q", qdm.hist_q, ehq, 1e-6)
    close(f"qdm-train-{years}-{calendar}-{kind}-nq{nq}", "af", af, eaf, 1e-6, 1e-5)
    return ta, ot, sim, qdm, af


def check_group_qdm(dev, years, calendar, kind, interp, nq, cells=CELLS, monkeypatch=None):
    """QuantileDeltaMapping.adjust with a day-of-year grouping: xh_qdm_adjust_groups up to 64 rows per group and 32 nodes, one
    xh_qdm_adjust per group beyond; the oracle ranks and interpolates inside every group (mode "group")."""
    from xclim_amd import kernels as K
    from xclim_amd import sdba as xsdba

    ta, ot, sim, qdm, af = _qdm_case(dev, years, calendar, kind, nq, cells)
    G = 366 if calendar == "standard" else 365
    fast = years <= 64 and nq <= 32
    for extrap in ("constant", "nan"):
        with traced(dev, monkeypatch) as tr:
            if interp == "linear" and extrap == "nan":
                # (the model refuses it with a sub-grouping: upstream's NaN region is the hull of ALL groups' nodes.  The kernel
                # has the per-group form: called as adjust() calls it)
                if not fast:
                    continue
                lay = xsdba._GroupMajor(qdm.group.index(ta, qdm.group_labels), G)
                got = K.qdm_adjust_groups(dev, dev.to_device(sim), lay.perm, lay.offs, qdm._af, qdm.quantiles, kind, interp, extrap)
                assert got is not None
                got = got.get()
            else:
                got = qdm.adjust(sim, interp=interp, extrapolation=extrap, time=ta)
        if fast:
            assert tr.count("xh_qdm_adjust_groups") == 1 and tr.count("xh_qdm_adjust") == 0, tr.names[:8]
        else:
            assert tr.count("xh_qdm_adjust_groups") == 0 and tr.count("xh_qdm_adjust") == G, (tr.count("xh_qdm_adjust"), tr.names[:8])
        exp = osdba.qdm_adjust_grouped(sim, ot, "dayofyear", qdm.group_labels, af, qdm.quantiles, kind, interp, extrap, mode="group")
        close(f"qdm-{years}-{calendar}-{kind}-{interp}-nq{nq}", extrap, got, exp, 1e-6, 1e-6 if interp == "linear" else 0.0)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("kind", ["+", "*"])
@pytest.mark.parametrize("years", LADDER_YEARS)
def test_group_size_ladder_qdm_adjust(dev, monkeypatch, years, kind, interp):
    check_group_qdm(dev, years, "noleap", kind, interp, 20, monkeypatch=monkeypatch)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_group_qdm_adjust_standard_calendar_64_years(dev, monkeypatch, interp):
    check_group_qdm(dev, 64, "standard", "+", interp, 20, monkeypatch=monkeypatch)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("nq", LADDER_NQ)
def test_group_qdm_adjust_node_limit(dev, monkeypatch, nq, interp):
    check_group_qdm(dev, 33, "noleap", "*", interp, nq, monkeypatch=monkeypatch)


# ---------------------------------------------------------------- the sliding window
def _window_route(tr, who, per_group, G):
    """(groups the window kernel served, per-group trainings) of one traced training; the G argument of every ACCEPTED window
    launch — a declined call (not the kernel's shape) is followed by the per-group route for every group."""
    n_train = tr.count(per_group)
    served = sum(int(args[9]) for name, args in tr.calls if name == who)
    return (0 if n_train == G else served), n_train


def check_window_training(dev, years, window, calendar, kind, cells=CELLS, monkeypatch=None, nq=12):
    """group="time.dayofyear" with a window, EQM and DQM: xh_eqm_train_window / xh_dqm_train_window while a step moves at most 64
    rows, the window holds at most 1024 and there are at most 32 nodes, every group from its gathered sample otherwise — one
    route, never a mixture of a declined stretch and finished ones."""
    from xclim_amd import sdba as xsdba

    ta, ot = _axes(years, calendar)
    ref, hist, _ = edge_fields(3000 + years + window, len(ta), cells)
    G = 366 if calendar == "standard" else 365
    case = f"window-{years}x{window}-{calendar}-{kind}-nq{nq}"
    if calendar == "noleap":
        fast, rest = years <= 64 and years * window <= 1024 and nq <= 32, 0
    elif years * window <= 1024:
        fast, rest = True, 1                  # day 366 from its gathered sample
    else:
        fast, rest = True, None               # (17 x 61: the ends of the year, where the window reaches beyond the series)
    with traced(dev, monkeypatch) as tr:
        eqm = xsdba.EmpiricalQuantileMapping.train(ref, hist, nquantiles=nq, kind=kind, group="time.dayofyear", window=window, time=ta, device=dev)
    served, n_train = _window_route(tr, "xh_eqm_train_window", "xh_eqm_train", G)
    print(f"[sdba-edges] {case}: xh_eqm_train_window x {tr.count('xh_eqm_train_window')} ({served} groups), xh_eqm_train x {n_train}")
    if not fast:
        assert served == 0 and n_train == G and tr.count("xh_eqm_train_window") <= 1
    else:
        assert served > 0 and served + n_train == G and (rest is None or n_train == rest), (served, n_train)
    eaf, ehq, labels = osdba.eqm_train_grouped(ref, hist, ot, "dayofyear", window, nq, kind)
    np.testing.assert_array_equal(eqm.group_labels, labels)
    close(case, "eqm hist_q", eqm.hist_q, ehq, 1e-6)
    close(case, "eqm af", eqm.af, eaf, 1e-6, 1e-5)
    with traced(dev, monkeypatch) as tr:
        dqm = xsdba.DetrendedQuantileMapping.train(ref, hist, nquantiles=nq, kind=kind, group="time.dayofyear", window=window, time=ta, device=dev)
    served, n_train = _window_route(tr, "xh_dqm_train_window", "xh_eqm_train", G)
    if not fast:
        assert served == 0 and n_train == G and tr.count("xh_dqm_train_window") <= 1
    else:
        assert served > 0 and served + n_train == G and (rest is None or n_train == rest), (served, n_train)
    labels, daf, dhq, dsc = osdba.dqm_train_grouped(ref, hist, ot, "dayofyear", nq, kind, window=window)
    close(case, "dqm scaling", dqm.scaling, dsc, 1e-6)
    close(case, "dqm hist_q", dqm.hist_q, dhq, 1e-5, 2e-6)
    close(case, "dqm af", dqm.af, daf, 1e-5, 1e-5)


@pytest.mark.parametrize("kind", ["+", "*"])
@pytest.mark.parametrize("years,window,calendar", WINDOW_CASES)
def test_sliding_window_training(dev, monkeypatch, years, window, calendar, kind):
    """33 x 15: the 64-slot sorts of the leaving / entering rows; 64 x 15: per 64, 960 rows; 65 x 15: per > 64, everything per
    group; 40 x 25: 1000 rows; 41 x 25: 1025 > the window's capacity, per group; 50 x 7 standard: day 366 from its gathered sample;
    17 x 61 standard: 1037 sample rows of which at most 1024 are valid at the ends of the year — the window kernel serves those
    stretches (it declined them while the padded row list was handed on)."""
    check_window_training(dev, years, window, calendar, kind, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kind", ["+", "*"])
@pytest.mark.parametrize("nq", WINDOW_NQ)
def test_sliding_window_node_limit(dev, monkeypatch, nq, kind):
    """33 years x 15 days at the window kernel's node limit.  32 nodes: 64 targets, one on every lane (the last picked key is
    slot 63, the last node 31), through xh_eqm_train_window / xh_dqm_train_window.  33: the whole route is declined — at most one
    window call, then exactly 365 per-group trainings."""
    check_window_training(dev, 33, 15, "noleap", kind, monkeypatch=monkeypatch, nq=nq)


def check_window_growing_past_capacity(dev):
    """A hand-made schedule whose FIRST window fits (n0 = 1020 rows) and which grows past 1024 valid rows on its second step
    (3 rows enter, none leave, twice): xh_eqm_train_window declines it.  The schedules of xclim_amd/sdba.py never have this
    shape — their first window is as large as any — so this is the only run of that branch."""
    from xclim_amd import kernels as K

    T, C, per = 1100, 5, 3
    ref, hist, _ = edge_fields(4500, T, FEW_CELLS[:C])
    rows0 = np.arange(1020)
    leave = np.full((2, per), -1)
    q = _q(5)
    d_ref, d_hist = dev.to_device(ref), dev.to_device(hist)
    grow = np.array([[1020, 1021, 1022], [1023, 1024, 1025]])          # 1023, then 1026 rows present
    assert K.eqm_train_window(dev, d_ref, d_hist, rows0, grow, leave, q, "+") is None
    assert K.eqm_train_window(dev, d_ref, d_hist, rows0, grow, leave, q, "+", normalised=True) is None
    fits = np.array([[1020, 1021, 1022], [1023, -1, -1]])               # 1023, then 1024: served, and the oracle's tables
    res = K.eqm_train_window(dev, d_ref, d_hist, rows0, fits, leave, q, "+")
    assert res is not None
    exp = [osdba.eqm_train(ref[:n], hist[:n], q, "+") for n in (1020, 1023, 1024)]
    close("window-capacity", "hist_q", res[1].get(), np.stack([e[1] for e in exp]), 1e-6)
    close("window-capacity", "af", res[0].get(), np.stack([e[0] for e in exp]), 1e-6, 1e-5)


def test_sliding_window_that_grows_past_its_capacity_is_declined(dev):
    check_window_growing_past_capacity(dev)


def check_window_kernel(dev, years, window, kind, G, cells=FEW_CELLS, nq=7):
    """xh_eqm_train_window itself on the first G groups of the ring schedule (the host simulation's size)."""
    from xclim_amd import kernels as K
    from xclim_amd import sdba as xsdba

    ta, ot = _axes(years, "noleap")
    ref, hist, _ = edge_fields(4000 + years, len(ta), cells)
    rows0, enter, leave = xsdba.Grouper("time.dayofyear", window).ring_schedule(ta)
    q = _q(nq)
    res = K.eqm_train_window(dev, dev.to_device(ref), dev.to_device(hist), rows0, enter[:G - 1], leave[:G - 1], q, kind)
    if nq > 32:
        assert res is None
        return
    assert res is not None, "xh_eqm_train_window declined the shape"
    af, hq = (a.get() for a in res)
    doy = np.asarray(ot.doy)
    exp = [osdba.eqm_train(osdba.grouped_sample(ref, ot, "dayofyear", window, lab), osdba.grouped_sample(hist, ot, "dayofyear", window, lab),
                           q, kind) for lab in np.unique(doy)[:G]]
    case = f"window-kernel-{years}x{window}-{kind}-nq{nq}"
    close(case, "hist_q", hq, np.stack([e[1] for e in exp]), 1e-6)
    close(case, "af", af, np.stack([e[0] for e in exp]), 1e-6, 1e-5)


# ---------------------------------------------------------------- empty groups
def _leap_model(dev):
    from xclim_amd import sdba as xsdba

    ta, ot = _axes(4, "standard", 2000)                 # 2000-2003: 366 labels
    ref, hist, _ = edge_fields(5000, len(ta), CELLS)
    qdm = xsdba.QuantileDeltaMapping.train(ref, hist, nquantiles=10, kind="+", group="time.dayofyear", time=ta, device=dev)
    assert len(qdm.group_labels) == 366
    af = qdm.af
    close("empty-model", "af", af, osdba.eqm_train_grouped(ref, hist, ot, "dayofyear", 1, 10, "+")[0], 1e-6, 1e-5)
    return qdm, af


def check_empty_trailing_groups(dev, interp, short, monkeypatch=None):
    """A model with day 366, a sim without: the trailing group of the table is empty (`short`: 181 days from 1 January — the
    groups 182 .. 366 are, a run of empty groups that ends the table)."""
    from xclim_amd import sdba as xsdba

    qdm, af = _leap_model(dev)
    ta, ot = _axes(3, "standard", 2001)
    if short:
        ta, ot = TimeAxis.daily("2001-01-01", 181), OTime.standard("2001-01-01", 181)
    lay = xsdba._GroupMajor(qdm.group.index(ta, qdm.group_labels), 366)
    assert lay.counts[-1] == 0 and lay.offs[-1] == lay.offs[-2] == len(ta)
    _, _, sim = edge_fields(5001, len(ta), CELLS)
    for extrap in ("constant", "nan") if interp == "nearest" else ("constant",):   # (linear + "nan": refused with a sub-grouping)
        with traced(dev, monkeypatch) as tr:
            got = qdm.adjust(sim, interp=interp, extrapolation=extrap, time=ta)
        assert tr.count("xh_qdm_adjust_groups") == 1 and tr.count("xh_qdm_adjust") == 0
        exp = osdba.qdm_adjust_grouped(sim, ot, "dayofyear", qdm.group_labels, af, qdm.quantiles, "+", interp, extrap, mode="group")
        close(f"empty-trailing-{'181d' if short else '3y'}-{interp}", extrap, got, exp, 1e-6, 1e-6 if interp == "linear" else 0.0)


def check_empty_middle_group(dev, interp):
    """xh_qdm_adjust_groups itself with a hand-made table: an empty group in the middle, an empty one at the end, rows that are in
    no group (they keep what `out` held)."""
    from xclim_amd import kernels as K

    T, G, nq = 90, 6, 7
    _, _, x = edge_fields(5002, T, CELLS)
    C = x.shape[1]
    rng = np.random.default_rng(5003)
    af = rng.normal(1.0, 0.3, (G, nq, C)).astype(np.float32)
    af[:, 2, 4] = np.nan
    gid = np.arange(T) % 5                                # groups 0 .. 4; group 2 is emptied below, group 5 has no rows
    gid[gid == 2] = -1
    gid[-4:] = -1
    rows = np.concatenate([np.nonzero(gid == g)[0] for g in range(G)])
    offs = np.concatenate([[0], np.cumsum([(gid == g).sum() for g in range(G)])]).astype(np.int64)
    assert offs[3] == offs[2] and offs[6] == offs[5] == len(rows)
    q = _q(nq)
    for kind, extrap in (("+", "constant"), ("*", "nan")):
        keep = np.float32(-3.0)
        out = dev.to_device(np.full((T, C), keep, np.float32))
        got = K.qdm_adjust_groups(dev, dev.to_device(x), rows, offs, dev.to_device(af), q, kind, interp, extrap, out=out)
        assert got is not None
        got = got.get()
        exp = np.full((T, C), keep, np.float32)
        for g in range(G):
            r = np.nonzero(gid == g)[0]
            if len(r):
                exp[r] = osdba.qdm_adjust(x[r], af[g], q, kind, interp, extrap)
        close(f"empty-middle-{interp}", f"{kind} {extrap}", got, exp, 1e-6, 1e-6 if interp == "linear" else 0.0)
        assert (got[gid < 0] == keep).all()


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("short", [False, True], ids=["2001-2003", "181-days"])
def test_qdm_adjust_with_trailing_empty_groups(dev, monkeypatch, interp, short):
    check_empty_trailing_groups(dev, interp, short, monkeypatch)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_qdm_adjust_groups_with_an_empty_group_in_the_middle(dev, interp):
    check_empty_middle_group(dev, interp)


def test_untrained_group_is_refused(dev):
    """The opposite mismatch: a sim WITH day 366 on a model trained without one."""
    from xclim_amd import sdba as xsdba

    ta, _ = _axes(3, "standard", 2001)                  # 2001-2003: no leap day, 365 labels
    ref, hist, _ = edge_fields(5004, len(ta), FEW_CELLS)
    ta4, _ = _axes(4, "standard", 2001)                 # 2001-2004
    _, _, sim = edge_fields(5005, len(ta4), FEW_CELLS)
    for cls in (xsdba.QuantileDeltaMapping, xsdba.EmpiricalQuantileMapping, xsdba.DetrendedQuantileMapping):
        model = cls.train(ref, hist, nquantiles=8, kind="+", group="time.dayofyear", time=ta, device=dev)
        with pytest.raises(ValueError, match="not trained"):
            model.adjust(sim, time=ta4)


# ---------------------------------------------------------------- tiny spans in the value-bin kernels
def tiny_columns(seed, T):
    """(T, 15) float32, columns on both sides of zero whose span is so small that (bins - 1) / span overflows float32 (the
    value bins must stay off), or just large enough not to: +-1e-37, +-3e-38, denormals, +-1e-35, [-1e-37, 0] with ONE positive
    sample; each plain, with 3 % NaN and heavily tied."""
    rng = np.random.default_rng(seed)
    cols = []
    for scale, lo in ((1e-37, -1.0), (3e-38, -1.0), (1e-40, -1.0), (1e-35, -1.0), (1e-37, None)):
        for variant in ("plain", "nan", "ties"):
            u = rng.uniform(-1.0, 1.0, T) if lo is not None else rng.uniform(-1.0, 0.0, T)
            if variant == "ties":
                u = np.round(u * 8) / 8
            if lo is None:
                u[rng.integers(0, T)] = 1.0
            c = (u * scale).astype(np.float32)
            if variant == "nan":
                c[rng.random(T) < 0.03] = np.nan
            cols.append(c)
    return np.stack(cols, axis=1)


def _qsets():
    return (np.array([0.37]), _q(20), np.linspace(0.0, 1.0, 33))


def check_tiny_quantiles(dev, T, time_axis):
    """K.quantile_series bit for bit: time_axis 1 — k_select_grp (T <= 512: the 384 | 385 instances), k_select_quantile beyond;
    time_axis 0 at a length the one-year register sort declines — the staged k_select_grp."""
    from xclim_amd import kernels as K

    x = tiny_columns(6000 + T, T)
    xd = dev.to_device(x if time_axis == 0 else np.ascontiguousarray(x.T))
    for q in _qsets():
        got = K.quantile_series(dev, xd, q, time_axis=time_axis).get()
        exp = osdba.quantile(x, q).astype(np.float32)
        assert np.isfinite(exp).all() and (exp != 0).any()
        np.testing.assert_array_equal(got, exp, err_msg=f"T={T} time_axis={time_axis} nq={len(q)}")


def check_tiny_qdm(dev, T):
    """K.qdm_adjust on time-minor columns (k_qdm_columns: its value bins clamp, or stay off, and the ranks stay exact)."""
    from xclim_amd import kernels as K

    x = tiny_columns(6100 + T, T)
    C, nq = x.shape[1], 20
    rng = np.random.default_rng(6101)
    q = _q(nq)
    xd = dev.to_device(np.ascontiguousarray(x.T))
    # "+": factors of order one, so that the sum IS the factor the sample's rank picked (a sum of two numbers near 1e-37 would
    # hide a wrong rank below any absolute tolerance); "*": the product keeps the sample's scale, relative tolerance alone
    for kind, af in (("+", rng.normal(0, 1, (nq, C)).astype(np.float32)), ("*", (1 + 0.1 * rng.normal(0, 1, (nq, C))).astype(np.float32))):
        for interp in ("nearest", "linear"):
            got = K.qdm_adjust(dev, xd, dev.to_device(af), q, kind, interp, "constant", time_axis=1).get().T
            exp = osdba.qdm_adjust(x, af, q, kind, interp, "constant")
            close(f"tiny-qdm-{T}", f"{kind} {interp}", got, exp, 1e-6, 1e-6 if (interp == "linear" and kind == "+") else 0.0)


def check_tiny_eqm(dev, T, monkeypatch=None):
    """EmpiricalQuantileMapping.train + adjust on the same columns (time-major API: the transposed pipeline at T = 800)."""
    from xclim_amd import sdba as xsdba

    ref, hist, sim = tiny_columns(6200 + T, T), tiny_columns(6201 + T, T), tiny_columns(6202 + T, T)
    eqm = xsdba.EmpiricalQuantileMapping.train(ref, hist, nquantiles=20, kind="+", device=dev)
    eaf, ehq = osdba.eqm_train(ref, hist, 20, "+")
    # An absolute tolerance of 1e-5 would pass anything at 1e-37.  Here: four float32 ulps of the column's largest magnitude
    # (a difference of two nodes, or a sample plus an interpolated factor, cancels: its error is absolute, a few roundings)
    ulps = 4 * np.maximum(2.0 ** -23 * np.maximum(np.nanmax(np.abs(ref), axis=0), np.nanmax(np.abs(hist), axis=0)), 2.0 ** -149)
    close(f"tiny-eqm-{T}", "hist_q", eqm.hist_q, ehq, 1e-6)
    close(f"tiny-eqm-{T}", "af", eqm.af, eaf, 1e-6, ulps)
    for interp in ("nearest", "linear"):
        got = eqm.adjust(sim, interp=interp)
        close(f"tiny-eqm-{T}", interp, got, osdba.eqm_adjust(sim, eqm.af, eqm.hist_q, "+", interp, "constant"), 1e-6,
              0.0 if interp == "nearest" else ulps)


SELECT_GRP_SPLITS = (384,)      # launch_select_grp_g: keys per lane for 384 | 512 steps


@pytest.mark.parametrize("T", sorted({300, 450, 800, 20000} | set(SELECT_GRP_SPLITS) | {s + 1 for s in SELECT_GRP_SPLITS}))
def test_tiny_span_quantiles_columns(dev, T):
    check_tiny_quantiles(dev, T, 1)


@pytest.mark.parametrize("T", [300, 450])
def test_tiny_span_quantiles_time_major_staged(dev, T):
    check_tiny_quantiles(dev, T, 0)


@pytest.mark.parametrize("T", [300, 3000])
def test_tiny_span_qdm_columns(dev, T):
    check_tiny_qdm(dev, T)


def test_tiny_span_eqm_train_and_adjust(dev):
    check_tiny_eqm(dev, 800)
