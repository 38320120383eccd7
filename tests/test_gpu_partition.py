"""The uncertainty-partitioning unit on the device against the recorded exact fits (tests/golden/partition_vectors.npz) and the
numpy restatement (tests/partitioncpu.py), through the C ABI (xclim_amd.kernels) and through the mirrors (xclim_amd.partitioning).

EXACT: NaN patterns, n_valid, the status byte and the ill-posed flag; a partition on 1 or 65 cells against the same cells of the
run on 130 (no result depends on another cell); general_partition with lafferty_sriver's descriptor table against
lafferty_sriver, component for component.  BOUNDS, all derived in tests/partitioncpu.py from the restatement alone: sm within
1e-12 of the sum of the absolute terms of its value, roll, g and every component within what follows from that.  Every test prints
the measured distance as a share of its bound; the largest shares measured on an MI355X are in profiles/r26/README.md."""
import numpy as np
import pytest

import partitioncpu as P
from poisoned import POISON, poisoned_outputs, unwritten  # noqa: F401
from xclim_amd import _capi, partitioning
from xclim_amd import kernels as K
from xclim_amd.fields import NotServed
from xclim_amd.timeaxis import TimeAxis

pytestmark = pytest.mark.gpu

_CACHE = {}


def annual(years):
    years = np.asarray(years)
    return TimeAxis(years, np.full(len(years), 12), np.full(len(years), 31), "standard")


def expected(name):
    """The restatement of a family on all 130 cells: computed once, shared, never changed."""
    if name not in _CACHE:
        res = P.restate(P.family(name))
        for a in res:
            a.setflags(write=False)
        _CACHE[name] = res
    return _CACHE[name]


def share(got, want, bound, what):
    """The largest |got - want| / bound, after the NaN patterns were found equal."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: the NaN pattern differs"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err, b = np.abs(got[ok] - want[ok]), bound[ok]
    assert not np.isnan(b).any(), f"{what}: a value without a bound"
    worst = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))
    print(f"measured {what}: {worst:.3e} of the bound")
    assert worst <= 1.0, (what, worst)
    return worst


def mirror(fam, da, dev, sm=None, **extra):
    time = annual(fam["years"])
    kw = dict(fam["kw"])
    if "baseline" in kw:
        kw["baseline"] = tuple(str(b) for b in kw["baseline"])
    if fam["func"] == "hs":
        return partitioning.hawkins_sutton(da, sm, time=time, device=dev, **kw, **extra)
    if fam["func"] == "ls":
        return partitioning.lafferty_sriver(da, sm, time=time, device=dev, **kw, **extra)
    return partitioning.general_partition(da, "poly" if sm is None else sm, time=time, dims=fam["dims"], device=dev, **kw, **extra)


@pytest.mark.parametrize("name", P.VALUE_FAMILIES)
def test_families_through_the_mirror(dev, name):
    fam = P.family(name)
    g_want, u_want, bg, bu = expected(name)
    sm = P.given_sm(fam) if fam["deg_given"] is not None else None
    sm_before = None if sm is None else sm.copy()
    g, u = mirror(fam, fam["da"], dev, sm)
    assert g.dtype == u.dtype == np.float64 and g.shape == g_want.shape and u.shape == u_want.shape
    share(g, g_want, bg, f"{name} g")
    for k in range(u.shape[0]):
        share(u[k], u_want[k], bu[k], f"{name} u[{k}]")
    if sm is not None:
        assert np.array_equal(sm, sm_before, equal_nan=True), "a given sm was modified"
    for C in (1, 65):   # one lane, and a ragged second wave: the same bits as those cells of the run on 130
        cut = None if sm is None else np.ascontiguousarray(sm[..., :C])
        g1, u1 = mirror(fam, np.ascontiguousarray(fam["da"][..., :C]), dev, cut)
        assert np.array_equal(g1, g[..., :C], equal_nan=True) and np.array_equal(u1, u[..., :C], equal_nan=True), C


@pytest.mark.parametrize("name", P.FAMILIES)
def test_smooth_through_the_c_abi(dev, name):
    v, fam = P.vectors(), P.family(name)
    da, years = fam["da"], fam["years"]
    T, C = da.shape[0], da.shape[-1]
    y = dev.to_device(np.ascontiguousarray(da.reshape(T, -1, C)))
    hs = fam["func"] == "hs"
    window, stat = (10, "mean") if hs else (11, "var")
    deg = fam["deg_given"] if fam["deg_given"] is not None else 4
    degs = range(5) if name == P.DEG_FAMILY else [deg]
    for d in degs:
        given = fam["deg_given"] is not None
        if given:
            s_in = dev.to_device(np.ascontiguousarray(P.given_sm(fam).reshape(T, -1, C)))
            res = K.partition_smooth(dev, y, sm_in=s_in, window=window, stat=stat)
        else:
            res = K.partition_smooth(dev, y, partitioning.poly_basis(annual(years), d), window=window, stat=stat)
        sm, roll = res["sm"].get(), res["roll"].get()
        assert not unwritten(sm).any() and not unwritten(roll).any()
        flat = da.reshape(T, -1, C)
        n_want, st_want = P.status_of(P.given_sm(fam).reshape(T, -1, C) if given else flat, d)
        if given:
            st_want = np.zeros_like(st_want)
        assert np.array_equal(res["n_valid"].get(), n_want) and np.array_equal(res["status"].get(), st_want)
        assert res["flag"].get()[0] == int((st_want == P.ILLPOSED).any())
        fitted = np.broadcast_to(st_want == P.FITTED, sm.shape)
        assert np.isnan(sm[~fitted]).all() and np.isnan(roll[~fitted]).all()
        want, tol = P.smooth(flat, P.stamps_ns(years), P.given_sm(fam).reshape(T, -1, C) if given else None, d)
        if not given:   # against the exact fits of the recorded cells, then against the restatement everywhere
            cells = list(P.EXACT_CELLS)
            ex = v[f"{name}/deg{d}/exact"]
            f3 = fitted[..., cells]
            share(np.where(f3, sm[..., cells], np.nan), np.where(f3, ex, np.nan), tol[..., cells], f"{name} deg {d} sm against the exact fit")
            ok = f3 & ~np.isnan(ex)
            rel = np.abs(sm[..., cells][ok] - ex[ok]).max() / np.abs(ex[ok]).max()
            print(f"measured {name} deg {d}: sm within {rel:.3e} of the largest exact value")
        share(np.where(fitted, sm, np.nan), np.where(fitted, want, np.nan), tol + (0.0 if given else P.restatement_slack(flat)),
              f"{name} deg {d} sm against the restatement")
        if d == deg:
            res_want = P.rolling(flat.astype(np.float64) - want, window, stat)
            wtol = P._winmax(tol, window)
            rb = wtol + P.RTOL * np.abs(res_want) if hs else P._vbound(res_want, wtol)
            share(np.where(fitted, roll, np.nan), np.where(fitted, res_want, np.nan), rb, f"{name} roll")


def test_the_baseline(dev):
    fam = P.family("hs_nan")
    da = fam["da"]
    T, C = da.shape[0], da.shape[-1]
    y = dev.to_device(np.ascontiguousarray(da.reshape(T, -1, C)))
    q = partitioning.poly_basis(annual(fam["years"]))
    plain = K.partition_smooth(dev, y, q, window=10, stat="mean")
    sm = plain["sm"].get()
    for kind in "+*":
        res = K.partition_smooth(dev, y, q, window=10, stat="mean", baseline=(1, 31), kind=kind)
        assert np.array_equal(res["roll"].get(), plain["roll"].get(), equal_nan=True)   # roll uses the unshifted fit
        with np.errstate(all="ignore"):
            rows = sm[1:31]
            ref = np.nansum(rows, axis=0) / (~np.isnan(rows)).sum(axis=0)
            want = sm - ref if kind == "+" else sm / ref
        got = res["sm"].get()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        with np.errstate(all="ignore"):   # the mean of up to 30 rows, added in row order here and there
            bound = 64 * 2.0 ** -53 * (np.abs(sm) + np.abs(ref) if kind == "+" else np.abs(want))
        assert (np.abs(got[ok] - want[ok]) <= bound[ok]).all(), kind
    empty = K.partition_smooth(dev, y, q, window=10, stat="mean", baseline=(5, 5)).get("sm").get()
    assert np.isnan(empty).all()   # a baseline without a row: ref is NaN


def test_components_through_the_c_abi(dev):
    """The descriptor table on a smoothed cube made by the restatement: every rule and weight, both variability rules."""
    fam = P.family("gp_nan")
    da = fam["da"][..., :70]
    T, C = da.shape[0], 70
    sm, e = P.smooth(da, P.stamps_ns(fam["years"]))
    roll = P.rolling(da - sm, 11, "var")
    d_sm, d_roll = dev.to_device(np.ascontiguousarray(sm.reshape(T, -1, C))), dev.to_device(np.ascontiguousarray(roll.reshape(T, -1, C)))
    w = np.array([1.0, 0.0])
    comps = [(0, "mean_then_var", "none"), (1, "var_then_mean", "count"), (2, "var_then_mean", "none"), (3, "var_then_mean", "user"),
             (1, "mean_then_var", "user"), (3, "mean_then_var", "none"), (0, "var_then_mean", "count"), (2, "mean_then_var", "user")]
    out, g = K.partition_components(dev, d_sm, d_roll, [2, 2, 2, 2], comps, weights=w, w_axis=3, g_order=(3, 1, 0, 2))
    out, g = out.get(), g.get()
    assert not unwritten(out).any() and not unwritten(g).any()
    zero = np.zeros((T, C))   # the cube is taken as exact here: the bound is the rounding of the reductions, RTOL of each value
    want = [P._moments(roll, (1, 2, 3, 4))[0]]
    for ax, rule, weight in comps:
        want.append(P.var_then_mean(sm, ax, 4, weight, w) if rule == "var_then_mean" else P.mean_then_var(sm, ax, 4, weight, w, 3))
    for k, u in enumerate(want):
        share(out[k], u, P._vbound(u, zero) + 1e-300, f"component {k}")
    assert np.array_equal(out[-1], _running_total(out[:-1]), equal_nan=True)
    share(g, P.nested_mean(sm, (3, 1, 0, 2), w, 3), P.RTOL * np.abs(g) + 1e-300, "g")
    # the HS rule on the same cube: the pooled variance of roll over (the other axes, rows >= 30) per entry of axis 3, weighted
    out_hs, _ = K.partition_components(dev, d_sm, d_roll, [2, 2, 2, 2], [], weights=[2.0, 1.0], w_axis=3, variab="hs", t0=30, with_g=False)
    pooled = np.moveaxis(roll[30:], 4, 0).reshape(2, -1, C)
    nv = P._moments(P._moments(pooled, 1)[1], 0, np.array([2.0, 1.0])[:, None])[0]
    got = out_hs.get()
    assert got.shape == (2, T, C) and np.array_equal(got[0], got[1], equal_nan=True)
    share(got[0], np.broadcast_to(nv, (T, C)), np.broadcast_to(P.RTOL * nv, (T, C)) + 1e-300, "the HS variability")


def _running_total(planes):
    total = planes[0].copy()
    for p in planes[1:]:
        total = total + p
    return total


def test_general_partition_with_lafferty_sriver_s_table_is_lafferty_sriver(dev):
    fam = P.family("ls_nan")
    time = annual(fam["years"])
    g1, u1 = partitioning.lafferty_sriver(fam["da"], time=time, device=dev)
    g2, u2 = partitioning.general_partition(fam["da"], var_first=["model", "downscaling"], mean_first=["scenario"], weights=["model", "downscaling"],
                                            time=time, dims=("scenario", "model", "downscaling"), device=dev)
    names = partitioning.general_components(["model", "downscaling"], ["scenario"])
    for k, name in enumerate(partitioning.LS_COMPONENTS):
        assert np.array_equal(u1[k], u2[names.index(name)], equal_nan=True), name
    # g takes its nested means model first there and scenario first here: with members missing those are two numbers; without,
    # one up to rounding
    clean = P.family("ls_main")
    ga, _ = partitioning.lafferty_sriver(clean["da"], time=time, device=dev)
    gb, _ = partitioning.general_partition(clean["da"], var_first=["model", "downscaling"], mean_first=["scenario"], weights=["model", "downscaling"],
                                           time=time, dims=("scenario", "model", "downscaling"), device=dev)
    np.testing.assert_allclose(ga, gb, rtol=0, atol=1e-14 * np.abs(ga).max())
    # the member axes in another order give the same partition up to the order of the sums
    da = np.ascontiguousarray(np.moveaxis(fam["da"], 2, 1))
    g3, u3 = partitioning.lafferty_sriver(da, time=time, dims=("model", "scenario", "downscaling"), device=dev)
    ok = ~np.isnan(u1)
    assert np.array_equal(np.isnan(u3), ~ok) and np.abs(u3[ok] - u1[ok]).max() <= 1e-12 * np.abs(u1[ok]).max()


def test_ill_posed_and_missing_members(dev):
    fam = P.family("ls_illposed")
    with pytest.raises(NotServed, match="fewer valid years than coefficients"):
        partitioning.lafferty_sriver(fam["da"], time=annual(fam["years"]), device=dev)
    da = fam["da"][..., :4]
    T = da.shape[0]
    res = K.partition_smooth(dev, dev.to_device(np.ascontiguousarray(da.reshape(T, -1, 4))), partitioning.poly_basis(annual(fam["years"])))
    status = res["status"].get().reshape(2, 3, 2, 4)
    assert status[1, 2, 0, 3] == P.ILLPOSED and (np.delete(status.ravel(), np.ravel_multi_index((1, 2, 0, 3), status.shape)) == P.FITTED).all()
    assert res["flag"].get()[0] == 1 and res["n_valid"].get().reshape(2, 3, 2, 4)[1, 2, 0, 3] == 4
    # the same series with degree 3 is fitted: four years, four coefficients
    res = K.partition_smooth(dev, dev.to_device(np.ascontiguousarray(da.reshape(T, -1, 4))), partitioning.poly_basis(annual(fam["years"]), 3))
    assert res["flag"].get()[0] == 0 and (res["status"].get() == P.FITTED).all()
    miss = P.family("hs_missing")
    with pytest.raises(ValueError, match="Some models are missing data for some scenarios"):
        partitioning.hawkins_sutton(miss["da"], time=annual(miss["years"]), device=dev)
    with pytest.raises(ValueError, match="Some models are missing data for some scenarios"):
        partitioning.hawkins_sutton(miss["da"], np.zeros_like(miss["da"]), time=annual(miss["years"]), device=dev)
    with pytest.raises(ValueError, match=r"^\^$"):
        partitioning.hawkins_sutton(P.family("hs_main")["da"], kind="^", time=annual(P.Y60), device=dev)
    ls = P.family("ls_nan")   # a member all NaN is no error for lafferty_sriver: status ALLNAN, count weights 0 and 1
    st = K.partition_smooth(dev, dev.to_device(np.ascontiguousarray(ls["da"].reshape(60, -1, P.CELLS))),
                            partitioning.poly_basis(annual(ls["years"])), outputs=("sm", "status", "flag"))
    st, fl = st["status"].get().reshape(2, 3, 2, P.CELLS), st["flag"].get()[0]
    assert fl == 0 and st[0, 1, 0, 5] == P.ALLNAN and (st[..., 9] == P.ALLNAN).all() and (st[..., 1] == P.FITTED).all()


C, LD, SN, LD_OUT = 70, 0, 83, 77


def _poison(dev, shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = POISON
    return dev.to_device(a)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["hs_nan", "ls_sm2"])
def test_smooth_on_pitched_strided_views(dev, name, dtype):
    """Series of stride SN > C inside rows of pitch N * SN + 9, the padding full of a value that would change every result; the
    outputs in poisoned buffers with pitches of their own.  Every element (., c < C) equals the dense call's, nothing else is
    touched."""
    fam = P.family(name)
    da = fam["da"][..., :C].astype(dtype)
    T = da.shape[0]
    flat = np.ascontiguousarray(da.reshape(T, -1, C))
    N = flat.shape[1]
    ld = N * SN + 9
    wide = np.full((T, ld), 1e30, dtype)
    given = fam["deg_given"] is not None
    s_flat = np.ascontiguousarray(P.given_sm(fam)[..., :C].astype(dtype).reshape(T, -1, C)) if given else None
    wide_s = wide.copy()
    for n in range(N):
        wide[:, n * SN:n * SN + C] = flat[:, n]
        if given:
            wide_s[:, n * SN:n * SN + C] = s_flat[:, n]
    window, stat = (10, "mean") if fam["func"] == "hs" else (11, "var")
    q = None if given else partitioning.poly_basis(annual(fam["years"]))
    kw = dict(window=window, stat=stat, baseline=(1, 31), kind="*")
    dense = K.partition_smooth(dev, dev.to_device(flat), q, sm_in=dev.to_device(s_flat) if given else None, **kw)
    sn_out, ld_out = LD_OUT, N * LD_OUT + 5
    outs = {"sm": _poison(dev, (T, ld_out), np.float64), "roll": _poison(dev, (T, ld_out), np.float64),
            "n_valid": _poison(dev, (N, LD_OUT + 2), np.int32), "status": _poison(dev, (N, LD_OUT + 2), np.uint8)}
    y3 = dev.to_device(wide)

    class View:   # (T, N, C) over the wide rows: the wrapper reads only ptr, shape and dtype
        def __init__(self, a):
            self.base, self.ptr, self.shape, self.dtype = a, a.ptr, (T, N, C), a.dtype

    d_s = dev.to_device(wide_s) if given else None
    K.partition_smooth(dev, View(y3), q, sm_in=View(d_s) if given else None, C_=C, ld=ld, stride_n=SN, outs=outs, ld_out=ld_out,
                       stride_n_out=sn_out, ld_nc=LD_OUT + 2, outputs=("sm", "roll", "n_valid", "status"), **kw)
    for k in ("sm", "roll"):
        got, want = outs[k].get(), dense[k].get()
        written = np.zeros((T, ld_out), bool)
        for n in range(N):
            assert np.array_equal(got[:, n * sn_out:n * sn_out + C], want[:, n], equal_nan=True), (k, n)
            written[:, n * sn_out:n * sn_out + C] = True
        assert unwritten(got[~written]).all(), f"{k}: written outside the series' columns"
        assert not unwritten(got[written]).any()
    for k in ("n_valid", "status"):
        got = outs[k].get()
        assert np.array_equal(got[:, :C], dense[k].get()) and unwritten(got[:, C:]).all(), k


def test_components_and_stats_on_pitched_views(dev, rng):
    T, dims = 7, [2, 3, 2]
    N = 12
    sm = rng.normal(0, 1, (T, N, C))
    sm[rng.random(sm.shape) < 0.1] = np.nan
    roll = np.abs(rng.normal(0, 1, (T, N, C)))
    roll[:2] = np.nan
    ld = N * SN + 3
    wide_s, wide_r = np.full((T, ld), 1e30), np.full((T, ld), 1e30)
    for n in range(N):
        wide_s[:, n * SN:n * SN + C], wide_r[:, n * SN:n * SN + C] = sm[:, n], roll[:, n]
    comps = [(0, "mean_then_var", "none"), (1, "var_then_mean", "count"), (2, "var_then_mean", "count")]

    class View:
        def __init__(self, a):
            self.base, self.ptr, self.shape, self.dtype = a, a.ptr, (T, N, C), a.dtype

    for kw in ({}, {"weights": [1.0, 2.0, 0.5], "w_axis": 1, "variab": "hs", "t0": 3}):
        dense, g = K.partition_components(dev, dev.to_device(sm), dev.to_device(roll), dims, comps, **kw)
        out, g_out = _poison(dev, (5 * T, LD_OUT), np.float64), _poison(dev, (T, LD_OUT), np.float64)
        K.partition_components(dev, View(dev.to_device(wide_s)), View(dev.to_device(wide_r)), dims, comps, C_=C, ld=ld, stride_n=SN, out=out,
                               g=g_out, ld_out=LD_OUT, **kw)
        got = out.get()
        assert np.array_equal(got[:, :C], dense.get().reshape(5 * T, C), equal_nan=True) and unwritten(got[:, C:]).all()
        assert not unwritten(got[:, :C]).any()
        got = g_out.get()
        assert np.array_equal(got[:, :C], g.get(), equal_nan=True) and unwritten(got[:, C:]).all()
    x = rng.normal(280, 5, (6, C)).astype(np.float32)
    x[rng.random(x.shape) < 0.2] = np.nan
    wide = np.full((6, SN), 1e30, np.float32)
    wide[:, :C] = x
    dense = K.ensemble_stats(dev, dev.to_device(x), [1, 2, 3, 0, 1, 1], 2)
    out = _poison(dev, (4, LD_OUT), np.float64)
    K.ensemble_stats(dev, dev.to_device(wide), [1, 2, 3, 0, 1, 1], 2, E_=C, ld=SN, out=out, ld_out=LD_OUT)
    got = out.get()
    assert np.array_equal(got[:, :C], dense.get(), equal_nan=True) and unwritten(got[:, C:]).all() and not unwritten(got[:, :C]).any()


def test_null_outputs(dev):
    fam = P.family("ls_nan")
    flat = np.ascontiguousarray(fam["da"][..., :65].reshape(60, -1, 65))
    y, q = dev.to_device(flat), partitioning.poly_basis(annual(fam["years"]))
    full = K.partition_smooth(dev, y, q)
    for outputs in (("sm",), ("roll",), ("sm", "status"), ("roll", "n_valid", "flag")):
        part = K.partition_smooth(dev, y, q, outputs=outputs)
        assert sorted(part) == sorted(outputs)
        for k in outputs:
            assert np.array_equal(part[k].get(), full[k].get(), equal_nan=True), (outputs, k)
    # sm given without y: sm is handed through (with the baseline), n_valid counts it
    s = dev.to_device(full["sm"].get())
    res = K.partition_smooth(dev, None, sm_in=s, outputs=("sm", "n_valid", "status"))
    assert np.array_equal(res["sm"].get(), full["sm"].get(), equal_nan=True) and np.array_equal(res["n_valid"].get(), full["n_valid"].get())
    out, g = K.partition_components(dev, full["sm"], full["roll"], [2, 3, 2], [], with_g=False)
    assert g is None and out.shape == (2, 60, 65) and np.array_equal(out.get()[0], out.get()[1], equal_nan=True)


def test_limits_and_argument_errors_answer_before_any_launch(dev):
    y = dev.to_device(np.zeros((20, 2, 3)))
    q = np.linalg.qr(np.vander(np.linspace(-1, 1, 20), 5))[0]
    err = _capi.XclimHipError
    with pytest.raises(err, match="at most 512 years, got 513"):
        K.partition_smooth(dev, dev.to_device(np.zeros((513, 1, 2))), np.zeros((513, 5)))
    for window, stat in ((11, "mean"), (10, "var"), (9, "mean"), (12, "var")):
        with pytest.raises(err, match="the rolling mean over 10 rows and the rolling variance over 11 rows are served"):
            K.partition_smooth(dev, y, q, window=window, stat=stat)
    with pytest.raises(err, match="a basis of degree 0 .. 4"):
        K.partition_smooth(dev, y, np.zeros((20, 6)))
    with pytest.raises(err, match="sm and roll are both NULL"):
        K.partition_smooth(dev, y, q, outputs=("n_valid",))
    with pytest.raises(err, match="y is needed"):
        K.partition_smooth(dev, None, sm_in=y, outputs=("sm", "roll"))
    with pytest.raises(err, match="baseline rows"):
        K.partition_smooth(dev, y, q, baseline=(3, 21))
    with pytest.raises(err, match="stride_n >= C"):
        K.partition_smooth(dev, y, q, stride_n=2)
    with pytest.raises(err, match="stride_n >= C"):
        K.partition_smooth(dev, y, q, ld=5)
    sm, roll = dev.to_device(np.zeros((5, 6, 3))), dev.to_device(np.zeros((5, 6, 3)))
    with pytest.raises(err, match="at most 64 entries per axis"):
        K.partition_components(dev, dev.to_device(np.zeros((2, 65, 1))), dev.to_device(np.zeros((2, 65, 1))), [65], [])
    with pytest.raises(err, match="at most 4096 members"):
        K.partition_components(dev, dev.to_device(np.zeros((1, 8192, 1))), dev.to_device(np.zeros((1, 8192, 1))), [64, 64, 2], [])
    with pytest.raises(err, match="count weights go with VAR_THEN_MEAN"):
        K.partition_components(dev, sm, roll, [2, 3], [(0, "mean_then_var", "count")])
    with pytest.raises(err, match="user weights need"):
        K.partition_components(dev, sm, roll, [2, 3], [(0, "var_then_mean", "user")])
    with pytest.raises(err, match="user weights need"):
        K.partition_components(dev, sm, roll, [2, 3], [(0, "var_then_mean", "user")], weights=[1, 1, 1], w_axis=1)
    with pytest.raises(err, match="user weights need"):
        K.partition_components(dev, sm, roll, [2, 3], [(1, "mean_then_var", "user")], weights=[1, 1, 1], w_axis=1)
    with pytest.raises(err, match="HS with weights"):
        K.partition_components(dev, sm, roll, [2, 3], [], variab="hs")
    with pytest.raises(err, match="t0 6 outside"):
        K.partition_components(dev, sm, roll, [2, 3], [], weights=[1, 1, 1], w_axis=1, variab="hs", t0=6)
    with pytest.raises(err, match="0 .. 8 components"):
        K.partition_components(dev, sm, roll, [2, 3], [(0, "var_then_mean", "none")] * 9)
    with pytest.raises(err, match="1 .. 65535 realizations"):
        K.ensemble_stats(dev, dev.to_device(np.zeros((0, 3))))


def test_keep_hands_the_smoothed_cube_back_as_sm(dev):
    fam = P.family("ls_nan")
    time = annual(fam["years"])
    g, u, sm = partitioning.lafferty_sriver(fam["da"], time=time, device=dev, keep=True)
    assert isinstance(sm, _capi.DeviceArray) and tuple(sm.shape) == (60, 12, P.CELLS) and np.dtype(sm.dtype) == np.float64
    before = sm.get()
    g2, u2 = partitioning.lafferty_sriver(fam["da"], sm, time=time, device=dev)
    assert np.array_equal(g, g2, equal_nan=True) and np.array_equal(u, u2, equal_nan=True)
    assert np.array_equal(sm.get(), before, equal_nan=True)
    g3, u3 = partitioning.general_partition(fam["da"], before.reshape(fam["da"].shape), ["model", "downscaling"], ["scenario"], ["model", "downscaling"],
                                            time=time, dims=("scenario", "model", "downscaling"), device=dev)
    assert np.array_equal(u3[[1, 0, 2, 3, 4]], u, equal_nan=True)
    ps = partitioning.poly_smooth(fam["da"], time, device=dev)
    assert np.array_equal(ps.reshape(60, 12, P.CELLS), before, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("E", [1, 65, 130])
def test_ensemble_statistics(dev, rng, E, dtype):
    x = rng.normal(280, 5, (7, E)).astype(dtype)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[:, 0] = np.nan
    x[1:, E // 2] = np.nan
    w = [1.0, 0.1, 3.5, 5.0, 0.0, 2.0, 1.0]
    for weights in (None, w):
        for min_members in (1, None, 2):
            got = partitioning.ensemble_mean_std_max_min(x.reshape(7, E, 1), min_members, weights, device=dev)
            want = P.ensemble_stats(x.reshape(7, E, 1), min_members, weights)
            assert sorted(got) == ["max", "mean", "min", "stdev"]
            for k in got:
                assert got[k].shape == (E, 1) and got[k].dtype == np.float64
                assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, weights, min_members)
                ok = ~np.isnan(want[k])
                if k in ("max", "min"):
                    assert np.array_equal(got[k][ok], want[k][ok])
                else:   # seven terms of magnitude up to max |x|: the customary 1e-12 of the sum of the absolute terms
                    assert (np.abs(got[k][ok] - want[k][ok]) <= 1e-12 * 300.0).all(), (k, weights, min_members)
    kept = partitioning.ensemble_mean_std_max_min(x, device=dev, keep=True)["stats"]
    assert kept.shape == (4, E)
