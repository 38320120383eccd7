"""A numpy restatement of the winter-chill indices as the device computes them (xclim_amd/csrc/chill.hip): the Dynamic Model
(_agro.py:1436-1465), the Utah weights (:1574-1592) and Linvill's hourly profile (helpers.py:977-1123).  TIME FIRST, float64
arithmetic on widened fields; the Utah comparisons in the dtype of the temperature they see.  The CPU-tier stand-in for the
kernels: tests/test_chill_cpu.py holds it against the reference's own outputs, tests/test_gpu_chill.py uses it where no
golden output exists."""
import numpy as np

E0, E1, A0, A1, SLP, TETMLT = 4153.5, 12888.8, 139500, 2.567e18, 1.6, 277
AA, EE = A0 / A1, E1 - E0


def delta_rows(tas_K, seg, sel=None):
    """delta (T, C) float64 of a (T, C) field in K: every period of ``seg`` (row offsets) restarts at E = 0, rows with
    ``sel`` False are skipped (delta 0, the state carries).  Also returns min |E - 1| over the selected rows."""
    t = np.asarray(tas_K, np.float64)
    T, C = t.shape
    sel = np.ones(T, bool) if sel is None else np.asarray(sel, bool)
    delta = np.zeros((T, C))
    margin = np.inf
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ft = SLP * TETMLT * (t - TETMLT) / t
        sr = np.exp(ft)
        xi = sr / (1 + sr)
        xs = AA * np.exp(EE / t)
        ak1 = A1 * np.exp(-E1 / t)
        eak = np.exp(-ak1)
        for a, b in zip(seg[:-1], seg[1:]):
            rows = np.arange(a, b)[sel[a:b]]
            E = np.zeros(C)
            prev = None
            for r in rows:
                if prev is not None:
                    S = np.where(E < 1, E, E - E * xi[prev])
                    E = xs[r] - (xs[r] - S) * eak[r]
                    delta[r] = np.where(E >= 1, E * xi[r], 0)
                    d = np.abs(E - 1)
                    if np.isfinite(d).any():
                        margin = min(margin, np.nanmin(d))
                prev = r
    return delta, margin


def portions(tas_K, seg, sel=None):
    """(cp (P, C), delta (T, C), valid (P, C))."""
    delta, _ = delta_rows(tas_K, seg, sel)
    T = delta.shape[0]
    s = np.ones(T, bool) if sel is None else np.asarray(sel, bool)
    ok = ~np.isnan(np.asarray(tas_K)) & s[:, None]
    cp = np.stack([delta[a:b].sum(axis=0) for a, b in zip(seg[:-1], seg[1:])])
    valid = np.stack([ok[a:b].sum(axis=0) for a, b in zip(seg[:-1], seg[1:])]).astype(np.int32)
    return cp, delta, valid


def utah_weights(tas_C):
    """The Utah weight of every hour, NaN for a NaN temperature (_agro.py:1574-1587), compared in the field's dtype."""
    t = np.asarray(tas_C)
    f = t.dtype.type
    with np.errstate(invalid="ignore"):
        w = np.where((t <= f(1.4)) | ((t > f(12.4)) & (t <= f(15.9))), 0.0,
                     np.where(((t > f(1.4)) & (t <= f(2.4))) | ((t > f(9.1)) & (t <= f(12.4))), 0.5,
                              np.where((t > f(2.4)) & (t <= f(9.1)), 1.0, np.where((t > f(15.9)) & (t <= f(17.9)), -0.5, -1.0))))
    return np.where(np.isnan(t), np.nan, w)


def units(tas_C, seg, positive_only=False, sel=None):
    """cu (P, C): the NaN-skipping sum of the weights per period; with positive_only the sum of the positive daily sums
    (24 rows per day from row 0)."""
    w = np.nan_to_num(utah_weights(tas_C), nan=0.0)
    if sel is not None:
        w = w * np.asarray(sel, bool)[:, None]
    if positive_only:
        day = w.reshape(-1, 24, w.shape[1]).sum(axis=1)
        day = np.where(day > 0, day, 0.0)
        return np.stack([day[a // 24:b // 24].sum(axis=0) for a, b in zip(seg[:-1], seg[1:])])
    return np.stack([w[a:b].sum(axis=0) for a, b in zip(seg[:-1], seg[1:])])


def hourly_temperature(tasmin, tasmax, dl):
    """make_hourly_temperature on arrays: tasmin / tasmax (D, C) of one dtype, dl (D, C) float64 day lengths -> (24 D, C)
    float64.  tasmax - tasmin in the fields' dtype, the last day's next tasmin its own."""
    tn, tx = np.asarray(tasmin), np.asarray(tasmax)
    D, C = tn.shape
    rng = (tx - tn).astype(np.float64)
    tnd = tn.astype(np.float64)
    nxt = np.concatenate([tnd[1:], tnd[-1:]])
    dl = np.asarray(dl, np.float64)
    out = np.empty((D, 24, C))
    with np.errstate(invalid="ignore", divide="ignore"):
        sunset = rng * np.sin((np.pi * dl) / (dl + 4)) + tnd
        slope = (sunset - nxt) / np.log(24 - (dl - 1))
        for h in range(24):
            day = rng * np.sin((np.pi * h) / (dl + 4)) + tnd
            nh = h + 1 - dl
            nh = np.where(nh < 1, 1.0, nh)
            night = sunset - slope * np.log(nh)
            out[:, h] = np.where(h < dl, day, night)
    return out.reshape(24 * D, C)
