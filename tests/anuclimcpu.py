"""A numpy restatement of the ANUCLIM variables BIO1-BIO19 (reference: src/xclim/indices/_anuclim.py:66-625 with
precip_accumulation, _multivariate.py:988-990, and select_resample_op, generic.py:110-125): what tests/golden/
make_anuclim_golden.py writes its expected values with and what the device is held against where no golden value exists.

Plain arithmetic, nothing shared with the package: sums run sequentially in row (or step) order, every window is summed
from its own W values, the standard deviations are two-pass.  ``single_pass=True`` swaps in Welford's accumulation for
BIO4 / BIO15, the formula the kernel uses, so that its distance from the two-pass value can be measured on the CPU.

Time is axis 0, cells axis 1.  The period and step tables are built here from (year, month) arrays with their own few lines
of integer arithmetic (``tables``)."""
import numpy as np

NAMES = tuple(f"bio{k}" for k in range(1, 20))
WHICH = ("wettest", "driest", "warmest", "coldest")
COUNTS = ("n_tas", "n_tasmin", "n_tasmax", "n_pr")
_MONTHS = ["JAN", "FEB", "MAR", "APR", "MAY", "JUN", "JUL", "AUG", "SEP", "OCT", "NOV", "DEC"]


def tables(year, month, kind, freq):
    """(step_off, seg_rows, seg_steps, W) of a gap-free series: ``kind`` "D" (7-day bins from the first row), "W" or "M" (a
    row is a step); ``freq`` YS[-MMM], QS[-MMM] or MS.  A step belongs to the period of its first row."""
    year, month = np.asarray(year, np.int64), np.asarray(month, np.int64)
    T = len(year)
    so = np.append(np.arange(0, T, 7), T) if kind == "D" else np.arange(T + 1)
    base, _, anchor = freq.partition("-")
    n = {"YS": 12, "QS": 3, "MS": 1}[base]
    off = (_MONTHS.index(anchor) if anchor else 0) % n
    key = (year * 12 + month - 1 - off) // n
    seg_rows = np.searchsorted(key, np.arange(key[0], key[-1] + 2), side="left")
    seg_steps = np.searchsorted(so[:-1], seg_rows, side="left")
    return so.astype(np.int64), seg_rows.astype(np.int64), seg_steps.astype(np.int64), 3 if kind == "M" else 13


def _seq_sum(rows):
    """Sequential sum of the present values down axis 0, and their count."""
    s, n = np.zeros(rows.shape[1]), np.zeros(rows.shape[1], np.int64)
    for v in rows:
        ok = ~np.isnan(v)
        s = np.where(ok, s + np.where(ok, v, 0.0), s)
        n += ok
    return s, n


def _mean(s, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def _cv_two_pass(rows):
    s, n = _seq_sum(rows)
    mean = _mean(s, n)
    s2, _ = _seq_sum((rows - mean) ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, 100 * (np.sqrt(s2 / np.maximum(n, 1)) / mean), np.nan)


def _cv_welford(rows):
    C = rows.shape[1]
    n, mean, m2 = np.zeros(C), np.zeros(C), np.zeros(C)
    for x in rows:
        ok = ~np.isnan(x)
        x = np.where(ok, x, 0.0)
        n1 = n + 1
        d = x - mean
        mean1 = mean + d / n1
        m21 = m2 + d * (x - mean1)
        n, mean, m2 = np.where(ok, n1, n), np.where(ok, mean1, mean), np.where(ok, m21, m2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, 100 * (np.sqrt(m2 / np.maximum(n, 1)) / mean), np.nan)


def _extreme(rows, op):
    ok = ~np.isnan(rows)
    fill = -np.inf if op == "max" else np.inf
    v = getattr(np, op)(np.where(ok, rows, fill), axis=0) if len(rows) else np.full(rows.shape[1], fill)
    return np.where(ok.any(axis=0), v, np.nan)


def steps(fields, step_off, factor, binned):
    """(tas steps, pr steps), each (S, C) float64 or None."""
    S = len(step_off) - 1
    out = []
    for name in ("tas", "pr"):
        x = fields.get(name)
        if x is None:
            out.append(None)
            continue
        x = np.asarray(x).astype(np.float64)
        if name == "pr":
            x = x * np.asarray(factor, np.float64)[:, None]
        st = np.empty((S, x.shape[1]))
        for s in range(S):
            tot, n = _seq_sum(x[step_off[s]:step_off[s + 1]])
            st[s] = _mean(tot, n) if name == "tas" else np.where(n > 0, tot, 0.0 if binned else np.nan)
        out.append(st)
    return out


def quarters(st, W, mean):
    """The quarter series of a step series: every window summed from its W values in step order."""
    q = np.full(st.shape, np.nan)
    for k in range(W - 1, len(st)):
        acc = st[k - W + 1].copy()
        for j in range(k - W + 2, k + 1):
            acc = acc + st[j]
        q[k] = acc / W if mean else acc
    return q


def _pick(crit, other, a, b, op):
    """(extreme of crit[a:b], other at its first index, that index or -1), NaN skipped."""
    C = crit.shape[1]
    best, val, idx = np.full(C, np.nan), np.full(C, np.nan), np.full(C, -1, np.int32)
    for k in range(a, b):
        c = crit[k]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(c) & ((idx < 0) | (c > best if op == "max" else c < best))
        best, idx = np.where(take, c, best), np.where(take, k, idx).astype(np.int32)
        if other is not None:
            val = np.where(take, other[k], val)
    return best, val, idx


def gaps(crit, a, b, op):
    """Relative distance between the best and the runner-up of crit[a:b] per cell (inf with fewer than two, 0 for a tie)."""
    out = np.full(crit.shape[1], np.inf)
    for c in range(crit.shape[1]):
        v = crit[a:b, c]
        v = np.sort(v[~np.isnan(v)])
        if len(v) >= 2:
            x, y = (v[-1], v[-2]) if op == "max" else (v[0], v[1])
            out[c] = 0.0 if x == y else abs(x - y) / max(abs(x), abs(y))
    return out


def bioclim(fields, step_off, factor, seg_rows, seg_steps, W, binned=True, kelvin_offset=0.0, cv_scale=1.0, thresh=0.0,
            single_pass=False, want_gap=False):
    """{bio1 .. bio19 (P, C) float64, wettest / driest / warmest / coldest (P, C) int32 step indices, n_* (P, C) int32} of the
    fields given (tas, tasmin, tasmax, pr; all of one dtype); what needs an absent field is left out.  ``want_gap`` adds
    "min_gap": the smallest non-zero relative best-to-runner-up distance over every (cell, period, criterion)."""
    f = {k: np.asarray(v) for k, v in fields.items() if v is not None}
    P = len(seg_rows) - 1
    out = {}
    cv = _cv_welford if single_pass else _cv_two_pass
    ts, ps = steps(f, step_off, factor, binned)
    qt = quarters(ts, W, True) if ts is not None else None
    qp = quarters(ps, W, False) if ps is not None else None
    min_gap = np.inf

    def per_period(fn):
        return np.stack([fn(int(seg_rows[p]), int(seg_rows[p + 1]), int(seg_steps[p]), int(seg_steps[p + 1])) for p in range(P)])

    def count(x):
        return per_period(lambda a, b, *_: (~np.isnan(x[a:b])).sum(axis=0)).astype(np.int32)

    if "tas" in f:
        x = f["tas"].astype(np.float64)
        out["n_tas"] = count(x)
        out["bio1"] = per_period(lambda a, b, *_: _mean(*_seq_sum(x[a:b])))
        out["bio4"] = per_period(lambda a, b, *_: cv(x[a:b] + kelvin_offset))
        for name, idx, op in (("bio10", "warmest", "max"), ("bio11", "coldest", "min")):
            r = [_pick(qt, qp, s0, s1, op) for s0, s1 in zip(seg_steps[:-1], seg_steps[1:])]
            out[name], out[idx] = np.stack([v[0] for v in r]), np.stack([v[2] for v in r])
            if qp is not None:
                out["bio18" if op == "max" else "bio19"] = np.stack([v[1] for v in r])
            if want_gap:
                g = np.concatenate([gaps(qt, s0, s1, op) for s0, s1 in zip(seg_steps[:-1], seg_steps[1:])])
                min_gap = min(min_gap, g[g > 0].min(initial=np.inf))
    if "tasmin" in f:
        out["n_tasmin"] = count(f["tasmin"])
        out["bio6"] = per_period(lambda a, b, *_: _extreme(f["tasmin"][a:b], "min")).astype(np.float64)
    if "tasmax" in f:
        out["n_tasmax"] = count(f["tasmax"])
        out["bio5"] = per_period(lambda a, b, *_: _extreme(f["tasmax"][a:b], "max")).astype(np.float64)
    if "tasmin" in f and "tasmax" in f:
        d = (f["tasmax"] - f["tasmin"]).astype(np.float64)       # the difference in the fields' dtype
        out["bio2"] = per_period(lambda a, b, *_: _mean(*_seq_sum(d[a:b])))
        dt = f["tasmax"].dtype
        out["bio7"] = (out["bio5"].astype(dt) - out["bio6"].astype(dt)).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["bio3"] = out["bio2"] / out["bio7"] * 100
    if "pr" in f:
        x = f["pr"].astype(np.float64)
        amt = x * np.asarray(factor, np.float64)[:, None]
        out["n_pr"] = count(x)
        with np.errstate(invalid="ignore"):
            kept = np.where(x >= thresh, amt, 0.0)
        out["bio12"] = per_period(lambda a, b, *_: _seq_sum(kept[a:b])[0])
        out["bio13"] = per_period(lambda a, b, *_: _extreme(amt[a:b], "max"))
        out["bio14"] = per_period(lambda a, b, *_: _extreme(amt[a:b], "min"))
        out["bio15"] = per_period(lambda a, b, *_: cv(x[a:b] * cv_scale))
        for name, idx, op in (("bio16", "wettest", "max"), ("bio17", "driest", "min")):
            r = [_pick(qp, qt, s0, s1, op) for s0, s1 in zip(seg_steps[:-1], seg_steps[1:])]
            out[name], out[idx] = np.stack([v[0] for v in r]), np.stack([v[2] for v in r])
            if qt is not None:
                out["bio8" if op == "max" else "bio9"] = np.stack([v[1] for v in r])
            if want_gap:
                g = np.concatenate([gaps(qp, s0, s1, op) for s0, s1 in zip(seg_steps[:-1], seg_steps[1:])])
                min_gap = min(min_gap, g[g > 0].min(initial=np.inf))
    if want_gap:
        out["min_gap"] = float(min_gap)
    return out
