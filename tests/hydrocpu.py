"""numpy / scipy restatement of the streamflow and snow-melt indices of the reference's src/xclim/indices/_hydrology.py, the oracle
of the hydrology unit (xclim_amd/csrc/hydro.hip, xclim_amd/hydrology.py).  The reference's own code needs xarray (and
pymannkendall for the Sen slope), which are not installable here; every function names the lines it restates.

Fields are ``(T, C)`` with time on axis 0, widened to float64 first.  Windows are added in row order with shifted copies of the
NaN-padded series, so a window sum rounds exactly as a loop over its rows would.  Where a value is a sum, its ``*_scale`` is the
sum of the absolute terms (the tolerance of the tests is 1e-12 of it); for a ratio the scales of the two parts are carried
through the division.  The periods come from ``TimeAxis.segments``, the p value from ``scipy.stats.norm.cdf``, the quantiles from
``np.nanquantile``."""

import numpy as np
from scipy.stats import norm

DAY = 86400.0


def widen(a):
    return np.asarray(a, dtype=np.float64)


def _shifted(a, before, after):
    """(T + before + after, C): ``a`` with NaN rows in front and behind."""
    T, C = a.shape
    return np.concatenate([np.full((before, C), np.nan), a, np.full((after, C), np.nan)])


def m7(q):
    """rolling(time=7, center=True).mean(skipna=False) (:84): the seven values added in row order, NaN at an overhang."""
    q = widen(q)
    T = q.shape[0]
    p = _shifted(q, 3, 3)
    s, sa = p[0:T], np.abs(p[0:T])
    for k in range(1, 7):
        s, sa = s + p[k:k + T], sa + np.abs(p[k:k + T])
    return s / 7, sa / 7


def flow_period_stats(q, seg):
    """base_flow_index (:84-89) and rb_flashiness_index (:125-128) with the period statistics behind them:
    ``{bfi, rbi, mean, sum, valid}`` (P, C) and their scales."""
    q = widen(q)
    T, C = q.shape
    P = len(seg) - 1
    mm, ma = m7(q)
    d = np.full((T, C), np.nan)
    d[1:] = np.abs(q[1:] - q[:-1])                                    # :125 (row 0 has no difference)
    out = {k: np.full((P, C), np.nan) for k in ("bfi", "rbi", "mean", "sum", "bfi_scale", "rbi_scale", "mean_scale", "sum_scale")}
    out["valid"] = np.zeros((P, C), np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for p in range(P):
            a, b = int(seg[p]), int(seg[p + 1])
            x = q[a:b]
            n = (~np.isnan(x)).sum(axis=0)
            s, sa = np.nansum(x, axis=0), np.nansum(np.abs(x), axis=0)
            mean = np.where(n > 0, s / np.maximum(n, 1), np.nan)
            mean_a = sa / np.maximum(n, 1)
            has = (~np.isnan(mm[a:b])).any(axis=0) if b > a else np.zeros(C, bool)
            low = np.full(C, np.nan)
            low_a = np.zeros(C)
            if b > a and has.any():
                filled = np.where(np.isnan(mm[a:b]), np.inf, mm[a:b])
                i = filled.argmin(axis=0)
                low = np.where(has, filled[i, np.arange(C)], np.nan)
                low_a = ma[a:b][i, np.arange(C)]
            ds = np.nansum(d[a:b], axis=0)
            out["valid"][p], out["sum"][p], out["mean"][p] = n, s, mean
            out["sum_scale"][p], out["mean_scale"][p] = sa, mean_a
            out["bfi"][p] = low / mean                                  # :88
            out["bfi_scale"][p] = np.nan_to_num(low_a / np.abs(mean) + np.abs(low / mean) * mean_a / np.abs(mean), posinf=0.0)
            out["rbi"][p] = ds / s                                      # :127
            out["rbi_scale"][p] = np.nan_to_num(ds / np.abs(s) + np.abs(ds / s) * sa / np.abs(s), posinf=0.0)
    return out


def melt_period_max(snw, pr, per_day, window, seg):
    """snow_melt_we_max (:392-399; ``pr`` None) and melt_and_precip_max (:429-439): ``{out, out_scale}`` (P, C)."""
    snw = widen(snw)
    T, C = snw.shape
    P = len(seg) - 1
    total, ta = np.full((T, C), np.nan), np.full((T, C), np.nan)
    if T > 1:
        melt = (snw[1:] - snw[:-1]) * -1.0
        ma = np.abs(snw[1:]) + np.abs(snw[:-1])
        if pr is not None:
            amount = widen(pr)[1:] * per_day                           # rate2amount
            total[1:], ta[1:] = amount + melt, np.abs(amount) + ma
        else:
            total[1:], ta[1:] = melt, ma
    tp, tap = _shifted(total, window - 1, 0), _shifted(ta, window - 1, 0)
    agg, agg_a = tp[0:T], tap[0:T]
    for k in range(1, window):                                         # rolling(time=window).sum(): row order
        agg, agg_a = agg + tp[k:k + T], agg_a + tap[k:k + T]
    out, scale = np.full((P, C), np.nan), np.zeros((P, C))
    for p in range(P):
        a, b = int(seg[p]), int(seg[p + 1])
        if b <= a:
            continue
        has = (~np.isnan(agg[a:b])).any(axis=0)
        filled = np.where(np.isnan(agg[a:b]), -np.inf, agg[a:b])
        i = filled.argmax(axis=0)
        out[p] = np.where(has, filled[i, np.arange(C)], np.nan)
        scale[p] = np.where(has, agg_a[a:b][i, np.arange(C)], 0.0)
    return {"out": out, "out_scale": scale}


def api_weights(window, p_exp):
    return np.asarray(list(reversed([p_exp ** (idx - 1) for idx in range(1, window + 1)])), np.float64)     # :700-703


def antecedent_precip(pr, per_day, weights):
    """antecedent_precipitation_index (:698-705): ``{out, out_scale}`` (T, C), the products added in window order."""
    v = widen(pr) * per_day
    T = v.shape[0]
    w = np.asarray(weights, np.float64)
    p = _shifted(v, len(w) - 1, 0)
    out, sc = w[0] * p[0:T], np.abs(w[0] * p[0:T])
    for k in range(1, len(w)):
        out, sc = out + w[k] * p[k:k + T], sc + np.abs(w[k] * p[k:k + T])
    return {"out": out, "out_scale": np.nan_to_num(sc)}


def mann_kendall(v):
    """pymannkendall.original_test on one series with NaN for a missing year: ``(slope, p, n)``.  Score, variance and p on the
    series with the NaN dropped; the slope is np.nanmedian of (x_j - x_i) / (j - i) over the ORIGINAL positions."""
    v = widen(v)
    idx = np.flatnonzero(~np.isnan(v))
    n = len(idx)
    if n < 2:
        return np.nan, np.nan, n
    i, j = np.triu_indices(n, 1)
    d = v[idx[j]] - v[idx[i]]
    slopes = d / (idx[j] - idx[i])
    slope = np.median(slopes[~np.isnan(slopes)])
    s = float(np.sign(d).sum())
    _, t = np.unique(v[idx], return_counts=True)
    var = (n * (n - 1) * (2 * n + 5) - float((t * (t - 1) * (2 * t + 5)).sum())) / 18
    z = (s - 1) / np.sqrt(var) if s > 0 else (s + 1) / np.sqrt(var) if s < 0 else 0.0
    return slope, 2 * (1 - norm.cdf(abs(z))), n


def sen_slope(x, period_of):
    """``{slope, p}`` float64 and ``n`` int32, (K, C), of the rows of ``x`` (P, C) that ``period_of`` (Y, K) names."""
    x = widen(x)
    period_of = np.asarray(period_of, np.int64)
    Y, K = period_of.shape
    C = x.shape[1]
    out = {"slope": np.full((K, C), np.nan), "p": np.full((K, C), np.nan), "n": np.zeros((K, C), np.int32)}
    for k in range(K):
        series = np.full((Y, C), np.nan)
        has = period_of[:, k] >= 0
        series[has] = x[period_of[has, k]]
        for c in range(C):
            out["slope"][k, c], out["p"][k, c], out["n"][k, c] = mann_kendall(series[:, c])
    return out


def season_year_table(time, freq):
    """split_time_to_season_year (core/calendar.py:1775-1802) on the periods of ``time.segments(freq)``: ``(period_of (Y, K),
    seasons (sorted, as unstack leaves them), years)``."""
    from xclim_amd.timeaxis import MONTHS, parse_freq

    base, anchor = parse_freq(freq)
    _, starts = time.segments(freq)
    base_month = anchor if base in "YQ" else 1
    labels = []
    for y, m in starts:
        lab = "annual" if base == "Y" else MONTHS[m - 1] if base == "M" else "".join("JFMAMJJASOND"[(m - 1 + i) % 12] for i in range(3))
        labels.append((y - 1 if m < base_month else y, lab))
    seasons = sorted({lab for _, lab in labels})
    years = np.arange(min(y for y, _ in labels), max(y for y, _ in labels) + 1)
    table = np.full((len(years), len(seasons)), -1, np.int64)
    for p, (y, lab) in enumerate(labels):
        table[y - years[0], seasons.index(lab)] = p
    return table, seasons, years


def period_mean(q, seg):
    q = widen(q)
    with np.errstate(invalid="ignore"):
        return np.array([np.nansum(q[a:b], axis=0) / (~np.isnan(q[a:b])).sum(axis=0) for a, b in zip(seg[:-1], seg[1:])])


def flow_index(q, p=0.95):
    q = widen(q)
    return np.nanquantile(q, p, axis=0) / np.nanquantile(q, 0.5, axis=0)            # :599-601


def flow_frequency(q, op, threshold, seg):
    q = widen(q)
    hit = q > threshold[None] if op == ">" else q < threshold[None]
    return np.array([hit[a:b].sum(axis=0) for a, b in zip(seg[:-1], seg[1:])], np.int32)


def high_flow_frequency(q, factor, seg):
    return flow_frequency(q, ">", factor * np.nanquantile(widen(q), 0.5, axis=0), seg)   # :633-635


def low_flow_frequency(q, factor, seg):
    q = widen(q)
    return flow_frequency(q, "<", factor * (np.nansum(q, axis=0) / (~np.isnan(q)).sum(axis=0)), seg)   # :666-668


def aridity_index(pr, pet, seg):
    return period_mean(pr, seg) / period_mean(pet, seg)                              # :809-811


def seasonal_bfi_ratio(q, time, freq="QS-DEC", numerator="DJF", denominator="JJA"):
    """base_flow_index_seasonal_ratio (:1034-1036): ``(bfi (K, Y, C), ratio (Y, C), seasons)``."""
    bfi = flow_period_stats(q, time.segments(freq)[0])["bfi"]
    table, seasons, _ = season_year_table(time, freq)
    split = np.full((len(seasons), table.shape[0], bfi.shape[1]), np.nan)
    for k in range(len(seasons)):
        has = table[:, k] >= 0
        split[k, has] = bfi[table[has, k]]
    den = split[seasons.index(denominator)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return split, split[seasons.index(numerator)] / np.where(den > 0, den, np.nan), seasons


# ---- seeded fields for the tests -----------------------------------------------------------------------------------------
def synth(time, C, dtype, seed=0):
    """``{q, snw, pr}`` (T, C) of ``dtype`` on the axis ``time`` with the NaN patterns the tests ask for, by cell index modulo 5:
    0 clean; 1 NaN on row 0, on the last row of every second period of "YS" / "MS" (the first included) and a few more; 2 the
    whole second year NaN (and the whole second month); 3 a whole NaN cell; 4 about 1 % NaN."""
    T = len(time)
    rng = np.random.default_rng(9000 + 31 * C + T + seed)
    doy = time.doy[:, None].astype(np.float64)
    q = 40 + 30 * np.sin(2 * np.pi * (doy - 120) / 365) ** 2 + rng.gamma(2.0, 6.0, (T, C))
    snw = np.maximum(60 * np.cos(2 * np.pi * (doy - 30) / 365) + np.cumsum(rng.normal(0, 2.0, (T, C)), axis=0) % 17, 0)
    pr = np.where(rng.random((T, C)) < 0.4, rng.gamma(0.8, 8.0, (T, C)), 0.0) / DAY
    f = {"q": q.astype(dtype), "snw": snw.astype(dtype), "pr": pr.astype(dtype)}
    ys, ms = np.asarray(time.segments("YS")[0]), np.asarray(time.segments("MS")[0])
    for v in f.values():
        for c in range(C):
            kind = c % 5
            if kind == 1 and T > 0:
                v[0, c] = np.nan
                for seg in (ys, ms):
                    v[seg[1:-1:2] - 1, c] = np.nan
                v[rng.integers(0, T, 3), c] = np.nan
            elif kind == 2:
                if len(ys) > 2:
                    v[ys[1]:ys[2], c] = np.nan
                if len(ms) > 2:
                    v[ms[1]:ms[2], c] = np.nan
            elif kind == 3:
                v[:, c] = np.nan
            elif kind == 4:
                v[rng.random(T) < 0.01, c] = np.nan
    return f


# ---- one run of a golden case (tests/golden/make_hydro_golden.py, tests/test_hydro_cpu.py) ---------------------------------
def spec_id(s):
    return ".".join(str(s[k]) for k in ("kind", "window", "p_exp", "freq", "pr") if k in s)


def run(s, fields, time, per_day=DAY):
    """The expected outputs of one run ``s`` of a case, with their scales.  A "sen" run also returns its inputs (``x``: the period
    means in the case's dtype, ``period_of``), so that the slope can be compared bit for bit wherever the means were made."""
    kind = s["kind"]
    if kind == "flow":
        return flow_period_stats(fields["q"], time.segments(s["freq"])[0])
    if kind == "melt":
        return melt_period_max(fields["snw"], fields["pr"] if s["pr"] == "pr" else None, per_day, s["window"], time.segments(s["freq"])[0])
    if kind == "api":
        return antecedent_precip(fields["pr"], per_day, api_weights(s["window"], s["p_exp"]))
    if kind == "sen":
        x = period_mean(fields["q"], time.segments(s["freq"])[0]).astype(fields["q"].dtype)
        table, _, _ = season_year_table(time, s["freq"])
        return dict(sen_slope(x, table), x=x, period_of=table)
    raise ValueError(kind)
