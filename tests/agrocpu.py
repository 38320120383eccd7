"""numpy restatement of xclim_amd/csrc/agro.hip and of the latitude coefficients behind it, in the reference's float64 order of
operations (indices/_agro.py:69-787, 1245-1384; indices/helpers.py:528-806; indices/generic.py:1417-1511; core/calendar.py:
1004-1072).  The reference's own code needs xarray, which the tests do not, so this module is the oracle: tests/test_agro_cpu.py holds it to
every reproducible known answer of the reference's own tests, and tests/golden/make_agro_golden.py writes its values, with the
SCALE of each (the sum of the absolute day or month terms that went into it), to tests/golden/agro_vectors.npz.  Sums run row
by row, one cell per column.  Test infrastructure only."""

import numpy as np

import petcpu
from xclim_amd import converters as xc
from xclim_amd.calendar import select_time_mask
from xclim_amd.timeaxis import TimeAxis, _is_leap, parse_freq

NAN = np.nan
QIAN_W = (0.0625, 0.25, 0.375, 0.25, 0.0625)
DI_K_NORTH = np.array([0, 0, 0, 0.1, 0.3, 0.5, 0.5, 0.5, 0.5, 0, 0, 0])
DI_K_SOUTH = np.array([0.5, 0.5, 0.5, 0, 0, 0, 0, 0, 0, 0.1, 0.3, 0.5])


def widen(x, sub=0.0):
    return np.asarray(x).astype(np.float64) - sub


def seqsum(terms):
    """(sum, sum of |terms|) down axis 0, row by row, NaN rows of a column skipped."""
    terms = np.asarray(terms, np.float64)
    s, sa = np.zeros(terms.shape[1:]), np.zeros(terms.shape[1:])
    for row in terms:
        ok = ~np.isnan(row)
        s = np.where(ok, s + np.where(ok, row, 0.0), s)
        sa = np.where(ok, sa + np.abs(np.where(ok, row, 0.0)), sa)
    return s, sa


# ---- the latitude coefficients (helpers.py:528-806) ------------------------------------------------------------------
def huglin_coefficient(lat, method, cap_value=np.nan):
    la = np.abs(np.asarray(lat, np.float64))
    if method == "huglin":
        k = np.full(la.shape, cap_value + 1)      # helpers.py:604: k = xr.full_like(lat_abs, _cap_value + 1)
        for f, lo, hi in [(0, -np.inf, 40), (0.02, 40, 42), (0.03, 42, 44), (0.04, 44, 46), (0.05, 46, 48), (0.06, 48, 50)]:
            k = np.where((lo < la) & (la <= hi), 1 + f, k)
        return k
    if method == "interpolated":
        return np.where(la <= 50, 1 + np.clip((la - 40) / 10, 0, None) * 0.06, cap_value)
    raise NotImplementedError(method)


def day_lengths(time, lats):
    """(T, L) hours, NaN in the polar day and night (helpers.py:450-525, "spencer"): the day-length half of
    petcpu.solar_table, without the radiation integral it also makes (the same bits; tests/test_agro_cpu.py compares them)."""
    da = np.asarray(xc.day_angle(time), np.float64)[:, None]
    sd = (0.006918 - 0.399912 * np.cos(da) + 0.070257 * np.sin(da) - 0.006758 * np.cos(2 * da)
          + 0.000907 * np.sin(2 * da) - 0.002697 * np.cos(3 * da) + 0.001480 * np.sin(3 * da))
    latr = np.asarray(lats, np.float64)[None, :] * (np.pi / 180)
    with np.errstate(invalid="ignore"):
        return (24 / np.pi) * np.arccos(-np.tan(latr) * np.tan(petcpu.wrap(sd)))


def gladstones_k_day(time, lat_cells):
    """(T, C): dl(t, lat) / dl(t, +-40) (helpers.py:671-676)."""
    lat = np.asarray(lat_cells, np.float64)
    with np.errstate(invalid="ignore"):
        dl = day_lengths(time, lat)
        piv = day_lengths(time, [40.0, -40.0])
        return np.where(lat[None, :] >= 0.0, dl / piv[:, :1], dl / piv[:, 1:])


def jones_k_period(time, lats, start_date="04-01", end_date="11-01", freq="YS", drop=False):
    """(P, L): 2.8311e-4 * (season sum of day lengths) + 0.30834; a period whose every latitude is below 1 is NaN; ValueError
    when every period is (helpers.py:763-797).  Latitudes with a NaN day length and periods without a season day change the
    reference's output shape: AssertionError here (the project raises NotServed for them), unless ``drop`` asks for the
    reference's own answer on such an axis, the periods that hold a season day."""
    if parse_freq(freq) not in (("Y", 1), ("Y", 7)):
        raise NotImplementedError(f"Freq {freq} not supported.")
    sel = select_time_mask(time, date_bounds=(start_date, end_date), include_bounds=(True, False))
    with np.errstate(invalid="ignore"):
        dl = day_lengths(time, lats)
    assert not np.isnan(dl[sel]).any(), "a latitude with a polar day or night in the season"
    seg = time.segments(freq)[0]
    P = len(seg) - 1
    k = np.full((P, dl.shape[1]), NAN)
    for p in range(P):
        a, b = int(seg[p]), int(seg[p + 1])
        assert drop or sel[a:b].any(), "a period without a season day"
        if sel[a:b].any():
            k[p] = 2.8311e-4 * seqsum(dl[a:b][sel[a:b]])[0] + 0.30834
    if drop:
        k = k[[p for p in range(P) if sel[int(seg[p]):int(seg[p + 1])].any()]]
    k[(k < 1.0).all(axis=1)] = NAN
    if np.isnan(k).all():
        raise ValueError("All latitudes for every growing season have a day length latitude coefficient below 1.0.")
    return k


# ---- xh_agro_degree_sum ---------------------------------------------------------------------------------------------
def degree_sum(tas, tasmin, tasmax, seg, sel=None, k=None, k_period=None, sub_C=273.15, thresh_hi=10.0, thresh_bedd=10.0,
               tr_adj=True, low_dtr=10.0, high_dtr=13.0, max_dd=9.0):
    """{"hi", "bedd", "valid", "hi_scale", "bedd_scale"} (P, C).  ``k``: None, (C) or (T, C) day factor; ``k_period`` (P, C)."""
    tx = widen(tasmax, sub_C)
    T, C = tx.shape
    kd = np.ones((T, C)) if k is None else np.broadcast_to(np.asarray(k, np.float64), (T, C))
    sel = np.ones(T, bool) if sel is None else np.asarray(sel, bool)
    present = ~np.isnan(tx)
    out = {}
    with np.errstate(invalid="ignore"):
        if tas is not None:
            tg = widen(tas, sub_C)
            present &= ~np.isnan(tg)
            t = (tg + tx) / 2 - thresh_hi
            t = np.where(t < 0, 0.0, t)
            out["hi"] = t * kd
        if tasmin is not None:
            tn = widen(tasmin, sub_C)
            present &= ~np.isnan(tn)
            adj = 0.0
            if tr_adj:
                dtr = tx - tn
                adj = 0.25 * np.where(dtr > high_dtr, dtr - high_dtr, np.where(dtr < low_dtr, dtr - low_dtr, 0.0))
            t = (tn + tx) / 2 - thresh_bedd
            t = np.where(t < 0, 0.0, t)
            t = t * kd + adj
            out["bedd"] = np.where(t > max_dd, max_dd, t)
    P = len(seg) - 1
    res = {n: np.zeros((P, C)) for n in out}
    res.update({n + "_scale": np.zeros((P, C)) for n in out})
    res["valid"] = np.zeros((P, C), np.int32)
    for p in range(P):
        rows = np.arange(int(seg[p]), int(seg[p + 1]))
        rows = rows[sel[rows]]
        res["valid"][p] = present[rows].sum(axis=0)
        for n, terms in out.items():
            s, sa = seqsum(terms[rows])
            if k_period is not None:
                s, sa = s * k_period[p], sa * np.abs(k_period[p])
            res[n][p], res[n + "_scale"][p] = s, sa
    return res


# ---- xh_agro_monthly ------------------------------------------------------------------------------------------------
def month_tables(time, freq="YS"):
    """(month_off (M + 1), month_cal (M), month_days (M), seg_months (P + 1)) of a gap-free daily axis."""
    key = time.year * 12 + time.month - 1
    months = np.arange(key[0], key[-1] + 1)
    month_off = np.searchsorted(key, np.append(months, key[-1] + 1), side="left").astype(np.int64)
    first = time.subset(month_off[:-1])
    seg = time.segments(freq)[0]
    seg_months = np.searchsorted(month_off[:-1], seg, side="left").astype(np.int64)
    return month_off, (months % 12 + 1).astype(np.int32), first.days_in_month().astype(np.int32), seg_months


def monthly(tasmin, tas, pr, evspsblpot, lat, month_off, month_cal, month_days, seg_months, hemisphere=None, sub_C=273.15,
            per_day=86400.0, wo=200.0):
    """{"cni", "mtwm", "di", "valid"} and their "_scale" (P, C), for the fields that are given."""
    ref = next(f for f in (tasmin, tas, pr) if f is not None)
    C = np.asarray(ref).shape[1]
    M, P = len(month_off) - 1, len(seg_months) - 1
    lat = np.zeros(C) if lat is None else np.asarray(lat, np.float64)
    north_cni = np.full(C, hemisphere == "north") if hemisphere else lat > 0
    north_di = np.full(C, hemisphere == "north") if hemisphere else lat >= 0
    res = {"valid": np.zeros((P, C), np.int32)}
    present = np.ones(np.asarray(ref).shape, bool)
    for f in (tasmin, tas, pr, evspsblpot):
        if f is not None:
            present &= ~np.isnan(np.asarray(f, np.float64))
    rows = lambda m: slice(int(month_off[m]), int(month_off[m + 1]))  # noqa: E731
    for p in range(P):
        m0, m1 = int(seg_months[p]), int(seg_months[p + 1])
        res["valid"][p] = present[int(month_off[m0]):int(month_off[m1])].sum(axis=0)
    if tasmin is not None:
        x = widen(tasmin, sub_C)
        res["cni"], res["cni_scale"] = np.full((P, C), NAN), np.zeros((P, C))
        for p in range(P):
            for north, month in ((True, 9), (False, 3)):
                cells = north_cni == north
                ms = [m for m in range(int(seg_months[p]), int(seg_months[p + 1])) if month_cal[m] == month]
                if not ms or not cells.any():
                    continue
                v = np.concatenate([x[rows(m)] for m in ms])[:, cells]
                s, sa = seqsum(v)
                n = (~np.isnan(v)).sum(axis=0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    res["cni"][p, cells] = np.where(n > 0, s / n, NAN)
                    res["cni_scale"][p, cells] = np.where(n > 0, sa / np.maximum(n, 1), 0.0)
    if tas is not None:
        x = widen(tas, sub_C)
        res["mtwm"], res["mtwm_scale"] = np.full((P, C), NAN), np.zeros((P, C))
        for p in range(P):
            for m in range(int(seg_months[p]), int(seg_months[p + 1])):
                v = x[rows(m)]
                s, sa = seqsum(v)
                n = (~np.isnan(v)).sum(axis=0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    mean = np.where(n > 0, s / n, NAN)
                    better = ~np.isnan(mean) & (np.isnan(res["mtwm"][p]) | (mean > res["mtwm"][p]))
                res["mtwm"][p] = np.where(better, mean, res["mtwm"][p])
                res["mtwm_scale"][p] = np.where(better, sa / np.maximum(n, 1), res["mtwm_scale"][p])
    if pr is not None:
        e_amt, p_amt = widen(evspsblpot) * per_day, widen(pr) * per_day
        term, tscale = np.zeros((M, C)), np.zeros((M, C))
        for m in range(M):
            E, Ea = seqsum(e_amt[rows(m)])
            Pm, Pa = seqsum(p_amt[rows(m)])
            k = np.where(north_di, DI_K_NORTH[month_cal[m] - 1], DI_K_SOUTH[month_cal[m] - 1])
            N = float(month_days[m])
            Pk = (k > 0) * Pm
            term[m] = Pk - E * k - (E / N) * (1 - k) * np.minimum(Pk / 5, N)
            tscale[m] = Pa + Ea     # |term| <= Pm + E (k <= 0.5, min(Pk / 5, N) <= N); the month sums err relative to these
        res["di"], res["di_scale"] = np.zeros((P, C)), np.zeros((P, C))
        for p in range(P):
            m0, m1 = int(seg_months[p]), int(seg_months[p + 1])
            for north, (a, b) in ((True, (m0, m1)), (False, (max(m0 - 6, 0), max(min(m1 - 6, M), 0)))):
                cells = north_di == north
                s, _ = seqsum(term[a:b][:, cells])
                res["di"][p, cells] = wo + s
                res["di_scale"][p, cells] = abs(wo) + tscale[a:b][:, cells].sum(axis=0)
    return res


# ---- xh_egdd --------------------------------------------------------------------------------------------------------
def _date_row(time, a, b, date):
    m, d = (int(v) for v in date.split("-"))
    idx = np.where((time.month[a:b] == m) & (time.day[a:b] == d))[0]
    return a + int(idx[0]) if idx.size else -1


def egdd_tables(time, freq="YS", after_date="07-01", start_date="01-01"):
    """(seg, doy, start_from, end_from, day0, label_doy, label_days) of a gap-free daily axis."""
    seg, starts = time.segments(freq)
    P = len(seg) - 1
    sf, ef, day0 = (np.full(P, -1, np.int64) for _ in range(3))
    ldoy, ldays = np.ones(P, np.int32), np.full(P, 365, np.int32)
    ordinal = time.ordinal()
    for p, (y, m) in enumerate(starts):
        a, b = int(seg[p]), int(seg[p + 1])
        label = TimeAxis(np.array([y]), np.array([m]), np.array([1]), time.calendar)
        ldoy[p] = label.doy[0]
        ldays[p] = 360 if time.calendar == "360_day" else 365 + int(bool(_is_leap(y, time.calendar)))
        day0[p] = 0
        if b > a:
            sf[p], ef[p] = _date_row(time, a, b, start_date), _date_row(time, a, b, after_date)
            day0[p] = int(ordinal[a] - label.ordinal()[0])
    return np.asarray(seg, np.int64), time.doy.astype(np.int32), sf, ef, day0, ldoy, ldays


def qian_wma(tas):
    x = widen(tas)
    out = np.full(x.shape, NAN)
    if len(x) >= 5:
        out[2:-2] = (((x[:-4] * QIAN_W[0] + x[1:-3] * QIAN_W[1]) + x[2:-2] * QIAN_W[2]) + x[3:-1] * QIAN_W[3]) + x[4:] * QIAN_W[4]
    return out


def days_since(v, label_doy, label_days):
    """doy_to_days_since(da) with start=None (calendar.py:1050-1059)."""
    return np.where(v >= label_doy, v, v + label_days) - label_doy


def egdd_bounds(cond, frost, seg, doy, sf, ef, window, plus):
    """(start_doy, end_doy) (P, C) float64 with NaN: the first run of ``window`` rows of ``cond`` from row sf[p] on, inside the
    period, as its day of year + ``plus``; the first row of ``frost`` from ef[p] on, as its day of year - 1."""
    P, C = len(seg) - 1, cond.shape[1]
    start, end = np.full((P, C), NAN), np.full((P, C), NAN)
    for p in range(P):
        a, b = int(seg[p]), int(seg[p + 1])
        run = np.zeros(C, np.int64)
        for r in range(a, b):
            ok = cond[r] & (sf[p] >= 0) & (r >= sf[p])
            run = np.where(ok, run + 1, 0)
            hit = np.isnan(start[p]) & (run >= window)
            start[p] = np.where(hit, doy[max(r - (window - 1), a)] + plus, start[p])
            if ef[p] >= 0 and r >= ef[p]:
                end[p] = np.where(np.isnan(end[p]) & frost[r], doy[r] - 1, end[p])
    return start, end


def egdd(tasmin, tasmax, seg, doy, sf, ef, day0, label_doy, label_days, method="bootsma", sub_C=273.15, thresh=5.0, qian=None,
         want_gap=False):
    """{"egdd", "start", "end", "valid", "egdd_scale"} (P, C).  ``qian``: the smoothed series to search the start in (default:
    qian_wma of tas), for the cross-check against xh_qian_wma's output."""
    tn, tx = widen(tasmin, sub_C), widen(tasmax, sub_C)
    tas = (tn + tx) / 2
    P, C = len(seg) - 1, tas.shape[1]
    with np.errstate(invalid="ignore"):
        if method == "bootsma":
            v, window, plus = tas, 1, 10
        elif method == "qian":
            v, window, plus = (qian_wma(tas) if qian is None else np.asarray(qian, np.float64)), 5, 0
        else:
            raise NotImplementedError(f"Method: {method}.")
        start, end = egdd_bounds(v > thresh, tn < 0, seg, doy, sf, ef, window, plus)
        deg = tas - thresh
        deg = np.where(deg < 0, 0.0, deg)
    res = {"start": start, "end": end, "egdd": np.full((P, C), NAN), "egdd_scale": np.zeros((P, C)),
           "valid": np.zeros((P, C), np.int32)}
    for p in range(P):
        a, b = int(seg[p]), int(seg[p + 1])
        res["valid"][p] = (~np.isnan(tas[a:b])).sum(axis=0)
        with np.errstate(invalid="ignore"):
            sd, ed = days_since(start[p], label_doy[p], label_days[p]), days_since(end[p], label_doy[p], label_days[p])
            ok = ~np.isnan(sd) & ~np.isnan(ed) & ~(sd > ed)
            d = (day0[p] + np.arange(b - a))[:, None]
            inside = (d >= sd[None, :]) & (d <= ed[None, :] - 1)
        s, sa = seqsum(np.where(inside, deg[a:b], NAN))
        res["egdd"][p] = np.where(ok, s, NAN)
        res["egdd_scale"][p] = np.where(ok, sa, 0.0)
    if want_gap:
        g = np.concatenate([np.abs(v - thresh).ravel(), np.abs(tn).ravel()])
        g = g[~np.isnan(g)]
        res["min_gap"] = float(g.min()) if g.size else np.inf
    return res


# ---- the element-wise pair ------------------------------------------------------------------------------------------
def corn_heat_units(tasmin, tasmax, sub_C=273.15, thresh_tasmin=4.44, thresh_tasmax=10.0):
    tn, tx = widen(tasmin, sub_C), widen(tasmax, sub_C)
    with np.errstate(invalid="ignore"):
        dx = tx - thresh_tasmax
        yn = np.where(tn > thresh_tasmin, 1.8 * (tn - thresh_tasmin), 0.0)
        yx = np.where(tx > thresh_tasmax, 3.33 * dx - 0.084 * (dx * dx), 0.0)
    return (yn + yx) / 2


# ---- one golden run ---------------------------------------------------------------------------------------------------
def factors(spec, time, lat, season):
    """The factor tables of a heat-sum run as the kernel takes them: ``{"k_cell" (C) | "k_day" (T, L) | "k_period" (P, L),
    "lat_idx" (C), "tr_adj"}``; the (T, C) / (P, C) forms the restatement takes are ``table[:, lat_idx]``."""
    method = spec["method"]
    lat = np.asarray(lat, np.float64)
    lat_u, li = np.unique(lat, return_inverse=True)
    out = {"tr_adj": not (spec["kind"] == "bedd" and method == "icclim"), "lat_idx": li.astype(np.int32)}
    if method in ("huglin", "interpolated"):
        out["k_cell"] = huglin_coefficient(lat, method, spec.get("cap_value", 1.0))
    elif method == "gladstones":
        out["k_day"] = gladstones_k_day(time, lat_u)
    elif method == "jones":
        out["k_period"] = jones_k_period(time, lat_u, season[0], spec["end_date"], spec["freq"])
    return out


def run(spec, fields, lat, time, sub_C, per_day, season):
    """The outputs (and their scales) of one run of a golden case.  ``spec``: kind "hi" / "bedd" / "both" (method, freq,
    end_date), "egdd" (method, freq), "monthly" (freq; cni / mtwm / di for the fields the case holds)."""
    kind, freq = spec["kind"], spec["freq"]
    if kind in ("hi", "bedd", "both"):
        f = factors(spec, time, lat, season)
        li = f["lat_idx"]
        k = f.get("k_cell")
        if "k_day" in f:
            k = f["k_day"][:, li]
        kp = f["k_period"][:, li] if "k_period" in f else None
        sel = select_time_mask(time, date_bounds=(season[0], spec["end_date"]), include_bounds=(True, False))
        return degree_sum(fields["tas"] if kind != "bedd" else None, fields["tasmin"] if kind != "hi" else None, fields["tasmax"],
                          time.segments(freq)[0], sel, k, kp, sub_C=sub_C, tr_adj=f["tr_adj"],
                          max_dd=spec.get("max_dd", 9.0))
    if kind == "egdd":
        return egdd(fields["tasmin"], fields["tasmax"], *egdd_tables(time, freq), method=spec["method"], sub_C=sub_C, want_gap=True)
    if kind == "monthly":
        return monthly(fields["tasmin"] if freq == "YS" else None, fields["tas"], fields.get("pr"), fields.get("evspsblpot"), lat,
                       *month_tables(time, freq), sub_C=sub_C, per_day=per_day, wo=spec.get("wo", 200.0))
    raise ValueError(kind)
