"""An independent numpy restatement of the Canadian Fire Weather Index System for the tests (not part of the package).

Vectorised over cells, one python step per day, time on AXIS 0 ((T, C) fields).  It states the reference's arithmetic
(src/xclim/indices/fire/_cffwis.py) the way the kernel does: the three moisture codes and the overwintered DC in float64,
rounded to float32 when stored and carried; ISI / BUI / FWI / DSR in float32 with float32 constants and exp / log / pow
evaluated in float64 and rounded; season thresholds and the dry-start threshold compared in float32; GFWED season means
as an in-order float32 sum and a float32 divide.  Used against tests/golden/fire_vectors.npz (tests/test_fire_cpu.py)
and as the oracle of fields larger than the golden cases (tests/test_gpu_fire.py).
"""

from __future__ import annotations

import numpy as np

F = np.float32
INDEXES = ("DC", "DMC", "FFMC", "ISI", "BUI", "FWI", "DSR")

# effective day length [h] per latitude band (rows) and month (columns), Van Wagner 1987 / Lawson & Armitage 2008
DAY_LENGTH = np.array([[11.5, 10.5, 9.2, 7.9, 6.8, 6.2, 6.5, 7.4, 8.7, 10.0, 11.2, 11.8],
                       [10.1, 9.6, 9.1, 8.5, 8.1, 7.8, 7.9, 8.3, 8.9, 9.4, 9.9, 10.2],
                       [9.0] * 12,
                       [7.9, 8.4, 8.9, 9.5, 9.9, 10.2, 10.1, 9.7, 9.1, 8.6, 8.1, 7.8],
                       [6.5, 7.5, 9.0, 12.8, 13.9, 13.9, 12.4, 10.9, 9.4, 8.0, 7.0, 6.0]])
DAY_LENGTH_FACTOR = np.array([[6.4, 5.0, 2.4, 0.4, -1.6, -1.6, -1.6, -1.6, -1.6, 0.9, 3.8, 5.8],
                              [1.39] * 12,
                              [-1.6, -1.6, -1.6, 0.9, 3.8, 5.8, 6.4, 5.0, 2.4, 0.4, -1.6, -1.6]])

DEFAULTS = {"temp_start_thresh": 12.0, "temp_end_thresh": 5.0, "snow_thresh": 0.01, "temp_condition_days": 3,
            "snow_condition_days": 3, "carry_over_fraction": 0.75, "wetting_efficiency_fraction": 0.75, "dc_start": 15,
            "dmc_start": 6, "ffmc_start": 85, "prec_thresh": 1.0, "dc_dry_factor": 5, "dmc_dry_factor": 2}


def band5(lat):
    lat = np.asarray(lat, dtype=np.float64)
    b = np.full(lat.shape, -1)
    for k, (lo, hi) in enumerate([(-90, -30), (-30, -15), (-15, 15), (15, 30)]):
        b[(lat >= lo) & (lat < hi)] = k
    b[(lat >= 30) & (lat <= 90)] = 4
    return b


def band3(lat):
    lat = np.asarray(lat, dtype=np.float64)
    b = np.full(lat.shape, -1)
    b[(lat >= -90) & (lat < -15)] = 0
    b[(lat >= -15) & (lat < 15)] = 1
    b[(lat >= 15) & (lat <= 90)] = 2
    return b


def day_length(lat, month):
    b = band5(lat)
    if np.any(b < 0):
        raise ValueError("Invalid lat specified.")
    return DAY_LENGTH[b, np.asarray(month) - 1]


def day_length_factor(lat, month):
    b = band3(lat)
    if np.any(b < 0):
        raise ValueError("Invalid lat specified.")
    return DAY_LENGTH_FACTOR[b, np.asarray(month) - 1]


def _pymax(a, b):  # python's max(a, b): a unless b > a
    return np.where(b > a, b, a)


def ffmc_step(t, p, w, h, ffmc0):
    t, p, w, h, f0 = (np.asarray(v, dtype=np.float64) for v in (t, p, w, h, ffmc0))
    with np.errstate(all="ignore"):
        mo = (147.2 * (101.0 - f0)) / (59.5 + f0)
        rf = p - 0.5
        wet = 42.5 * rf * np.exp(-100.0 / (251.0 - mo)) * (1.0 - np.exp(-6.93 / rf))
        mo_r = np.where(mo > 150.0, (mo + wet) + (0.0015 * (mo - 150.0) ** 2) * np.sqrt(rf), mo + wet)
        mo_r = np.where(250.0 < mo_r, 250.0, mo_r)
        mo = np.where(p > 0.5, mo_r, mo)
        e1 = np.exp((h - 100.0) / 10.0)
        dry = 0.18 * (21.1 - t) * (1.0 - 1.0 / np.exp(0.115 * h))
        ed = 0.942 * h ** 0.679 + 11.0 * e1 + dry
        ew = 0.618 * h ** 0.753 + 10.0 * e1 + dry
        r1 = (100.0 - h) / 100.0
        kw1 = (0.424 * (1.0 - r1 ** 1.7) + (0.0694 * np.sqrt(w)) * (1.0 - r1 ** 8.0)) * (0.581 * np.exp(0.0365 * t))
        r2 = h / 100.0
        kw2 = (0.424 * (1.0 - r2 ** 1.7) + (0.0694 * np.sqrt(w)) * (1.0 - r2 ** 8.0)) * (0.581 * np.exp(0.0365 * t))
        m_wet = np.where(mo < ew, ew - (ew - mo) / 10.0 ** kw1, mo)
        m = np.where(mo < ed, m_wet, np.where(mo == ed, mo, ed + (mo - ed) / 10.0 ** kw2))
        ffmc = (59.5 * (250.0 - m)) / (147.2 + m)
    return np.where(ffmc > 101.0, 101.0, np.where(ffmc <= 0.0, 0.0, ffmc))


def dmc_step(t, p, h, dl, dmc0):
    t, p, h, dl, d0 = (np.asarray(v, dtype=np.float64) for v in (t, p, h, dl, dmc0))
    with np.errstate(all="ignore"):
        rk = np.where(t < -1.1, 0.0, 1.894 * (t + 1.1) * (100.0 - h) * dl * 0.0001)
        rw = 0.92 * p - 1.27
        wmi = 20.0 + 280.0 / np.exp(0.023 * d0)
        b = np.where(d0 <= 33.0, 100.0 / (0.5 + 0.3 * d0), np.where(d0 <= 65.0, 14.0 - 1.3 * np.log(d0), 6.2 * np.log(d0) - 17.2))
        wmr = wmi + (1000.0 * rw) / (48.77 + b * rw)
        pr = np.where(p > 1.5, 43.43 * (5.6348 - np.log(wmr - 20.0)), d0)
        pr = _pymax(pr, 0.0)
        dmc = _pymax(pr + rk, 0.0)
    return np.where(np.isnan(d0), np.nan, dmc)


def dc_step(t, p, fl, dc0):
    t, p, fl, d0 = (np.asarray(v, dtype=np.float64) for v in (t, p, fl, dc0))
    with np.errstate(all="ignore"):
        t = _pymax(t, -2.8)
        pe = _pymax((0.36 * (t + 2.8) + fl) / 2.0, 0.0)
        rw = 0.83 * p - 1.27
        smi = 800.0 * np.exp(-d0 / 400.0)
        dr = d0 - 400.0 * np.log(1.0 + ((3.937 * rw) / smi))
        wet = np.where(dr > 0.0, dr + pe, np.where(np.isnan(d0), np.nan, pe))
    return np.where(p > 2.8, wet, d0 + pe)


def _e(x):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, dtype=np.float64)).astype(F)


def _l(x):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, dtype=np.float64)).astype(F)


def _p(a, b):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(a, dtype=np.float64), np.float64(F(b))).astype(F)


def isi_step(ws, ffmc):
    ws, ffmc = np.asarray(ws, F), np.asarray(ffmc, F)
    with np.errstate(all="ignore"):
        mo = (F(147.2) * (F(101.0) - ffmc)) / (F(59.5) + ffmc)
        ff = (F(19.1152) * _e(mo * F(-0.1386))) * (F(1.0) + _p(mo, 5.31) / F(49300000.0))
        return ff * _e(F(0.05039) * ws)


def bui_step(dmc, dc):
    dmc, dc = np.asarray(dmc, F), np.asarray(dc, F)
    with np.errstate(all="ignore"):
        denom = dmc + F(0.4) * dc
        a = ((F(0.8) * dc) * dmc) / denom
        b = dmc - (F(1.0) - (F(0.8) * dc) / denom) * (F(0.92) + _p(F(0.0114) * dmc, 1.7))
        bui = np.where(dmc <= F(0.4) * dc, a, b)
        bui = np.where((dmc == 0) & (dc == 0), F(0), bui)
        return np.where(bui < 0, F(0), bui).astype(F)


def fwi_step(isi, bui):
    isi, bui = np.asarray(isi, F), np.asarray(bui, F)
    with np.errstate(all="ignore"):
        fwi = np.where(bui <= F(80.0), (F(0.1) * isi) * (F(0.626) * _p(bui, 0.809) + F(2.0)),
                       (F(0.1) * isi) * (F(1000.0) / (F(25.0) + F(108.64) / _e(F(0.023) * bui)))).astype(F)
        return np.where(fwi > 1, _e(F(2.72) * _p(F(0.434) * _l(fwi), 0.647)), fwi).astype(F)


def dsr_step(fwi):
    return (F(0.0272) * _p(np.asarray(fwi, F), 1.77)).astype(F)


def overwintering_dc(last_dc, wpr, a, b, min_dc):
    d, w = np.asarray(last_dc, np.float64), np.asarray(wpr, np.float64)
    with np.errstate(all="ignore"):
        qs = a * (800.0 * np.exp(-d / 400.0)) + b * (3.94 * w)
        out = _pymax(400.0 * np.log(800.0 / qs), float(min_dc))
    return np.where(np.isnan(d) | np.isnan(w), np.nan, out)


def fire_season(tas, snd, method, temp_start_thresh, temp_end_thresh, snow_thresh, temp_condition_days, snow_condition_days):
    """(T, C) boolean season mask; thresholds compared in float32."""
    tas = np.asarray(tas, F)
    T = tas.shape[0]
    ts, te, sth = F(temp_start_thresh), F(temp_end_thresh), F(snow_thresh)
    N, S = int(temp_condition_days), int(snow_condition_days)
    out = np.zeros(tas.shape, bool)
    first = N + 1 if method == "WF93" else max(N, S)
    for it in range(first, T):
        if method == "WF93":
            w = tas[it - N:it]
            su, sd = np.all(w > ts, axis=0), np.all(w < te, axis=0)
        elif method == "LA08":
            su = np.all(snd[it - S + 1:it + 1] <= sth, axis=0)
            sd = (snd[it] > sth) | np.all(tas[it - N + 1:it + 1] < te, axis=0)
        else:
            with np.errstate(all="ignore"):
                st_, ss_ = np.zeros(tas.shape[1], F), np.zeros(tas.shape[1], F)
                for k in range(it - N + 1, it + 1):
                    st_ = (st_ + tas[k]).astype(F)
                for k in range(it - S + 1, it + 1):
                    ss_ = (ss_ + snd[k]).astype(F)
                mt, ms = (st_ / F(N)).astype(F), (ss_ / F(S)).astype(F)
            su, sd = (mt > ts) & (ms < sth), (ms >= sth) | (mt < te)
        out[it] = (out[it - 1] | su) & ~sd
    return out


def fire_weather(tas, pr, hurs, ws, snd, month, lat, *, indexes=INDEXES, season_method=None, season_mask=None, dc0=None,
                 dmc0=None, ffmc0=None, winter_pr=None, overwintering=False, dry_start=None, initial_start_up=True, **params):
    """(T, C) inputs -> dict of outputs like _fire_weather_calc (season_mask when computed, winter_pr with overwintering)."""
    p = dict(DEFAULTS)
    p.update(params)
    tas = np.asarray(tas, F)
    T, C = tas.shape
    nanc = np.full(C, np.nan, F)
    dc0 = nanc if dc0 is None else np.asarray(dc0, F)
    dmc0 = nanc if dmc0 is None else np.asarray(dmc0, F)
    ffmc0 = nanc if ffmc0 is None else np.asarray(ffmc0, F)
    wpr = np.zeros(C, F) if winter_pr is None else np.asarray(winter_pr, F).copy()
    out = {k: np.full((T, C), np.nan, F) for k in indexes}
    prev = {"DC": dc0.copy(), "DMC": dmc0.copy(), "FFMC": ffmc0.copy()}
    if season_method is None:
        mask = np.ones((T, C), bool)
        for k, s in (("DC", "dc_start"), ("DMC", "dmc_start"), ("FFMC", "ffmc_start")):
            prev[k] = np.where(np.isnan(prev[k]), F(p[s]), prev[k]).astype(F)
    elif season_method == "mask":
        mask = np.asarray(season_mask).astype(bool)
    else:
        mask = fire_season(tas, snd, season_method, p["temp_start_thresh"], p["temp_end_thresh"], p["snow_thresh"],
                           p["temp_condition_days"], p["snow_condition_days"])
        out["season_mask"] = mask
    m16 = mask.astype(np.int16)
    ow_dc, ow_dmc = dc0.copy(), dmc0.copy()
    if overwintering and "DC" in indexes:
        prev["DC"] = nanc.copy()
    if dry_start:
        if not overwintering:
            ow_dc = np.where(np.isnan(dc0), F(p["dc_start"]), dc0).astype(F)
        ow_dmc = np.where(np.isnan(dmc0), F(p["dmc_start"]), dmc0).astype(F)
    pthr = F(p["prec_thresh"])
    b5, b3 = band5(lat), band3(lat)
    for it in range(T):
        if season_method is not None:
            if it == 0:
                delta = m16[0] if initial_start_up else 0 * m16[0]
            else:
                delta = m16[it] - m16[it - 1]
            sd, winter, su = delta == -1, (delta == 0) & (m16[it] == 0), delta == 1
            wet = pr[it] > pthr
            if "DC" in indexes:
                if overwintering:
                    ow_dc = np.where(sd, prev["DC"], ow_dc)
                    wpr = np.where(sd, pr[it], wpr).astype(F)
                    wpr = np.where(winter, wpr + pr[it], wpr).astype(F)
                    new = np.where(np.isnan(ow_dc), p["dc_start"], overwintering_dc(ow_dc, wpr, p["carry_over_fraction"],
                                                                                 p["wetting_efficiency_fraction"], p["dc_start"]))
                    prev["DC"] = np.where(su, new.astype(F), prev["DC"])
                    ow_dc = np.where(su, np.nan, ow_dc).astype(F)
                    wpr = np.where(su, np.nan, wpr).astype(F)
                elif dry_start:
                    ow_dc = _dry(ow_dc, sd, su, winter, wet, dry_start, F(p["dc_start"]), F(p["dc_dry_factor"]))
                    prev["DC"] = np.where(su, ow_dc, prev["DC"])
                    ow_dc = np.where(su, np.nan, ow_dc).astype(F)
                else:
                    prev["DC"] = np.where(su, F(p["dc_start"]), prev["DC"])
                prev["DC"] = np.where(sd, np.nan, prev["DC"]).astype(F)
            if "DMC" in indexes:
                if dry_start:
                    ow_dmc = _dry(ow_dmc, sd, su, winter, wet, dry_start, F(p["dmc_start"]), F(p["dmc_dry_factor"]))
                    prev["DMC"] = np.where(su, ow_dmc, prev["DMC"])
                    ow_dmc = np.where(su, np.nan, ow_dmc).astype(F)
                else:
                    prev["DMC"] = np.where(su, F(p["dmc_start"]), prev["DMC"])
                prev["DMC"] = np.where(sd, np.nan, prev["DMC"]).astype(F)
            if "FFMC" in indexes:
                prev["FFMC"] = np.where(sd, np.nan, np.where(su, F(p["ffmc_start"]), prev["FFMC"])).astype(F)
        mth = int(month[it])
        if "DC" in indexes:
            if np.any(b3 < 0):
                raise ValueError("Invalid lat specified.")
            out["DC"][it] = dc_step(tas[it], pr[it], DAY_LENGTH_FACTOR[b3, mth - 1], prev["DC"])
        if "DMC" in indexes:
            if np.any((b5 < 0) & ~np.isnan(prev["DMC"])):
                raise ValueError("Invalid lat specified.")
            out["DMC"][it] = dmc_step(tas[it], pr[it], hurs[it], DAY_LENGTH[np.maximum(b5, 0), mth - 1], prev["DMC"])
        if "FFMC" in indexes:
            out["FFMC"][it] = ffmc_step(tas[it], pr[it], ws[it], hurs[it], prev["FFMC"])
        if "ISI" in indexes:
            out["ISI"][it] = isi_step(ws[it], out["FFMC"][it])
        if "BUI" in indexes:
            out["BUI"][it] = bui_step(out["DMC"][it], out["DC"][it])
        if "FWI" in indexes:
            out["FWI"][it] = fwi_step(out["ISI"][it], out["BUI"][it])
        if "DSR" in indexes:
            out["DSR"][it] = dsr_step(out["FWI"][it])
        for k in ("DC", "DMC", "FFMC"):
            if k in indexes:
                prev[k] = out[k][it].copy()
    if overwintering:
        out["winter_pr"] = wpr
    return out


def _dry(ow, sd, su, winter, wet, mode, start, factor):
    ow = np.where(sd, start, ow).astype(F)
    if mode == "GFWED":
        sel = su | winter
        ow = np.where(sel & wet, F(0), np.where(sel & ~wet, ow + factor, ow)).astype(F)
    else:
        ow = np.where(winter & wet, start, np.where(winter & ~wet, ow + factor, ow)).astype(F)
    return ow
