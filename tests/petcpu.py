"""numpy restatement of xclim_amd/csrc/pet.hip: the solar table over (row, distinct latitude), then PET per element
(daily methods) or per cell and month (TW48, DA02), in the kernels' float64 operation order.  Used by tests/test_pet_cpu.py
(against the reference's golden outputs) and tests/test_gpu_pet.py (against the device).  Test infrastructure only."""

import os

import numpy as np

from xclim_amd import converters as xc

PI = np.pi


def wrap(x):
    return ((x + PI) % (2 * PI)) - PI


def _sunlit(decl, lat, hss, hs, he):
    """_sunlit_integral_of_cosine_of_solar_zenith_angle for the daily interval (hs = -pi, he just below pi)."""
    out = np.empty(np.broadcast(decl, lat, hss).shape)
    decl, lat, hss = (np.broadcast_to(v, out.shape) for v in (decl, lat, hss))
    for idx in np.ndindex(out.shape):
        d, la, ss = decl[idx], lat[idx], hss[idx]
        sr = -ss
        if np.isnan(ss) and d * la > 0:
            num, den = np.sin(he) - np.sin(hs), (he + 2 * PI - hs if he < hs else he - hs)
        elif np.isnan(ss) and d * la < 0:
            out[idx] = 0.0
            continue
        elif (hs > ss and he < sr) or (hs < sr and he < sr) or (hs > ss and he > ss):
            out[idx] = 0.0
            continue
        else:  # the daily interval covers the whole sunlit part
            h1 = hs if hs > sr else sr
            h2 = he if he < ss else ss
            num, den = np.sin(h2) - np.sin(h1), h2 - h1
        out[idx] = np.sin(d) * np.sin(la) * den + np.cos(d) * np.cos(la) * num
    return out


def solar_table(dang, lat_deg, solar_constant=1361.0):
    """(Ra [J m-2 d-1], day length [h]) of shape (R, L)."""
    da = np.asarray(dang, np.float64)[:, None]
    sd = (0.006918 - 0.399912 * np.cos(da) + 0.070257 * np.sin(da) - 0.006758 * np.cos(2 * da)
          + 0.000907 * np.sin(2 * da) - 0.002697 * np.cos(3 * da) + 0.001480 * np.sin(3 * da))
    decl = wrap(sd)
    latr = np.asarray(lat_deg, np.float64)[None, :] * (PI / 180)
    dr = 1.0001100 + 0.034221 * np.cos(da) + 0.001280 * np.sin(da) + 0.000719 * np.cos(2 * da) + 0.000077 * np.sin(2 * da)
    lw = wrap(latr)
    with np.errstate(invalid="ignore"):
        tt = -np.tan(lw) * np.tan(decl)
        hss = np.where(np.abs(tt) <= 1, np.arccos(np.clip(tt, -1, 1)), np.nan)
        cz = _sunlit(decl, lw, wrap(hss), wrap(-PI), wrap(PI - 1e-9))
        ra = solar_constant * 86400.0 * (1 / (2 * PI)) * cz * dr
        dl = (24 / PI) * np.arccos(-np.tan(latr) * np.tan(decl))
    return ra, dl


def _f(x):
    return None if x is None else np.asarray(x, np.float64)


def pet_daily(method, time, lat_cells, tasmin=None, tasmax=None, tas=None, hurs=None, rsds=None, rsus=None, rlds=None,
              rlus=None, sfcWind=None, pr=None, peta=0.00516409319477, petb=0.0874972822289, time_of_day=0.0):
    """(pet, wb) [kg m-2 s-1] of a daily method on (T, C) fields; ``lat_cells`` (C)."""
    m = xc.METHODS[method]
    tn, tx, tm0 = _f(tasmin), _f(tasmax), _f(tas)
    with np.errstate(invalid="ignore", divide="ignore"):
        if m != "FAO_PM98":
            lu, li = np.unique(np.asarray(lat_cells, np.float64), return_inverse=True)
            ra = solar_table(xc.day_angle(time, time_of_day), lu, 1367.0 if m == "MB05" else 1361.0)[0][:, li]
        if m == "BR65":
            k2f = lambda k: (k - (233.15 + 200.0 / 9)) / (5.0 / 9)  # noqa: E731
            tnf, txf = k2f(tn), k2f(tx)
            re = ra * (1e-4 / 4.184)
            pet = 0.094 * (-87.03 + 0.928 * txf + 0.933 * (txf - tnf) + 0.0486 * re)
            pet = np.where(pet < 0, 0.0, pet)
        elif m == "HG85":
            tnc, txc = tn - 273.15, tx - 273.15
            tmc = tm0 - 273.15 if tm0 is not None else (tnc + txc) / 2
            pet = 0.0023 * (ra * 1e-6 * 0.408) * (tmc + 17.8) * np.sqrt(txc - tnc)
            pet = np.where(pet < 0, 0.0, pet)
        elif m == "MB05":
            tmc = tm0 - 273.15 if tm0 is not None else ((tn - 273.15) + (tx - 273.15)) / 2
            rl = ra / (4185.5 * (751.78 - 0.5655 * (tmc + 273.15)))
            pet = rl * peta * tmc + rl * petb
        else:
            txc, tnc = tx - 273.15, tn - 273.15
            hu = _f(hurs) / 100
            w2 = _f(sfcWind) * np.log(67.8 * 2 - 5.42) / np.log(67.8 * 10 - 5.42)
            tmc = (txc + tnc) / 2

            def svp(t):
                return 100 * np.exp(-6096.9385 / t + 16.635794 + -2.711193e-2 * t + 1.673952e-5 * (t * t)
                                    + 2.433502 * np.log(t))

            es = (1.0 / 2) * (svp(txc + 273.15) + svp(tnc + 273.15)) * 1e-3
            ea = es * hu
            delta = 4098 * es / ((tmc + 237.3) * (tmc + 237.3))
            rn = (_f(rsds) - _f(rsus) - (_f(rlus) - _f(rlds))) * 0.0864
            gamma = 0.665e-03 * 101.325
            a1 = 0.408 * delta * (rn - 0.0)
            a2 = gamma * 900 / (tmc + 273.15) * w2 * (es - ea)
            a3 = delta + (gamma * (1 + 0.34 * w2))
            pet = (a1 + a2) / a3
    rate = pet / 86400
    return rate, (None if pr is None else _f(pr) - rate)


def _mean(x, f32):
    n = np.sum(~np.isnan(x), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.nansum(x, axis=0) / n
    return m.astype(np.float32).astype(np.float64) if f32 else m


def pet_monthly(method, time, lat_cells, tasmin=None, tasmax=None, tas=None, pr=None):
    """(pet, wb, months) of TW48 / DA02 on (T, C) fields: (M, C) [kg m-2 s-1]."""
    m = xc.METHODS[method]
    f32 = any(np.asarray(a).dtype == np.float32 for a in (tasmin, tasmax, tas, pr) if a is not None)
    tn, tx, tm0, p = _f(tasmin), _f(tasmax), _f(tas), _f(pr)
    seg, months, days, dseg, ndays = xc._months(time)
    lu, li = np.unique(np.asarray(lat_cells, np.float64), return_inverse=True)
    ra, dl = solar_table(xc.day_angle(days), lu)
    M, C = len(months), len(li)
    pet = np.empty((M, C))
    wb = np.empty((M, C)) if p is not None else None
    with np.errstate(invalid="ignore", divide="ignore"):
        tab = np.empty((M, len(lu)))
        for j in range(M):
            a, b = dseg[j], dseg[j + 1]
            if m == "TW48":
                tab[j] = _mean(dl[a:b] / 12, False)
            else:
                tab[j] = np.nansum(ra[a:b] * 1e-6, axis=0) * 0.408
        tab = tab[:, li]
        if m == "TW48":
            tc = tm0 - 273.15 if tm0 is not None else ((tn - 273.15) + (tx - 273.15)) / 2
            tc = np.where(tc < 0, 0.0, tc)
            tmv = np.stack([_mean(tc[seg[j]:seg[j + 1]], f32) for j in range(M)])
            yr = months.year
            for y in np.unique(yr):
                js = np.flatnonzero(yr == y)
                idm = (tmv[js] / 5) ** 1.514
                hi = np.nansum(idm, axis=0)
                ex = 6.75e-7 * hi ** 3.0 - 7.71e-5 * (hi * hi) + 0.01791 * hi + 0.49239
                pet[js] = 10 * (1.6 * tab[js] * (10 * tmv[js] / hi) ** ex)
        else:
            tnc, txc = tn - 273.15, tx - 273.15
            tc = tm0 - 273.15 if tm0 is not None else (tnc + txc) / 2
            for j in range(M):
                s = slice(seg[j], seg[j + 1])
                tr = _mean(txc[s], f32) - _mean(tnc[s], f32)
                tr = np.where(tr > 0, tr, 0.0)
                ab = tr - 0.0123 * _mean(p[s] * 2629800.0, f32)
                p76 = ab ** 0.76
                v = 0.0013 * tab[j] * (_mean(tc[s], f32) + 17.0) * p76
                v = np.where(np.isnan(p76), 0.0, v)
                pet[j] = np.where(v < 0, 0.0, v)
        pet = pet / (ndays * 86400.0)[:, None]
        if p is not None:
            for j in range(M):
                wb[j] = _mean(p[seg[j]:seg[j + 1]], f32) - pet[j]
    return pet, wb, months


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pet_vectors.npz")
FIELDS = ("tasmin", "tasmax", "tas", "hurs", "rsds", "rsus", "rlds", "rlus", "sfcWind", "pr")


def decode(q, dtype, pr=False):
    """tests/golden/make_pet_golden.py: int16 tenths (-32768 = NaN) -> the field the reference saw."""
    v = np.where(q == -32768, np.nan, q.astype(np.float64) / 10)
    if pr:
        v = v / 86400
    return v.astype(dtype)


def golden_cases():
    """[(name, dict)] with method, dtype, TimeAxis, time_of_day, lat (C), fields (T, C), peta / petb and the outputs."""
    z = np.load(GOLDEN)
    out = []
    for n in z["names"]:
        n = str(n)
        method, dt, cal, hour, peta, petb = (str(v) for v in z[f"{n}/meta"])
        y, m, d, T = (int(v) for v in z[f"{n}/start"])
        c = {"method": method, "dtype": np.dtype(dt), "time_of_day": float(hour), "lat": z["lats"],
             "time": _daily(y, m, d, T, cal), "pet": z[f"{n}/pet"], "pet_dtype": str(z[f"{n}/pet_dtype"]),
             "fields": {k: decode(z[f"{n}/{k}"], dt, pr=k == "pr") for k in FIELDS if f"{n}/{k}" in z},
             "kw": {k: float(v) for k, v in (("peta", peta), ("petb", petb)) if v}}
        for k in ("wb", "ra", "dl"):
            if f"{n}/{k}" in z:
                c[k] = z[f"{n}/{k}"]
        out.append((n, c))
    return out


def _daily(y, m, d, n, cal):
    from xclim_amd.timeaxis import TimeAxis

    ys, ms, ds = [], [], []
    for _ in range(n):
        ys.append(y), ms.append(m), ds.append(d)
        d += 1
        if d > int(xc._days_in_month(y, m, cal)):
            d, m = 1, m + 1
            if m > 12:
                m, y = 1, y + 1
    return TimeAxis(ys, ms, ds, cal)


def restated(c):
    """(pet, wb) of petcpu for a golden case (wb None without pr)."""
    f = c["fields"]
    if xc.METHODS[c["method"]] in ("TW48", "DA02"):
        pet, wb, _ = pet_monthly(c["method"], c["time"], c["lat"], **{k: f.get(k) for k in ("tasmin", "tasmax", "tas", "pr")})
        return pet, wb
    return pet_daily(c["method"], c["time"], c["lat"], time_of_day=c["time_of_day"], **f, **c["kw"])


def close(got, ref, f32, tw48=False):
    """The fixed tolerances: 1e-12 relative on float64 fields (1e-10 for TW48's power chain), 2e-5 relative on float32
    fields, where the reference rounds its intermediates in float32; an absolute floor of the same size relative to the
    case's largest magnitude applies near the clip(0) zeros and sign changes."""
    rtol = 2e-5 if f32 else (1e-10 if tw48 else 1e-12)
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
    scale = np.nanmax(np.abs(ref)) if np.isfinite(ref).any() else 0.0
    err = np.abs(got - ref)
    bound = rtol * np.abs(ref) + rtol * scale
    ok = np.isnan(ref) | (err <= bound)
    assert ok.all(), f"worst {np.nanmax(err / np.where(bound > 0, bound, 1))} x tolerance at {np.argwhere(~ok)[:5]}"
