"""A numpy restatement of xclim_amd/csrc/ffdi.hip (the McArthur fire danger system) for the CPU tier of the tests.

It states the kernel's arithmetic — float64, the reference's evaluation order, Python's min / max (a NaN first argument
survives), N ** 1.3 from the same table, the 20-day window rescanned every day, FFDI on numpy's dtypes with exp / pow
evaluated in float64 and rounded once — vectorised over the cells, one time step at a time.  Inputs are (T, C) time
first; outputs float64 (T, C).  tests/test_ffdi_cpu.py checks it against the reference's own outputs; the GPU tests use
it where no golden output exists (the 30-year field).
"""

import numpy as np

WL = 20
N13 = np.array([n ** 1.3 for n in range(1, WL + 1)], dtype=np.float64)  # python's pow, as numba


def pymin(a, b):
    """Python's ``min(a, b)``: a unless b < a."""
    return np.where(b < a, b, a)


def pymax(a, b):
    return np.where(b > a, b, a)


def kbdi(pr, tasmax, pr_annual, kbdi0=None):
    pr, t = np.asarray(pr, np.float64), np.asarray(tasmax, np.float64)
    T, C = pr.shape
    den = 1 + 10.88 * np.exp(-0.00173 * np.broadcast_to(np.asarray(pr_annual, np.float64), (C,)))
    k = np.zeros(C) if kbdi0 is None else np.broadcast_to(np.asarray(kbdi0, np.float64), (C,)).copy()
    rr = np.full(C, 5.0)
    out = np.empty((T, C))
    with np.errstate(invalid="ignore"):
        for d in range(T):
            p = pr[d]
            dry = p <= 0.0
            r = np.where(dry, p, pymin(p, rr))
            rr = np.where(dry, 5.0, rr - r)
            peff = p - r
            et = 1e-3 * (203.2 - k) * (0.968 * np.exp(0.0875 * t[d] + 1.5552) - 8.3) / den
            k = k + (et - peff)
            k = pymin(pymax(k, 0.0), 203.2)
            out[d] = k
    return out


def df_window(w, smd, lim):
    """DF of one day from the window ``w`` (20, C), oldest first, and that day's smd (C)."""
    C = w.shape[1]
    run = np.zeros(C, bool)
    pmax, P, x, nn = np.zeros(C), np.zeros(C), np.ones(C), np.full(C, N13[0])
    for iw in range(WL):
        v = w[iw]
        event = v > 2.0
        P = np.where(event, P + v, P)
        new_max = event & (v >= pmax)
        nn = np.where(new_max, N13[WL - 1 - iw], nn)
        pmax = np.where(new_max, v, pmax)
        run = run | event
        close = (~event & run) | (event & (iw == WL - 1))
        xe = nn / (nn + P - 2.0)
        x = np.where(close, pymin(xe, x), x)
        run = run & ~close
        P = np.where(close, 0.0, P)
        pmax = np.where(close, 0.0, pmax)
    if lim == 0:
        xlim = np.where(smd < 20, 1 / (1 + 0.1135 * smd), 75 / (270.525 - 1.267 * smd))
        x = pymin(x, xlim)
    dfw = 10.5 * (1 - np.exp(-(smd + 30) / 40)) * (41 * (x * x) + x) / (40 * (x * x) + x + 1)
    if lim == 1:
        dflim = np.select([smd < 25.0, (smd >= 25.0) & (smd < 42.0), (smd >= 42.0) & (smd < 65.0),
                           (smd >= 65.0) & (smd < 100.0)], [6.0, 7.0, 8.0, 9.0], 10.0)
        dfw = pymin(dfw, dflim)
    return pymin(dfw, 10.0)


def drought_factor(pr, smd, lim=0):
    pr, smd = np.asarray(pr, np.float64), np.asarray(smd, np.float64)
    T, C = pr.shape
    out = np.full((T, C), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(WL - 1, T):
            out[d] = df_window(pr[d - WL + 1:d + 1], smd[d], lim)
    return out


def ffdi(df, tasmax, hurs, sfcWind):
    """The kernel's FFDI: numpy's dtypes, exp / pow in float64 rounded once for float32 results; float64 (T, C)."""
    tasmax, hurs, sfcWind, df = (np.asarray(a) for a in (tasmax, hurs, sfcWind, df))
    with np.errstate(invalid="ignore"):
        if tasmax.dtype == np.float32:
            c = [np.float32(v) for v in (0.0338, 0.0345, 0.0234, 0.243147)]
            s = c[0] * tasmax - c[1] * hurs.astype(np.float32) + c[2] * sfcWind.astype(np.float32) + c[3]
            e = np.exp(s.astype(np.float64)).astype(np.float32)
        else:
            e = np.exp(0.0338 * tasmax - 0.0345 * hurs + 0.0234 * sfcWind + 0.243147)
        if df.dtype == np.float32:
            pw = np.power(df.astype(np.float64), np.float64(np.float32(0.987))).astype(np.float32)
            return (pw * e).astype(np.float64)
        return np.power(df.astype(np.float64), 0.987) * e.astype(np.float64)


def chain(pr, tasmax, hurs, sfcWind, pr_annual, kbdi0=None, lim=0):
    k = kbdi(pr, tasmax, pr_annual, kbdi0)
    d = drought_factor(pr, k, lim)
    return k, d, ffdi(d, tasmax, hurs, sfcWind)
