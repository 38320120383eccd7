"""Numpy / python restatement of xclim_amd/csrc/stdidx.hip (the standardized-index fits and transform), step for step:
numpy's pairwise sums, _loc_estimation, the _fit_start closed forms, scipy's brentq for the gamma floc case and fmin's
Nelder–Mead on _penalized_nnlf.  tests/test_stdidx_cpu.py checks it against tests/golden/spi_vectors.npz (the reference's
own fits), which validates the kernel's algorithm without a GPU."""

import math

import numpy as np
import scipy.special as sc
import scipy.stats

LOGXMAX = math.log(np.finfo(float).max)


def pw_sum(a):
    """np.add.reduce of a float64 sequence (pairwise_sum for n <= 128; 8 interleaved sums beyond, like the kernel)."""
    n = len(a)
    if n < 8:
        r = 0.0
        for v in a:
            r += v
        return r
    r = list(a[:8])
    nfull = n - n % 8
    for i in range(8, nfull):
        r[i & 7] += a[i]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(nfull, n):
        res += a[i]
    return res


def digamma_pos(x):
    w = 0.0
    while x < 10.0:
        w += 1.0 / x
        x += 1.0
    z = 1.0 / (x * x)
    y = z * (8.33333333333333333333e-2 + z * (-8.33333333333333333333e-3 + z * (3.96825396825396825397e-3 + z * (
        -4.16666666666666666667e-3 + z * (7.57575757575757575758e-3 + z * (-2.10927960927960927961e-2 + z * 8.33333333333333333333e-2))))))
    return math.log(x) - 0.5 / x - y - w


def _isfinite(v):
    return not (math.isinf(v) or math.isnan(v))


def nnlf(dist, s, p0, loc, scale):
    if not (p0 > 0.0) or not (scale > 0.0):
        return math.inf
    if dist == "gamma":
        cst, am1 = math.lgamma(p0), p0 - 1.0
    else:
        cst, am1 = math.log(p0) + 0.0, -p0 - 1.0
    terms, bad = [], 0
    for v in s:
        x = (v - loc) / scale
        if not (x >= 0.0):
            bad += 1
            continue
        with np.errstate(all="ignore"):
            if dist == "gamma":
                xl = 0.0 if am1 == 0.0 else (am1 * math.log(x) if x > 0 else (-math.inf if am1 > 0 else math.inf))
                lp = xl - x - cst
            elif x == 0.0:
                cm1 = p0 - 1.0
                lp = cst + (0.0 if cm1 == 0.0 else (-math.inf if cm1 > 0 else math.inf)) - 2.0 * math.log1p(0.0)
            else:
                try:
                    pw = x ** (-p0)
                except OverflowError:
                    pw = math.inf
                lp = (cst + am1 * math.log(x)) - 2.0 * (math.log1p(pw) if pw != math.inf else math.inf)
        if not _isfinite(lp):
            bad += 1
            continue
        terms.append(lp)
    return (-(0.0 + pw_sum(terms)) + bad * LOGXMAX * 100.0) + len(s) * math.log(scale)


def loc_estimation(s):
    xs = sorted(s)
    x1, x2, xn = xs[0], xs[1], xs[-1]
    den = x1 + xn - 2.0 * x2
    num = x1 * xn - x2 * x2
    loc0 = num / den if den != 0 else (math.copysign(math.inf, num) if num != 0 else math.nan)
    return loc0 if loc0 < x1 else x1 - 0.0001 * abs(x1)


def fit_start(dist, s, loc0):
    xp = [v - loc0 for v in s if v - loc0 > 0.0]
    n = len(xp)
    if n == 0:
        return math.nan, math.nan
    m = pw_sum(xp) / n
    if dist == "gamma":
        A = math.log(m) - pw_sum([math.log(v) for v in xp]) / n
        if A == 0:
            return math.inf, 0.0
        p0 = (1.0 + math.sqrt(1.0 + 4.0 * A / 3.0)) / (4.0 * A)
        return p0, m / p0
    m2 = pw_sum([v * v for v in xp]) / n
    scale0 = 2.0 * m ** 3 / (m2 + m ** 2)
    d = m2 - m ** 2
    p0 = math.pi * m / math.sqrt(3) / math.sqrt(d) if d > 0 else math.nan
    return p0, scale0


def gamma_shape_root(s):
    if not (s > 0):  # identical values: the bracket is [inf, inf] and brentq fails in the reference
        return math.nan
    aest = (3.0 - s + math.sqrt((s - 3.0) ** 2 + 24.0 * s)) / (12.0 * s)
    f = lambda a: math.log(a) - digamma_pos(a) - s  # noqa: E731
    xpre, xcur = aest * (1.0 - 0.4), aest * (1.0 + 0.4)
    xtol, rtol = 2e-12, 4 * np.finfo(float).eps
    xblk = fblk = spre = scur = 0.0
    fpre, fcur = f(xpre), f(xcur)
    if fpre == 0:
        return xpre
    if fcur == 0:
        return xcur
    if math.copysign(1, fpre) == math.copysign(1, fcur):
        return math.nan
    for _ in range(100):
        if fpre != 0 and fcur != 0 and math.copysign(1, fpre) != math.copysign(1, fcur):
            xblk, fblk = xpre, fpre
            spre = scur = xcur - xpre
        if abs(fblk) < abs(fcur):
            xpre, xcur, xblk = xcur, xblk, xcur
            fpre, fcur, fblk = fcur, fblk, fcur
        delta = (xtol + rtol * abs(xcur)) / 2
        sbis = (xblk - xcur) / 2
        if fcur == 0 or abs(sbis) < delta:
            return xcur
        if abs(spre) > delta and abs(fcur) < abs(fpre):
            if xpre == xblk:
                stry = -fcur * (xcur - xpre) / (fcur - fpre)
            else:
                dpre = (fpre - fcur) / (xpre - xcur)
                dblk = (fblk - fcur) / (xblk - xcur)
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre))
            if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):
                spre, scur = scur, stry
            else:
                spre = scur = sbis
        else:
            spre = scur = sbis
        xpre, fpre = xcur, fcur
        xcur += scur if abs(scur) > delta else (delta if sbis > 0 else -delta)
        fcur = f(xcur)
    return xcur


def nelder_mead(func, x0):
    """fmin(xtol=ftol=1e-4): the kernel's loop (stable ordering, budget checked before every call).  -> (x, nfev)"""
    N = len(x0)
    maxfun = maxiter = 200 * N
    sim = [list(x0)]
    for k in range(N):
        y = list(x0)
        y[k] = (1.0 + 0.05) * y[k] if y[k] != 0 else 0.00025
        sim.append(y)
    fs = [func(v) for v in sim]
    ncall = [N + 1]

    def order():
        idx = sorted(range(N + 1), key=lambda i: fs[i])  # stable
        sim[:] = [sim[i] for i in idx]
        fs[:] = [fs[i] for i in idx]

    class Budget(Exception):
        pass

    def ev(v):
        if ncall[0] >= maxfun:
            raise Budget
        ncall[0] += 1
        return func(v)

    order()
    it = 1
    while ncall[0] < maxfun and it < maxiter:
        if all(abs(sim[j][k] - sim[0][k]) <= 1e-4 for j in range(1, N + 1) for k in range(N)) and \
                all(abs(fs[0] - fs[j]) <= 1e-4 for j in range(1, N + 1)):
            break
        xbar = []
        for k in range(N):
            t = sim[0][k]
            for j in range(1, N):
                t = t + sim[j][k]
            xbar.append(t / N)
        try:
            xr = [2.0 * xbar[k] - sim[N][k] for k in range(N)]
            fxr = ev(xr)
            if fxr < fs[0]:
                xe = [3.0 * xbar[k] - 2.0 * sim[N][k] for k in range(N)]
                fxe = ev(xe)
                sim[N], fs[N] = (xe, fxe) if fxe < fxr else (xr, fxr)
            elif fxr < fs[N - 1]:
                sim[N], fs[N] = xr, fxr
            else:
                shrink = False
                if fxr < fs[N]:
                    xc = [1.5 * xbar[k] - 0.5 * sim[N][k] for k in range(N)]
                    fxc = ev(xc)
                    if fxc <= fxr:
                        sim[N], fs[N] = xc, fxc
                    else:
                        shrink = True
                else:
                    xcc = [0.5 * xbar[k] + 0.5 * sim[N][k] for k in range(N)]
                    fxcc = ev(xcc)
                    if fxcc < fs[N]:
                        sim[N], fs[N] = xcc, fxcc
                    else:
                        shrink = True
                if shrink:
                    for j in range(1, N + 1):
                        sim[j] = [sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]) for k in range(N)]
                        fs[j] = ev(sim[j])
            it += 1
        except Budget:
            pass
        order()
    return sim[0], ncall[0]


def fit_one(sample, dist, method, floc):
    """One (cell, group): the sample already without NaN (and zeros when zero-inflated).  -> (params[3], nfev)"""
    s = [float(v) for v in sample]
    nan3 = [math.nan] * 3
    if len(s) <= 1:
        return nan3, 0
    nfev = 0
    if method == "APP":
        p0, sc0 = fit_start(dist, s, floc)
        pr = [p0, floc, sc0]
    elif dist == "gamma" and floc is not None:
        if not all(v > floc for v in s):
            return nan3, 0
        d = [v - floc if floc != 0 else v for v in s]
        xbar = pw_sum(d) / len(d)
        sv = math.log(xbar) - pw_sum([math.log(v) for v in d]) / len(d)
        a = gamma_shape_root(sv)
        pr = [a, floc, xbar / a]
    else:
        loc0 = floc if floc is not None else loc_estimation(s)
        p0, sc0 = fit_start(dist, s, loc0)
        if any(math.isnan(v) for v in (p0, loc0, sc0)):
            return nan3, 0
        if floc is None:
            x, nfev = nelder_mead(lambda v: nnlf(dist, s, v[0], v[1], v[2]), [p0, loc0, sc0])
            pr = list(x)
        else:
            x, nfev = nelder_mead(lambda v: nnlf(dist, s, v[0], floc, v[1]), [p0, sc0])
            pr = [x[0], floc, x[1]]
        if not (pr[0] > 0 and pr[2] > 0):
            return nan3, nfev
    if any(math.isnan(v) for v in pr):
        return nan3, nfev
    return pr, nfev


def fit(xp, gidx, G, dist, method, zero_inflated, floc):
    """(T, C) float32 -> params (G, 3, C), nzeros, nnotnull (G, C) float64 (NaN for groups without rows), nfev."""
    C = xp.shape[1]
    params = np.full((G, 3, C), np.nan)
    nz = np.full((G, C), np.nan)
    nn = np.full((G, C), np.nan)
    nfev = np.zeros((G, C), np.int32)
    for g in range(G):
        rows = np.flatnonzero(gidx == g)
        if len(rows) == 0:
            continue
        for c in range(C):
            v = xp[rows, c].astype(np.float64)
            nz[g, c] = np.sum(v == 0)
            nn[g, c] = np.sum(~np.isnan(v))
            keep = ~np.isnan(v) & ((v != 0) if zero_inflated else True)
            params[g, :, c], nfev[g, c] = fit_one(v[keep], dist, method, floc)
    return params, nz, nn, nfev


def index(xp, gidx, params, dist, nz=None, nn=None, interp=1.0, alpha=0.0, beta=1.0):
    """The transform: cdf (scipy's regularized incomplete gamma / the fisk closed form), mixture, ndtri, clip."""
    p = params[gidx]
    v = xp.astype(np.float64)
    with np.errstate(all="ignore"):
        a, loc, scale = p[:, 0], p[:, 1], p[:, 2]
        x = (v - loc) / scale
        if dist == "gamma":
            core = sc.gammainc(a, np.where(x > 0, x, 1.0))
        else:
            core = 1.0 / (1.0 + np.where(x > 0, x, 1.0) ** (-a))
        cdf = np.where(x > 0, core, 0.0)
        cdf = np.where(np.isinf(x) & (x > 0), 1.0, cdf)
        cdf = np.where((a > 0) & (scale > 0) & ~np.isnan(x), cdf, np.nan)
        if nz is not None:
            den = ((nn[gidx] + 1.0) - alpha) - beta
            r1 = (1.0 - alpha) / den
            rn = (nz[gidx] - alpha) / den
            prob = np.where(v == 0, (1.0 - interp) * r1 + interp * rn, rn + (1.0 - rn) * cdf)
        else:
            prob = cdf
        return np.clip(scipy.stats.norm.ppf(prob), -8.21, 8.21)
