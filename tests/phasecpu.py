"""numpy restatement of the snow / rain partition and the period indices on it, written from the reference's text
(indices/converters.py:1088-1373, indices/_multivariate.py:871-1171 and :1797-1829, indices/_threshold.py:1701-1967) with no
line of the device path: ``np.interp`` for brown and auer, ``np.tanh`` for dai, the resample helpers of oracle/ for the periods.
Everything is float64 on the widened fields, the binary select excepted (the dtype of ``pr``); sums are added in row order.

Thresholds are plain numbers: ``thresh`` and ``tas_thresh`` in the units of ``tas`` ("K" / "degC"), the thresholds on ``pr`` in the
units of ``pr``, the thresholds on snow in mm of the daily amount ``snow * per_day``."""
import numpy as np

from oracle.generic import _resample_reduce
from oracle.timeutil import OTime, groups

K2C = 273.15
PER_DAY = {"kg m-2 s-1": 86400.0, "mm/s": 86400.0, "mm/d": 1.0}
OUTPUTS = ("pr_sum", "solid_sum", "liquid_sum", "pr_n", "solid_n", "liquid_n", "tas_n", "snow_days", "snow_sum_over", "snow_n_over",
           "first_snow", "last_snow", "hplt_days", "rofg_days")
SNOW_HIGH = 1e6 * 86400.0

# a, b, c, d of the dai methods: {(phase, land): annual}, {(phase, land): rows a, b, c, d over DJF, MAM, JJA, SON}
DAI_ANNUAL = {("snow", True): (-48.2292, 0.7205, 1.1662, 1.0223), ("snow", False): (-47.1472, 0.4049, 1.9280, 1.0203),
              ("rain", True): (-47.8337, -0.6866, 1.4913, 1.0420), ("rain", False): (-47.3041, -0.4263, 2.5687, 1.0784)}
DAI_SEASONAL = {
    ("snow", True): [[-48.2372, -48.2493, -46.4000, -48.3251], [0.7449, 0.6634, 0.7013, 0.7798], [1.0919, 1.3388, 0.8362, 1.1502],
                     [1.0209, 1.0270, 1.0217, 1.0180]],
    ("snow", False): [[-47.1823, -47.0035, -47.1472, -46.8494], [0.4003, 0.4090, 0.4049, 0.4162], [2.1735, 1.7372, 1.9280, 2.0474],
                      [1.0255, 1.0226, 1.0203, 1.0155]],
    ("rain", True): [[-47.5770, -47.9077, -46.8303, -48.0315], [-0.6856, -0.6603, -0.6595, -0.7663], [1.3942, 1.6927, 1.1582, 1.4640],
                     [1.0438, 1.0358, 1.1056, 1.0412]],
    ("rain", False): [[-47.0262, -47.2828, -47.3041, -47.2107], [-0.4360, -0.4299, -0.4263, -0.4280], [2.8572, 2.3397, 2.5687, 2.7118],
                      [1.0731, 1.0800, 1.0784, 1.0911]],
}


def otime(start, rows, calendar="standard"):
    """The oracle's time coordinate of a daily axis that starts on ``YYYY-MM-DD``."""
    if calendar == "standard":
        return OTime.standard(start, rows)
    y, m, d = (int(p) for p in start.split("-"))
    assert (m, d) == (1, 1)
    return OTime.noleap(y, rows, calendar)


def seasons(month):
    """0 = DJF, 1 = MAM, 2 = JJA, 3 = SON of every month number."""
    return (np.asarray(month) % 12) // 3


def auer_nodes():
    t = np.concatenate([[-273.15], np.linspace(0, 6, 100, endpoint=False), [6, 1e10]])
    f = np.clip(np.polynomial.polynomial.polyval(t, [100, 4.6664, -15.038, -1.5089, 2.0399, -0.366, 0.0202]), 0, 100) / 100
    f[0] = 1
    f[-2:] = 0
    return t, f


def _dai(phase, method, t_c, month, land, clip_temp):
    """The clipped dai fraction of one coefficient set (land True / False) at ``t_c`` (T, C) degC."""
    if method == "dai_annual":
        a, b, c, d = (np.float64(v) for v in DAI_ANNUAL[phase, land])
    else:
        a, b, c, d = (np.asarray(row)[seasons(month)][:, None] for row in DAI_SEASONAL[phase, land])

    def frac(tt):
        return a * (np.tanh(b * (tt - c)) - d) / 100

    f = frac(t_c)
    if clip_temp is not None:
        lo, hi = (frac(clip_temp), frac(-clip_temp)) if phase == "snow" else (frac(-clip_temp), frac(clip_temp))
        f = (f - lo) / (hi - lo)
    return np.clip(f, 0, 1)


def split(pr, tas, method="binary", thresh=None, units="K", month=None, clip_temp=None, landmask=True):
    """(snow, rain) of every sample of ``pr`` (T, C) by ``tas``; ``landmask`` a bool or a bool (C) array (which, as in the reference,
    drops ``clip_temp``)."""
    pr, tas = np.asarray(pr), np.asarray(tas)
    off = K2C if units == "K" else 0.0
    thresh = off if thresh is None else thresh
    with np.errstate(invalid="ignore"):
        if method == "binary":
            thr = np.float32(thresh) if pr.dtype == np.float32 else thresh
            snow = np.where(tas <= thr, pr, pr.dtype.type(0))
            return snow, pr - snow
        pr64, t64 = pr.astype(np.float64), tas.astype(np.float64)
        if method == "brown":
            upper = ((thresh - off) + 2) + off
            f = np.interp(t64, [-np.inf, thresh, upper, np.inf], [1.0, 1.0, 0.0, 0.0])
            f = np.where(t64 <= thresh, 1.0, np.where(t64 >= upper, 0.0, f))   # (np.interp's 0 * inf on the outer intervals)
            f = np.where(np.isnan(t64), np.nan, f)
        elif method == "auer":
            nodes, vals = auer_nodes()
            dtas = (t64 + (K2C - off)) - (thresh + (K2C - off))
            f = np.where(np.isnan(dtas), np.nan, np.interp(dtas, nodes, vals))
        elif method in ("dai_annual", "dai_seasonal"):
            t_c = t64 - off
            if isinstance(landmask, (bool, np.bool_)):
                fs, fr = (_dai(ph, method, t_c, month, bool(landmask), clip_temp) for ph in ("snow", "rain"))
            else:
                m = np.asarray(landmask, bool).reshape(1, -1)
                fs, fr = (np.where(m, _dai(ph, method, t_c, month, True, None), _dai(ph, method, t_c, month, False, None))
                          for ph in ("snow", "rain"))
            return pr64 * fs, pr64 * fr
        else:
            raise ValueError(method)
        snow = pr64 * f
        return snow, pr64 - snow


def _sum(x, time, freq):
    """NaN-skipping sum of every period, rows added in order (an all-NaN period gives 0)."""
    return _resample_reduce(np.where(np.isnan(x), 0.0, x), time, freq, lambda g: np.add.reduce(g, axis=0) if len(g) else np.zeros(g.shape[1:]))


def _count(mask, time, freq):
    return _resample_reduce(mask.astype(np.float64), time, freq, lambda g: g.sum(axis=0))


def rofg_marks(pr, tas, thresh, frz, window=7):
    """The days of rain on frozen ground: ``tas > frz`` after ``window`` rows that are not (NaN included), ``pr > thresh``; never on
    the first ``window`` rows of the series (rolling(window + 1) with min_periods)."""
    with np.errstate(invalid="ignore"):
        warm = np.asarray(tas) > frz
        wet = np.asarray(pr) > thresh
    out = np.zeros(warm.shape, bool)
    for r in range(window, warm.shape[0]):
        out[r] = warm[r] & ~warm[r - window:r].any(axis=0) & wet[r]
    return out


def period_outputs(pr, second, time: OTime, freq, *, given=False, per_day=86400.0, method="binary", thresh=None, units="K", clip_temp=None,
                   landmask=True, snow_low=0.0, snow_high=SNOW_HIGH, snow_thresh=1.0, pr_thresh=None, tas_thresh=None, rofg_thresh=None,
                   window=7):
    """Every output of the period kernel, ``{name: (P, C) float64}``; ``second`` is ``tas``, or ``prsn`` itself with ``given``."""
    pr, second = np.asarray(pr), np.asarray(second)
    off = K2C if units == "K" else 0.0
    if given:
        snow, rain = second, pr - second
    else:
        snow, rain = split(pr, second, method, thresh, units, time.month, clip_temp, landmask)
    am, sm, lm = (np.asarray(v, np.float64) * per_day for v in (pr, snow, rain))
    out = {"pr_sum": _sum(am, time, freq), "solid_sum": _sum(sm, time, freq), "liquid_sum": _sum(lm, time, freq)}
    for n, v in (("pr_n", am), ("solid_n", sm), ("liquid_n", lm), ("tas_n", second)):
        out[n] = _count(~np.isnan(v), time, freq)
    with np.errstate(invalid="ignore"):
        out["snow_days"] = _count((sm > snow_low) & (sm <= snow_high), time, freq)   # domain_count: compare(>) * compare(<=)
        over = sm >= snow_thresh
    out["snow_sum_over"] = _sum(np.where(over, sm, 0.0), time, freq)
    out["snow_n_over"] = _count(over, time, freq)
    first, last = [], []
    for _, idx in groups(time, freq):
        f, la = np.full(pr.shape[1], np.nan), np.full(pr.shape[1], np.nan)
        for r in idx:
            f = np.where(over[r] & np.isnan(f), time.doy[r], f)
            la = np.where(over[r], time.doy[r], la)
        first.append(f), last.append(la)
    out["first_snow"], out["last_snow"] = np.stack(first), np.stack(last)
    if not given:
        pt = 0.4 / per_day if pr_thresh is None else pr_thresh
        tt = -0.2 + off if tas_thresh is None else tas_thresh
        rt = 1.0 / per_day if rofg_thresh is None else rofg_thresh
        if pr.dtype == np.float32:
            pt, tt, rt, frz = (np.float32(v) for v in (pt, tt, rt, off))
        else:
            frz = off
        with np.errstate(invalid="ignore"):
            out["hplt_days"] = _count((pr >= pt) & (second < tt), time, freq)
        out["rofg_days"] = _count(rofg_marks(pr, second, rt, frz, window), time, freq)
    return out


# ---- the reference's functions on the outputs ---------------------------------------------------------------------------
def precip_accumulation(pr, tas, phase, time, freq, per_day, **kw):
    name = {None: "pr", "solid": "solid", "liquid": "liquid"}[phase]
    return period_outputs(pr, pr if tas is None else tas, time, freq, given=tas is None, per_day=per_day, **kw)[name + "_sum"]


def precip_average(pr, tas, phase, time, freq, per_day, **kw):
    name = {None: "pr", "solid": "solid", "liquid": "liquid"}[phase]
    o = period_outputs(pr, pr if tas is None else tas, time, freq, given=tas is None, per_day=per_day, **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return o[name + "_sum"] / o[name + "_n"]


def liquid_precip_ratio(pr, second, time, freq, given=False, **kw):
    o = period_outputs(pr, second, time, freq, given=given, per_day=1.0, **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (o["pr_sum"] - o["solid_sum"]) / o["pr_sum"]


def winter(time, freq):
    """bool (P): the periods labelled in December."""
    return np.array([(label[1] if isinstance(label, tuple) else label.month) == 12 for label, _ in groups(time, freq)])


def snowfall_frequency(o):
    with np.errstate(invalid="ignore", divide="ignore"):
        return o["snow_days"] / o["solid_n"] * 100


def snowfall_intensity(o):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(o["snow_n_over"] > 0, o["snow_sum_over"] / o["snow_n_over"], 0.0)
