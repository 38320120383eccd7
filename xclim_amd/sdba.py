"""Host mirror of the sdba empirical-quantile-mapping path (``xclim.sdba`` == third-party ``xsdba >= 0.4.0``;
reference shim src/xclim/sdba.py:1-28; object API pinned by tests/test_xsdba.py:44-155).

Names follow xsdba: ``EmpiricalQuantileMapping.train(ref, hist, nquantiles=20, kind="+", group="time")`` then
``.adjust(sim, interp="nearest", extrapolation="constant")``, with ``ds.af`` / ``ds.hist_q`` exposed as ``.af`` /
``.hist_q``; ``nbutils.quantile`` and ``utils.equally_spaced_nodes`` as module functions.  Arrays: TIME ON AXIS 0, numpy
or device arrays; all arithmetic is in ``xh_eqm_train`` / ``xh_eqm_adjust``.

Grouping (first slice): :class:`Grouper` ``"time"``, ``"time.month"``, ``"time.season"`` and ``"time.dayofyear"`` with
an odd ``window`` (xsdba: the samples of a group are the centred ``window`` days around every time step of the group —
the same sample sets as ``percentile_doy``).  Training gathers each group's rows (``xh_select_rows``) and runs the
per-column multi-quantile kernels on them; ``af`` / ``hist_q`` get a leading group axis ``(group, quantiles, *cells)``.
``adjust`` maps every time step with the factors of ITS group (rows are permuted group-major once, one ``xh_eqm_adjust``
launch per group on a contiguous row block, one gather back).  For "linear" xsdba interpolates over the (quantile, group)
PLANE (``utils.interp_on_quantiles`` -> ``_interp_on_quantiles_2D``: ``scipy.interpolate.griddata`` with a fractional group
index — the documented standard use, docs/sdba.rst:64-65, CHANGELOG.rst:338): built since round 5 for month / day-of-year
groupings (``xh_plane_linear``: the Delaunay triangle of every step is located by a walk, no triangulation is stored; one
launch over the whole series); "cubic" with a sub-grouping (griddata's Clough-Tocher scheme) raises
``NotImplementedError`` (:func:`_check_group_interp`) — an interpolation along the quantile axis inside each group would
silently differ from it.  "nearest" with a month / day-of-year grouping
follows xsdba since round 4: ``griddata(method="nearest")`` in the (hist_q, group coordinate) plane over the nodes of ALL
groups — where the own group's nearest node is more than one unit away a node of a NEIGHBOURING group can win — and the
own group's end factors outside its nodes (``xh_plane_nearest``: one launch over the whole series;
``grouped_nearest="group"`` restores the own-group rule of rounds 2-3, which "time.season" still uses).

The host plumbing exists once ("sdba host plumbing"): :class:`_GroupMajor` (the group-major layout of the rows),
:func:`_group` (the one view cut out of a table), :func:`_result`, :func:`_grouper`, :func:`_train_front` / :func:`_train_groups` and
``_adjust_front``.

:class:`QuantileDeltaMapping` (``group="time"`` or a sub-grouping: the ranks are then taken inside each group's own steps):
trained like EQM; ``adjust`` looks the factor up at the QUANTILE of every sim value within the sim series itself
(``rank(sim, pct=True)``), so that the simulated change of every quantile is preserved — ``xh_qdm_adjust`` ranks each column
exactly (average ranks, NaN skipped) and interpolates in fp64 ("nearest", "linear"; "cubic" for ``group="time"``: the
not-a-knot spline of the EQM path over the quantile nodes).  :class:`DetrendedQuantileMapping`: ``group="time"`` or a
sub-grouping, with or without a window (with one, the trend is fitted on the centred window mean: ``xh_window_nanmean``),
``Grouper("time", add_dims=...)`` (one trend, fitted on the mean over the pooled members);
with "linear" and a month grouping the scaling is interpolated over the group coordinate like xsdba's ``u.broadcast`` does.

PARITY UNPINNED like everything xsdba (oracle/sdba.py).
"""

from __future__ import annotations

import numpy as np

from . import kernels as K
from ._capi import DeviceArray, get_device
from .calendar import _flatten

ADDITIVE, MULTIPLICATIVE = "+", "*"


class Grouper:
    """xsdba.base.Grouper for the groupings of the quantile-mapping path: ``Grouper("time")``, ``Grouper("time.month")``,
    ``Grouper("time.dayofyear", window=31)``.

    ``add_dims`` (xsdba: "additional dimensions that should be reduced in grouping operations", e.g. the realizations of an
    ensemble — /root/reference/docs/sdba.rst:64-66): the host mirrors take numpy arrays, so the dimensions are AXIS NUMBERS of
    the training arrays and must be the axes right behind time (``add_dims=1`` or ``(1, 2)``): their samples are pooled with
    the time steps of a group when the quantiles are taken (``nbutils.quantile(ds.ref, quantiles, dim)`` with
    ``dim = [time, (window), *add_dims]``), the factors have no such axis, and ``adjust`` maps every member of a ``sim`` that
    still has it with the same factors."""

    def __init__(self, group: str = "time", window: int = 1, add_dims=None):
        if isinstance(group, Grouper):
            group, window, add_dims = group.name, group.window, group.add_dims if add_dims is None else add_dims
        if group not in ("time", "time.month", "time.dayofyear", "time.season"):
            raise NotImplementedError(f"group={group!r}: supported are 'time', 'time.month', 'time.dayofyear', 'time.season'")
        if window < 1 or window % 2 == 0:
            raise ValueError("window must be a positive odd number of time steps")
        if group == "time" and window != 1:
            raise ValueError("a window needs a sub-grouping ('time.month' / 'time.dayofyear')")
        self.name, self.window = group, int(window)
        self.prop = group.split(".")[1] if "." in group else "group"
        dims = () if add_dims is None else tuple(int(a) for a in np.atleast_1d(add_dims))
        if dims != tuple(range(1, len(dims) + 1)):
            raise NotImplementedError(f"add_dims={add_dims!r}: the pooled axes must be the ones right behind time (1, 2, ...): "
                                      "move them there (np.moveaxis) first")
        self.add_dims = dims

    def __repr__(self):
        extra = f", add_dims={self.add_dims}" if self.add_dims else ""
        return f"Grouper(name={self.name!r}, window={self.window}{extra})"

    def pool(self, dev, x: DeviceArray, cell_shape):
        """(T, R * C) field whose leading cell axes are ``add_dims`` -> ((T * R, C) view, R, cell shape without them): row
        ``t * R + r`` is member ``r`` of step ``t`` — the C-contiguous layout already is that matrix."""
        k = len(self.add_dims)
        if k == 0:
            return x, 1, tuple(cell_shape)
        if len(cell_shape) < k:
            raise ValueError(f"add_dims={self.add_dims}: the array has no such axes (shape behind time: {tuple(cell_shape)})")
        R = int(np.prod(cell_shape[:k]))
        cells = tuple(cell_shape[k:])
        C_ = int(np.prod(cells)) if cells else 1
        return x.reshape(x.shape[0] * R, C_), R, cells   # (a view that keeps its parent alive: the caller drops `x`)

    def _ring(self, time):
        """``(tb, rows_at)`` when the samples of consecutive day-of-year groups form a ring — a window, and every year holds every
        day (noleap, 360_day ...) — else None.  ``tb``: the (years, doys) table of time steps; ``rows_at(d, off)``: the rows
        ``tb[:, d] + off`` of every year, -1 beyond the series."""
        if not (self.prop == "dayofyear" and self.window > 1):
            return None
        tb = np.asarray(time.doy_table()[0], dtype=np.int64)      # (years, doys) -> time index
        if not (tb.shape[1] == len(self.labels(time)) and tb.shape[1] > 1 and tb.min() >= 0
                and bool((tb[:, 1:] == tb[:, :-1] + 1).all())):
            return None
        T = len(time)

        def rows_at(d, off):
            r = tb[:, d] + off
            return np.where((r < 0) | (r >= T), -1, r)

        return tb, rows_at

    def group_samples(self, dev, fields, time, R: int = 1):
        """For every group (in label order) the training sample of each field of ``fields`` ((T * R, C) device matrices) as a
        (rows, C) device matrix: the gathered rows of :meth:`sample_rows`.  The matrices of one group are only valid until the
        next one is asked for.

        Day-of-year groups with a window on a series where every year holds every day (noleap, 360_day ...): the sample of
        day d + 1 is the sample of day d with ONE row per year replaced (the order of a sample's rows does not matter), so
        the matrix is kept as a ring — ``window`` slots per year — and 1 / window of it is gathered per group (30 years,
        window 31: 930 rows -> 30)."""
        ring = self._ring(time) if R == 1 else None
        if ring is None:
            for g, rows in enumerate(self.sample_rows(time)):
                rows = self.pooled_rows(rows, R)
                yield g, [K.select_rows(dev, f, rows) for f in fields]
            return
        tb, rows_at = ring
        W, half, ny = self.window, self.window // 2, tb.shape[0]
        bufs = [dev.empty((ny * W, f.shape[1]), np.float32) for f in fields]
        first = np.full(ny * W, -1, dtype=np.int64)
        for off in range(-half, half + 1):
            first[np.arange(ny) * W + (off % W)] = rows_at(0, off)       # slot of day d + off: (d + off) mod W, d = 0
        for f, b in zip(fields, bufs):
            K.select_rows(dev, f, first, out=b)
        yield 0, bufs
        for d in range(1, tb.shape[1]):
            new = rows_at(d, half)                                        # day d + half enters, day d - 1 - half leaves: same slot
            for f, b in zip(fields, bufs):
                K.select_rows(dev, f, new, out=b, out_row=(d + half) % W, out_stride_rows=W)
            yield d, bufs

    def ring_schedule(self, time):
        """The sliding form of the day-of-year samples (see :meth:`group_samples`): ``(rows0, enter, leave)`` — the time steps of
        group 0's sample (years x window, -1 beyond the series) and, per step from group d to d + 1, the steps that enter and
        leave (one per year) — or None when the grouping is not a ring (no window, another property, calendar gaps)."""
        ring = self._ring(time)
        if ring is None:
            return None
        tb, rows_at = ring
        half = self.window // 2
        rows0 = np.concatenate([rows_at(0, off) for off in range(-half, half + 1)])
        enter = np.stack([rows_at(d, half) for d in range(1, tb.shape[1])])
        leave = np.stack([rows_at(d - 1, -half) for d in range(1, tb.shape[1])])
        return rows0, enter, leave

    def sliding_stretches(self, time, max_per: int = 64, cap: int = 1024, min_len: int = 8):
        """The general form of :meth:`ring_schedule` for calendars with gaps (leap days: the standard calendar): from the groups'
        sample rows, the stretches of CONSECUTIVE groups whose samples differ by at most ``max_per`` rows each way —
        ``[(g0, rows0, enter, leave), ...]`` with ``enter`` / ``leave`` of shape (groups - 1, per), -1 padded — and the groups
        no stretch covers (day 366 of a standard calendar: only the leap years have it, its sample shares little with its
        neighbours').  A gap-free calendar gives one stretch with the rows of :meth:`ring_schedule`."""
        ring = self.ring_schedule(time)
        rows_of = None
        if ring is not None:
            return [(0,) + ring], [], rows_of
        if not (self.prop == "dayofyear" and self.window > 1):
            return [], None, rows_of
        rows_of = self.sample_rows(time)
        sets = [np.unique(r[r >= 0]) for r in rows_of]
        G = len(sets)
        ent = [np.setdiff1d(sets[g + 1], sets[g], assume_unique=True) for g in range(G - 1)]
        lev = [np.setdiff1d(sets[g], sets[g + 1], assume_unique=True) for g in range(G - 1)]
        ok = [max(len(ent[g]), len(lev[g])) <= max_per and len(sets[g]) <= cap and len(sets[g + 1]) <= cap for g in range(G - 1)]
        stretches, covered, g = [], np.zeros(G, dtype=bool), 0
        while g < G - 1:
            if not ok[g]:
                g += 1
                continue
            e = g
            while e < G - 1 and ok[e]:
                e += 1
            if e - g + 1 >= min_len:   # groups g .. e
                per = max(1, max(max(len(ent[k]), len(lev[k])) for k in range(g, e)))
                en = np.full((e - g, per), -1, dtype=np.int64)
                lv = np.full((e - g, per), -1, dtype=np.int64)
                for k in range(g, e):
                    en[k - g, :len(ent[k])] = ent[k]
                    lv[k - g, :len(lev[k])] = lev[k]
                # The cap above counts the VALID rows, the kernel's limit is on the list it is handed: where the -1 padding of a
                # series end takes the list beyond it (17 years x window 61: 1037 entries, 1024 valid rows) the valid rows alone
                # are passed — else the kernel declines and every group is silently redone from its gathered sample.  A list
                # within the limit goes on as it is, padding included (the kernel skips -1): the recorded launch plans of
                # tests/golden/sdba_plans.json hold those lists byte for byte
                rows0 = rows_of[g] if len(rows_of[g]) <= cap else rows_of[g][rows_of[g] >= 0]
                stretches.append((g, rows0, en, lv))
                covered[g:e + 1] = True
            g = e + 1
        return stretches, [int(k) for k in np.nonzero(~covered)[0]], rows_of

    @staticmethod
    def pooled_rows(rows: np.ndarray, R: int) -> np.ndarray:
        """Sample rows of the time axis -> rows of the pooled (T * R, C) matrix (-1 stays -1, R times)."""
        if R == 1:
            return rows
        out = rows[:, None] * R + np.arange(R)[None, :]
        out[rows < 0] = -1
        return out.reshape(-1)

    _SEASON_OF_MONTH = np.array(["", "DJF", "DJF", "MAM", "MAM", "MAM", "JJA", "JJA", "JJA", "SON", "SON", "SON", "DJF"])

    def values(self, time) -> np.ndarray:
        """The group coordinate of every time step: month, day of year, or the season name (``time.dt.season``)."""
        if self.prop == "month":
            return np.asarray(time.month)
        if self.prop == "season":
            return self._SEASON_OF_MONTH[np.asarray(time.month)]
        return np.asarray(time.doy)

    def coordinate(self, time, interp: bool = False) -> np.ndarray:
        """xsdba ``Grouper.get_index(da, interp=...)``: the group coordinate of every time step as float64.  With
        ``interp=True`` (every interpolation but "nearest") the month becomes fractional — ``month - 0.5 + day /
        days_in_month``, the middle of a month on its integer — and the day of year stays an integer."""
        if self.prop == "month" and interp:
            return time.month - 0.5 + time.day / time.days_in_month()
        if self.prop in ("month", "dayofyear"):
            return np.asarray(self.values(time), dtype=np.float64)
        raise NotImplementedError(f"group coordinate of {self.name!r}")

    def labels(self, time) -> np.ndarray:
        """Group coordinate values present on `time` (months 1..12 / days of year / season names), sorted like xarray's
        groupby sorts them (the seasons alphabetically: DJF, JJA, MAM, SON)."""
        if self.prop == "group":
            return np.array([0])
        return np.unique(self.values(time))

    def index(self, time, labels=None) -> np.ndarray:
        """Position of every time step's group in `labels` (default: the labels of `time`); -1 when absent."""
        if self.prop == "group":
            return np.zeros(len(time), dtype=np.int64)
        lab = self.labels(time) if labels is None else np.asarray(labels)
        val = self.values(time)
        pos = np.clip(np.searchsorted(lab, val), 0, len(lab) - 1)
        return np.where(lab[pos] == val, pos, -1)

    def small_groups(self, time, most: int = 64):
        """``(rows, offs)`` — the time steps of group 0, then of group 1, ... and where each group starts — for a sub-grouping
        WITHOUT a window whose groups hold at most ``most`` steps (a day-of-year grouping: one per year), else None: the
        shape of the one-launch training kernels (xh_eqm_train_groups)."""
        if self.prop == "group" or self.window != 1:
            return None
        lay = _GroupMajor(self.index(time), len(self.labels(time)))
        return None if lay.counts.max(initial=0) > most else (lay.perm.astype(np.int64), lay.offs)

    def sample_rows(self, time) -> list:
        """For every group the rows of its training sample: the centred window around each of its time steps, -1 (NaN)
        beyond the ends of the series — rolling(time=window, center=True).construct + groupby in xsdba."""
        T = len(time)
        gi = self.index(time)
        half = self.window // 2
        off = np.arange(-half, half + 1)
        out = []
        for g in range(len(self.labels(time))):
            t = np.nonzero(gi == g)[0]
            rows = (t[:, None] + off[None, :]).reshape(-1)
            rows[(rows < 0) | (rows >= T)] = -1
            out.append(rows.astype(np.int64))
        return out


def _check_group_interp(group: "Grouper", interp: str, who: str, labels=None, extrapolation: str = "constant") -> None:
    """Sub-groupings interpolate over the (quantile, group) PLANE in xsdba when interp != "nearest"
    (``utils.interp_on_quantiles`` -> ``_interp_on_quantiles_2D`` = ``scipy.interpolate.griddata``).  Built: "linear"
    (Delaunay interpolation, ``xh_plane_linear``) for month / day-of-year groupings whose labels are 1 .. G, with
    ``extrapolation="constant"``.  Refused loudly: "cubic" (griddata's Clough-Tocher scheme estimates gradients by a global
    iteration over the whole triangulation), "time.season" (upstream's season coordinate is not restated),
    ``extrapolation="nan"`` with "linear" (upstream then skips its extrapolation step and keeps griddata's own NaN outside
    the convex hull of ALL nodes — a different region than the per-group bounds)."""
    if group.prop == "group" or interp == "nearest":
        return
    if interp == "cubic":
        raise NotImplementedError(
            f"{who}: interp='cubic' with group={group.name!r} is scipy griddata's Clough-Tocher interpolation over the "
            "(quantile, group) plane in xsdba — not built; use 'linear' or 'nearest' (or group='time')")
    lab = None if labels is None else np.asarray(labels)
    if group.prop not in ("month", "dayofyear") or lab is None or not np.array_equal(lab, np.arange(1, len(lab) + 1)):
        raise NotImplementedError(
            f"{who}: interp={interp!r} over the (quantile, group) plane is built for 'time.month' / 'time.dayofyear' groupings "
            f"whose labels are 1 .. G (got group={group.name!r})")
    if extrapolation != "constant":
        raise NotImplementedError(
            f"{who}: interp={interp!r} with a sub-grouping is built for extrapolation='constant' (with 'nan' xsdba keeps "
            "griddata's NaN outside the convex hull of all nodes)")


class _GroupMajor:
    """The group-major layout of T rows with group index ``gi`` (every entry in 0 .. G - 1: callers refuse or never produce a
    -1): ``perm`` lists the rows group after group (in time order inside a group: a stable sort), ``counts`` / ``offs``
    (G + 1) say where each group lies in it.  Iterating yields ``(g, off, n)`` for the non-empty groups; the rows
    [off, off + n) of a group-major (T, C) matrix are ``_group(x, off, n)``."""

    def __init__(self, gi, G: int):
        self.perm = np.argsort(gi, kind="stable")
        self.counts = np.bincount(gi, minlength=G)
        self.offs = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    def __iter__(self):
        return ((g, int(self.offs[g]), int(n)) for g, n in enumerate(self.counts) if n)

    def rows(self, off: int, n: int) -> np.ndarray:
        """The time steps of the block [off, off + n)."""
        return self.perm[off:off + n]

    def gather(self, dev, x: DeviceArray) -> DeviceArray:
        """A (T, C) field in time order -> group-major."""
        return K.select_rows(dev, x, self.perm)

    def scatter(self, dev, x: DeviceArray) -> DeviceArray:
        """A group-major (T, C) result -> time order (a gather by the inverse permutation)."""
        inv = np.empty(len(self.perm), dtype=np.int64)
        inv[self.perm] = np.arange(len(self.perm))
        return K.select_rows(dev, x, inv)


def _group(tab: DeviceArray, g: int, n: int | None = None) -> DeviceArray:
    """Group ``g`` of a (G, ..., C) device table as a (..., C) view — with ``n`` the groups g .. g + n - 1 as (n, ..., C), which
    for a (T, C) matrix are its rows [g, g + n).  The one place where a view is cut out of a buffer by pointer arithmetic; it keeps its buffer alive."""
    step = int(np.prod(tab.shape[1:], dtype=np.int64)) * tab.dtype.itemsize
    view = tab.dev.wrap(tab.ptr + g * step, tab.shape[1:] if n is None else (n,) + tab.shape[1:], tab.dtype)
    view._owner = tab
    return view


def _result(scen: DeviceArray, keep: bool, shape, sync: bool = False):
    """What a public call returns: the device array (``keep``) or its host copy in the caller's shape.  ``sync``: wait for
    the device first (every sub-grouping path does; ``group="time"`` is one launch and the download orders itself)."""
    if sync:
        scen.dev.sync()
    return scen if keep else scen.get().reshape(shape)


def _tile_members(dev, tab: DeviceArray, E: int) -> DeviceArray:
    """(..., C) -> (..., E * C): row i of the (rows, C) view repeated E times IS row i of (rows, E * C)."""
    lead, C_ = int(np.prod(tab.shape[:-1])), tab.shape[-1]
    out = K.select_rows(dev, tab.reshape(lead, C_), np.repeat(np.arange(lead), E))
    return out.reshape(*(tuple(tab.shape[:-1]) + (E * C_,)))


def equally_spaced_nodes(n: int, eps=None) -> np.ndarray:
    """xsdba.utils.equally_spaced_nodes: n nodes q_i = (i + 1/2) / n; with ``eps`` the end points eps and 1 - eps are
    added (n + 2 nodes), so that the adjustment factors are also defined near the ends of the distribution."""
    dq = 1.0 / n / 2.0
    q = np.linspace(dq, 1.0 - dq, n)
    if eps is None:
        return q
    return np.insert(np.append(q, 1.0 - eps), 0, eps)


def quantile(da, q, dim="time", *, device=None, keep=False):
    """xsdba.nbutils.quantile along time: (nq, *cells) in float32."""
    if dim != "time":
        raise NotImplementedError("quantile: only dim='time' (axis 0) is supported on the HIP path")
    dev = device or get_device()
    x, cell_shape = _flatten(da, dev)
    out = K.quantile_series(dev, x, np.asarray(q, dtype=np.float64))
    return _result(out, keep, (out.shape[0],) + tuple(cell_shape))


def _grouper(group, window) -> Grouper:
    return group if isinstance(group, Grouper) else Grouper(group, 1 if window is None else window)


def _train_front(grp, ref, hist, kind, nquantiles, time, device, adapt_freq_thresh=None, adapt_freq_seed=0):
    """What ``train`` does before any arithmetic: the kind, both fields flattened to (T, cells) and compared, the quantile
    nodes, the members of ``grp.add_dims`` pooled with the time steps (rows t * R + r of a (T * R, C) view), and — for a
    sub-grouping — the ``time`` axis.  ``adapt_freq_thresh``: hist goes through :func:`adapt_freq` against ref first.
    Returns ``(dev, ref, hist, cell shape, R, nodes)``."""
    if kind not in (ADDITIVE, MULTIPLICATIVE):
        raise ValueError(f"kind must be '+' or '*', got {kind!r}")
    dev = device or get_device()
    r, cell_shape = _flatten(ref, dev)
    h, cell_shape_h = _flatten(hist, dev)
    if tuple(cell_shape) != tuple(cell_shape_h) or r.shape != h.shape:
        raise ValueError("ref and hist must have the same shape")  # _check_matching_time_sizes analogue
    if adapt_freq_thresh is not None:
        if grp.add_dims:
            raise NotImplementedError("adapt_freq_thresh with Grouper(add_dims=...) is not built")
        h, _, _ = adapt_freq(r, h, adapt_freq_thresh, group=grp, time=time, seed=adapt_freq_seed, device=dev, keep=True)
    q = equally_spaced_nodes(nquantiles) if np.isscalar(nquantiles) else np.asarray(nquantiles, dtype=np.float64)
    T = r.shape[0]
    r, R, cells = grp.pool(dev, r, cell_shape)
    h, _, _ = grp.pool(dev, h, cell_shape_h)
    if grp.prop != "group" and (time is None or len(time) != T):
        raise ValueError(f"group={grp.name!r} needs time=TimeAxis of the training series")
    return dev, r, h, cells, R, q


def adapt_freq(ref, sim, thresh: float, *, group="time", window: int | None = None, time=None, seed: int = 0, device=None,
               keep=False):
    """xsdba.processing.adapt_freq (``_processing._adapt_freq``, Themeßl et al. 2012): adapt the frequency of values
    ``<= thresh`` in ``sim`` to that of ``ref`` — the pre-processing a multiplicative quantile mapping of precipitation
    needs when the model has too many dry days.  Per cell and group:

        P0 = count(x <= thresh) / count(valid)   for sim and ref (over the group's windowed sample)
        dP0 = (P0_sim - P0_ref) / P0_sim         the share of sim's values <= thresh that has to become wet
        pth = quantile(ref, P0_sim)  where dP0 > 0  (``nbutils.vecquantiles``: the value of ref at sim's dry-day rank)
        sim_ad = sim, except: where dP0 >= 0 the samples whose percentage rank (average ranks over the group's own time
                 steps) lies in [P0_ref, P0_sim] get a uniform random value in [thresh, pth)

    Returns ``(sim_ad, pth, dP0)``: sim_ad float32 in the shape of sim, pth / dP0 per cell (``(groups, *cells)`` with a
    sub-grouping).  ``thresh`` in the units of the data.  The random numbers: upstream draws from numpy's global
    generator (not reproducible across runs); here a counter-based uniform keyed by ``(seed, time step, cell)`` —
    ``xh_adapt_freq``, restated in oracle/sdba.py.  ``ref`` and ``sim`` need the same number of time steps only with a
    sub-grouping (one ``time`` axis for both).  Parity unpinned (xsdba is not in the reference tree)."""
    grp = _grouper(group, window)
    if grp.add_dims:
        raise NotImplementedError("adapt_freq with Grouper(add_dims=...) is not built")
    dev = device or get_device()
    r, cell_shape = _flatten(ref, dev)
    s_, cell_shape_s = _flatten(sim, dev)
    if tuple(cell_shape) != tuple(cell_shape_s):
        raise ValueError("ref and sim must have the same grid")
    T, C_ = s_.shape
    thresh = float(thresh)

    def one_group(ref_sample, sim_sample, sim_main, tindex, out):
        """P0 / dP0 / pth from the (windowed) samples, the replacement on the group's own steps"""
        def p0(x):
            seg = np.array([0, x.shape[0]], dtype=np.int64)
            cnt, val = K.threshold_count(dev, x, "<=", seg, scalar=thresh)
            cnt, val = cnt.get()[0].astype(np.float64), val.get()[0].astype(np.float64)
            with np.errstate(all="ignore"):
                return cnt / val
        p0_sim, p0_ref = p0(sim_sample), p0(ref_sample)
        with np.errstate(all="ignore"):
            dp0 = (p0_sim - p0_ref) / p0_sim
        pth = K.quantile_cells(dev, ref_sample, p0_sim).get()
        pth = np.where(dp0 > 0, pth, np.float32(np.nan)).astype(np.float32)
        K.adapt_freq(dev, sim_main, p0_ref, p0_sim, dp0, pth, thresh, seed, tindex=tindex, out=out)
        return pth, dp0

    if grp.prop == "group":
        out = dev.empty(tuple(s_.shape), np.float32)
        pth, dp0 = one_group(r, s_, s_, None, out)
        return _result(out, keep, (T,) + tuple(cell_shape)), pth.reshape(cell_shape), dp0.reshape(cell_shape)
    if time is None or len(time) != T or r.shape[0] != T:
        raise ValueError(f"group={grp.name!r} needs time=TimeAxis common to ref and sim")
    # group-major blocks (every group's own steps contiguous), one gather back at the end — like the grouped adjust
    G = len(grp.labels(time))
    lay = _GroupMajor(grp.index(time), G)
    s_perm = lay.gather(dev, s_)
    ad_perm = dev.empty((T, C_), np.float32)
    rows_of = grp.sample_rows(time)
    pths, dp0s = [], []
    for g, off, n in lay:
        pth, dp0 = one_group(K.select_rows(dev, r, rows_of[g]), K.select_rows(dev, s_, rows_of[g]), _group(s_perm, off, n),
                             lay.rows(off, n), _group(ad_perm, off, n))
        pths.append(pth)
        dp0s.append(dp0)
    res = _result(lay.scatter(dev, ad_perm), keep, (T,) + tuple(cell_shape), sync=True)
    return res, np.stack(pths).reshape((G,) + tuple(cell_shape)), np.stack(dp0s).reshape((G,) + tuple(cell_shape))


def _dqm_train_sample(dev, rg, hg, q, kind, out=None):
    """dqm_train on one sample: ``(af, hist_q, scaling)`` — the tables of the series normalised by their means, and
    scaling = get_correction(mu_hist, mu_ref): a (C,) HOST table — O(C) arithmetic on the two mean vectors."""
    inv = "-" if kind == ADDITIVE else "/"
    mu_r, _ = K.poly_trend(dev, rg, 0)
    mu_h, _ = K.poly_trend(dev, hg, 0)
    af, hq = K.eqm_train(dev, K.trend_apply(dev, rg, mu_r, None, inv), K.trend_apply(dev, hg, mu_h, None, inv), q, kind, out=out)
    mr, mh = mu_r.get(), mu_h.get()
    with np.errstate(all="ignore"):
        return af, hq, (mr - mh if kind == ADDITIVE else mr / mh)


def _train_groups(dev, grp, time, r, h, q, kind, R: int = 1, normalised: bool = False):
    """The training of a sub-grouping: ``(af, hist_q, scaling)`` as (G, nq, C) float32 / (G, C) float64 device tables.
    ``normalised`` (dqm_train): every sample is normalised by its own mean first and ``scaling`` is returned (else None).
    Three routes, all bit-identical to the last one: all (small) groups in one launch, a sorted window that slides from one
    day of the year to the next, the gathered sample of every group.  None for a normalised training WITHOUT a window whose
    groups are too large for the one launch: the caller has a cheaper route than the gathered samples for it."""
    small = grp.small_groups(time) if R == 1 else None
    if small is not None:
        # no window, small groups (365 days of the year x one row per year): all groups in ONE launch per field, keys in
        # registers (xh_eqm_train_groups, round 6: 121 -> ~10 ms for 30 years x 1440 x 90; xh_dqm_train_groups: 470 -> ~10 ms)
        res = K.eqm_train_groups(dev, r, h, small[0], small[1], q, kind, normalised=normalised)
        if res is not None:
            dev.sync()
            return res[0], res[1], (res[2] if normalised else None)
    if normalised and grp.window == 1:
        return None
    G, nq, C_ = len(grp.labels(time)), len(q), r.shape[1]
    af = dev.empty((G, nq, C_), np.float32)
    hq = dev.empty((G, nq, C_), np.float32)

    def sample(g, rg, hg):  # the tables of group g from its gathered sample; normalised: its scaling row (host)
        out = (_group(af, g), _group(hq, g))
        if normalised:
            return _dqm_train_sample(dev, rg, hg, q, kind, out)[2]
        K.eqm_train(dev, rg, hg, q, kind, out=out)

    stretches, rest, rows_of = grp.sliding_stretches(time) if R == 1 else ([], None, None)
    if stretches:
        # day-of-year groups with a window: every cell keeps its window sorted from one day to the next (xh_eqm_train_window,
        # round 6: 508 -> ~60 ms for 30 years x 1440 x 90).  Normalised, the sorted window also carries the mean of every
        # group's sample and normalises the samples it picks (xh_dqm_train_window: 3 970 -> ~190 ms; per group otherwise: a
        # gather, two means, two normalisations, two selections and a host round trip of the means)
        scal_d, muh = (dev.empty((G, C_), np.float64), dev.empty((G, C_), np.float64)) if normalised else (None, None)
        done = True
        for g0, rows0, en, lv in stretches:
            n = en.shape[0] + 1
            out = (_group(af, g0, n), _group(hq, g0, n)) + ((_group(scal_d, g0, n), _group(muh, g0, n)) if normalised else ())
            if K.eqm_train_window(dev, r, h, rows0, en, lv, q, kind, normalised=normalised, out=out) is None:
                done = False   # (not the kernel's shape after all: everything through the per-group path below)
                break
        if done:
            for g in rest:     # the groups no stretch covers (day 366 of a standard calendar): from their gathered sample
                sg = sample(g, K.select_rows(dev, r, rows_of[g]), K.select_rows(dev, h, rows_of[g]))
                if normalised:
                    row = dev.to_device(np.ascontiguousarray(sg), dtype=np.float64)
                    dev.copy_d2d(_group(scal_d, g).ptr, row.ptr, C_ * 8)
            dev.sync()
            return af, hq, scal_d
    scal = np.empty((G, C_), np.float64) if normalised else None
    for g, (rg, hg) in grp.group_samples(dev, (r, h), time, R):
        sg = sample(g, rg, hg)
        if normalised:
            scal[g] = sg
    dev.sync()
    return af, hq, (dev.to_device(scal, dtype=np.float64) if normalised else None)


class EmpiricalQuantileMapping:
    """Empirical quantile mapping bias adjustment (train on ref/hist quantiles, adjust sim by node search)."""

    def __init__(self, dev, af: DeviceArray, hist_q: DeviceArray, quantiles, kind, cell_shape, group=None, labels=None):
        self._dev = dev
        self._af, self._hist_q = af, hist_q
        self.quantiles = np.asarray(quantiles)
        self.kind = kind
        self.cell_shape = tuple(cell_shape)
        self.group = group or Grouper("time")
        self.group_labels = np.array([0]) if labels is None else np.asarray(labels)
        self.adj_params = {"group": self.group.name if self.group.window == 1 else repr(self.group), "kind": kind,
                           "nquantiles": len(self.quantiles)}

    def _member_axes(self, sim):
        """The extra axes of a ``sim`` right behind time — the members that ``Grouper(add_dims=...)`` pooled in training, or any
        other axis the factors do not have (xsdba: the factors broadcast against it in ``interp_on_quantiles``).  None when
        sim has the trained shape (or one that fits in no way: the grid check refuses it)."""
        shp = tuple(sim.shape[1:])
        n = len(self.cell_shape)
        if shp == self.cell_shape or len(shp) <= n or (n and shp[len(shp) - n:] != self.cell_shape):
            return None
        return shp[:len(shp) - n]

    def _member_model(self, extra):
        """The model whose tables are repeated for every member, so that the (time, members x cells) matrix goes through the
        same kernels."""
        cache = self.__dict__.setdefault("_member_models", {})
        if extra not in cache:
            E = int(np.prod(extra))
            cache[extra] = type(self)(self._dev, _tile_members(self._dev, self._af, E), _tile_members(self._dev, self._hist_q, E),
                                      self.quantiles, self.kind, extra + self.cell_shape, self.group,
                                      None if self.group.prop == "group" else self.group_labels)
        return cache[extra]

    def _adjust_front(self, sim, interp, extrapolation, time, *, grouped_nearest="griddata", detrend=1, dqm_order=False,
                      untrained="sim holds time steps whose group was not trained (e.g. day 366 with a 365-day training set)"):
        """What every ``adjust`` checks before it launches anything.  Returns ``(extra, s, gi)``: the member axes of a sim that
        has some (then s and gi are None: the caller maps the members), else the flattened sim and — for a sub-grouping — the
        group index of every time step, all of them trained.  ``dqm_order``: DetrendedQuantileMapping looks at the (quantile,
        group) interpolation only after the grid, and maps members itself only for ``group="time"``."""
        who = f"{type(self).__name__}.adjust"
        if interp not in ("nearest", "linear", "cubic"):
            raise ValueError(f"interp={interp!r} not in ('nearest', 'linear', 'cubic')")
        if grouped_nearest not in ("griddata", "group"):
            raise ValueError("grouped_nearest must be 'griddata' or 'group'")
        if detrend not in (0, 1):
            raise NotImplementedError(f"{who}: detrend must be 0 or 1 (polynomial degree)")
        if not dqm_order:
            _check_group_interp(self.group, interp, who, self.group_labels, extrapolation)
        extra = self._member_axes(sim)
        if extra is not None and (self.group.prop == "group" or not dqm_order):
            return extra, None, None
        s, cell_shape = _flatten(sim, self._dev)
        if tuple(cell_shape) != self.cell_shape:
            raise ValueError("sim does not match the trained grid")
        if self.group.prop == "group":
            return None, s, None
        if dqm_order:
            _check_group_interp(self.group, interp, who, self.group_labels, extrapolation)
        if time is None or len(time) != s.shape[0]:
            raise ValueError(f"group={self.group.name!r} needs time=TimeAxis of sim")
        gi = self.group.index(time, self.group_labels)
        if (gi < 0).any():
            raise ValueError(untrained)
        return None, s, gi

    @classmethod
    def train(cls, ref, hist, *, nquantiles=20, kind: str = ADDITIVE, group="time", window: int | None = None, time=None,
              device=None, adapt_freq_thresh: float | None = None, adapt_freq_seed: int = 0):
        """``group``: "time" (default), "time.month", "time.dayofyear" or a :class:`Grouper`; sub-groupings need the
        common ``time`` axis (TimeAxis) of ref and hist.  ``adapt_freq_thresh`` (in the units of the data): hist goes
        through :func:`adapt_freq` against ref (same grouping) before the quantiles are taken — xsdba's
        ``EmpiricalQuantileMapping.train(adapt_freq_thresh=...)`` (``_adjustment.eqm_train`` -> ``_adapt_freq_hist``)."""
        grp = _grouper(group, window)
        dev, r, h, cell_shape, R, q = _train_front(grp, ref, hist, kind, nquantiles, time, device, adapt_freq_thresh, adapt_freq_seed)
        if grp.prop == "group":
            af, hq = K.eqm_train(dev, r, h, q, kind)
            return cls(dev, af, hq, q, kind, cell_shape, grp)
        af, hq, _ = _train_groups(dev, grp, time, r, h, q, kind, R)
        return cls(dev, af, hq, q, kind, cell_shape, grp, grp.labels(time))

    def adjust(self, sim, *, interp: str = "nearest", extrapolation: str = "constant", time=None, keep=False,
               grouped_nearest: str = "griddata"):
        """``grouped_nearest`` (sub-groupings only): "griddata" (default) = what xsdba does — the nearest node in the (hist_q,
        group) PLANE over the nodes of all groups (``_interp_on_quantiles_2D``: a neighbouring group's node wins where the own
        group's nearest node is more than one unit away), own-group factors outside the own group's nodes; "group" = always
        the nearest node of the step's own group (rounds 2-3).  "time.season", groupings whose labels are not 1 .. G and
        models with more than 32 quantile nodes (a warning is raised) take "group" (upstream's season coordinate is not
        restated; the plane kernel keeps a group's nodes in registers).

        ``interp="linear"`` with a month / day-of-year grouping is xsdba's interpolation over the (quantile, group) plane
        (``xh_plane_linear``; :func:`_check_group_interp`): months at their fractional coordinate, days of year on their row."""
        extra, s, gi = self._adjust_front(sim, interp, extrapolation, time, grouped_nearest=grouped_nearest)
        if extra is not None:
            return self._member_model(extra).adjust(sim, interp=interp, extrapolation=extrapolation, time=time, keep=keep,
                                                    grouped_nearest=grouped_nearest)
        dev, shape = self._dev, (s.shape[0],) + self.cell_shape
        if gi is None:
            return _result(K.eqm_adjust(dev, s, self._af, self._hist_q, self.kind, interp, extrapolation), keep, shape)
        if interp == "linear":
            # xsdba's 2-D branch: ONE launch over the whole series, every step at its (fractional) group coordinate
            scen = K.plane_linear(dev, s, self.group.coordinate(time, interp=True), self._af, xq_all=self._hist_q, kind=self.kind)
            return _result(scen, keep, shape, sync=True)
        if self._plane_nearest(grouped_nearest):
            # xsdba's nearest node in the (hist_q, group) plane: ONE launch over the whole series (round 5; rounds 3-4 permuted
            # the rows group-major and launched xh_eqm_adjust_g2d per group: 145 ms against 15 for a 30-year 1440 x 90 band
            # with 365 groups)
            scen = K.plane_nearest(dev, s, gi + 1.0, self._af, self._hist_q, self.kind, extrapolation)
            return _result(scen, keep, shape, sync=True)
        # every step through the nodes of its OWN group: group-major row blocks, one xh_eqm_adjust per group
        lay = _GroupMajor(gi, len(self.group_labels))
        s_perm = lay.gather(dev, s)
        scen_perm = dev.empty(s.shape, np.float32)
        for g, off, n in lay:
            K.eqm_adjust(dev, _group(s_perm, off, n), _group(self._af, g), _group(self._hist_q, g), self.kind, interp, extrapolation,
                         out=_group(scen_perm, off, n))
        return _result(lay.scatter(dev, scen_perm), keep, shape, sync=True)

    def _plane_nearest(self, grouped_nearest: str) -> bool:
        """xsdba's 2-D nearest applies: a month / day-of-year grouping whose labels are 1 .. G (the coordinates upstream's
        add_cyclic_bounds extends to 0 and G + 1) and at most 32 nodes."""
        lab = self.group_labels
        ok = (grouped_nearest == "griddata" and self.group.prop in ("month", "dayofyear")
              and np.array_equal(lab, np.arange(1, len(lab) + 1)))
        if ok and len(self.quantiles) > 32:
            import warnings

            warnings.warn(f"grouped interp='nearest' with {len(self.quantiles)} > 32 quantile nodes: xh_eqm_adjust_g2d keeps a "
                          "group's nodes in registers (<= 32), so every step takes the nearest node of its OWN group "
                          "(grouped_nearest='group') instead of xsdba's nearest node in the (quantile, group) plane",
                          stacklevel=3)
            return False
        return ok

    def _shape(self):
        lead = (len(self.quantiles),) if self.group.prop == "group" else (len(self.group_labels), len(self.quantiles))
        return lead + self.cell_shape

    @property
    def af(self) -> np.ndarray:
        return self._af.get().reshape(self._shape())

    @property
    def hist_q(self) -> np.ndarray:
        return self._hist_q.get().reshape(self._shape())


class QuantileDeltaMapping(EmpiricalQuantileMapping):
    """Quantile delta mapping (xsdba.QuantileDeltaMapping): the same training as EQM (incl. its groupings), the adjustment
    factor of a sim value is taken at ITS quantile in the sim series: ``sim_q = rank(sim, pct=True)``,
    ``af = interp_on_quantiles(sim_q, quantiles, af)``, ``scen = sim (+|*) af``.  With a sub-grouping the ranks are taken
    inside each group's own time steps (xsdba: ``group.apply(rank, sim, main_only=True)`` — the window only widens the
    TRAINING sample) and every step uses the factors of its group ("nearest"), or the factors interpolated over the
    (quantile, group) plane ("linear": see :meth:`adjust`).  ``interp="cubic"`` is built for ``group="time"`` (a spline
    over the quantile nodes, <= 32 of them); with a sub-grouping it is xsdba's 2-D griddata "cubic": refused.

    Series of up to 32768 steps are ranked inside one workgroup (``xh_qdm_adjust``: keys in registers); longer ones
    (1950-2100 daily = 55 152 steps) go through a global sort in column batches (qdm3.hip) — exact, not tuned.  -0.0
    and +0.0 tie, as in
    ``scipy.stats.rankdata``."""

    def adjust(self, sim, *, interp: str = "nearest", extrapolation: str = "constant", time=None, keep=False):
        extra, s, gi = self._adjust_front(sim, interp, extrapolation, time)
        if extra is not None:   # (the ranks are taken along time only — group.apply(rank, sim, main_only=True): per member)
            return self._member_model(extra).adjust(sim, interp=interp, extrapolation=extrapolation, time=time, keep=keep)
        dev, shape = self._dev, (s.shape[0],) + self.cell_shape
        if gi is None and interp == "cubic":
            # interp_on_quantiles(sim_q, quantiles, af, method="cubic"): scipy interp1d(kind="cubic") over the quantile nodes —
            # the rank kernels give sim_q (kind "factor" on a table whose factors are the nodes themselves, "linear": the
            # rank itself inside the node range; outside it the first / last node for "constant" — where the spline returns
            # the end factor exactly as interp1d's fill_value does — or NaN), the not-a-knot spline of the EQM path
            # (xh_eqm_adjust, interp 2) evaluates the factor there, xh_apply_factor puts it onto sim
            if len(self.quantiles) > 32:
                raise NotImplementedError("QuantileDeltaMapping.adjust: interp='cubic' supports at most 32 quantile nodes")
            qrows = dev.to_device(np.repeat(self.quantiles.astype(np.float32)[:, None], s.shape[1], axis=1))
            sim_q = K.qdm_adjust(dev, s, qrows, self.quantiles, "factor", "linear", extrapolation)
            af_t = K.eqm_adjust(dev, sim_q, self._af, qrows, "factor", "cubic", extrapolation)
            return _result(K.apply_factor(dev, s, af_t, self.kind, out=sim_q), keep, shape)
        if gi is None:
            return _result(K.qdm_adjust(dev, s, self._af, self.quantiles, self.kind, interp, extrapolation), keep, shape)
        lay = _GroupMajor(gi, len(self.group_labels))  # group-major: every group one contiguous row block, ranked on its own
        plane = interp == "linear" and self.group.prop == "month"
        if not plane:
            # small groups (a day-of-year grouping: one step per year, up to 64): every group ranked in registers, ONE launch over
            # the series where it lies (xh_qdm_adjust_groups, round 6: 80 -> ~8 ms for 365 groups of a 30-year 1440 x 90 band;
            # the loop below gathers and launches per group) — bit-identical
            scen = K.qdm_adjust_groups(dev, s, lay.perm, lay.offs, self._af, self.quantiles, self.kind, interp, extrapolation)
            if scen is not None:
                return _result(scen, keep, shape, sync=True)
        s_perm = lay.gather(dev, s)
        scen_perm = dev.empty(s.shape, np.float32)
        # "linear" over the (quantile, group) plane (xsdba: interp_on_quantiles(sim_q, quantiles, af) with the quantile
        # nodes THEMSELVES as abscissa, the same in every group: a regular grid).  Day of year: the group coordinate is an
        # integer, every query lies ON its group's row, and the row's edges belong to every Delaunay triangulation of a grid
        # whose node spacing (1 / nq) is below the row spacing (1) — the plane interpolation IS the 1-D linear interpolation
        # inside the own group: the loop below.  Month: the coordinate is fractional; the percentage ranks come from the
        # same rank kernels (kind "factor" on a table whose "factors" are the nodes themselves: sim_q clamped to the node
        # range, which is all the plane needs — outside it the row-interpolated end factor applies), then one plane launch.
        qrows = None
        if plane:
            qrows = dev.to_device(np.repeat(self.quantiles.astype(np.float32)[:, None], s.shape[1], axis=1))
        for g, off, n in lay:
            blk, out = _group(s_perm, off, n), _group(scen_perm, off, n)
            if plane:
                K.qdm_adjust(dev, blk, qrows, self.quantiles, "factor", "linear", "constant", out=out)
            else:
                K.qdm_adjust(dev, blk, _group(self._af, g), self.quantiles, self.kind, interp, extrapolation, out=out)
        scen = lay.scatter(dev, scen_perm)
        if plane:  # scen holds sim_q so far
            scen = K.plane_linear(dev, scen, self.group.coordinate(time, interp=True), self._af, xq_common=self.quantiles, base=s,
                                  kind=self.kind)
        return _result(scen, keep, shape, sync=True)


class DetrendedQuantileMapping(EmpiricalQuantileMapping):
    """Detrended quantile mapping (xsdba.DetrendedQuantileMapping; Cannon et al. 2015).  ``group="time"``, or a
    sub-grouping ("time.month", "time.season", "time.dayofyear": everything below happens per group, the trend is fitted
    over the group's own steps on their time coordinate; with a ``window`` the training sample of a group is the windowed
    one and the trend is fitted on the centred window mean of the scaled series, as ``PolyDetrend`` does).

    train (``dqm_train``): ref and hist are normalised by their time means (``x - mean`` for "+", ``x / mean`` for "*"),
    ``af`` / ``hist_q`` come from the quantiles of the NORMALISED series, ``scaling = mean(ref) - mean(hist)`` (resp. the
    ratio).  adjust (``dqm_adjust``): ``sim`` is shifted by ``scaling``, its polynomial trend of degree ``detrend`` (0 or 1,
    ``PolyDetrend``: least squares over the valid steps) is removed, the detrended series goes through the EQM node
    lookup, the trend is put back.  Every stage is float32 on the device with float64 arithmetic inside the kernels
    (means, fit, trend evaluation).  PARITY UNPINNED (oracle/sdba.py: dqm_*)."""

    def __init__(self, *args, scaling=None, **kw):
        super().__init__(*args, **kw)
        self._scaling = scaling  # (C,) float64 device array

    @classmethod
    def train(cls, ref, hist, *, nquantiles=20, kind: str = ADDITIVE, group="time", window=None, time=None, device=None):
        # Grouper(add_dims=...): means and quantiles over the time steps AND the members (ds.ref.mean(dim), dim = [time, *add_dims])
        grp = _grouper(group, window)
        if grp.add_dims and grp.prop != "group":
            raise NotImplementedError("DetrendedQuantileMapping with Grouper(add_dims=...) is built for group='time' only")
        dev, r, h, cell_shape, _, q = _train_front(grp, ref, hist, kind, nquantiles, time, device)

        def model(af, hq, scaling, labels=None):
            if not isinstance(scaling, DeviceArray):
                scaling = dev.to_device(np.ascontiguousarray(scaling), dtype=np.float64)
            return cls(dev, af, hq, q, kind, cell_shape, grp, labels, scaling=scaling)

        if grp.prop == "group":
            return model(*_dqm_train_sample(dev, r, h, q, kind))
        labels = grp.labels(time)
        res = _train_groups(dev, grp, time, r, h, q, kind, normalised=True)
        if res is not None:
            return model(*res, labels)
        # no window: every step is in exactly one group, so the group means are ONE xh_poly_trend_groups per field over the
        # series where it lies (summed in time order: what xh_poly_trend gives on the gathered block), the normalisation is
        # ONE xh_trend_apply_groups per field, and the tables are the grouped EQM training of the normalised series —
        # bit-identical to the per-group samples (month groups of a 30-year 1440 x 90 band: 128 -> ~40 ms)
        inv = "-" if kind == ADDITIVE else "/"
        lay = _GroupMajor(grp.index(time, labels), len(labels))
        zero_u = dev.zeros((r.shape[0],), np.float64)
        mu_r, _ = K.poly_trend_groups(dev, r, lay.perm, lay.offs, zero_u, 0)
        mu_h, _ = K.poly_trend_groups(dev, h, lay.perm, lay.offs, zero_u, 0)
        rn = K.trend_apply_groups(dev, r, lay.perm, lay.offs, mu_r, None, inv)
        hn = K.trend_apply_groups(dev, h, lay.perm, lay.offs, mu_h, None, inv)
        eq = EmpiricalQuantileMapping.train(rn, hn, nquantiles=q, kind=kind, group=grp, time=time, device=dev)
        mr, mh = mu_r.get(), mu_h.get()
        with np.errstate(all="ignore"):
            return model(eq._af, eq._hist_q, mr - mh if kind == ADDITIVE else mr / mh, labels)

    @property
    def scaling(self) -> np.ndarray:
        lead = () if self.group.prop == "group" else (len(self.group_labels),)
        return self._scaling.get().reshape(lead + self.cell_shape)

    def adjust(self, sim, *, interp: str = "nearest", extrapolation: str = "constant", detrend: int = 1, time=None, keep=False,
               grouped_nearest: str = "griddata"):
        extra, s, gi = self._adjust_front(sim, interp, extrapolation, time, detrend=detrend, dqm_order=True,
                                          untrained="sim holds time steps whose group was not trained")
        dev = self._dev
        fwd, inv = ("+", "-") if self.kind == ADDITIVE else ("*", "/")
        if extra is not None:
            return self._adjust_members(_flatten(sim, dev)[0], extra, interp, extrapolation, detrend, keep, fwd, inv)
        if gi is not None:
            return self._adjust_grouped(s, gi, interp, extrapolation, detrend, time, keep, fwd, inv, grouped_nearest)
        scaled = K.trend_apply(dev, s, self._scaling, None, fwd)
        p0, p1 = K.poly_trend(dev, scaled, detrend)
        detr = K.trend_apply(dev, scaled, p0, p1, inv)
        del scaled
        scen0 = K.eqm_adjust(dev, detr, self._af, self._hist_q, self.kind, interp, extrapolation)
        scen = K.trend_apply(dev, scen0, p0, p1, fwd, out=detr)  # (distinct buffers: the kernels' pointers are __restrict__)
        return _result(scen, keep, (s.shape[0],) + self.cell_shape)

    def _adjust_members(self, s, extra, interp, extrapolation, detrend, keep, fwd, inv):
        """group="time", a sim with member axes right behind time ((T, members x cells) here).  Every member is scaled and mapped
        with the same tables (repeated per member).  The trend: a model trained with ``Grouper(add_dims=...)`` detrends with
        ``PolyDetrend(group=that grouper)``, which fits ONE polynomial on the mean over the pooled members
        (``_polydetrend_get_trend``: ``da.mean(dim[1:])`` ahead of polyfit) and removes it from every member; without
        ``add_dims`` the extra axes are ordinary ones and every series has its own trend."""
        dev = self._dev
        T = s.shape[0]
        E, C_ = int(np.prod(extra)), int(np.prod(self.cell_shape)) if self.cell_shape else 1

        def tile64(a):   # (C,) float64 table -> (E * C,)
            return dev.to_device(np.tile(a.get().reshape(-1), E), dtype=np.float64)

        scaled = K.trend_apply(dev, s, tile64(self._scaling), None, fwd)
        if self.group.add_dims:
            # the mean over the members of every step: the (T, E x C) matrix is (T x E, C) with E rows per step
            mean, _ = K.resample_reduce(dev, scaled.reshape(T * E, C_), "mean", np.arange(0, T * E + 1, E, dtype=np.int64), want_valid=False)
            p0, p1 = K.poly_trend(dev, mean, detrend)
            p0, p1 = tile64(p0), (tile64(p1) if p1 is not None else None)
        else:
            p0, p1 = K.poly_trend(dev, scaled, detrend)
        detr = K.trend_apply(dev, scaled, p0, p1, inv)
        del scaled
        scen0 = K.eqm_adjust(dev, detr, _tile_members(dev, self._af, E), _tile_members(dev, self._hist_q, E), self.kind, interp,
                             extrapolation)
        scen = K.trend_apply(dev, scen0, p0, p1, fwd, out=detr)
        return _result(scen, keep, (T,) + tuple(extra) + self.cell_shape)

    def _interpolated_scaling(self, s, gcoord, fwd):
        """xsdba: u.broadcast(scaling, sim, group=group, interp=interp) — for every interpolation but "nearest" (and every
        grouping but the day of year) the scaling of a step is INTERPOLATED over the group coordinate (cyclic copies at
        0 and G + 1, DataArray.interp "linear"): scaling_t = S[r0] + (S[r0 + 1] - S[r0]) (g_t - r0).  Steps are handled
        interval by interval of the coordinate (G + 1 of them, group-major like the groups): x OP (p0 + p1 u) is
        xh_trend_apply_u.  Returns the scaled series in time order."""
        dev = self._dev
        G = len(self.group_labels)
        S = self._scaling.get().reshape(G, s.shape[1])
        r0 = np.clip(np.floor(gcoord).astype(np.int64), 0, G)
        row = lambda r: (r - 1) % G                                  # coordinate 0 .. G + 1 -> group (cyclic)
        lay = _GroupMajor(r0, G + 1)
        s_perm = lay.gather(dev, s)
        sc_perm = dev.empty(s.shape, np.float32)
        for r, off, n in lay:
            a0, a1 = S[row(r)], S[row(r + 1)]
            p0 = dev.to_device(np.ascontiguousarray(a0), dtype=np.float64)
            p1 = dev.to_device(np.ascontiguousarray(a1 - a0), dtype=np.float64)
            uf = dev.to_device(np.ascontiguousarray(gcoord[lay.rows(off, n)] - r), dtype=np.float64)
            K.trend_apply(dev, _group(s_perm, off, n), p0, p1, fwd, out=_group(sc_perm, off, n), u=uf)
        return lay.scatter(dev, sc_perm)

    def _adjust_grouped(self, s, gi, interp, extrapolation, detrend, time, keep, fwd, inv, grouped_nearest="griddata"):
        """dqm_adjust with a sub-grouping: group-major row blocks like the grouped EQM; per block the group's
        scaling (``u.broadcast``), the trend fitted over the group's OWN steps on their time coordinate (days since the
        group's mean date: ``PolyDetrend(group=...)`` -> polyfit along time), the group's nodes, the trend put back."""
        dev, shape = self._dev, (s.shape[0],) + self.cell_shape
        lay = _GroupMajor(gi, len(self.group_labels))
        days = np.asarray(time.ordinal(), dtype=np.float64)
        gcoord = self.group.coordinate(time, interp=True) if interp == "linear" else None
        prescaled = interp == "linear" and self.group.prop == "month"
        src = self._interpolated_scaling(s, gcoord, fwd) if prescaled else s
        windowed = self.group.window > 1
        if interp == "linear" or self._plane_nearest(grouped_nearest):
            # the (quantile, group) plane serves the whole series in one launch, and so do the scaling, the per-group fit and the
            # trend (xh_trend_apply_groups / xh_poly_trend_groups, round 6: a group is a list of rows, the coefficients are
            # (G, C) tables, nothing is permuted) — bit-identical to the per-group loop below, which launched four kernels per
            # group on gathered blocks (365 groups: 87 ms for a 30-year 1440 x 90 band, now ~20)
            perm, offs = lay.perm, lay.offs
            u_time = np.zeros(s.shape[0], dtype=np.float64)
            for g, off, n in lay:
                r = lay.rows(off, n)
                u_time[r] = days[r] - days[r].mean()
            u_d = dev.to_device(u_time, dtype=np.float64)
            scaled = src if prescaled else K.trend_apply_groups(dev, s, perm, offs, self._scaling, None, fwd)
            fit_on = K.window_nanmean(dev, scaled, self.group.window) if windowed else scaled
            p0, p1 = K.poly_trend_groups(dev, fit_on, perm, offs, u_d, detrend)
            del fit_on
            detr = K.trend_apply_groups(dev, scaled, perm, offs, p0, p1, inv, u=u_d)
            del scaled
            if interp == "linear":
                scen0 = K.plane_linear(dev, detr, gcoord, self._af, xq_all=self._hist_q, kind=self.kind)
            else:
                scen0 = K.plane_nearest(dev, detr, gi + 1.0, self._af, self._hist_q, self.kind, extrapolation)
            scen = K.trend_apply_groups(dev, scen0, perm, offs, p0, p1, fwd, u=u_d, out=detr)
            return _result(scen, keep, shape, sync=True)
        s_perm = lay.gather(dev, src)
        scen_perm = dev.empty(s.shape, np.float32)
        wm_perm = None
        if windowed:
            # PolyDetrend with a windowed Grouper (xsdba.detrending._polydetrend_get_trend: ``da.mean(dim[1:])`` before polyfit):
            # the trend of a group is fitted on the centred WINDOW MEAN of the scaled series at the group's steps — neighbours
            # carry the scaling of their own groups, so the whole series is scaled first (group-major blocks), brought back to
            # time order, averaged, and permuted again
            if not prescaled:
                for g, off, n in lay:
                    K.trend_apply(dev, _group(s_perm, off, n), _group(self._scaling, g), None, fwd, out=_group(scen_perm, off, n))
                s_perm, scen_perm = scen_perm, s_perm          # s_perm: the scaled series, group-major
                src = lay.scatter(dev, s_perm)                 # ... and in time order
            wm_perm = lay.gather(dev, K.window_nanmean(dev, src, self.group.window))
        # (what is left here: every step through the nodes of its OWN group — grouped_nearest="group", seasons, more than 32
        # nodes, "cubic": one xh_eqm_adjust per group on its gathered block)
        for g, off, n in lay:
            rows = lay.rows(off, n)
            u = dev.to_device(np.ascontiguousarray(days[rows] - days[rows].mean()), dtype=np.float64)
            blk = _group(s_perm, off, n)
            scaled = blk if (prescaled or windowed) else K.trend_apply(dev, blk, _group(self._scaling, g), None, fwd)
            fit_on = scaled if not windowed else _group(wm_perm, off, n)
            p0, p1 = K.poly_trend(dev, fit_on, detrend, u=u)
            detr = K.trend_apply(dev, scaled, p0, p1, inv, u=u)
            scen0 = K.eqm_adjust(dev, detr, _group(self._af, g), _group(self._hist_q, g), self.kind, interp, extrapolation)
            K.trend_apply(dev, scen0, p0, p1, fwd, out=_group(scen_perm, off, n), u=u)
        return _result(lay.scatter(dev, scen_perm), keep, shape, sync=True)
