"""Footprint harness (test infrastructure only): one bad sample may change the outputs whose window, period or cell holds it,
and no other.

A :class:`Case` names the fields of one entry point, the device call, a float64 reference of the same operation, the field to
perturb and the positions read off the KERNEL's decomposition (wave seams, chunk ends, the ragged tail).  :func:`check` then

  * computes ``ref(clean)`` and ``ref(perturbed)``; the FOOTPRINT is where they differ, bit for bit with NaN equal to NaN.  It
    comes from the reference alone, never from the device;
  * runs the device on both (the modules that use this import ``poisoned_outputs``: every output buffer starts as poison) and
    asserts that no element is left unwritten;
  * A1 (always): outside the footprint ``device(perturbed)`` meets the tolerance of the entry point's parity test against the
    reference;
  * A2 (unless the case waives it with a written reason): outside the footprint ``device(perturbed)`` is bit-identical to
    ``device(clean)``;
  * B: inside the footprint, for NaN and -9999, ``device(perturbed)`` meets the same tolerance against ``ref(perturbed)`` with
    the same NaN pattern.  For 1e20 and the netCDF default fill value only "written" is claimed there: the reference's
    float32 stages may overflow where the kernel's float64 does not;
  * not vacuous: the footprint is non-empty, lies in the perturbed cell, and covers at most a quarter of that cell's outputs
    (window and period cases) — or is free to be the whole cell (``whole_cell`` cases: whole-series fits and recurrences)."""
from dataclasses import dataclass, field as _dc_field
from typing import Callable

import numpy as np

from poisoned import unwritten

# the netCDF default _FillValue of a float variable; float32(9.96921e36) and the float64 constant are the same number
NC_FILL = 9.969209968386869e36
PERTURBATIONS = {"nan": np.nan, "-9999": -9999.0, "1e20": 1e20, "ncfill": NC_FILL}
EXACT_INSIDE = ("nan", "-9999")   # B compares values inside the footprint for these only


def kelvin(rng, T, C, dtype=np.float32):
    """Temperature in kelvin, 283 +- 4."""
    return (283.0 + rng.normal(0.0, 4.0, (T, C))).astype(dtype)


def flux(rng, T, C, dtype=np.float32):
    """Precipitation flux in kg m-2 s-1: gamma(0.6, 3e-5) with about 40 % exact zeros."""
    return np.where(rng.random((T, C)) < 0.4, 0.0, rng.gamma(0.6, 3e-5, (T, C))).astype(dtype)


FIELDS = {"kelvin": kelvin, "flux": flux}


@dataclass
class Case:
    """``make(rng, kind, dtype)`` -> dict of numpy fields; ``device(dev, fields)`` and ``ref(fields)`` -> a list of numpy
    arrays whose LAST axis is the cell.  ``tol``: one dict of assert_allclose keywords per output (None: exact), taken from
    the parity test named in ``tol_from``; ``dict(scale=k, rtol=r)`` bounds the error by ``r`` times the reference's k-th
    array instead (the restatements of the newer units return, after their outputs, the sum of magnitudes behind each).
    ``rows``: the rows of ``target`` to perturb, paired round-robin with ``cells``."""
    name: str
    lib: str                      # the simulation library that holds the entry point ("shared", "agro", "hydro", ...)
    make: Callable
    device: Callable
    ref: Callable
    target: str
    rows: tuple
    tol: tuple
    tol_from: str
    cells: tuple = (0, 63, 64, 69)
    C: int = 70
    kinds: tuple = ("kelvin", "flux")
    dtypes: tuple = (np.float32,)
    whole_cell: bool = False
    waive_a2: str | None = None   # the reason, naming the code that legitimately switches paths
    dropped: dict = _dc_field(default_factory=dict)   # perturbation -> one-line reason
    # the reason why the reference may stay as it is at SOME positions (then nothing at all may move there); every
    # perturbation still has to move the reference at one position at least
    may_be_empty: str | None = None
    seed: int = 20240925

    def positions(self):
        n = max(len(self.rows), len(self.cells))
        return [(self.rows[i % len(self.rows)], self.cells[i % len(self.cells)]) for i in range(n)]


def same_bits(a, b):
    """Elementwise: equal bit for bit, with every NaN equal to every NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        u = f"u{a.dtype.itemsize}"
        return (np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _close(got, exp, tol, where, what, refs=()):
    if not where.any():
        return
    g, e = np.asarray(got)[where], np.asarray(exp)[where]
    if tol is None or g.dtype.kind != "f":
        bad = ~same_bits(g, e.astype(g.dtype))
        assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} differ, first at {np.argwhere(where)[np.flatnonzero(bad)[0]]}"
        return
    assert np.array_equal(np.isnan(g), np.isnan(e)), f"{what}: NaN pattern differs at {int((np.isnan(g) != np.isnan(e)).sum())} of {g.size}"
    with np.errstate(all="ignore"):
        g64, e64 = g.astype(np.float64), e.astype(np.float64)
        bound = tol.get("atol", 0.0) + tol.get("rtol", 0.0) * (np.abs(e64) if "scale" not in tol else np.asarray(refs[tol["scale"]], np.float64)[where])
        bad = ~(np.abs(g64 - e64) <= bound) & ~np.isnan(e64) & ~(g64 == e64)
    if bad.any():
        i = np.flatnonzero(bad)
        rel = np.abs(g64[i] - e64[i]) / np.maximum(np.abs(e64[i]), 1e-300)
        raise AssertionError(f"{what}: {len(i)} of {g.size} beyond {tol}; worst relative error {rel.max():.3g}; "
                             f"first at {np.argwhere(where)[i[0]]}: got {g[i[0]]!r}, expected {e[i[0]]!r}")


_CLEAN = {}


def check(dev, case: Case, kind: str, dtype, *, perturbations=None, report=None):
    """Every perturbation at every position of ``case`` on one field kind and dtype.  ``report``: a list that receives one line
    per (perturbation, position) with the footprint's size."""
    rng = np.random.default_rng(case.seed)
    fields = case.make(rng, kind, dtype)
    key = (id(dev), case.name, kind, np.dtype(dtype).name)
    if key not in _CLEAN:   # (the clean reference and the clean device run: once per case, shared, never changed)
        r, d = case.ref(fields), case.device(dev, fields)
        for a in r + d:
            a.setflags(write=False)
        _CLEAN[key] = (r, d)
    ref_clean, dev_clean = _CLEAN[key]
    assert len(ref_clean) >= len(dev_clean) == len(case.tol)   # (what the reference returns beyond the outputs: scales)
    for k, (r, d) in enumerate(zip(ref_clean, dev_clean)):
        assert r.shape == d.shape, (case.name, k, r.shape, d.shape)
        assert not unwritten(d).any(), f"{case.name}: output {k} of the clean run has {int(unwritten(d).sum())} unwritten elements"
        _close(d, r, case.tol[k], np.ones(r.shape, bool), f"{case.name} clean output {k}", ref_clean)
    for pname in (perturbations or PERTURBATIONS):
        if pname in case.dropped:
            continue
        moved = 0
        for (t, c) in case.positions():
            pert = dict(fields)
            pert[case.target] = fields[case.target].copy()
            pert[case.target][t, c] = PERTURBATIONS[pname]
            ref_p = case.ref(pert)
            dev_p = case.device(dev, pert)
            tag = f"{case.name}[{kind}-{np.dtype(dtype).name}] {pname} at row {t}, cell {c}"
            total = inside = 0
            for k, (rc, rp, dc, dp) in enumerate(zip(ref_clean, ref_p, dev_clean, dev_p)):
                foot = ~same_bits(rc, rp)
                # not vacuous, from the reference alone: inside the perturbed cell, and a small part of it
                other = np.delete(foot, c, axis=-1)
                assert not other.any(), f"{tag}: the REFERENCE of output {k} changes {int(other.sum())} elements of other cells"
                n_cell = foot[..., c].size
                total += n_cell
                inside += int(foot[..., c].sum())
                if not case.whole_cell:
                    assert foot[..., c].sum() <= 0.25 * n_cell, f"{tag}: footprint {int(foot[..., c].sum())} of {n_cell} outputs of the cell"
                assert not unwritten(dp).any(), f"{tag}: output {k} has {int(unwritten(dp).sum())} unwritten elements"
                _close(dp, rp, case.tol[k], ~foot, f"{tag}: A1 output {k} outside the footprint against the reference", ref_p)
                if case.waive_a2 is None:
                    bad = ~same_bits(dp, dc) & ~foot
                    assert not bad.any(), (f"{tag}: A2 output {k}: {int(bad.sum())} elements outside the footprint differ from the clean "
                                           f"device run, at {np.argwhere(bad)[:6].tolist()}")
                if pname in EXACT_INSIDE:
                    _close(dp, rp, case.tol[k], foot, f"{tag}: B output {k} inside the footprint", ref_p)
            assert inside > 0 or case.may_be_empty, f"{tag}: the reference does not change at all: the case tests nothing"
            moved += inside > 0
            if report is not None:
                report.append(f"{tag}: footprint {inside} of {total} outputs of the cell")
        assert moved, f"{case.name}[{kind}] {pname}: the reference does not change at any position: the case tests nothing"
