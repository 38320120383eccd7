"""Writes tests/golden/partition_vectors.npz: for every family of tests/partitioncpu.py and every cell of EXACT_CELLS, the EXACT
least-squares fit of each series (the rational solution of the normal equations, fractions.Fraction, rounded to float64), the
restatement's own largest distance from it in units of the bound's scale, and the restatement's g and u on those cells.  The
fields themselves are not stored: partitioncpu.family() makes them from an integer generator.  The reference's tests carry no
numerical answers and xarray cannot be executed where this was built, so nothing here runs the reference.

    python tests/golden/make_partition_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import partitioncpu as P  # noqa: E402


def exact_cube(da, years, deg):
    """(T, N, len(EXACT_CELLS)) exact fits; a series with fewer than deg + 1 valid years stays NaN."""
    days = P.stamps_days(years)
    T = da.shape[0]
    flat = da.reshape(T, -1, da.shape[-1])
    out = np.full((T, flat.shape[1], len(P.EXACT_CELLS)), np.nan)
    for k, c in enumerate(P.EXACT_CELLS):
        for n in range(flat.shape[1]):
            e = P.exact_fit(flat[:, n, c], days, deg)
            if e is not None:
                out[:, n, k] = e
    return out


def main():
    out = {}
    cells = list(P.EXACT_CELLS)
    for name in P.FAMILIES:
        fam = P.family(name)
        da, years = fam["da"], fam["years"]
        x = P.stamps_ns(years)
        degs = range(5) if name == P.DEG_FAMILY else [fam["deg_given"] if fam["deg_given"] is not None else 4]
        for deg in degs:
            ex = exact_cube(da, years, deg)
            sm, mag = P.fit(da[..., cells], x, deg)
            T = da.shape[0]
            sm, mag = sm.reshape(T, -1, len(cells)), mag.reshape(T, -1, len(cells))
            n, _ = P.status_of(da[..., cells].reshape(T, -1, len(cells)), deg)
            fitted = np.broadcast_to(n >= deg + 1, sm.shape)
            assert np.array_equal(np.isnan(ex[fitted]), np.isnan(sm[fitted])), name
            ok = fitted & ~np.isnan(ex)
            dist = float((np.abs(sm[ok] - ex[ok]) / mag[ok]).max())
            rel = float((np.abs(sm[ok] - ex[ok]) / np.abs(ex[ok]).max()).max())
            assert dist < 1e-13, (name, deg, dist)   # the restatement itself uses at most a tenth of the device's bound
            key = f"{name}/deg{deg}"
            out[f"{key}/exact"] = ex
            out[f"{key}/restated_dist"] = np.array([dist, rel])
            print(f"{key}: restatement within {dist:.2e} of the scale, {rel:.2e} of the largest value")
        if name in P.VALUE_FAMILIES:
            g, u, _, _ = P.restate(fam, cells)
            out[f"{name}/g"], out[f"{name}/u"] = g, u
    fam = P.family("ls_nan")
    cond = P.gram_condition(fam["da"][:, 1, 0, 1, 2], P.stamps_ns(fam["years"]))
    assert cond < 1e3, cond
    out["ls_nan/bunched_cond"] = np.array(cond)
    worst = 1.0
    for name in P.VALUE_FAMILIES:   # the condition of every fitted series of the recorded cells
        fam = P.family(name)
        if fam["deg_given"] is not None:
            continue
        flat = fam["da"][..., cells].reshape(fam["da"].shape[0], -1)
        x = P.stamps_ns(fam["years"])
        for j in range(flat.shape[1]):
            if (~np.isnan(flat[:, j])).sum() >= 5:
                worst = max(worst, P.gram_condition(flat[:, j], x))
    out["worst_cond"] = np.array(worst)
    print(f"cond(G): bunched {cond:.3g}, worst recorded {worst:.3g}")
    path = P.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    main()
