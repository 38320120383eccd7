"""Generate tests/golden/distfit_vectors.npz and distfit_known_answers.json by EXECUTING the reference's fitting code with scipy.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_distfit_golden.py

src/xclim/indices/stats.py cannot be imported (xarray).  ``_fit_start`` and ``_fitfunc_1d`` are AST-extracted (nothing is copied
into this repository) and run with scipy on every cell.  For the Nelder–Mead fits ``optimizer=`` travels through ``fitkwargs``:
a wrapper around ``optimize.fmin(..., full_output=True)``, so the reference's own call is recorded with its evaluation count and
its warn flag.  Per case the file holds

* ``codes`` (T, C) int16 and ``scale``: the input is ``codes * scale`` in the case's dtype (``decode``), -32768 = NaN;
* ``params`` (nparams, C), ``nfev`` / ``warnflag`` (C), ``status`` (C) uint8 with the XH_DISTFIT_* codes: 1 where the reference
  gives NaN (or raises for the cell: ``raised``), 2 where fmin stopped at its budget, 3 where a value lies at or below ``floc``;
* ``levels_max`` / ``levels_min`` (3, C): the return levels for ``t = [2, 10, 100]`` through scipy's ``isf`` / ``ppf`` exactly
  as ``parametric_quantile`` switches (every q > 0.5: ``isf(1 - q)``; with t = 2, q = 0.5 and both modes take ``ppf``), and
  ``levels_isf``: mode max for ``t = [5, 20, 100]``, which takes ``isf``;
* ``v`` (3) and ``cdf`` / ``pdf`` (3, C) at those values;
* ``penalty_at_start`` (C): the start values leave a value outside the support (genextreme).

The condition of the Nelder–Mead families — none of the reference's own fits stopped at the budget — is asserted here and again
by tests/test_distfit_cpu.py on the stored flags.
"""

import ast
import json
import os
import warnings

import numpy as np
import scipy.optimize
import scipy.stats

REF = "/root/reference/src/xclim/indices/stats.py"
HERE = os.path.dirname(os.path.abspath(__file__))
NAN_CODE = -32768
T_RETURN = [2, 10, 100]
T_RETURN_ISF = [5, 20, 100]   # every q = 1 - 1 / t above 0.5: the isf route of parametric_quantile
NM = {("genextreme", "ML", False), ("gamma", "ML", False), ("fisk", "ML", False), ("fisk", "ML", True)}   # (dist, method, floc given)
KNOWN = [279, 302, 450, 272, 401, 222, 311, 327, 294, 299, 348, 286, 492, 296, 227, 437, 340, 376, 444, 177]


def extract():
    tree = ast.parse(open(REF).read())
    ns = {"np": np, "scipy": scipy, "warnings": warnings}
    body = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("_fit_start", "_fitfunc_1d"):
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            if node.args.kwarg is not None:
                node.args.kwarg.annotation = None
            body.append(node)
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF, "exec"), ns)
    assert "_fit_start" in ns and "_fitfunc_1d" in ns
    return ns


def decode(codes, scale, dtype):
    x = codes.astype(dtype) * np.dtype(dtype).type(scale)
    x[codes == NAN_CODE] = np.nan
    return x


def is_nm(dist, method, floc):
    return (dist, method, floc is not None) in NM


def fit_cell(ns, v, dist, method, floc):
    """(params or None, nfev, warnflag, status, raised) of one cell: the reference's _fitfunc_1d on the float64 values."""
    sdist = getattr(scipy.stats, dist)
    nparams = 2 if dist in ("norm", "gumbel_r") else 3
    rec = {"nfev": 0, "warnflag": 0}

    def optimizer(func, x0, args=(), disp=0):
        xopt, _, _, funcalls, warnflag = scipy.optimize.fmin(func, x0, args=args, disp=0, full_output=True)
        rec.update(nfev=funcalls, warnflag=warnflag)
        return xopt

    fk = {} if floc is None else {"floc": floc}
    if is_nm(dist, method, floc):
        fk["optimizer"] = optimizer
    valid = v[~np.isnan(v)]
    if floc is not None and method == "ML" and dist in ("gamma", "lognorm") and len(valid) > 1 and valid.min() <= floc:
        return None, 0, 0, 3, True   # scipy's FitDataError, a ValueError for the whole call
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            p = np.asarray(ns["_fitfunc_1d"](v, dist=sdist, nparams=nparams, method=method, **fk), float)
    except Exception:   # FitError, brentq without a bracket, a NaN function value: the reference fails; the device gives NaN
        return None, rec["nfev"], rec["warnflag"], 1, True
    if np.isnan(p).any():
        return None, rec["nfev"], rec["warnflag"], 1, False
    return p, rec["nfev"], rec["warnflag"], 2 if rec["warnflag"] else 0, False


def sample(rng, kind, T, C):
    """(T, C) float64 and the code scale of a family."""
    if kind == "norm":
        return rng.normal(10.0, 5.0, (T, C)), 0.01
    if kind == "gumbel":
        return scipy.stats.gumbel_r.rvs(loc=5.0, scale=1.3, size=(T, C), random_state=rng), 0.001
    if kind == "gumbel_wide":   # scale about 50: the first bracket (0.5, 2) holds no root
        return scipy.stats.gumbel_r.rvs(loc=300.0, scale=50.0, size=(T, C), random_state=rng), 0.05
    if kind == "gev":
        c = np.linspace(-0.3, 0.3, C) if C > 1 else np.array([0.15])
        c[C // 2] = 1e-4 if C > 1 else c[0]   # c near 0
        return scipy.stats.genextreme.rvs(c[None, :], loc=100.0, scale=20.0, size=(T, C), random_state=rng), 0.05
    if kind == "gamma5":   # Nelder-Mead over (a, loc, scale) is ill-conditioned on short samples: 150 values of shape 5 converge
        return rng.gamma(5.0, 10.0, (T, C)), 0.01
    if kind == "gamma":
        return np.maximum(rng.gamma(2.0, 10.0, (T, C)), 0.01), 0.01
    if kind == "lognorm":
        return np.exp(rng.normal(2.0, 0.5, (T, C))), 0.01
    if kind == "fisk":
        return scipy.stats.fisk.rvs(3.0, loc=-20.0, scale=30.0, size=(T, C), random_state=rng), 0.02
    raise KeyError(kind)


CLOSED_SHAPES = [(30, 130, "f8"), (33, 65, "f4"), (150, 65, "f8"), (32, 1, "f4")]
APP_SHAPES = [(33, 65, "f8"), (30, 1, "f4")]
CASES = []   # name, dist, method, floc, kind, T, C, dtype
for T, C, dt in CLOSED_SHAPES:
    for name, dist, floc, kind in [("norm", "norm", None, "norm"), ("gumbel", "gumbel_r", None, "gumbel"),
                                   ("gumbelwide", "gumbel_r", None, "gumbel_wide"), ("gamma_floc0", "gamma", 0.0, "gamma"),
                                   ("gamma_flocneg", "gamma", -5.0, "gamma"), ("lognorm_floc0", "lognorm", 0.0, "lognorm"),
                                   ("lognorm_flocneg", "lognorm", -2.5, "lognorm")]:
        CASES.append((f"{name}_ml_{T}x{C}{dt}", dist, "ML", floc, kind, T, C, dt))
for T, C, dt in APP_SHAPES:
    for name, dist, floc, kind in [("gev", "genextreme", None, "gev"), ("gamma", "gamma", None, "gamma"), ("gamma_floc0", "gamma", 0.0, "gamma"),
                                   ("fisk", "fisk", None, "fisk"), ("fisk_flocneg", "fisk", -40.0, "fisk"),
                                   ("lognorm", "lognorm", None, "lognorm"), ("lognorm_floc0", "lognorm", 0.0, "lognorm")]:
        CASES.append((f"{name}_app_{T}x{C}{dt}", dist, "APP", floc, kind, T, C, dt))
for T, C, dt in [(30, 130, "f8"), (32, 65, "f4"), (33, 65, "f8"), (150, 65, "f4"), (30, 1, "f8")]:
    CASES.append((f"gev_ml_{T}x{C}{dt}", "genextreme", "ML", None, "gev", T, C, dt))
CASES += [("gamma_ml_150x65f8", "gamma", "ML", None, "gamma5", 150, 65, "f8"), ("fisk_ml_32x65f4", "fisk", "ML", None, "fisk", 32, 65, "f4"),
          ("fisk_flocneg_ml_33x65f8", "fisk", "ML", -40.0, "fisk", 33, 65, "f8"), ("fisk_ml_150x1f8", "fisk", "ML", None, "fisk", 150, 1, "f8")]


def make_case(ns, rng, spec):
    name, dist, method, floc, kind, T, C, dt = spec
    raw, scale = sample(rng, kind, T, C)
    codes = np.clip(np.round(raw / scale), -32000, 32000).astype(np.int16)
    if floc is not None and floc >= 0 and kind in ("gamma", "lognorm"):
        codes = np.maximum(codes, 1)
    nm = is_nm(dist, method, floc)
    if C >= 65:
        codes[:, 0] = NAN_CODE                       # a cell with all NaN
        codes[1:, 1] = NAN_CODE                      # a cell with one value
        if not nm:
            codes[2:, 2] = NAN_CODE                  # a cell with two values
        if dist == "norm" and T <= 128:
            # A constant cell, where the sums of both sides are the same additions (numpy's pairwise sum up to 128 values).  The
            # other closed forms are left out: on identical values gumbel_r's bracket ends at a NaN function value and scipy
            # returns (inf, tiny) from it, gamma's and lognorm's shape hangs on the last bit of a difference of logarithms.
            codes[:, 4] = codes[0, 4]
        nnan = min(20, T - 30) if nm else T // 3     # NaNs scattered; a Nelder-Mead family keeps at least 30 values
        if nnan > 0:
            codes[rng.choice(T, nnan, replace=False), 3] = NAN_CODE
        if dist == "lognorm" and method == "ML":
            codes[T // 2, 5] = int(round(floc / scale))   # the minimum equals floc
            codes[:, 5] = np.maximum(codes[:, 5], codes[T // 2, 5])
    x = decode(codes, scale, np.float64 if dt == "f8" else np.float32)
    x64 = x.astype(np.float64)                       # float32: the reference runs on the widened values
    nparams = 2 if dist in ("norm", "gumbel_r") else 3
    sdist = getattr(scipy.stats, dist)
    params = np.full((nparams, C), np.nan)
    nfev, warnflag = np.zeros(C, np.int32), np.zeros(C, np.int32)
    status, raised = np.zeros(C, np.uint8), np.zeros(C, bool)
    penalty = np.zeros(C, bool)
    for c in range(C):
        p, nfev[c], warnflag[c], status[c], raised[c] = fit_cell(ns, x64[:, c], dist, method, floc)
        if p is not None:
            params[:, c] = p
        if dist == "genextreme":
            v = x64[:, c][~np.isnan(x64[:, c])]
            if len(v) > 1:
                args, kw = ns["_fit_start"](v, "genextreme")
                a, b = sdist.support(*args, **kw)
                penalty[c] = bool(((v < a) | (v > b)).any())
    pl = [params[k][None, :] for k in range(nparams)]

    def levels(t, mode):   # fa (stats.py:466-482) and the switch of parametric_quantile (:254-262)
        t = np.atleast_1d(t)
        q = 1 - 1.0 / t if mode == "max" else 1.0 / t
        return sdist.isf((1 - q)[:, None], *pl) if np.all(q > 0.5) else sdist.ppf(q[:, None], *pl)

    # (t = 2 in max mode is q = 0.5, which is not above 0.5: both modes of T_RETURN go through ppf, T_RETURN_ISF through isf)
    assert not np.all(1 - 1.0 / np.array(T_RETURN) > 0.5) and np.all(1 - 1.0 / np.array(T_RETURN_ISF) > 0.5)
    finite = x64[np.isfinite(x64)]
    v = np.round(np.percentile(finite, [10, 50, 90]), 2)
    with np.errstate(all="ignore"):
        out = {"codes": codes, "scale": np.float64(scale), "params": params, "nfev": nfev, "warnflag": warnflag, "status": status,
               "raised": raised, "penalty_at_start": penalty, "v": v,
               "levels_max": levels(T_RETURN, "max"), "levels_min": levels(T_RETURN, "min"), "levels_isf": levels(T_RETURN_ISF, "max"),
               "cdf": sdist.cdf(v[:, None], *pl), "pdf": sdist.pdf(v[:, None], *pl)}
    meta = {"dist": dist, "method": method, "floc": floc, "T": T, "C": C, "dtype": dt, "nm": nm, "kind": kind}
    return out, meta


def known_answer(ns):
    x = np.asarray(KNOWN)
    p = ns["_fitfunc_1d"](x, dist=scipy.stats.genextreme, nparams=3, method="ML")
    np.testing.assert_allclose(p, (0.20949, 297.954091, 75.7911863), 1e-5)   # the reference's test_genextreme_fit
    return {"test_genextreme_fit": {"values": KNOWN, "dist": "genextreme", "method": "ML", "expected": [0.20949, 297.954091, 75.7911863],
                                    "rtol": 1e-5, "scipy": [float(v) for v in p]}}


def main():
    ns = extract()
    rng = np.random.default_rng(20261020)
    arrays, metas = {}, {}
    for spec in CASES:
        out, meta = make_case(ns, rng, spec)
        for k, v in out.items():
            arrays[f"{spec[0]}__{k}"] = v
        metas[spec[0]] = meta
        print(spec[0], "status counts:", np.bincount(out["status"], minlength=4).tolist(), "raised:", int(out["raised"].sum()),
              "max nfev:", int(out["nfev"].max()), "penalty:", int(out["penalty_at_start"].sum()))
        if meta["nm"]:
            assert not out["warnflag"].any(), f"{spec[0]}: a reference fit stopped at the budget"
            fitted = out["status"] == 0
            assert fitted.sum() >= meta["C"] - 2
    assert any(arrays[f"{n}__penalty_at_start"].any() for n, m in metas.items() if m["dist"] == "genextreme" and m["method"] == "ML")
    arrays["meta"] = np.array(json.dumps(metas))
    path = os.path.join(HERE, "distfit_vectors.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "distfit_known_answers.json"), "w") as f:
        json.dump(known_answer(ns), f, indent=1)


if __name__ == "__main__":
    main()
