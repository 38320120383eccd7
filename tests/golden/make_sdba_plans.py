"""Record the LAUNCH PLANS of xclim_amd/sdba.py — for a matrix of train / adjust / adapt_freq calls, what reaches the C ABI:

    python tests/golden/make_sdba_plans.py          # writes tests/golden/sdba_plans.json
    python tests/golden/make_sdba_plans.py --check  # records again and compares with the committed file

The calls run on tools/mock_device.MockDevice: every compute entry point is a no-op (the tables it would fill stay zero), the
host planning — groupings, permutations, offsets, views, the order of the launches — is the real one.  Per case the fixture holds

    names     the ``xh_*`` entry points in call order, run-length compressed (``3*(xh_a xh_b)``: a block repeated 3 times);
              ``sync`` stands for Device.sync()
    digest    sha256 (16 hex digits) over the full records: the name and every argument in order — integers and floats as
              values, device pointers as NULL or the number of the distinct address within the call (two arguments that share a
              buffer share a number), host tables (kernels.np_ptr) as the hash of their bytes
    h2d, d2h  [count, bytes] of the uploads and downloads (compared as totals: their order is not part of the plan)
    error     [exception type, message] or null;  warnings: the texts

The file was recorded BEFORE sdba.py's group-major plumbing was shared (one layout helper, one training routine, one adjust
front end) and is the reference of tests/test_sdba_plans_cpu.py: it is regenerated only when a launch plan is MEANT to change,
never to make that test pass.
"""

import ctypes
import hashlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT,):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.mock_device import MockDevice  # noqa: E402
from xclim_amd import kernels as K  # noqa: E402
from xclim_amd import sdba  # noqa: E402
from xclim_amd.timeaxis import TimeAxis  # noqa: E402

FIXTURE = os.path.join(HERE, "sdba_plans.json")
C_, NQ = 5, 8
CALENDARS = {"noleap": ("noleap", 4 * 365), "standard": ("standard", 6 * 365 + 1 + 1)}   # standard: 2004 is a leap year, + one day
GROUPS = {"time": ("time", 1), "month": ("time.month", 1), "season": ("time.season", 1), "doy": ("time.dayofyear", 1),
          "doy_w7": ("time.dayofyear", 7)}
CLASSES = {"EQM": sdba.EmpiricalQuantileMapping, "QDM": sdba.QuantileDeltaMapping, "DQM": sdba.DetrendedQuantileMapping}


class _HostPtr(ctypes.c_void_p):
    """kernels.np_ptr's result, remembering the bytes of the host table it points to."""


def _np_ptr(a):
    p = _HostPtr(a.ctypes.data)
    p.digest = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    return p


def _encode(args):
    seen, out = {}, []
    for a in args:
        if isinstance(a, _HostPtr):
            out.append("h:" + a.digest)
        elif a is None or isinstance(a, ctypes.c_void_p):
            v = None if a is None else a.value
            out.append("null" if not v else f"p{seen.setdefault(v, len(seen))}")
        elif isinstance(a, (bool, int, np.integer)):
            out.append(f"i:{int(a)}")
        elif isinstance(a, (float, np.floating)):
            out.append(f"f:{float(a)!r}")
        else:
            out.append(f"?:{a!r}")
    return out


def compress(names, longest=8):
    """Run-length compression over repeated blocks of up to ``longest`` names."""
    out, i = [], 0
    while i < len(names):
        best = (1, 1)
        for p in range(1, longest + 1):
            blk, n = names[i:i + p], 1
            while len(blk) == p and names[i + n * p:i + (n + 1) * p] == blk:
                n += 1
            if n > 1 and n * p > best[0] * best[1]:
                best = (p, n)
        p, n = best
        blk = " ".join(names[i:i + p])
        out.append(blk if n == 1 else f"{n}*({blk})" if p > 1 else f"{n}*{blk}")
        i += p * n
    return out


def record(fn, patch=None, full=False):
    """Run ``fn(dev)`` on a fresh mock device with the trace on; ``patch``: {name in kernels: replacement} for the call."""
    dev = MockDevice(0)
    saved = {n: getattr(K, n) for n in ("np_ptr", *(patch or {}))}
    K.np_ptr = _np_ptr
    for n, f in (patch or {}).items():
        setattr(K, n, f)
    error, texts = None, []
    try:
        prepared = fn(dev, None)           # (untraced: the model an adjust case needs)
        trace = dev.start_trace()
        sync = dev.sync
        dev.sync = lambda: (trace.append(("sync", ())), sync())[1]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                fn(dev, prepared)
            except Exception as e:  # noqa: BLE001 — the refusals are part of the record
                error = [type(e).__name__, str(e)]
        texts = [str(w.message) for w in caught]
    finally:
        dev.stop_trace()
        for n, f in saved.items():
            setattr(K, n, f)
    calls = [(n, _encode(a)) for n, a in trace if n.startswith("xh_") or n == "sync"]
    copies = {k: [a[0] for n, a in trace if n == k] for k in ("h2d", "d2h")}
    res = {"names": compress([n for n, _ in calls]),
           "digest": hashlib.sha256(json.dumps(calls).encode()).hexdigest()[:16],
           "h2d": [len(copies["h2d"]), int(sum(copies["h2d"]))], "d2h": [len(copies["d2h"]), int(sum(copies["d2h"]))],
           "error": error, "warnings": texts}
    if full:
        res["calls"] = calls
    return res


def field(T, seed, *lead):
    """A deterministic float32 field (T, *lead, C_) without a random generator."""
    n = T * int(np.prod(lead, dtype=np.int64)) * C_
    x = np.sin(np.arange(n, dtype=np.float64) * (0.37 + 0.11 * seed)) * 5.0 + 10.0 + seed
    return x.astype(np.float32).reshape((T, *lead, C_))


def time_axis(cal):
    name, T = CALENDARS[cal]
    return TimeAxis.daily("2001-01-01", T, name)


def none_of_them(*a, **k):
    return None


def cases():
    """{case id: (fn(dev, prepared), patch)} — ``fn(dev, None)`` prepares (untraced) and returns what the traced call needs."""
    out = {}

    def trainer(cls, cal, gname, kind="+", nq=NQ, lead=(), group=None, **kw):
        ta = time_axis(cal)
        grp = group if group is not None else sdba.Grouper(*GROUPS[gname])

        def train(dev):
            return CLASSES[cls].train(field(len(ta), 1, *lead), field(len(ta), 2, *lead), nquantiles=nq, kind=kind, group=grp, time=ta,
                                      device=dev, **kw)
        return train, ta

    def add_train(cid, train, patch=None):
        out[cid] = (lambda dev, prepared: True if prepared is None else train(dev), patch)

    def add_adjust(cid, train, call, patch=None):
        out[cid] = (lambda dev, prepared: train(dev) if prepared is None else call(prepared), patch)

    for cal in CALENDARS:
        for gname in GROUPS:
            for cls in CLASSES:
                for kind in ("+", "*") if cls == "DQM" else ("+",):
                    train, ta = trainer(cls, cal, gname, kind)
                    base = f"{cal}/{cls}{kind if cls == 'DQM' else ''}/{gname}"
                    add_train(base + "/train", train)
                    sim = field(len(ta), 3)
                    for interp in ("nearest", "linear", "cubic"):
                        for extra in ("constant", "nan"):
                            for gn in ("griddata", "group") if cls != "QDM" else (None,):
                                for detrend in (0, 1) if cls == "DQM" else (None,):
                                    kw = dict(interp=interp, extrapolation=extra, time=ta)
                                    cid = f"{base}/adjust/{interp}/{extra}"
                                    if gn is not None:
                                        kw["grouped_nearest"] = gn
                                        cid += "/" + gn
                                    if detrend is not None:
                                        kw["detrend"] = detrend
                                        cid += f"/detrend{detrend}"
                                    add_adjust(cid, train, lambda m, kw=kw, sim=sim: m.adjust(sim, **kw))
        ta = time_axis(cal)
        sim = field(len(ta), 3)
        # ---- forced fall-backs (the mock never answers XH_ERR_NOTIMPL) ----
        for cls in ("EQM", "DQM"):
            add_train(f"{cal}/{cls}/doy_w7/train/no_eqm_train_window", trainer(cls, cal, "doy_w7")[0], {"eqm_train_window": none_of_them})
            add_train(f"{cal}/{cls}/doy/train/no_eqm_train_groups", trainer(cls, cal, "doy")[0], {"eqm_train_groups": none_of_them})
        for interp in ("nearest", "linear"):
            add_adjust(f"{cal}/QDM/doy/adjust/{interp}/no_qdm_adjust_groups", trainer("QDM", cal, "doy")[0],
                       lambda m, interp=interp, sim=sim, ta=ta: m.adjust(sim, interp=interp, time=ta), {"qdm_adjust_groups": none_of_them})
        # ---- adapt_freq, alone and in EQM training ----
        for gname in ("time", "month", "doy_w7"):
            g, w = GROUPS[gname]
            out[f"{cal}/adapt_freq/{gname}"] = (lambda dev, prepared, g=g, w=w, ta=ta: True if prepared is None else sdba.adapt_freq(
                field(len(ta), 1), field(len(ta), 2), 9.0, group=g, window=w, time=ta, seed=3, device=dev), None)
        for gname in ("time", "month"):
            add_train(f"{cal}/EQM/{gname}/train/adapt_freq_thresh", trainer("EQM", cal, gname, "*", adapt_freq_thresh=9.0, adapt_freq_seed=3)[0])
        # ---- keep=True, 40 nodes, member axes ----
        for cls in CLASSES:
            train, _ = trainer(cls, cal, "month")
            add_adjust(f"{cal}/{cls}/month/adjust/nearest/keep", train, lambda m, sim=sim, ta=ta: m.adjust(sim, time=ta, keep=True))
            add_adjust(f"{cal}/{cls}/time/adjust/nearest/keep", trainer(cls, cal, "time")[0], lambda m, sim=sim: m.adjust(sim, keep=True))
            train40, _ = trainer(cls, cal, "month", nq=40)
            add_train(f"{cal}/{cls}/month/train/40nodes", train40)
            for interp in ("nearest", "linear"):
                add_adjust(f"{cal}/{cls}/month/adjust/{interp}/40nodes", train40, lambda m, interp=interp, sim=sim, ta=ta: m.adjust(sim, interp=interp, time=ta))
            pooled, _ = trainer(cls, cal, "time", lead=(3,), group=sdba.Grouper("time", add_dims=1))
            add_train(f"{cal}/{cls}/time/train/add_dims", pooled)
            sim3 = field(len(ta), 3, 3)
            for interp in ("nearest", "linear", "cubic"):
                add_adjust(f"{cal}/{cls}/time/adjust/{interp}/add_dims", pooled, lambda m, interp=interp, sim3=sim3: m.adjust(sim3, interp=interp))
                add_adjust(f"{cal}/{cls}/time/adjust/{interp}/members", trainer(cls, cal, "time")[0],
                           lambda m, interp=interp, sim3=sim3: m.adjust(sim3, interp=interp))
            add_adjust(f"{cal}/{cls}/month/adjust/nearest/members", train, lambda m, sim3=sim3, ta=ta: m.adjust(sim3, time=ta))
            add_adjust(f"{cal}/{cls}/month/adjust/linear/members", train, lambda m, sim3=sim3, ta=ta: m.adjust(sim3, interp="linear", time=ta, keep=True))
            add_train(f"{cal}/{cls}/month/train/add_dims", trainer(cls, cal, "month", lead=(3,), group=sdba.Grouper("time.month", add_dims=1))[0])
            add_train(f"{cal}/{cls}/doy_w7/train/add_dims", trainer(cls, cal, "doy_w7", lead=(3,), group=sdba.Grouper("time.dayofyear", 7, add_dims=1))[0])
            # ---- the error paths ----
            add_train(f"{cal}/{cls}/month/train/no_time", lambda dev, cls=cls, ta=ta: CLASSES[cls].train(
                field(len(ta), 1), field(len(ta), 2), nquantiles=NQ, group="time.month", device=dev))
            add_train(f"{cal}/{cls}/month/train/short_time", lambda dev, cls=cls, ta=ta: CLASSES[cls].train(
                field(len(ta) - 1, 1), field(len(ta) - 1, 2), nquantiles=NQ, group="time.month", time=ta, device=dev))
            add_train(f"{cal}/{cls}/time/train/shapes_differ", lambda dev, cls=cls, ta=ta: CLASSES[cls].train(
                field(len(ta), 1), field(len(ta) - 1, 2), nquantiles=NQ, device=dev))
            add_train(f"{cal}/{cls}/time/train/grids_differ", lambda dev, cls=cls, ta=ta: CLASSES[cls].train(
                field(len(ta), 1), field(len(ta), 2, 2), nquantiles=NQ, device=dev))
            add_train(f"{cal}/{cls}/time/train/bad_kind", lambda dev, cls=cls, ta=ta: CLASSES[cls].train(
                field(len(ta), 1), field(len(ta), 2), nquantiles=NQ, kind="-", device=dev))
            add_adjust(f"{cal}/{cls}/month/adjust/no_time", train, lambda m, sim=sim: m.adjust(sim))
            add_adjust(f"{cal}/{cls}/month/adjust/bad_interp", train, lambda m, sim=sim, ta=ta: m.adjust(sim, interp="spline", time=ta))
            for gname in ("time", "month"):
                add_adjust(f"{cal}/{cls}/{gname}/adjust/grid_differs", trainer(cls, cal, gname)[0],
                           lambda m, ta=ta: m.adjust(field(len(ta), 3)[:, :4], time=ta))
        out[f"{cal}/adapt_freq/month/no_time"] = (lambda dev, prepared, ta=ta: True if prepared is None else sdba.adapt_freq(
            field(len(ta), 1), field(len(ta), 2), 9.0, group="time.month", device=dev), None)
        out[f"{cal}/adapt_freq/time/grids_differ"] = (lambda dev, prepared, ta=ta: True if prepared is None else sdba.adapt_freq(
            field(len(ta), 1), field(len(ta), 2, 2), 9.0, device=dev), None)
    # ---- a sim whose time axis holds a day the model was not trained on (day 366 against a noleap training set) ----
    other = time_axis("standard")
    for cls in CLASSES:
        add_adjust(f"noleap/{cls}/doy/adjust/untrained_day", trainer(cls, "noleap", "doy")[0],
                   lambda m, other=other: m.adjust(field(len(other), 3), time=other))
    return out


def build(only=None, full=False):
    return {cid: record(fn, patch, full) for cid, (fn, patch) in cases().items() if only is None or cid in only}


def main():
    plans = build()
    if "--check" in sys.argv[1:]:
        with open(FIXTURE) as f:
            stored = json.load(f)
        bad = [k for k in sorted(set(plans) | set(stored)) if plans.get(k) != stored.get(k)]
        if bad:
            sys.exit(f"{len(bad)} launch plans differ from tests/golden/sdba_plans.json: " + ", ".join(bad[:8]))
        print(f"sdba_plans.json: {len(stored)} plans, as recorded")
        return
    with open(FIXTURE, "w") as f:   # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(plans[k], sort_keys=True)}" for k in sorted(plans)) + "\n}\n")
    print(f"{len(plans)} plans, {sum(p['error'] is not None for p in plans.values())} refusals -> {FIXTURE}")


if __name__ == "__main__":
    main()
