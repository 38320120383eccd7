"""The recorded reference results of the distribution-fit unit (tests/golden/distfit_vectors.npz, made by
tests/golden/make_distfit_golden.py), shared by tests/test_distfit_cpu.py and tests/test_gpu_distfit.py: loaded once, read-only."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VECTORS = np.load(os.path.join(GOLDEN, "distfit_vectors.npz"))
META = json.loads(str(VECTORS["meta"]))
KNOWN = json.load(open(os.path.join(GOLDEN, "distfit_known_answers.json")))
CASES = sorted(META)
NM_CASES = [c for c in CASES if META[c]["nm"]]
DIRECT_CASES = [c for c in CASES if not META[c]["nm"]]   # closed forms, root-found fits and every APP
NAN_CODE = -32768
T_RETURN = [2, 10, 100]        # both modes go through ppf (t = 2 in max mode is q = 0.5)
T_RETURN_ISF = [5, 20, 100]    # max mode: every q above 0.5, the isf route


def get(case, key):
    a = VECTORS[f"{case}__{key}"]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def field(case):
    """The (T, C) input of a case in its dtype: codes * scale, -32768 = NaN (the generator's decode)."""
    codes, scale = get(case, "codes"), float(get(case, "scale"))
    dtype = np.float64 if META[case]["dtype"] == "f8" else np.float32
    x = codes.astype(dtype) * dtype(scale)
    x[codes == NAN_CODE] = np.nan
    x.setflags(write=False)
    return x


def budget(case):
    """fmin's maxfun = 200 N of a Nelder-Mead case: N = 3 parameters, 2 with floc."""
    return 200 * (2 if META[case]["floc"] is not None else 3)
