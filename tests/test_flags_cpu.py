"""The data-quality flags without a GPU: the numpy restatement tests/flagscpu.py reproduces the known answers of the reference's
own tests (tests/golden/flags_known_answers.json, with the defaults of tests/golden/flags_defaults.json); the names of the flags;
what the mirror does not serve; the mirrors of the header's #defines (tests/test_abi_cpu.py checks header, ctypes table and library).  ``check_known_answers`` and ``refusals`` are shared with
tests/test_gpu_flags.py (the device) and, through it, tests/test_hostsim_flags_cpu.py (the host simulation).

Every flag is a boolean: every comparison is exact."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import flagscpu as R
import stridedabi as S
from stridedabi import FLAGS_TABLE
from xclim_amd import _capi, dataflags
from xclim_amd.timeaxis import TimeAxis

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "xclim_hip_flags.h")
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "flags_known_answers.json")))
DEFAULTS = json.load(open(os.path.join(ROOT, "tests", "golden", "flags_defaults.json")))
K2C = 273.15
_vp = ctypes.c_void_p


# ---- the reference's known answers -------------------------------------------------------------------------------------------
def axis(rows):
    return TimeAxis.daily(KNOWN["axis"]["start"], rows, KNOWN["axis"]["calendar"])


def temperature_set(rows, dtype=np.float64):
    return {v: (off + K2C + np.sin(2 * np.pi * np.arange(rows) / 366)).astype(dtype)[:, None] for v, off in KNOWN["temperature_offsets"].items()}


def precipitation(case):
    pr = np.zeros(case["rows"])
    for kind, lo, hi, v in case["steps"]:
        if kind == "add_mm":
            pr[lo:hi] += v / 3600 / 24
        elif kind == "set_mm":
            pr[lo:hi] = v / 3600 / 24
        else:
            pr[lo:hi] = v
    return pr[:, None]


class Restated:
    """``data_flags`` of the restatement behind the signature ``mirror_api`` gives the mirror's."""

    @staticmethod
    def data_flags(da, ds, name, units, time, flags=None, raise_flags=False):
        out = R.data_flags(da, ds, flags, name=name, time=time, units=units, variables=DEFAULTS)
        if raise_flags and any(v is not None and v.any() for v in out.values()):
            plans = dataflags.describe(name, flags, ds, units, DEFAULTS)
            raise dataflags.DataQualityException(out, descriptions={k: v[1] for k, v in plans.items() if v is not None})
        return out

    @staticmethod
    def specific_discharge_extremely_high(da, thresh, units):
        return R.mask(da, dataflags._plan("specific_discharge_extremely_high", {"thresh": thresh}, "qspec", units)[0])


def mirror_api(dev):
    class Mirror:
        @staticmethod
        def data_flags(da, ds, name, units, time, flags=None, raise_flags=False):
            return dataflags.data_flags(da, ds, flags, raise_flags=raise_flags, name=name, time=time, units=units, variables=DEFAULTS, device=dev)

        @staticmethod
        def specific_discharge_extremely_high(da, thresh, units):
            return dataflags.specific_discharge_extremely_high(da, thresh=thresh, units=units, device=dev)

    return Mirror


def expect(got, want, what):
    assert list(got) == list(want) or set(got) == set(want), (what, list(got))
    for k, w in want.items():
        if w is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].dtype == bool and got[k].shape == () and bool(got[k]) is w, (what, k, got[k])


def check_known_answers(f=Restated, dtypes=(np.float64, np.float32)):
    n = 0
    for dtype in dtypes:     # the two temperature datasets hold in float32 as well
        case = KNOWN["tas_clean"]
        for sub in case["cases"]:
            fields = {k: v for k, v in temperature_set(case["rows"], dtype).items() if k not in sub["dropped"]}
            got = f.data_flags(fields["tas"], fields, "tas", case["units"], axis(case["rows"]))
            expect(got, dict(case["always"], **sub["expected"]), f"tas clean {sub['dropped']} {np.dtype(dtype).name}")
            n += 1
        case = KNOWN["tas_suspicious"]
        fields = temperature_set(case["rows"], dtype)
        fields["tasmin"], fields["tasmax"] = fields["tasmax"], fields["tasmin"]
        for lo, hi, c in case["set_celsius"]["tas"]:
            fields["tas"][lo:hi] = c + K2C
        expect(f.data_flags(fields["tas"], fields, "tas", case["units"], axis(case["rows"])), case["expected"], "tas suspicious")
        n += 1
    for key in ("pr_clean", "pr_suspicious"):
        case = KNOWN[key]
        pr = precipitation(case)
        expect(f.data_flags(pr, {"pr": pr}, "pr", case["units"], axis(case["rows"])), case["expected"], key)
        n += 1
    case = KNOWN["raises"]
    fields = {k: v for k, v in temperature_set(case["rows"]).items() if k in case["present"]}
    got = f.data_flags(fields["tasmax"], fields, "tasmax", case["units"], axis(case["rows"]), raise_flags=True)
    assert got["tas_exceeds_tasmax"] is None and not any(v.any() for v in got.values() if v is not None)
    fields["tasmin"], fields["tasmax"] = fields["tasmax"], fields["tasmin"]
    with pytest.raises(dataflags.DataQualityException, match=case["match"]) as err:
        f.data_flags(fields["tasmax"], fields, "tasmax", case["units"], axis(case["rows"]), raise_flags=True)
    assert str(err.value).startswith(case["message"]) and case["match"] in err.value.flags
    n += 1
    case = KNOWN["specific_discharge"]
    for sub in case["cases"]:
        q = np.full((case["rows"], 1), case["fill"], np.dtype(case["dtype"]))
        q[case["row"]] = sub["value"]
        got = f.specific_discharge_extremely_high(q, sub["thresh"], case["units"])
        assert got.shape == q.shape and got.dtype == bool and bool(got.any()) is sub["flagged"] and got.sum() == int(sub["flagged"]), sub
        n += 1
    assert n == 13
    return n


def test_restatement_reproduces_the_known_answers():
    check_known_answers()


def test_the_recorded_defaults():
    assert [next(iter(e)) for e in DEFAULTS["tas"]["data_flags"]] == [
        "temperature_extremely_high", "temperature_extremely_low", "tas_exceeds_tasmax", "tas_below_tasmin",
        "values_repeating_for_n_or_more_days", "outside_n_standard_deviations_of_climatology"]
    assert [next(iter(e)) for e in DEFAULTS["pr"]["data_flags"]].count("values_op_thresh_repeating_for_n_or_more_days") == 2
    checks = {c for v in DEFAULTS.values() for e in v["data_flags"] for c in e}
    assert checks <= set(dataflags.CHECK_NAMES) and len(dataflags.CHECK_NAMES) == 13
    assert "test_era5_ecad_qc_flag" in KNOWN["left_out"]


def test_the_names_of_the_flags():
    case = KNOWN["names"]
    (check, kwargs), = case["flags"].items()
    assert dataflags.flag_name(check, kwargs) == case["name"]
    assert list(dataflags.describe("pr", case["flags"], {}, "kg m-2 s-1")) == [case["name"]]
    names = {var: [dataflags.flag_name(c, k) for e in v["data_flags"] for c, k in e.items()] for var, v in DEFAULTS.items()}
    assert names["pr"] == ["negative_accumulation_values", "very_large_precipitation_events", "values_eq_5_repeating_for_5_or_more_days",
                           "values_eq_1_repeating_for_10_or_more_days"]
    assert names["sfcWind"] == ["wind_values_outside_of_bounds", "values_gt_2_repeating_for_6_or_more_days"]
    assert names["tas"][-2:] == ["values_repeating_for_5_or_more_days", "outside_5_standard_deviations_of_climatology"]
    f = dataflags.flag_name
    rep = "values_op_thresh_repeating_for_n_or_more_days"
    assert [f(rep, dict(n=3, thresh="2.5 m s-1", op=o)) for o in (">", "<", ">=", "<=", "==", "!=")] == [
        f"values_{o}_2point5_repeating_for_3_or_more_days" for o in ("gt", "lt", "ge", "le", "eq", "ne")]
    assert f(rep, dict(n=3, thresh=-2.0, op="le")) == "values_le_minus2_repeating_for_3_or_more_days"
    assert f(rep, dict(n=3, thresh="1e-3 mm/d", op="ne")) == "values_ne_0point001_repeating_for_3_or_more_days"
    assert f("outside_n_standard_deviations_of_climatology", dict(n=4)) == "outside_4_standard_deviations_of_climatology"
    with pytest.raises(TypeError, match="missing required"):
        f(rep, dict(n=3))
    with pytest.raises(TypeError, match="unexpected keyword"):
        f("negative_accumulation_values", dict(n=3))


def test_thresholds_in_the_units_of_the_field():
    c = dataflags.convert_threshold
    assert c("60 degC", "K") == 60 + K2C and c("-90 degC", "K") == -90 + K2C and c("300 K", "degC") == 300 - K2C and c("5 degC", "degC") == 5.0
    for v in (1, 5):     # the two rates the defaults of pr compare with ==
        assert c(f"{v} mm d-1", "kg m-2 s-1") == v / 3600 / 24 == v / 86400
    assert c("300 mm d-1", "mm/d") == 300.0 and c("2 mm/s", "mm/d") == 2 * 86400.0 and c("2 kg m-2 s-1", "mm/s") == 2.0
    assert c("46.0 m s-1", "m/s") == 46.0 and c(7, "anything") == 7.0 and c(np.float32(1.5), None) == 1.5 and c("3 Pa", "Pa") == 3.0


def test_what_is_not_served():
    t = TimeAxis.daily("1971-01-01", 1096)
    x = np.ones((1096, 2))
    NS = dataflags.NotServed
    with pytest.raises(NS, match="int64"):                                   # integer fields
        dataflags.negative_accumulation_values(x.astype(np.int64))
    with pytest.raises(NS, match="float32"):                                 # mixed dtypes in one call
        dataflags.tas_exceeds_tasmax(x, x.astype(np.float32))
    with pytest.raises(NS, match="array thresholds"):
        dataflags.temperature_extremely_high(x, thresh=x)
    with pytest.raises(NS, match="no conversion"):
        dataflags.temperature_extremely_high(x, thresh="100 degF", units="K")
    with pytest.raises(NS, match="no conversion"):
        dataflags.specific_discharge_extremely_high(x, units="m s-1")        # "100 mm d-1" as a speed is the reference's hydro context
    with pytest.raises(NS, match="needs the units"):
        dataflags.temperature_extremely_high(x)
    with pytest.raises(NS):                                                  # flags=None without the reference's table
        dataflags.data_flags(x, name="tas", time=t, units="K")
    gappy = t.subset(np.r_[0:10, 11:1096])
    clim = {"outside_n_standard_deviations_of_climatology": {"n": 5}}
    with pytest.raises(NS):
        dataflags.data_flags(x[:1095], flags=clim, name="tas", time=gappy)
    with pytest.raises(NS):
        dataflags.data_flags(x[:1095], flags={"negative_accumulation_values": None}, freq="YS", name="tas", time=gappy)
    with pytest.raises(NS, match="last day of year"):                        # 1971 alone: no day 366
        dataflags.data_flags(x[:365], flags=clim, name="tas", time=t.subset(slice(0, 365)))
    with pytest.raises(NS, match="dims"):
        dataflags.data_flags(x, flags={"negative_accumulation_values": None}, dims=("lat",), name="pr")
    with pytest.raises(NS, match="neither of its operands"):
        dataflags.data_flags(x, {"tasmax": x, "tasmin": x}, {"tasmax_below_tasmin": None}, name="tas")
    with pytest.raises(ValueError, match="at least 1"):
        dataflags.values_repeating_for_n_or_more_days(x, n=0)
    with pytest.raises(NotImplementedError):
        dataflags.values_op_thresh_repeating_for_n_or_more_days(x, n=2, thresh=1.0, op="approx")
    assert dataflags.data_flags(x, name="rls", variables=DEFAULTS) == {}
    with pytest.raises(NotImplementedError, match="do not exist for 'rls'"):
        dataflags.data_flags(x, name="rls", variables=DEFAULTS, raise_flags=True)
    assert dataflags.ADAPTED == ("data_flags",) and dataflags.FLAGS_MAX_CHECKS == _capi.FLAGS_MAX_CHECKS == 16
    assert "#define XH_FLAGS_MAX_CHECKS 16" in open(HEADER).read()


def test_no_launch_for_nothing_to_do():
    """No rows or no cells: the mirror answers without a device."""
    t = TimeAxis.daily("1971-01-01", 0)
    got = dataflags.data_flags(np.ones((0, 3)), flags=DEFAULTS["pr"]["data_flags"], name="pr", time=t, units="kg m-2 s-1", device=object())
    assert len(got) == 4 and all(v.shape == () and not v for v in got.values())
    got = dataflags.data_flags(np.ones((5, 0)), flags=DEFAULTS["hurs"]["data_flags"], dims=None, name="hurs", device=object())
    assert got["percentage_values_outside_of_bounds"].shape == (5, 0)


# ---- the C ABI (tests/test_abi_cpu.py checks the header against the ctypes table, the library and the registry) ---------
def test_the_unit_is_built_and_its_operand_table_is_the_header_s():
    assert set(S.prototypes(HEADER)) == set(FLAGS_TABLE)
    make = open(os.path.join(ROOT, "xclim_amd", "csrc", "Makefile")).read()
    assert "dataflags.hip" in make and "xclim_hip_flags.h" in make
    txt = open(HEADER).read()
    assert '#include "xclim_hip.h"' in txt and "ASSUMPTION" in txt
    assert len(re.findall(r"/\* host \*/", txt)) == 4                     # the host tables are marked


def test_the_check_kinds_and_the_check_record_mirror_the_header():
    txt = open(HEADER).read()
    kinds = (_capi.FLAG_CMP, _capi.FLAG_OUTSIDE, _capi.FLAG_PAIR, _capi.FLAG_REPEAT, _capi.FLAG_CLIM)
    assert kinds == (0, 1, 2, 3, 4)
    for code, name in zip(kinds, ("CMP", "OUTSIDE", "PAIR", "REPEAT", "CLIM")):
        assert re.search(rf"#define XH_FLAG_{name} {code}\b", txt)
    # struct xh_flag_check { int32_t kind, op, n, other; double a, b; }: 32 bytes, the numpy record of _capi
    dt = _capi.FLAG_CHECK_DTYPE
    assert dt.itemsize == 32 and dt.names == ("kind", "op", "n", "other", "a", "b") and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 24]
    body = re.search(r"typedef struct xh_flag_check \{(.*?)\} xh_flag_check;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(int32_t|double)\s+([\w, ]+);", body) == [("int32_t", "kind"), ("int32_t", "op"), ("int32_t", "n"), ("int32_t", "other"),
                                                                 ("double", "a, b")]


def test_entry_points_reject_a_null_context():
    lib = _capi.load_library()
    null, some = _vp(0), _vp(64)   # never dereferenced: the check fails first
    assert lib.xh_data_flags(null, 10, 4, 4, 0, some, null, 4, null, 4, 1, some, 1, some, null, 0, null, null, 4, 0, some, 4) == _capi.XH_ERR_ARG
    assert lib.xh_doy_bounds(null, 10, 4, 4, 0, some, some, 1, 10, 5, 5.0, some, some, 4) == _capi.XH_ERR_ARG


def checks_of(*rows):
    """A host array of xh_flag_check from (kind, op, n, other, a, b) rows."""
    return np.array(list(rows), dtype=_capi.FLAG_CHECK_DTYPE).reshape(-1)


def refusals(dev):
    """Every refusal is a code that answers before anything is launched: the sentinel in the outputs is intact afterwards, and the
    same call with nothing wrong then runs.  On the device (tests/test_gpu_flags.py) and, through it, on the host simulation."""
    from newunit_cases import shared_refusals

    ARG, LAYOUT, LIMIT = _capi.XH_ERR_ARG, _capi.XH_ERR_LAYOUT, _capi.XH_ERR_LIMIT
    T, C, P, D = 40, 8, 2, 5
    x = dev.to_device(np.linspace(1.0, 9.0, T * C).reshape(T, C))
    tab = dev.to_device(np.full((D, C), 5.0))
    out = dev.to_device(np.full((16 * P, C), 7, np.uint8))
    p = lambda a: _vp(0) if a is None else a.ctypes.data_as(_vp)  # noqa: E731
    d = lambda a: _vp(0) if a is None else _vp(a.ptr)             # noqa: E731
    seg = np.array([0, 20, T], np.int64)
    tidx = (np.arange(T) % D).astype(np.int32)
    CMP, OUT, PAIR, REP, CLIM = range(5)
    good = checks_of((CMP, 0, 0, 0, 5.0, 0.0))
    df, db = (getattr(dev.lib, n) for n in FLAGS_TABLE)

    def flags(ld=C, ld_out=C, seg=seg, P=P, xx=x, y0=None, y1=None, ld_y0=C, ld_y1=C, chk=good, K=None, tidx=tidx, D=D, lo=tab, hi=tab, ld_tab=C,
              red=0, o=out, T=T, C=C, ctx=dev.ctx):
        return df(ctx, T, C, ld, 1, d(xx), d(y0), ld_y0, d(y1), ld_y1, len(chk) if K is None else K, p(chk), P, p(seg), p(tidx), D, d(lo), d(hi),
                  ld_tab, red, d(o), ld_out)

    assert flags(xx=None) == ARG and flags(o=None) == ARG and flags(chk=None, K=1) == ARG and flags(K=-1) == ARG and flags(P=-1) == ARG
    many = checks_of(*[(CMP, 0, 0, 0, 5.0, 0.0)] * 17)
    assert flags(chk=many) == LIMIT                                                          # K > 16
    assert flags(chk=checks_of((5, 0, 0, 0, 0.0, 0.0))) == ARG and flags(chk=checks_of((-1, 0, 0, 0, 0.0, 0.0))) == ARG     # an unknown kind
    for kind in (CMP, PAIR, REP):                                                            # an unknown operator
        assert flags(chk=checks_of((kind, 6, 1, 0, 0.0, 0.0)), y0=x) == ARG and flags(chk=checks_of((kind, -2, 1, 0, 0.0, 0.0)), y0=x) == ARG
    assert flags(chk=checks_of((CMP, -1, 0, 0, 0.0, 0.0))) == ARG                            # "no threshold" is REPEAT's alone
    assert flags(chk=checks_of((PAIR, 0, 0, 0, 0.0, 0.0))) == ARG                            # PAIR without its companion
    assert flags(chk=checks_of((PAIR, 0, 0, 1, 0.0, 0.0)), y0=x) == ARG and flags(chk=checks_of((PAIR, 0, 0, 2, 0.0, 0.0)), y0=x, y1=x) == ARG
    assert flags(chk=checks_of((PAIR, 0, 0, 0, 0.0, 0.0)), y0=x, ld_y0=C - 1) == LAYOUT
    assert flags(chk=checks_of((REP, -1, 0, 0, 0.0, 0.0))) == ARG and flags(chk=checks_of((REP, 4, -3, 0, 0.0, 0.0))) == ARG     # n < 1
    clim = checks_of((CLIM, 0, 0, 0, 0.0, 0.0))
    assert flags(chk=clim, lo=None) == ARG and flags(chk=clim, hi=None) == ARG and flags(chk=clim, tidx=None) == ARG    # CLIM without tables / tidx
    assert flags(chk=clim, D=0) == ARG and flags(chk=clim, ld_tab=C - 1) == LAYOUT
    bad = tidx.copy()
    bad[T - 1] = D
    assert flags(chk=clim, tidx=bad) == ARG                                                  # tidx outside [0, D)
    bad[T - 1] = -1
    assert flags(chk=clim, tidx=bad) == ARG
    assert flags(seg=np.array([1, 20, T], np.int64)) == ARG and flags(seg=np.array([0, 20, T - 1], np.int64)) == ARG    # seg does not cover [0, T]
    shared_refusals(flags, T, C, [("seg", seg, T, None)])

    tb = np.arange(T, dtype=np.int32).reshape(2, 20)

    def bounds(ld=C, ld_out=C, xx=x, tbase=tb, ny=2, nd=20, w=5, lo=out, hi=out, T=T, C=C, ctx=dev.ctx):
        return db(ctx, T, C, ld, 1, d(xx), p(tbase), ny, nd, w, 5.0, d(lo), d(hi), ld_out)

    assert bounds(xx=None) == ARG and bounds(tbase=None) == ARG and bounds(lo=None) == ARG and bounds(hi=None) == ARG
    assert bounds(ny=0) == ARG and bounds(nd=-1) == ARG and bounds(w=0) == ARG
    far = tb.copy()
    far[1, 19] = T
    assert bounds(tbase=far) == ARG
    far[1, 19] = -2
    assert bounds(tbase=far) == ARG
    shared_refusals(bounds, T, C)

    dev.sync()
    np.testing.assert_array_equal(out.get(), np.full((16 * P, C), 7, np.uint8))         # nothing was launched: the sentinels are intact
    assert flags() == 0 and flags(chk=clim) == 0
    dev.sync()
    got = out.get()
    assert (got[:P] == 1).all() and (got[P:] == 7).all()                                 # (5 is not strictly inside (5, 5))
