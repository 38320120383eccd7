"""The C ABI without a GPU, for every header under include/: the ctypes table ``_capi.SIGNATURES`` against the declarations
(tests/stridedabi.py: header_declarations, is_ctypes_kind), the built library against the table, and the operand registry of
tests/stridedabi.py against the unit headers.  A new unit adds its header, its rows in SIGNATURES, its operands in stridedabi and
its count to COUNTS; nothing here is copied."""
import ctypes
import inspect
import os
import re

import pytest

import stridedabi as S
from xclim_amd import _capi

NAMES = [os.path.basename(h) for h in S.HEADERS]
DECLS = {os.path.basename(h): S.header_declarations(h) for h in S.HEADERS}
COUNTS = {"xclim_hip.h": 125, "xclim_hip_agro.h": 5, "xclim_hip_flags.h": 2, "xclim_hip_hydro.h": 4, "xclim_hip_phase.h": 2,
          "xclim_hip_rain.h": 2}
# xh_data_flags reads two companion fields and a pair of bound tables, each with a pitch of its own next to ld and ld_out
EXTRA_PITCHES = {"xh_data_flags": {"ld_y0", "ld_y1", "ld_tab"}}


def test_the_headers_and_their_counts():
    assert NAMES == list(COUNTS)
    assert {h: len(d) for h, d in DECLS.items()} == COUNTS


@pytest.mark.parametrize("header", NAMES)
def test_every_declared_entry_point_is_in_the_table_with_the_kinds_of_its_declaration(header):
    assert DECLS[header]
    for name, decl in DECLS[header].items():
        sig = _capi.SIGNATURES.get(name)
        assert sig is not None, f"{name} has no ctypes prototype"
        assert len(decl) == len(sig), name
        for (text, param), argtype in zip(decl, sig):
            assert S.is_ctypes_kind(text, argtype), (name, text, argtype)


def test_no_name_is_declared_twice_and_the_table_holds_exactly_the_declared_names():
    declared = [name for d in DECLS.values() for name in d]
    assert len(declared) == len(set(declared)) == 140
    assert set(declared) == set(_capi.SIGNATURES)
    assert set(S.PROTOS) == set(DECLS["xclim_hip.h"]) and set(S.UNIT_PROTOS) == set(declared) - set(S.PROTOS)
    for header, text in ((h, open(p).read()) for h, p in zip(NAMES, S.HEADERS)):   # a header declares each of its names once
        for name in DECLS[header]:
            assert len(re.findall(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))) == 1, (header, name)


def test_no_key_is_written_twice_in_the_literal():
    """A dict literal keeps the last of two equal keys without a word: the keys of the source against the dict."""
    source = inspect.getsource(_capi)
    literal = source[source.index("SIGNATURES: dict[str, list] = {"):]
    literal = literal[:literal.index("\n}\n")]
    keys = re.findall(r'^\s*"(xh_\w+)":', literal, flags=re.M)
    assert len(keys) == len(set(keys)) == len(_capi.SIGNATURES) == 140, sorted(k for k in set(keys) if keys.count(k) > 1)
    assert keys == list(_capi.SIGNATURES)
    groups = re.findall(r"^\s*# include/(xclim_hip\w*\.h) \(", literal, flags=re.M)   # one comment line per header over its rows
    assert sorted(groups) == NAMES


def test_the_library_exports_every_name_with_the_table_s_argtypes():
    lib = _capi.load_library()
    assert set(_capi._RESTYPES) <= set(_capi.SIGNATURES)
    for name, sig in _capi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes or ()) == sig, name
        assert fn.restype is _capi._RESTYPES.get(name, ctypes.c_int), name


@pytest.mark.parametrize("header", NAMES[1:])
def test_every_pointer_and_pitch_of_a_unit_header_is_in_the_registry(header):
    assert '#include "xclim_hip.h"' in open(os.path.join(S.INCLUDE, header)).read()
    for name, decl in DECLS[header].items():
        names = [n for _, n in decl]
        text = dict((n, t) for t, n in decl)
        assert names == S.UNIT_PROTOS[name] and names[0] == "ctx"
        ops = S.PITCHED[name]
        assert len({op.ptr for op in ops}) == len(ops), name
        listed = {op.ptr for op in ops} | set(S.HOST_TABLES[name])
        pointers = {n for n in names if "*" in text[n] and n != "ctx"}
        assert pointers == listed, (name, pointers ^ listed)
        pitches = {n for n in names if n.startswith("ld")}
        assert pitches == {op.stride for op in ops} == {"ld", "ld_out"} | EXTRA_PITCHES.get(name, set()), name
        for op in ops:                             # inputs are const, outputs are not
            assert op.mode in ("r", "w") and ("const" in text[op.ptr].split("*")[0]) == (op.mode == "r"), (name, op.ptr)
        for t in S.HOST_TABLES[name]:              # the host tables and the dense inputs are const
            assert "const" in text[t].split("*")[0], (name, t)


def test_the_registry_names_the_unit_headers_and_the_pitched_units_of_the_main_header():
    assert set(S.HOST_TABLES) == set(S.UNIT_PROTOS) == set(S.PITCHED) - set(S.PROTOS)
    assert set(S.PITCHED) & set(S.PROTOS) == {"xh_chill_hourly", "xh_chill_daily", "xh_bioclim"} and not set(S.PITCHED) & set(S.TABLE)
    for header, table in zip(NAMES[1:], (S.AGRO_TABLE, S.FLAGS_TABLE, S.HYDRO_TABLE, S.PHASE_TABLE, S.RAIN_TABLE)):
        assert set(table) == set(DECLS[header]), header
    for name, ops in S.PITCHED.items():            # every entry names parameters of its prototype, in its expressions too
        params = S.parameters(name)[1:]
        for op in ops:
            assert {op.ptr, op.stride} <= set(params) and op.minor is None, (name, op)
            for expr in (op.rows, op.width, op.dtype, op.ptrs):
                if isinstance(expr, str) and expr not in S._DTYPES:
                    used = set(compile(expr, name, "eval").co_names)
                    assert used <= set(params), f"{name}: {expr!r} uses {sorted(used - set(params))}"
