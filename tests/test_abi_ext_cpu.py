"""The C ABI of the headers under include/ext/ without a GPU: the ctypes table ``_capi.EXT_SIGNATURES`` against the declarations
(tests/stridedabi.py: header_declarations, is_ctypes_kind), the built library against the table, and the mirrors of the headers'
``#define``s.  The headers directly under include/ and ``_capi.SIGNATURES`` are the business of tests/test_abi_cpu.py."""
import ctypes
import glob
import inspect
import os
import re

import stridedabi as S
from xclim_amd import _capi

EXT = os.path.join(S.INCLUDE, "ext")
HEADERS = sorted(glob.glob(os.path.join(EXT, "*.h")))
DECLS = {os.path.basename(h): S.header_declarations(h) for h in HEADERS}


def _defines(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"^#define\s+(XH_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}


def test_the_headers_and_their_counts():
    assert [os.path.basename(h) for h in HEADERS] == ["xclim_hip_analog.h"]
    assert {h: len(d) for h, d in DECLS.items()} == {"xclim_hip_analog.h": 1}
    for h in HEADERS:
        assert '#include "../xclim_hip.h"' in open(h).read()


def test_every_declared_entry_point_is_in_the_table_with_the_kinds_of_its_declaration():
    for header, decls in DECLS.items():
        for name, decl in decls.items():
            sig = _capi.EXT_SIGNATURES.get(name)
            assert sig is not None, f"{name} has no ctypes prototype"
            assert len(decl) == len(sig), name
            assert decl[0][1] == "ctx"
            for (text, param), argtype in zip(decl, sig):
                assert S.is_ctypes_kind(text, argtype), (name, text, argtype)


def test_each_name_is_declared_once_and_in_one_table_only():
    declared = [name for d in DECLS.values() for name in d]
    assert len(declared) == len(set(declared)) and set(declared) == set(_capi.EXT_SIGNATURES)
    assert not set(_capi.EXT_SIGNATURES) & set(_capi.SIGNATURES)
    main = {name for h in S.HEADERS for name in S.header_declarations(h)}
    assert not set(declared) & main
    for header, path in zip(DECLS, HEADERS):
        text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for name in DECLS[header]:
            assert len(re.findall(rf"\b{name}\s*\(", text)) == 1, (header, name)
    source = inspect.getsource(_capi)   # a dict literal keeps the last of two equal keys without a word
    literal = source[source.index("EXT_SIGNATURES: dict[str, list] = {"):]
    literal = literal[:literal.index("\n}\n")]
    keys = re.findall(r'^\s*"(xh_\w+)":', literal, flags=re.M)
    assert keys == list(_capi.EXT_SIGNATURES)
    groups = re.findall(r"^\s*# include/ext/(xclim_hip\w*\.h) \(xclim_amd/csrc/(\w+\.hip)\)", literal, flags=re.M)
    assert groups == [("xclim_hip_analog.h", "analog.hip")]


def test_the_library_exports_every_name_with_the_table_s_argtypes():
    lib = _capi.load_library()
    for name, sig in _capi.EXT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes or ()) == sig, name
        assert fn.restype is _capi._RESTYPES.get(name, ctypes.c_int), name
    for name, sig in _capi.SIGNATURES.items():   # ... in addition to the 140 of the main table, which stay declared
        assert list(getattr(lib, name).argtypes or ()) == sig, name


def test_the_mirrors_of_the_defines():
    d = _defines(os.path.join(EXT, "xclim_hip_analog.h"))
    methods = {k[len("XH_ANALOG_"):].lower(): v for k, v in d.items()
               if k not in ("XH_ANALOG_NMETHODS", "XH_ANALOG_MAX_D", "XH_ANALOG_KS_MAX_D", "XH_ANALOG_MAX_SAMPLE", "XH_ANALOG_MAX_K", "XH_ANALOG_MAX_NK")}
    assert methods == _capi.ANALOG_METHODS and sorted(methods.values()) == list(range(d["XH_ANALOG_NMETHODS"]))
    assert d["XH_ANALOG_NMETHODS"] == _capi.ANALOG_NMETHODS == len(_capi.ANALOG_METHODS)
    assert (d["XH_ANALOG_MAX_D"], d["XH_ANALOG_KS_MAX_D"], d["XH_ANALOG_MAX_SAMPLE"], d["XH_ANALOG_MAX_K"], d["XH_ANALOG_MAX_NK"]) == (
        _capi.ANALOG_MAX_D, _capi.ANALOG_KS_MAX_D, _capi.ANALOG_MAX_SAMPLE, _capi.ANALOG_MAX_K, _capi.ANALOG_MAX_NK)
    assert len(d) == 14   # every #define of the header has a mirror above
    assert 2 * _capi.ANALOG_MAX_SAMPLE >= 366   # a year of daily samples against a year
