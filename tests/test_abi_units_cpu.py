"""The C ABI of the headers under include/units/ without a GPU: the ctypes table ``_capi.UNIT_SIGNATURES`` against the declarations
(tests/stridedabi.py: header_declarations, is_ctypes_kind), the built library against the table, and the mirrors of the headers'
``#define``s.  What tests/test_abi_ext_cpu.py checks for include/ext/, written so that the next unit does not edit this module:
the headers come from the directory and from the group comments of the table, and the two lists must agree; the mirrors of a
header are its entry in ``_capi.UNIT_DEFINES``."""
import ctypes
import glob
import inspect
import os
import re

import stridedabi as S
from xclim_amd import _capi

UNITS = os.path.join(S.INCLUDE, "units")
HEADERS = sorted(glob.glob(os.path.join(UNITS, "*.h")))
DECLS = {os.path.basename(h): S.header_declarations(h) for h in HEADERS}
CSRC = os.path.join(os.path.dirname(S.INCLUDE), "xclim_amd", "csrc")


def _table_literal():
    source = inspect.getsource(_capi)   # a dict literal keeps the last of two equal keys without a word
    literal = source[source.index("UNIT_SIGNATURES: dict[str, list] = {"):]
    return literal[:literal.index("\n}\n")]


def _groups():
    """[(header, .hip file, [entry points])] from the group comments of the table and the keys under each."""
    groups = []
    for line in _table_literal().splitlines()[1:]:
        m = re.match(r"^\s*# include/units/(xclim_hip\w*\.h) \(xclim_amd/csrc/(\w+\.hip)\)", line)
        if m:
            groups.append((m.group(1), m.group(2), []))
            continue
        k = re.match(r'^\s*"(xh_\w+)":', line)
        if k:
            assert groups, f"{k.group(1)} stands before the first group comment"
            groups[-1][2].append(k.group(1))
    return groups


def _defines(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"^#define\s+(XH_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}


def test_the_directory_and_the_group_comments_name_the_same_headers():
    assert HEADERS, "include/units/ holds no header"
    groups = _groups()
    assert sorted(g[0] for g in groups) == [os.path.basename(h) for h in HEADERS]
    assert len({g[0] for g in groups}) == len(groups)
    for header, hip, names in groups:
        assert names == list(DECLS[header]), f"{header}: the rows of its group are its declarations, in the header's order"
        assert os.path.exists(os.path.join(CSRC, hip)), hip
        assert f"include/units/{header}" in open(os.path.join(CSRC, hip)).read()
    for h in HEADERS:
        assert '#include "../xclim_hip.h"' in open(h).read()
        assert DECLS[os.path.basename(h)], f"{h} declares no entry point"
        assert f"include/units/{os.path.basename(h)}" in open(os.path.join(CSRC, "Makefile")).read()


def test_every_declared_entry_point_is_in_the_table_with_the_kinds_of_its_declaration():
    for header, decls in DECLS.items():
        for name, decl in decls.items():
            sig = _capi.UNIT_SIGNATURES.get(name)
            assert sig is not None, f"{name} has no ctypes prototype"
            assert len(decl) == len(sig), name
            assert decl[0][1] == "ctx"
            for (text, param), argtype in zip(decl, sig):
                assert S.is_ctypes_kind(text, argtype), (name, text, argtype)


def test_each_name_is_declared_once_and_in_one_table_only():
    declared = [name for d in DECLS.values() for name in d]
    assert len(declared) == len(set(declared)) and set(declared) == set(_capi.UNIT_SIGNATURES)
    assert not set(_capi.UNIT_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.EXT_SIGNATURES))
    others = {name for h in S.HEADERS + sorted(glob.glob(os.path.join(S.INCLUDE, "ext", "*.h"))) for name in S.header_declarations(h)}
    assert not set(declared) & others
    for header, path in zip(DECLS, HEADERS):
        text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for name in DECLS[header]:
            assert len(re.findall(rf"\b{name}\s*\(", text)) == 1, (header, name)
    keys = re.findall(r'^\s*"(xh_\w+)":', _table_literal(), flags=re.M)
    assert keys == list(_capi.UNIT_SIGNATURES)


def test_the_library_exports_every_name_with_the_table_s_argtypes():
    lib = _capi.load_library()
    for name, sig in _capi.UNIT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes or ()) == sig, name
        assert fn.restype is _capi._RESTYPES.get(name, ctypes.c_int), name
    for table in (_capi.SIGNATURES, _capi.EXT_SIGNATURES):   # ... in addition to the other two tables, which stay declared
        for name, sig in table.items():
            assert list(getattr(lib, name).argtypes or ()) == sig, name


def test_the_mirrors_of_the_defines():
    assert sorted(_capi.UNIT_DEFINES) == [os.path.basename(h) for h in HEADERS]
    for h in HEADERS:
        defines = _defines(h)
        assert defines, h
        assert defines == _capi.UNIT_DEFINES[os.path.basename(h)], os.path.basename(h)
        # no #define of the header escapes the pattern above (a value that is not a plain integer would have no mirror)
        text = re.sub(r"/\*.*?\*/", " ", open(h).read(), flags=re.S)
        assert len(re.findall(r"^#define\s+XH_\w+\s+\S", text, flags=re.M)) == len(defines), h


def test_ext_call_finds_both_extension_tables():
    from xclim_amd import kernels as K

    calls = []

    class Dev:
        def call(self, name, *args):
            calls.append((name, args))

    for table in (_capi.EXT_SIGNATURES, _capi.UNIT_SIGNATURES):
        name, sig = next(iter(table.items()))
        K._ext_call(Dev(), name, *([0] * (len(sig) - 1)))
        assert calls[-1][0] == name and [type(a) for a in calls[-1][1]] == sig[1:]
    try:
        K._ext_call(Dev(), name, *([0] * len(sig)))
    except TypeError as err:
        assert f"{len(sig) - 1} arguments" in str(err)
    else:
        raise AssertionError("a wrong argument count was accepted")
