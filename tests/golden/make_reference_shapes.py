"""Record, with ``ast``, two tables of facts about the reference sources for tests/test_host_cpu.py:

    reference_signatures.json  — the parameter list (positional, keyword-only, variadic names) of every top-level function
                                 of the modules whose functions the DataArray-level wrappers replace
    reference_call_sites.json  — every call of a bare name or of ``rl.<attr>`` inside the index functions of
                                 indices/{_threshold,_multivariate,_simple}.py: [file, function, line, callee, number of
                                 positional arguments, keyword names ("**" for a ``**mapping``)]

Run where the reference tree exists (the same tree as make_call_programs.py):

    python tests/golden/make_reference_shapes.py           # (re)write both files
    python tests/golden/make_reference_shapes.py --check   # exit 1 when a stored file differs from a fresh recording

Only names and counts are stored, no source: the tests compare the wrappers' signatures and the recorded call programs
against these tables, so they hold without the reference tree.
"""

import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_call_programs import REF  # noqa: E402

SIGNATURE_MODULES = ("indices/generic.py", "core/calendar.py", "indices/run_length.py", "core/utils.py")
INDEX_MODULES = ("_threshold.py", "_multivariate.py", "_simple.py")


def _parse(rel):
    with open(os.path.join(REF, rel)) as f:
        return ast.parse(f.read())


def signatures():
    out = {}
    for rel in SIGNATURE_MODULES:
        out[rel] = {}
        for n in _parse(rel).body:
            if isinstance(n, ast.FunctionDef):
                a = n.args
                out[rel][n.name] = {"args": [x.arg for x in a.posonlyargs + a.args], "kwonly": [x.arg for x in a.kwonlyargs],
                                    "vararg": a.vararg.arg if a.vararg else None, "kwarg": a.kwarg.arg if a.kwarg else None}
    return out


def call_sites():
    out = []
    for f in INDEX_MODULES:
        for fn in (n for n in _parse(os.path.join("indices", f)).body if isinstance(n, ast.FunctionDef)):
            for node in (n for n in ast.walk(fn) if isinstance(n, ast.Call)):
                if isinstance(node.func, ast.Name):
                    name = node.func.id
                elif isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name) and node.func.value.id == "rl":
                    name = "rl." + node.func.attr
                else:
                    continue
                out.append([f, fn.name, node.lineno, name, len(node.args), [k.arg or "**" for k in node.keywords]])
    return sorted(out, key=lambda s: (s[0], s[2], s[3], s[4], s[5]))


TABLES = {"reference_signatures.json": signatures, "reference_call_sites.json": call_sites}


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not present; the tables can only be recorded where it exists")
    check = "--check" in sys.argv[1:]
    stale = []
    for fname, make in TABLES.items():
        fresh = json.loads(json.dumps(make()))
        path = os.path.join(HERE, fname)
        if check:
            with open(path) as f:
                if json.load(f) != fresh:
                    stale.append(fname)
            continue
        with open(path, "w") as f:   # (one function / one call site per line)
            if isinstance(fresh, dict):
                f.write("{\n" + ",\n".join(f"{json.dumps(rel)}: {{\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(s)}" for n, s in sigs.items())
                                           + "\n}" for rel, sigs in fresh.items()) + "\n}\n")
            else:
                f.write("[\n" + ",\n".join(json.dumps(s) for s in fresh) + "\n]\n")
        print(f"{fname}: {sum(len(v) for v in fresh.values()) if isinstance(fresh, dict) else len(fresh)} entries")
    if stale:
        sys.exit(f"stale (regenerate with python tests/golden/make_reference_shapes.py): {', '.join(stale)}")


if __name__ == "__main__":
    main()
