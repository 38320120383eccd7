#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, object file by object file (CPU only).

    python tools/device_code_diff.py OLD/build NEW/build

Per `*.o` of either directory: the `.hip_fatbin` section is dumped (llvm-objcopy), the gfx950 code object unbundled
(clang-offload-bundler), and its FUNC symbols read (llvm-readelf).  Reported per object file: kernel names present on one
side only, kernels whose bytes inside .text (symbol value .. value + size) differ, and kernels whose AMDGPU metadata note
(register counts, LDS and private-segment sizes, argument layout) differs.  Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """{kernel name: (bytes of its code, its metadata text)} of one host object file; {} when it holds no device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    if ".hip_fatbin" not in _run("llvm-readelf", "-SW", obj):   # (a unit of host code only)
        return {}
    _run("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o"))
    _run("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    if os.path.getsize(co) == 0:
        return {}
    text = None   # (address, file offset) of .text
    for line in _run("llvm-readelf", "-SW", co).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (int(m.group(1), 16), int(m.group(2), 16))
    blob = open(co, "rb").read()
    code = {}
    for line in _run("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            off = int(f[1], 16) - text[0] + text[1]
            code[f[7]] = blob[off:off + int(f[2], 0)]
    # the metadata note is YAML: one "- .agpr_count: ... " entry per kernel under amdhsa.kernels, keyed by .name
    meta, notes = {}, _run("llvm-readelf", "--notes", co)
    kernels = notes.split("amdhsa.kernels:", 1)[-1].split("amdhsa.target:", 1)[0]
    for entry in re.split(r"\n  - ", "\n" + kernels)[1:]:
        m = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if m:
            meta[m.group(1).strip("'\"")] = entry.strip()   # (the last entry carries the end of the list)
    return {k: (v, meta.get(k, "")) for k, v in code.items()}


def main(old_dir, new_dir):
    names = sorted({f for d in (old_dir, new_dir) for f in os.listdir(d) if f.endswith(".o")})
    bad = total = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            paths = [os.path.join(d, name) for d in (old_dir, new_dir)]
            if not all(map(os.path.exists, paths)):
                print(f"{name}: only in {old_dir if os.path.exists(paths[0]) else new_dir}")
                bad += 1
                continue
            old, new = (code_object(p, tmp) for p in paths)
            only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
            both = sorted(set(old) & set(new))
            code = [k for k in both if old[k][0] != new[k][0]]
            meta = [k for k in both if old[k][1] != new[k][1]]
            total += len(both)
            bad += len(only_old) + len(only_new) + len(code) + len(meta)
            print(f"{name}: {len(both)} kernels on both sides, {len(only_old)} only old, {len(only_new)} only new, "
                  f"{len(code)} differ in code, {len(meta)} differ in metadata")
            for what, ks in (("only old", only_old), ("only new", only_new), ("code differs", code), ("metadata differs", meta)):
                for k in ks:
                    print(f"    {what}: {k}")
    print(f"TOTAL: {len(names)} object files, {total} kernels compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
