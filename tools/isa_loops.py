"""ISA audit of streaming loops: for every loop (a backward branch) of the named kernels in a gfx950 assembly file, count
the buffer/global loads, LDS ops, scratch (spill) accesses and `s_waitcnt vmcnt(0)` inside the loop body.  A scratch reload
inside a streaming loop is followed by vmcnt(0), which drains the loads in flight.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only -I xclim_amd/csrc x.hip -o x.s
  python tools/isa_loops.py x.s k_hs_fused

`kernels(path, pat)` gives the same figures as data (tests/test_isa_count_loop_cpu.py holds the one-year count kernel to
its loop shape with it).
"""
import re
import sys


def kernels(path, pat):
    """{kernel name: [loop, ...]} for the kernels whose mangled name contains `pat`; a loop is a dict of counts (see audit)."""
    lines = open(path).read().split("\n")
    out = {}
    # kernel bodies: from "<name>:" to ".Lfunc_end"
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and pat in m.group(1):
            name = m.group(1)
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[name] = audit(lines[i:j])
            i = j
        i += 1
    return out


def audit(body):
    label_at = {}
    for k, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = k
    loops = []
    for k, l in enumerate(body):
        m = re.search(r"\bs_cbranch_\w+\s+(\.LBB\d+_\d+)|\bs_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in label_at and label_at[tgt] <= k:
                loops.append((label_at[tgt], k, tgt))
    rows = []
    for a, b, tgt in sorted(loops):
        seg = body[a:b + 1]
        cnt = lambda rx, s=seg: sum(1 for l in s if re.search(rx, l))
        nload = cnt(r"\b(buffer_load|global_load|flat_load)")
        if nload == 0 and cnt(r"\bscratch_") == 0:
            continue
        rows.append(dict(label=tgt, first=a, last=b, instr=b - a, ld=nload, st=cnt(r"(buffer|global|flat)_store"), ds=cnt(r"\bds_"),
                         sl=cnt(r"scratch_load"), ss=cnt(r"scratch_store"), w0=cnt(r"vmcnt\(0\)"), valu=cnt(r"^\s+v_"),
                         # branches inside the body (the closing backward branch is not counted)
                         br=cnt(r"\bs_(c?branch|setpc|call)", seg[:-1]),
                         # an innermost loop holds no other loop
                         inner=not any(a <= a2 and b2 <= b and (a2, b2) != (a, b) for a2, b2, _ in loops)))
    return rows


def main():
    for name, rows in kernels(sys.argv[1], sys.argv[2]).items():
        print("==", name)
        for c in rows:
            print("  loop %-12s lines %6d-%6d (%5d instr)  vmem loads %3d  stores %3d  ds %4d  scratch ld/st %3d/%3d  vmcnt(0) %2d  "
                  "branches %2d  valu %5d" % (c["label"], c["first"], c["last"], c["instr"], c["ld"], c["st"], c["ds"], c["sl"], c["ss"],
                                              c["w0"], c["br"], c["valu"]))


if __name__ == "__main__":
    main()
