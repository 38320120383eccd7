"""The batch loop of the one-year day-of-year count kernel (k_tcount_year, reduce.hip) keeps its shape in the gfx950 ISA: every
load of a batch of R rows (R float4 samples + 2R double2 table pieces) is issued before the first is consumed, so the
batch pays ONE memory latency.  A compiler or a batch-size change that re-serialises the loads (R = 8 does: the scheduler
trades the batch for registers) costs 7 % of the tx90p headline silently; here it fails a test.  Cross-compiled: no GPU
needed, skipped only without hipcc."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xclim_amd", "csrc")


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def reduce_asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("isa") / "reduce.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "reduce.hip"), "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def test_count_year_batch_loop_shape(reduce_asm):
    R = int(re.search(r"#define XH_TCY_R (\d+)", open(os.path.join(CSRC, "reduce.hip")).read()).group(1))
    ks = _isa_loops().kernels(reduce_asm, "k_tcount_year")
    assert len(ks) == 12, sorted(ks)  # six operators x (period bounds in the arguments | uploaded)
    for name, loops in ks.items():
        assert all(l["sl"] == 0 and l["ss"] == 0 for l in loops), (name, loops)  # no scratch anywhere in the march
        inner = [l for l in loops if l["inner"]]
        batch = max(inner, key=lambda l: l["ld"])
        print(name, batch)
        assert batch["ld"] == 3 * R, (name, batch)   # R samples + 2R table pieces, nothing reloaded
        assert batch["br"] == 0, (name, batch)       # no branch inside the batch
        assert batch["w0"] <= 1, (name, batch)       # one drain per batch at the most
        assert batch["st"] == 0 and batch["ds"] == 0, (name, batch)


def test_count_year_kernels_have_no_scratch(reduce_asm):
    text = open(reduce_asm).read()
    sizes = re.findall(r"\.set (_Z\w*k_tcount_year\w*)\.private_seg_size, (\d+)", text)
    assert len(sizes) == 12, sizes
    assert all(int(s) == 0 for _, s in sizes), sizes
