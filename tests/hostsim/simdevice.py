"""A Device whose C ABI is the HOST SIMULATION build of the translation units that need neither LDS nor wave intrinsics
(tests/hostsim/hip/hip_runtime.h: every kernel runs thread by thread on the CPU).  Test infrastructure for the `-m "not gpu"`
tier only — it pins kernel arithmetic and entry-point dispatch against the oracle on machines without a GPU; entry points
that are not simulated raise (never a silent no-op), and nothing of this is reachable from the product package."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
CSRC = os.path.join(ROOT, "xclim_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mock_device import MockDevice, _MockLib  # noqa: E402
from xclim_amd import _capi  # noqa: E402

SIMULATED_UNITS = ("detrend", "window", "runlen", "reduce", "spell", "elemwise", "eqm", "plane", "wquantile",
                   # one cell (or cell pair) per lane, no traffic between lanes; stdidx.hip's k_si_fit stages every lane's sample in
                   # a private LDS column (lds + threadIdx.x, stride FIT_BLOCK): its `extern __shared__` becomes the launch's block
                   "fire", "ffdi", "pet", "stdidx", "f64red")
# the units that joined together with the stand-alone sanitizer driver (tests/hostsim/standalone)
NEW_UNITS = ("fire", "ffdi", "pet", "stdidx", "f64red", "f64run")
NEW_ENTRY_POINTS = (
    "xh_fire_weather", "xh_overwintering_dc", "xh_mcarthur", "xh_solar_table", "xh_pet_month_table", "xh_pet_daily", "xh_pet_monthly",
    "xh_si_fit", "xh_si_apply", "xh_si_fit_f64", "xh_si_apply_f64", "xh_thresholded_reduce_f64", "xh_range_reduce_f64",
    "xh_domain_count_f64", "xh_bivariate_count_f64", "xh_rolling_reduce_f64", "xh_compare_map_f64", "xh_run_stats_f64",
    "xh_spell_mask_f64", "xh_spell_run_stats_f64", "xh_run_stats_doy_f64", "xh_percentile_doy_f64")
# compiled, but their kernels (or the selection kernels behind them) speak to the wave: refused
WAVE_ENTRY_POINTS = ()
# eqm.hip votes `__all(m == nq)` only to pick between two forms that are each right for the lane that takes them
UNIT_DEFINES = {"eqm": ["-D__all(x)=((x)!=0)"],
                # plane.hip appends to its work lists wave by wave and keeps lane-private LDS columns: see wave_of_one.h
                "plane": ["-include", os.path.join(HERE, "wave_of_one.h")],
                # wquantile.hip's LDS arrays are lane-private columns ([i * 64 + lane]): static arrays do
                "wquantile": ["-D__shared__=static"],
                # (the dynamic LDS of a launch as a heap block of exactly its size: simt.h)
                "f64run": ["-DSIM_EXACT_DYN_LDS=1"], "hydro": ["-DSIM_EXACT_DYN_LDS=1"], "rainseason": ["-DSIM_EXACT_DYN_LDS=1"]}
# thread-by-thread units that declare dynamic LDS (lane-private columns): the declaration is rewritten as in the fiber units
DYN_LDS_UNITS = ("stdidx",)


# units whose kernels talk through LDS / the wave in WAVE-UNIFORM control flow: every workgroup as a set of fibers (simt.h).
# This is also the fiber half of the shared library that build() makes.
FIBER_UNITS = ("f64", "select", "select5", "tcount", "qdm", "quantile", "doystats", "core", "reduce2", "pdoy_top", "pdoy_quad", "pdoy_walk", "select3", "qdm2", "select2", "select4", "winsel",
               # f64run.hip: k_percentile_doy_f64 sorts its columns in LDS by all threads of the workgroup (barriers, an LDS atomicAdd)
               "f64run")
# How a unit is compiled is one thing, which library holds it another: these are compiled on fibers as well, but only the unit
# libraries below hold them.  unit -> the number of `extern __shared__` declarations that must be rewritten, no more and no fewer.
#   hydro.hip: k_sen_slope sorts its slopes in LDS by the whole workgroup (barriers)
#   rainseason.hip: the ring of k_rain_season is dynamic LDS, so that a ring slot past the ring lands outside the heap block
UNIT_LIBRARY_FIBER_UNITS = {"hydro": 3, "rainseason": 1}

# The small simulation libraries of single units (libxclimhip_hostsim_<name>.so: the unit, unchanged, the units of the entry points
# its GPU tests also call, and sim_runtime.cpp; the shared library of build() is left as it is) and their stand-alone sanitizer
# programs: name -> (units of the library, units of the driver, driver source under standalone/).
UNIT_LIBRARIES = {
    # chill.hip has one lane per (cell, period) and no traffic between lanes: thread by thread.  pet.hip: xh_solar_table gives
    # the day lengths.
    "chill": (("chill", "pet"), (), None),
    # bioclim.hip: one lane per (cell, period), thread by thread.  f64.hip (xh_resample_reduce_f64) and f64red.hip
    # (xh_range_reduce_f64) hold the entry points the cross-checks call.
    "bioclim": (("bioclim", "f64", "f64red"), ("bioclim",), "bioclim_driver.cpp"),
    # agro.hip: one lane per (cell, period) or per cell, thread by thread.  pet.hip: the solar table behind the Gladstones and
    # Jones coefficients; f64.hip: xh_resample_reduce_f64 of the warmest-month cross-check.
    "agro": (("agro", "pet", "f64"), ("agro",), "agro_driver.cpp"),
    # hydro.hip on fibers (above).  f64.hip and reduce.hip + tcount.hip + window.hip: the period means, the per-cell threshold
    # counts and the float64 quantiles the other indices are built from.
    "hydro": (("hydro", "f64", "reduce", "tcount", "window"), ("hydro",), "hydro_driver.cpp"),
    # rainseason.hip on fibers (above).  f64.hip and reduce.hip + tcount.hip + window.hip: the period minima of hardiness_zones
    # and the counts of the missing mask (reduce.hip links against the launchers of tcount.hip, f64.hip against window.hip).
    "rain": (("rainseason", "f64", "reduce", "tcount", "window"), ("rainseason",), "rain_driver.cpp"),
}
# topnet.h (the comparator networks of the register percentile kernels) issues v_min_f32 / v_max_f32 and a NaN-replace-and-count
# triple as inline ISA: four statements, rewritten to the C++ they stand for (NaN never enters the min / max: the callers replace
# it first), in a copy of the header that the fiber units include instead
HEADER_REWRITES = {"topnet.h": [
    ('asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));', "r = a < b ? a : b;"),
    ('asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));', "r = a > b ? a : b;"),
    ('''  asm("v_cmp_u_f32 vcc, %2, %2\\n\\tv_cndmask_b32 %0, %2, %3, vcc\\n\\tv_addc_co_u32 %1, vcc, 0, %1, vcc"
      : "=&v"(key), "+v"(nn)
      : "v"(raw), "v"(sentinel)
      : "vcc");''', "  { const bool n_ = raw != raw; key = n_ ? sentinel : raw; nn += n_ ? 1 : 0; }"),
    ('''  asm("v_cmp_u_f32 vcc, %0, %0\\n\\tv_cndmask_b32 %0, %0, %2, vcc\\n\\tv_addc_co_u32 %1, vcc, 0, %1, vcc"
      : "+v"(v), "+v"(nn)
      : "v"(sentinel)
      : "vcc");''', "  { const bool n_ = v != v; v = n_ ? sentinel : v; nn += n_ ? 1 : 0; }"),
]}
# The register sorting networks (select3.hip, qdm2.hip) split a sorted column across the lane pair with DPP moves written as ISA:
# xor with the lane's sign mask, take the partner's complement (v_not_b32_dpp quad_perm [1,0,3,2]), keep the larger — the same in C++
# with a shuffle; qdm2.hip's key conversion counts NaN with a compare / select / add-with-carry triple.
_SPLIT_PAIR = (r"#define XH_SP\(i, j\).*?\n  \}\n",
               "#define XH_SP(i, j) { k##i ^= mA3; k##j ^= mA3; const uint32_t t0_ = ~__shfl_xor(k##j, 1), t1_ = ~__shfl_xor(k##i, 1); "
               "k##i = k##i > t0_ ? k##i : t0_; k##j = k##j > t1_ ? k##j : t1_; }\n")
_SPLIT_ONE = (r"#define XH_SM\(m\).*?\n  \}\n",
              "#define XH_SM(m) { k##m ^= mA3; const uint32_t t0_ = ~__shfl_xor(k##m, 1); k##m = k##m > t0_ ? k##m : t0_; }\n")
UNIT_REWRITES = {
    # select2.hip counts through the wave on VCC (v_cmp + s_bcnt1_i32_b64): a vote + a population count
    "select2": [(r'asm volatile\("v_cmp_o_f32 vcc, %3, %3\\n\\ts_bcnt1_i32_b64 %1, vcc\\n\\tv_cndmask_b32 %0, -1, %2, vcc"\s*: "=v"\(o\), "=s"\(c\)\s*: "v"\(kk\), "v"\(u\)\s*: "vcc", "scc"\);',
                 "{ const bool o_ = __uint_as_float(u) == __uint_as_float(u); c = (uint32_t)__popcll(__ballot(o_)); o = o_ ? kk : 0xFFFFFFFFu; }"),
                (r'asm volatile\("v_cmp_eq_u32 vcc, %1, %2\\n\\ts_bcnt1_i32_b64 %0, vcc" : "=s"\(c\) : "v"\(key\[k\]\), "v"\(kmin\) : "vcc", "scc"\);',
                 "c = (uint32_t)__popcll(__ballot(key[k] == kmin));")],
    "select3": [_SPLIT_PAIR, _SPLIT_ONE],
    # select4.hip (the streaming two-pass selection): the lane-xor exchanges of its wave-wide bitonic sort are DPP moves (quad_perm,
    # row_shl / row_shr / row_ror) = the value of lane ^ m; the sign of a float difference is one v_med3_i32 on its bits; column
    # extremes through v_min / v_max (which return the other operand for a NaN one, like fminf / fmaxf); the candidate appends are
    # sixteen LDS writes under the execution mask (v_cmpx) at an address kept as a 32-bit LDS offset
    # winsel.hip (the sliding sorted window of the day-of-year training): the same DPP lane exchanges as select4's wave sort
    "winsel": [(r"(__device__ __forceinline__ uint32_t ws_lane_xor\(uint32_t v, int m\) \{).*?\n\}\n", r"\1 return (uint32_t)__shfl_xor((int)v, m); }\n")],
    "select4": [
        (r"(__device__ __forceinline__ uint32_t hs_lane_xor\(uint32_t v, int m\) \{).*?\n\}\n", r"\1 return (uint32_t)__shfl_xor((int)v, m); }\n"),
        (r'asm\("v_med3_i32 %0, %1, -1, 1" : "=v"\(r\) : "v"\(z\)\);', "{ int zi_; memcpy(&zi_, &z, 4); r = zi_ < -1 ? -1 : (zi_ > 1 ? 1 : zi_); }"),
        (r'asm\("v_min_f32 %0, %0, %1" : "\+v"\((\w+)\) : "v"\(([^;]+?)\)\);', r"\1 = fminf(\1, \2);"),
        (r'asm\("v_max_f32 %0, %0, %1" : "\+v"\((\w+)\) : "v"\(([^;]+?)\)\);', r"\1 = fmaxf(\1, \2);"),
        (r'asm\("v_min3_f32 %0, %0, %1, %2" : "\+v"\((\w+)\) : "v"\(([^;]+?)\), "v"\(([^;]+?)\)\);', r"\1 = fminf(fminf(\1, \2), \3);"),
        (r'asm\("v_max3_f32 %0, %0, %1, %2" : "\+v"\((\w+)\) : "v"\(([^;]+?)\), "v"\(([^;]+?)\)\);', r"\1 = fmaxf(fmaxf(\1, \2), \3);"),
        # (round 6: hs_qdm_pick scans the column's records in LDS — no v_readlane from divergent code is left to emulate)
        (r"typedef __attribute__\(\(address_space\(3\)\)\) uint32_t lds_u32;", ""),
        (r"uint32_t addr = \(uint32_t\)\(uintptr_t\)\(lds_u32\*\)\(cand \+ lbase\[colo\]\) \+ pos \* 4u;", "uint32_t* addr = (uint32_t*)(cand + lbase[colo]) + pos;"),
        (r'asm volatile\(\s*"s_mov_b64 %\[sv\], exec\\n\\t".*?: "vcc", "memory"\);', "(void)sv; if (bit) { uint32_t b_; memcpy(&b_, &v[u], 4); *addr++ = b_; }"),
    ],
    "qdm2": [_SPLIT_PAIR, _SPLIT_ONE,
             (r'asm volatile\("v_cmp_u_f32 vcc, %2, %2\\n\\tv_cndmask_b32_e64 %0, %0, -1, vcc\\n\\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc" \\\n\s*: "\+v"\(kk_\), "\+v"\(nanc\) : "v"\(f_\) : "vcc"\);',
              "{ const bool n_ = f_ != f_; kk_ = n_ ? 0xFFFFFFFFu : kk_; nanc += n_ ? 1u : 0u; }")],
}
_DYN_LDS = re.compile(r"extern\s+__shared__\s+(?:__attribute__\(\(aligned\(\d+\)\)\)\s+)?([\w ]+?)\s+(\w+)\[\];")


def _prepare_headers(workdir: str) -> None:
    for header, rules in HEADER_REWRITES.items():
        text = open(os.path.join(CSRC, header)).read()
        for old, new in rules:
            if old not in text:
                raise RuntimeError(f"{header}: the statement the simulation rewrites has changed: {old[:60]!r}")
            text = text.replace(old, new)
        open(os.path.join(workdir, header), "w").write(text)


def _prepare_unit(unit: str, workdir: str, san: str = ""):
    """(source file, extra flags) of one unit: the source unchanged, or its rewritten copy in workdir."""
    src = os.path.join(CSRC, unit + ".hip")
    extra = list(UNIT_DEFINES.get(unit, []))
    fibers = unit in FIBER_UNITS or unit in UNIT_LIBRARY_FIBER_UNITS
    if not fibers and unit not in DYN_LDS_UNITS:
        return src, extra
    text = open(src).read()
    if unit == "core":   # the runtime half of core.hip is sim_runtime.cpp's job: only its kernels (synthetic fields, transposes)
        text = '#include "common.h"\n' + text[text.index("// ---- synthetic generator"):]
    text, nsub = _DYN_LDS.subn(lambda m: f"{m.group(1)}* {m.group(2)} = ({m.group(1)}*)sim_dynamic_lds();", text)
    if nsub != UNIT_LIBRARY_FIBER_UNITS.get(unit, nsub) or (nsub == 0 and unit in DYN_LDS_UNITS):
        raise RuntimeError(f"{unit}.hip: an `extern __shared__` declaration the simulation rewrites has changed ({nsub} rewritten)")
    if fibers:
        # the LDS-only workgroup barrier (s_waitcnt lgkmcnt(0); s_barrier) is a workgroup barrier; empty asm statements are
        # compiler fences whose operand class "v" / "s" (a VGPR / SGPR) becomes "r"
        text = text.replace('asm volatile("s_waitcnt lgkmcnt(0)\\n\\ts_barrier" ::: "memory")', "__syncthreads()")
        text = re.sub(r'asm volatile\(""\s*:\s*"\+[vs]"', 'asm volatile("" : "+r"', text)
        for pat, rep in UNIT_REWRITES.get(unit, []):
            text, nsub = re.subn(pat, rep, text, flags=re.S)
            if nsub == 0:
                raise RuntimeError(f"{unit}.hip: the statement the simulation rewrites has changed: {pat[:50]!r}")
        extra += ["-DSIM_FIBERS=1", "-D__shared__=static"]
        if unit == "select4" and san and "undefined" in san and not os.environ.get("HOSTSIM_SANITIZE_BOUNDS_ONLY"):
            # g++ 11: with ALL of -fsanitize=undefined the index check of `v[u]` on the ring's register set (a reference to
            # an array handed to a lambda) reads a wrong temporary and the access after it faults — with the loop variable
            # verified intact by an explicit check in front of it.  Either half alone is clean: this build carries every
            # check but `bounds`; HOSTSIM_SANITIZE=bounds HOSTSIM_SANITIZE_BOUNDS_ONLY=1 is the other half.
            extra += ["-fno-sanitize=bounds"]
    src = os.path.join(workdir, unit + ".sim.cpp")
    open(src, "w").write(text)
    return src, extra


def _gxx(args) -> None:
    """One g++ run.  A failure carries the compiler's stderr on its CalledProcessError (for the caller's failure text); the
    warnings of a run that succeeds are passed on."""
    sys.stderr.write(subprocess.run(["g++", *args], check=True, stderr=subprocess.PIPE, text=True).stderr)


def _compile_all(units, workdir, flags, san=""):
    from concurrent.futures import ThreadPoolExecutor

    def compile_unit(unit):
        obj = os.path.join(workdir, unit + ".o")
        src, extra = _prepare_unit(unit, workdir, san)
        _gxx(["-x", "c++", *flags, *extra, "-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:   # (g++ runs outside the GIL)
        objs = list(pool.map(compile_unit, units))
    obj = os.path.join(workdir, "sim_runtime.o")
    _gxx([*flags, "-c", os.path.join(HERE, "sim_runtime.cpp"), "-o", obj])
    return objs + [obj]


def _library(units, workdir: str, name: str, san: str = "") -> str:
    """g++ the units + sim_runtime.cpp into the shared library workdir/name: the one flag list of everything loaded into Python."""
    if shutil.which("g++") is None:
        raise RuntimeError("no g++")
    os.makedirs(workdir, exist_ok=True)
    _prepare_headers(workdir)
    flags = ["-std=c++17", "-O1", "-fPIC", "-ffp-contract=off", "-I", workdir, "-I", HERE, "-I", CSRC]
    if san:
        flags += ["-g", f"-fsanitize={san}", "-fno-sanitize-recover=all" if os.environ.get("HOSTSIM_SANITIZE_FATAL") else "-fsanitize-recover=all"]
    objs = _compile_all(units, workdir, flags, san)
    out = os.path.join(workdir, name)
    _gxx(["-shared", *([f"-fsanitize={san}"] if san else []), "-o", out, *objs])
    return out


def build(workdir: str) -> str:
    """g++ the simulated translation units (sources unchanged, except that an `extern __shared__ T name[];` of a fiber unit
    becomes a pointer to the workgroup's LDS buffer) + sim_runtime.cpp into workdir/libxclimhip_hostsim.so."""
    # HOSTSIM_SANITIZE=undefined (the switches are in README.md): an audit build of the kernels under the compiler's sanitizers —
    # out-of-bounds LDS / scratch accesses, shifts, signed overflow
    return _library(SIMULATED_UNITS + FIBER_UNITS, workdir, "libxclimhip_hostsim.so", os.environ.get("HOSTSIM_SANITIZE") or "")


def build_unit_library(name: str, workdir: str) -> str:
    """One of UNIT_LIBRARIES into workdir/libxclimhip_hostsim_<name>.so.  It is loaded into Python, so it never carries a
    sanitizer: HOSTSIM_SANITIZE reaches build() alone, and the sanitizers of these units run in build_unit_driver's programs."""
    return _library(UNIT_LIBRARIES[name][0], workdir, f"libxclimhip_hostsim_{name}.so")


def build_shared(basetemp: str) -> str:
    """build() once per pytest session: the modules that need the library (tests/test_hostsim_cpu.py,
    tests/test_hostsim_sanitize_cpu.py) hand in the session's base temporary directory and share one build.  A failed build is
    not remembered: every caller sees its CalledProcessError."""
    work = os.path.join(basetemp, "hostsim_shared")
    out = os.path.join(work, "libxclimhip_hostsim.so")
    if not os.path.exists(out):
        os.makedirs(work, exist_ok=True)
        build(work)
    return out


STANDALONE_SANITIZE = "address,undefined"


def _program(units, workdir: str, source: str) -> str:
    """A stand-alone sanitizer program (a C++ program with its own main, no Python in the process, nothing preloaded): the
    units' rewritten sources + sim_runtime.cpp + standalone/<source>, all with -g -O1 -fsanitize=address,undefined
    -fno-sanitize-recover=all, linked into workdir/<source without .cpp>."""
    if shutil.which("g++") is None:
        raise RuntimeError("no g++")
    os.makedirs(workdir, exist_ok=True)
    _prepare_headers(workdir)
    # (-fno-var-tracking: line tables without variable-location tracking, which alone takes a minute on f64red / f64run)
    flags = ["-std=c++17", "-g", "-fno-var-tracking", "-O1", "-ffp-contract=off", f"-fsanitize={STANDALONE_SANITIZE}", "-fno-sanitize-recover=all",
             "-I", workdir, "-I", HERE, "-I", CSRC, "-I", os.path.join(ROOT, "include")]
    objs = _compile_all(units, workdir, flags, STANDALONE_SANITIZE)
    out = os.path.join(workdir, source[:-len(".cpp")])
    # (the sanitizer runtimes linked statically: the program needs no particular order of shared libraries at start-up, whatever
    # the environment it is started in loads first)
    _gxx([*flags, "-static-libasan", "-static-libubsan", "-o", out, os.path.join(HERE, "standalone", source), *objs])
    return out


def build_standalone(workdir: str) -> str:
    """The manifest replayer of the NEW_UNITS (standalone/san_driver.cpp) as workdir/san_driver."""
    return _program(NEW_UNITS, workdir, "san_driver.cpp")


def build_unit_driver(name: str, workdir: str) -> str:
    """The stand-alone sanitizer program of one of UNIT_LIBRARIES as workdir/<name>_driver."""
    _, units, source = UNIT_LIBRARIES[name]
    return _program(units, workdir, source)


class _SimLib:
    """The simulated entry points with the prototypes of xclim_amd._capi; memory entry points on host buffers (MockDevice's);
    anything else raises."""

    def __init__(self, path: str):
        self._dll = C.CDLL(path)
        self._mock = _MockLib()

    def __getattr__(self, name):
        if not name.startswith("xh_"):
            raise AttributeError(name)
        try:
            if name in WAVE_ENTRY_POINTS:
                raise AttributeError(name)
            fn = getattr(self._dll, name)
        except AttributeError:
            # memory entry points on host buffers; fences between the copy lanes and page-locking are no-ops here (one thread,
            # everything in order, host memory)
            if name in _MockLib._SPECIAL or name in ("xh_malloc", "xh_free", "xh_timer_start", "xh_lane_fence", "xh_lane_sync",
                                                      "xh_host_register", "xh_host_unregister"):
                return getattr(self._mock, name)
            raise NotImplementedError(f"{name}: not simulated on the host (kernels written at ISA level, or a runtime service the "
                                      "simulation does not provide)") from None
        fn.argtypes = _capi.SIGNATURES.get(name)
        fn.restype = _capi._RESTYPES.get(name, C.c_int)
        setattr(self, name, fn)
        return fn


class SimDevice(MockDevice):
    def __init__(self, path: str):
        super().__init__(0)
        self.path = path
        self.lib = _SimLib(path)
        ctx = C.c_void_p()
        self.lib._dll.xh_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        assert self.lib._dll.xh_create(0, C.byref(ctx)) == 0
        self.ctx = ctx
        self.lock = threading.RLock()

    def sync(self):
        return None


_ASAN_SWAPCONTEXT_NOTE = "WARNING: ASan doesn't fully support makecontext/swapcontext functions"


class SanitizerReport(AssertionError):
    """The stand-alone driver ended with a sanitizer report (or any other failure of the process)."""


class _ReplayLib(_SimLib):
    """The simulation library, except that every call of one of NEW_ENTRY_POINTS runs in a FRESH PROCESS of the stand-alone
    sanitizer driver: the call's memory blocks go to a case directory as raw arrays, the driver copies each into a malloc
    block of exactly the allocation's size, calls the entry point, dumps the blocks, and they are copied back here."""

    def __init__(self, path: str, driver: str, casedir: str, dev):
        super().__init__(path)
        self._driver, self._casedir, self._dev, self._err = driver, casedir, dev, b""
        self.replayed = {}   # entry point -> the int64 arguments (T, C, strides ...) of every sanitized call
        self.in_process = ()  # entry points a test wants from the in-process library for a while (a table it only needs as input)

    def __getattr__(self, name):
        if name == "xh_last_error":   # (read once by _capi._check after a failed call: a replayed call's text, else the library's)
            return self._last_error
        if name in NEW_ENTRY_POINTS:
            return lambda ctx, *args: (super(_ReplayLib, self).__getattr__(name)(ctx, *args) if name in self.in_process
                                       else self._replay(name, args))
        return super().__getattr__(name)

    def _last_error(self):
        err, self._err = self._err, b""
        if err:
            return err
        fn = self._dll.xh_last_error
        fn.restype = C.c_char_p
        return fn()

    def _block(self, p, blocks):
        """(id, offset) of the memory block an address lies in: an allocation of the device, or a host array handed over with
        np_ptr (ctypes keeps the array on the pointer)."""
        addr = p.value if hasattr(p, "value") else int(p or 0)
        if not addr:
            return None
        arr = getattr(p, "_arr", None)
        if arr is not None:
            base, n = arr.ctypes.data, arr.nbytes
        else:
            for base, n in self._dev._exact.items():
                if base <= addr < base + max(n, 1):
                    break
            else:
                raise RuntimeError(f"address {addr:#x} lies in no block the simulated device allocated")
        if base not in blocks:
            blocks[base] = (f"b{len(blocks)}", n)
        return blocks[base][0], addr - base

    def _replay(self, name, args):
        case = os.path.join(self._casedir, f"{sum(len(v) for v in self.replayed.values()):05d}_{name}")
        os.makedirs(case)
        blocks, lines = {}, [f"entry {name}", "arg ctx"]
        for a in args:
            if isinstance(a, C.Array):
                refs = [self._block(C.c_void_p(v), blocks) for v in a]
                lines.append(f"arg v {len(refs)} " + " ".join("-" if r is None else f"{r[0]} {r[1]}" for r in refs))
            elif isinstance(a, (C.c_void_p, C._Pointer)) or hasattr(a, "_arr"):
                r = self._block(a, blocks)
                lines.append("arg n" if r is None else f"arg p {r[0]} {r[1]}")
            elif isinstance(a, (bool, int, np.integer)):
                lines.append(f"arg i {int(a)}")
            elif isinstance(a, (float, np.floating)):
                lines.append(f"arg d {float(a).hex() if np.isfinite(a) else repr(float(a))}")
            else:
                raise TypeError(f"{name}: cannot record an argument of type {type(a).__name__}")
        for base, (bid, n) in blocks.items():
            lines.insert(1, f"buf {bid} {n}")
            with open(os.path.join(case, bid + ".in"), "wb") as f:
                f.write(C.string_at(base, n))
        open(os.path.join(case, "manifest.txt"), "w").write("\n".join(lines) + "\n")
        res = subprocess.run([self._driver, case], capture_output=True, text=True)
        # (the swapcontext interceptor of g++ 11's ASan prints one fixed warning on its first call, annotated fibers or not)
        report = "\n".join(ln for ln in res.stderr.splitlines() if ln.strip() and _ASAN_SWAPCONTEXT_NOTE not in ln)
        if res.returncode != 0 or report:
            raise SanitizerReport(f"{name} ({case}): exit status {res.returncode}\n{res.stderr[-4000:]}")
        for base, (bid, n) in blocks.items():
            data = open(os.path.join(case, bid + ".out"), "rb").read()
            assert len(data) == n
            C.memmove(base, data, n)
        rc, _, msg = open(os.path.join(case, "result.txt")).read().partition("\n")
        self._err = msg.rstrip("\n").encode()
        self.replayed.setdefault(name, []).append(tuple(int(a) for a, t in zip(args, _capi.SIGNATURES[name][1:]) if t is C.c_int64))
        shutil.rmtree(case)
        return int(rc)


class ReplayDevice(SimDevice):
    """A SimDevice whose allocations are remembered with their EXACT sizes and whose calls of the NEW_ENTRY_POINTS run in the
    stand-alone sanitizer driver (tests/test_hostsim_sanitize_cpu.py)."""

    def __init__(self, path: str, driver: str, casedir: str):
        super().__init__(path)
        self._exact = {}
        self.lib = _ReplayLib(path, driver, casedir, self)

    def empty(self, shape, dtype):
        a = super().empty(shape, dtype)
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        self._exact[a.ptr] = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        return a

    def _release(self, ptr: int, nbytes: int) -> None:
        self._exact.pop(ptr, None)
        super()._release(ptr, nbytes)
