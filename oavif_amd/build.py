"""Build the gfx950 shared libraries in-tree (oavif_amd/lib/liboavif_hip.so and its nine siblings).

Every source is compiled once, to an object under oavif_amd/lib/obj; the libraries are links of those objects
(LIBRARIES, and MAP_LIBRARIES, CHROMA_LIBRARIES, YUVA_LIBRARIES, RBATCH_LIBRARIES, HBATCH_LIBRARIES and ABATCH_LIBRARIES beside it).  hipcc cross-compiles without a GPU; the built libraries are git-ignored.
"""
from __future__ import annotations

import concurrent.futures
import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip.so")              # the product: C ABI of include/ssimu2_hip.h, oavif_tq.h
INSTR_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_instr.so")  # + include/ssimu2_hip_internal.h (bench / tests only)
EXT_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_ext.so")      # + include/ssimu2_hip_ext.h (RGBA input)
YUV_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_yuv.so")      # + include/ssimu2_hip_yuv.h (YUV input)
MAP_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_map.so")      # + include/ssimu2_hip_map.h (error maps of every input, section 15)
CHROMA_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_chroma.so")  # + include/ssimu2_hip_chroma.h (4:2:2 / 4:2:0 YUV, section 16)
YUVA_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_yuva.so")      # + include/ssimu2_hip_yuva.h (YUV with an alpha plane, section 17)
RBATCH_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_rbatch.so")  # + include/ssimu2_hip_rbatch.h (batches in every blur mode, section 18)
HBATCH_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_hbatch.so")  # + include/ssimu2_hip_hbatch.h (16-bit and YUV batches, section 19)
ABATCH_LIB_PATH = os.path.join(LIB_DIR, "liboavif_hip_abatch.so")  # + include/ssimu2_hip_abatch.h (RGBA and YUV-with-alpha batches, section 20)
HOST_PATH = os.path.join(LIB_DIR, "oavif_host")   # csrc/oavif_host.c: main.zig's flow in C over the two public headers + libavif
SERVICE_PATH = os.path.join(LIB_DIR, "oavif_scored")  # csrc/oavif_scored.cpp: the resident scoring service
OBJ_DIR = os.path.join(LIB_DIR, "obj")  # one object per source, whichever libraries it is linked into
# Library -> the units linked into it.  A front end (csrc/ssimu2_host.h is what it may use) is a unit of its own on top of
# the objects of the library below it: the same scorer object, not the same text compiled again.  The instrumented
# library is another build of the scorer (ssimu2_instrument.hip includes ssimu2_hip.hip under its macro), so it shares
# only the support objects.
SUPPORT_SOURCES = ["tq.cpp", "png_ingest.cpp", "remote_client.cpp"]
SOURCES = ["ssimu2_hip.hip", *SUPPORT_SOURCES]
EXT_SOURCES = [*SOURCES, "ssimu2_ext.hip"]
YUV_SOURCES = [*EXT_SOURCES, "ssimu2_yuv.hip"]
INSTR_SOURCES = ["ssimu2_instrument.hip", *SUPPORT_SOURCES]
LIBRARIES = {LIB_PATH: SOURCES, INSTR_LIB_PATH: INSTR_SOURCES, EXT_LIB_PATH: EXT_SOURCES, YUV_LIB_PATH: YUV_SOURCES}
# The fifth library, in a table of its own beside LIBRARIES: the YUV library's objects plus one unit over ssimu2_host.h.
# build() compiles the units it adds (map_units()) with the others and links it after them.
MAP_SOURCES = [*YUV_SOURCES, "ssimu2_map.hip"]
MAP_LIBRARIES = {MAP_LIB_PATH: MAP_SOURCES}
# The sixth library, in a third table: the map library's objects plus one unit over ssimu2_host.h (chroma_units()).
CHROMA_SOURCES = [*MAP_SOURCES, "ssimu2_chroma.hip"]
CHROMA_LIBRARIES = {CHROMA_LIB_PATH: CHROMA_SOURCES}
# The seventh library, in a fourth table: the chroma library's objects plus one unit over ssimu2_host.h (yuva_units()).
YUVA_SOURCES = [*CHROMA_SOURCES, "ssimu2_yuva.hip"]
YUVA_LIBRARIES = {YUVA_LIB_PATH: YUVA_SOURCES}
# The eighth library, in a fifth table: the YUVA library's objects plus one unit over ssimu2_host.h (rbatch_units()).
RBATCH_SOURCES = [*YUVA_SOURCES, "ssimu2_rbatch.hip"]
RBATCH_LIBRARIES = {RBATCH_LIB_PATH: RBATCH_SOURCES}
# The ninth library, in a sixth table: the rbatch library's objects plus one unit over ssimu2_host.h (hbatch_units()).
HBATCH_SOURCES = [*RBATCH_SOURCES, "ssimu2_hbatch.hip"]
HBATCH_LIBRARIES = {HBATCH_LIB_PATH: HBATCH_SOURCES}
# The tenth library, in a seventh table: the hbatch library's objects plus one unit over ssimu2_host.h (abatch_units()).
ABATCH_SOURCES = [*HBATCH_SOURCES, "ssimu2_abatch.hip"]
ABATCH_LIBRARIES = {ABATCH_LIB_PATH: ABATCH_SOURCES}
MAX_COMPILES = 6  # compiles in flight; never the machine's CPU count
_PROGRAMS = ("oavif_host.c", "oavif_scored.cpp")  # linked against the library, not into it
# The flags that shape device code: the libraries' compile lines, the ISA tests and scripts/isa_ab.py all take them here.
DEVICE_FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17",
                "-ffp-contract=off",    # arithmetic contract: every FMA is an explicit fmaf()
                "-fno-slp-vectorize")   # v_pk_*_f32 + operand shuffles are slower than scalar VALU here


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build the gfx950 library)")


def _newer_than(t: float, paths) -> bool:
    return any(os.path.getmtime(d) > t for d in paths)


def _headers():
    inc = os.path.join(os.path.dirname(_HERE), "include")
    return [os.path.join(inc, s) for s in os.listdir(inc)]


def compile_units():
    """Every source of LIBRARIES, once, in the table's order: what build() compiles."""
    return list(dict.fromkeys(s for sources in LIBRARIES.values() for s in sources))


def map_units():
    """The sources of MAP_LIBRARIES that no library of LIBRARIES has: compiled once each, like compile_units()."""
    have = set(compile_units())
    return list(dict.fromkeys(s for sources in MAP_LIBRARIES.values() for s in sources if s not in have))


def chroma_units():
    """The sources of CHROMA_LIBRARIES that neither LIBRARIES nor MAP_LIBRARIES has: compiled once each."""
    have = {*compile_units(), *map_units()}
    return list(dict.fromkeys(s for sources in CHROMA_LIBRARIES.values() for s in sources if s not in have))


def yuva_units():
    """The sources of YUVA_LIBRARIES that none of the other three tables has: compiled once each."""
    have = {*compile_units(), *map_units(), *chroma_units()}
    return list(dict.fromkeys(s for sources in YUVA_LIBRARIES.values() for s in sources if s not in have))


def rbatch_units():
    """The sources of RBATCH_LIBRARIES that none of the other four tables has: compiled once each."""
    have = {*compile_units(), *map_units(), *chroma_units(), *yuva_units()}
    return list(dict.fromkeys(s for sources in RBATCH_LIBRARIES.values() for s in sources if s not in have))


def hbatch_units():
    """The sources of HBATCH_LIBRARIES that none of the other five tables has: compiled once each."""
    have = {*compile_units(), *map_units(), *chroma_units(), *yuva_units(), *rbatch_units()}
    return list(dict.fromkeys(s for sources in HBATCH_LIBRARIES.values() for s in sources if s not in have))


def abatch_units():
    """The sources of ABATCH_LIBRARIES that none of the other six tables has: compiled once each."""
    have = {*compile_units(), *map_units(), *chroma_units(), *yuva_units(), *rbatch_units(), *hbatch_units()}
    return list(dict.fromkeys(s for sources in ABATCH_LIBRARIES.values() for s in sources if s not in have))


def libs_need_build() -> bool:
    libs = (*LIBRARIES, *MAP_LIBRARIES, *CHROMA_LIBRARIES, *YUVA_LIBRARIES, *RBATCH_LIBRARIES, *HBATCH_LIBRARIES,
            *ABATCH_LIBRARIES)
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    return _newer_than(t, [os.path.join(CSRC, s) for s in os.listdir(CSRC) if s not in _PROGRAMS] + _headers())


def host_needs_build() -> bool:
    if not os.path.exists(HOST_PATH):
        return True
    return _newer_than(os.path.getmtime(HOST_PATH), [os.path.join(CSRC, "oavif_host.c"), LIB_PATH] + _headers())


def service_needs_build() -> bool:
    if not os.path.exists(SERVICE_PATH):
        return True
    deps = [os.path.join(CSRC, "oavif_scored.cpp"), os.path.join(CSRC, "remote_client.h"), LIB_PATH] + _headers()
    return _newer_than(os.path.getmtime(SERVICE_PATH), deps)


def needs_build() -> bool:
    return libs_need_build() or host_needs_build() or service_needs_build()


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    # several ranks of one job may get here at once on a fresh checkout: one compiles (file
    # lock), the others wait and find the library up to date; the .so appears atomically
    import fcntl
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not needs_build():
            return LIB_PATH
        if force or libs_need_build():
            _build_libs(verbose)
        build_host(verbose)
        build_service(verbose)
    return LIB_PATH


def _run_to(target: str, cmd, verbose: bool) -> None:
    """Run cmd + ["-o", a temporary name], then put the result at `target` atomically."""
    tmp = target + f".tmp{os.getpid()}"
    cmd = [*cmd, "-o", tmp]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, target)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


def _build_libs(verbose: bool) -> None:
    """Objects, then links: each unit of compile_units(), map_units(), chroma_units(), yuva_units(), rbatch_units(),
    hbatch_units() and abatch_units() to OBJ_DIR (MAX_COMPILES at a time), each library of the seven tables from its own."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    flags = [*DEVICE_FLAGS, "-fPIC",
             "-fvisibility=hidden", "-fvisibility-inlines-hidden",  # exports = the headers' functions
             "-Wall", "-Wno-unused-function"]
    flags += os.environ.get("OAVIF_AMD_EXTRA_HIPCC_FLAGS", "").split()  # A/B builds of experiments
    hipcc = _hipcc()
    obj = {s: os.path.join(OBJ_DIR, s + ".o") for s in (*compile_units(), *map_units(), *chroma_units(), *yuva_units(), *rbatch_units(), *hbatch_units(), *abatch_units())}
    with concurrent.futures.ThreadPoolExecutor(MAX_COMPILES) as pool:
        jobs = [pool.submit(_run_to, o, [hipcc, *flags, "-c", os.path.join(CSRC, s)], verbose) for s, o in obj.items()]
    for job in jobs:
        job.result()  # the first failed compile raises here
    for target, sources in (*LIBRARIES.items(), *MAP_LIBRARIES.items(), *CHROMA_LIBRARIES.items(), *YUVA_LIBRARIES.items(),
                            *RBATCH_LIBRARIES.items(), *HBATCH_LIBRARIES.items(), *ABATCH_LIBRARIES.items()):
        _run_to(target, [hipcc, *flags, "-shared", *(obj[s] for s in sources), "-lz"], verbose)  # -lz: png_ingest.cpp


def build_host(verbose: bool = False) -> str:
    """The C host (plain C over include/*.h; libavif is opened with dlopen at run time).  Linked against the
    product library next to it ($ORIGIN), the HIP runtime resolved through the library's own dependencies."""
    inc = os.path.join(os.path.dirname(_HERE), "include")
    tmp = HOST_PATH + f".tmp{os.getpid()}"
    cmd = [os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", inc,
           os.path.join(CSRC, "oavif_host.c"), "-o", tmp, "-L", LIB_DIR, "-loavif_hip", "-ldl", "-lm", "-lpthread",
           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    try:
        subprocess.run(cmd, check=True)
        os.replace(tmp, HOST_PATH)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return HOST_PATH


def build_service(verbose: bool = False, scorer=None, out=None, flags=()) -> str:
    """The scoring service (plain C++ over include/ssimu2_hip.h), linked against the product library next to it like
    the C host.  `scorer` (tests): C sources of a stand-in scorer to link instead of the library, `out` the program to
    write, `flags` extra compiler flags (sanitizers)."""
    inc = os.path.join(os.path.dirname(_HERE), "include")
    target = out or SERVICE_PATH
    tmp = target + f".tmp{os.getpid()}"
    cxx = os.environ.get("CXX", "g++")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", inc, os.path.join(CSRC, "oavif_scored.cpp"), "-o", tmp]
    objs = []
    try:
        if scorer:
            for i, src in enumerate(scorer):
                obj = f"{tmp}.{i}.o"
                subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-std=gnu11", *flags, "-I", inc, "-c", src, "-o", obj], check=True)
                objs.append(obj)
            cmd += objs + ["-lm", "-lpthread"]
        else:
            cmd += ["-L", LIB_DIR, "-loavif_hip", "-lpthread", "-Wl,-rpath,$ORIGIN",
                    "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
        os.replace(tmp, target)
    finally:
        for f in objs + [tmp]:
            if os.path.exists(f):
                os.unlink(f)
    return target


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
