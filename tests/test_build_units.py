"""The scorer is compiled once: the RGBA and YUV front ends are translation units of their own over
oavif_amd/csrc/ssimu2_host.h, and the four libraries are links of objects (oavif_amd/build.py).
CPU only: the device-only compiles that isa_text.py shares (a few seconds per front end), build.py's table, the text of
the header."""
import os
import re
import shutil
import subprocess

import pytest

import isa_text
from oavif_amd import build

YUV_KERNELS = {f"k_yuv_to_codes<{s}, {mono}>" for s in (1, 2) for mono in ("false", "true")}


def _kernels(unit):
    """Names of the kernels the device code of `unit` defines, templates with their arguments."""
    asm = isa_text.unit_asm(unit)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    assert names and len(set(names)) == len(names)
    cxxfilt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    plain = subprocess.run([cxxfilt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
    # "void ssimu2::k_yuv_to_codes<1, false>(args)" / "ssimu2::k_composite_rgba8(args)" -> the name and its arguments
    return {re.sub(r"^(void )?(\w+::)*", "", s.split("(")[0]) for s in plain if s}


def test_the_rgba_unit_defines_its_one_kernel():
    assert _kernels("ssimu2_ext.hip") == {"k_composite_rgba8"}


def test_the_yuv_unit_defines_its_four_kernels():
    assert _kernels("ssimu2_yuv.hip") == YUV_KERNELS


@pytest.mark.parametrize("unit", ["ssimu2_ext.hip", "ssimu2_yuv.hip"])
def test_a_front_end_has_no_constant_block(unit):
    """c_k is the scorer unit's: a second one in a library would be a block nobody uploads."""
    assert "_ZN6ssimu23c_kE" in isa_text.scorer_asm()  # ssimu2::c_k, where it is
    assert "c_k" not in isa_text.unit_asm(unit), unit


def test_every_source_is_compiled_once_and_the_libraries_are_a_chain():
    units = build.compile_units()
    assert len(units) == len(set(units))
    assert set(units) == {s for sources in build.LIBRARIES.values() for s in sources}
    assert set(units) == {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_instrument.hip",
                          "tq.cpp", "png_ingest.cpp", "remote_client.cpp"}
    for sources in build.LIBRARIES.values():
        assert len(sources) == len(set(sources))
        assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in sources)
    product, ext, yuv, instr = (set(build.LIBRARIES[p]) for p in
                                (build.LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH, build.INSTR_LIB_PATH))
    assert product < ext < yuv
    assert ext - product == {"ssimu2_ext.hip"} and yuv - ext == {"ssimu2_yuv.hip"}
    # the instrumented library is another build of the scorer: it shares the support objects and nothing else
    assert instr & yuv == set(build.SUPPORT_SOURCES) and instr - yuv == {"ssimu2_instrument.hip"}
    assert build.MAX_COMPILES <= 6


def _includes(path):
    with open(path) as f:
        return {os.path.basename(m) for m in re.findall(r'^\s*#\s*include\s+[<"]([^>"]+)[>"]', f.read(), re.M)}


def test_the_front_end_header_includes_no_kernel_header():
    seen, todo = set(), ["ssimu2_host.h"]
    while todo:  # the header and every header of csrc it reaches
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(build.CSRC, name)):
            continue
        seen.add(name)
        todo += _includes(os.path.join(build.CSRC, name))
    assert "ssimu2_host.h" in seen and "remote_client.h" in seen
    assert not seen & {"ssimu2_kernels.h", "ssimu2_recursive.h", "ssimu2_hip.hip"}, seen
    with open(os.path.join(build.CSRC, "ssimu2_host.h")) as f:
        text = f.read()
    assert "__global__" not in re.sub(r"//.*", "", text) and "__constant__" not in re.sub(r"//.*", "", text)
    for unit in ("ssimu2_ext.hip", "ssimu2_yuv.hip"):  # and the front ends reach the scorer through it alone
        inc = _includes(os.path.join(build.CSRC, unit))
        assert "ssimu2_host.h" in inc and not inc & {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_kernels.h", "ssimu2_recursive.h"}


def test_the_instrumented_layout_is_refused_outside_the_scorer_unit():
    """ssimu2_ctx has tail fields under SSIMU2_INSTRUMENTED_BUILD: a front end built with the macro must not compile."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc missing")
    p = subprocess.run([hipcc, *build.DEVICE_FLAGS, "-DSSIMU2_INSTRUMENTED_BUILD=1", "-E", "-o", os.devnull,
                        os.path.join(build.CSRC, "ssimu2_ext.hip")], capture_output=True, text=True)
    assert p.returncode != 0 and "ssimu2_host.h under SSIMU2_INSTRUMENTED_BUILD" in p.stderr
