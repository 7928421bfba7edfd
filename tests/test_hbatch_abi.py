"""The library of 16-bit and YUV batches without a GPU (include/ssimu2_hip_hbatch.h): the header
against the binding table, the library's exports (the rbatch library's and the six new calls, nothing else) and the other
eight libraries' (what their tables say, none of the new calls), the header as C, build.py's tables (the five earlier
ones as they were, the ninth library in a sixth), the budgets of the two new kernels from the compiler's metadata, what
every new call answers to a null context, and the Python flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import isa_text
from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes
from test_build_units import _includes

HEADER = "ssimu2_hip_hbatch.h"
UNIT = "ssimu2_hbatch.hip"
NAMES = ["ssimu2_hbatch_score_rgb16", "ssimu2_hbatch_score_against_reference_rgb16", "ssimu2_hbatch_score_rgb16_device",
         "ssimu2_hbatch_score_against_reference_rgb16_device", "ssimu2_hbatch_score_against_reference_yuv",
         "ssimu2_hbatch_convert_yuv"]


@pytest.fixture(scope="module")
def hbatch_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.hbatch_lib()


def _plain(path):
    return {s for s in _exported(path) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.HBATCH_FUNCTIONS) == NAMES                          # header order
    assert _lib.HBATCH_SYMBOLS == tuple(_lib.HBATCH_FUNCTIONS)
    assert set(_declared_functions(HEADER)) == set(NAMES)
    assert list(prototypes(HEADER)) == NAMES
    others = (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS) |
              set(_lib.MAP_FUNCTIONS) | set(_lib.CHROMA_FUNCTIONS) | set(_lib.YUVA_FUNCTIONS) | set(_lib.RBATCH_FUNCTIONS))
    assert not set(NAMES) & others
    assert os.path.basename(_lib.HBATCH_LIB_PATH) == "liboavif_hip_hbatch.so"
    with open(os.path.join(isa_text.ROOT, "include", HEADER)) as f:
        assert '#include "ssimu2_hip_rbatch.h"' in f.read()


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.HBATCH_FUNCTIONS[name]
    check(name, prototypes(HEADER)[name], restype, argtypes)


def test_the_library_exports_the_rbatch_library_plus_the_six_calls(hbatch_lib):
    from oavif_amd import _lib
    plain, below = _plain(_lib.HBATCH_LIB_PATH), _plain(_lib.RBATCH_LIB_PATH)
    assert plain - below == set(NAMES) and below <= plain
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = (public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS) | set(_lib.CHROMA_SYMBOLS) |
            set(_lib.YUVA_SYMBOLS) | set(_lib.RBATCH_SYMBOLS) | set(NAMES))
    assert plain == want, plain ^ want
    for name in want:
        assert hasattr(hbatch_lib, name), name


def test_the_other_eight_libraries_export_what_they_did(hip_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    ext, yuv, maps = set(_lib.EXT_SYMBOLS), set(_lib.YUV_SYMBOLS), set(_lib.MAP_SYMBOLS)
    chroma, yuva, rbatch = set(_lib.CHROMA_SYMBOLS), set(_lib.YUVA_SYMBOLS), set(_lib.RBATCH_SYMBOLS)
    want = {_lib.LIB_PATH: public, _lib.INSTR_LIB_PATH: public | set(_lib.INSTR_SYMBOLS), _lib.EXT_LIB_PATH: public | ext,
            _lib.YUV_LIB_PATH: public | ext | yuv, _lib.MAP_LIB_PATH: public | ext | yuv | maps,
            _lib.CHROMA_LIB_PATH: public | ext | yuv | maps | chroma,
            _lib.YUVA_LIB_PATH: public | ext | yuv | maps | chroma | yuva,
            _lib.RBATCH_LIB_PATH: public | ext | yuv | maps | chroma | yuva | rbatch}
    assert len(want) == 8
    for path, names in want.items():
        got = {s for s in _exported(path) if s.startswith(("ssimu2_", "oavif_"))}
        assert got == names, (path, got ^ names)
        assert not got & set(NAMES), path


def test_the_two_public_headers_and_the_shim_know_nothing_of_it():
    for header in ("ssimu2_hip.h", "oavif_tq.h"):
        assert not set(_declared_functions(header)) & set(NAMES)
    with open(os.path.join(isa_text.ROOT, "oavif_amd", "zig", "fssimu2.zig")) as f:
        assert "hbatch" not in f.read()


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "ssimu2_hip_hbatch.h"\n'
                   "int main(void) {\n"
                   "    double out[1];\n"
                   "    uint16_t codes[3];\n"
                   "    ssimu2_yuv_frame f = {{0, 0, 0}, {0, 0, 0}, 8, SSIMU2_YUV_420, 1, 6};\n"
                   "    int rc = ssimu2_hbatch_score_rgb16(0, 0, 0, 0, 8, 8, 10, out);\n"
                   "    rc |= ssimu2_hbatch_score_against_reference_rgb16(0, 0, 0, 10, out);\n"
                   "    rc |= ssimu2_hbatch_score_rgb16_device(0, 0, 0, (size_t)0, 0, 8, 8, 10, out);\n"
                   "    rc |= ssimu2_hbatch_score_against_reference_rgb16_device(0, 0, (size_t)0, 0, 10, out);\n"
                   "    rc |= ssimu2_hbatch_score_against_reference_yuv(0, &f, 1, 16, SSIMU2_CHROMA_BILINEAR, out);\n"
                   "    rc |= ssimu2_hbatch_convert_yuv(0, &f, 1, 1, 1, 16, SSIMU2_CHROMA_NEAREST, codes);\n"
                   "    rc |= ssimu2_rbatch_score_against_reference(0, 0, 0, out);\n"   # the header below comes with it
                   "    return rc == 0 ? SSIMU2_MAX_BATCH : 0;\n"
                   "}\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(isa_text.ROOT, "include"), str(src)], check=True)


def test_build_keeps_its_five_tables_and_knows_the_ninth_library_in_a_sixth(hip_lib):
    from oavif_amd import _lib, build
    assert list(build.LIBRARIES) == [build.LIB_PATH, build.INSTR_LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH]
    assert build.MAP_LIBRARIES == {build.MAP_LIB_PATH: [*build.YUV_SOURCES, "ssimu2_map.hip"]}
    assert build.CHROMA_LIBRARIES == {build.CHROMA_LIB_PATH: [*build.MAP_SOURCES, "ssimu2_chroma.hip"]}
    assert build.YUVA_LIBRARIES == {build.YUVA_LIB_PATH: [*build.CHROMA_SOURCES, "ssimu2_yuva.hip"]}
    assert build.RBATCH_LIBRARIES == {build.RBATCH_LIB_PATH: [*build.YUVA_SOURCES, "ssimu2_rbatch.hip"]}
    assert build.HBATCH_LIBRARIES == {build.HBATCH_LIB_PATH: build.HBATCH_SOURCES}
    assert build.HBATCH_SOURCES == [*build.RBATCH_SOURCES, UNIT]
    for table in (build.LIBRARIES, build.MAP_LIBRARIES, build.CHROMA_LIBRARIES, build.YUVA_LIBRARIES, build.RBATCH_LIBRARIES):
        assert build.HBATCH_LIB_PATH not in table
    assert build.hbatch_units() == [UNIT]
    assert build.rbatch_units() == ["ssimu2_rbatch.hip"]
    assert UNIT not in (*build.compile_units(), *build.map_units(), *build.chroma_units(), *build.yuva_units(),
                        *build.rbatch_units())
    assert os.path.samefile(os.path.dirname(build.HBATCH_LIB_PATH), os.path.dirname(_lib.HBATCH_LIB_PATH))
    assert os.path.basename(build.HBATCH_LIB_PATH) == "liboavif_hip_hbatch.so"
    assert os.path.exists(os.path.join(build.CSRC, UNIT)) and os.path.exists(build.HBATCH_LIB_PATH)   # built by build.build()


def test_build_rebuilds_when_the_ninth_library_is_missing(hip_lib, monkeypatch, tmp_path):
    from oavif_amd import build
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "HBATCH_LIBRARIES", {str(tmp_path / "liboavif_hip_hbatch.so"): build.HBATCH_SOURCES})
    assert build.libs_need_build()


def test_the_unit_is_a_front_end_over_the_host_header():
    from oavif_amd import build
    inc = _includes(os.path.join(build.CSRC, UNIT))
    assert "ssimu2_host.h" in inc and HEADER in inc and "ssimu2_yuv_pixel.h" in inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_kernels.h", "ssimu2_recursive.h"}
    assert "c_k" not in isa_text.unit_asm(UNIT)


# ---- budgets of the two new kernels, from the compiler's metadata ---------------------------------------------------
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _kernels(asm):
    meta = {}
    for block in asm.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1)) for k in KEYS}
    return meta


def test_every_conversion_kernel_has_no_lds_no_scratch_and_no_spill():
    hits = {n: k for n, k in _kernels(isa_text.unit_asm(UNIT)).items() if "k_yuv_batch_to_codes" in n}
    # <S, FMT, BILINEAR>: two sample sizes x (4:4:4, 4:0:0, and 4:2:2 and 4:2:0 with either upsampling)
    assert len(hits) == 12, sorted(hits)
    for name, k in hits.items():
        assert k["group_segment_fixed_size"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
    assert len(_kernels(isa_text.unit_asm(UNIT))) == 12            # the unit's only kernels
    print("measured VGPRs:", {n: k["vgpr_count"] for n, k in hits.items()})


def test_the_batched_16_bit_conversion_keeps_the_budget_of_its_single_counterpart():
    meta = _kernels(isa_text.scorer_asm())
    batch = {n: k for n, k in meta.items() if "k_pyramid_bands_xyb16_batch" in n}
    single = {n: k for n, k in meta.items() if "k_pyramid_bands_xyb16ILi3" in n}
    assert len(batch) == 1 and len(single) == 1, (sorted(batch), sorted(single))   # CH = 3 only: nothing uses 4
    (b,), (s,) = batch.values(), single.values()
    assert b["vgpr_spill_count"] == 0 and b["sgpr_spill_count"] == 0 and b["private_segment_fixed_size"] == 0, b
    assert b["group_segment_fixed_size"] <= s["group_segment_fixed_size"], (b, s)
    print(f"measured VGPRs: k_pyramid_bands_xyb16_batch<3> {b['vgpr_count']}, k_pyramid_bands_xyb16<3> {s['vgpr_count']}")


# ---- the calls and the Python side ---------------------------------------------------------------------------------
def test_null_context_is_an_invalid_argument(hbatch_lib):
    from oavif_amd import _lib
    L, E, out = hbatch_lib, _lib.ERR_INVALID_ARG, (ctypes.c_double * 2)()
    f = np.zeros((8, 8, 3), np.uint16)
    pp = (ctypes.POINTER(ctypes.c_uint16) * 2)(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))] * 2)
    y = np.zeros((8, 8), np.uint8)
    frames = (_lib.YuvFrameC * 2)()
    for fr in frames:
        fr.planes[0], fr.row_bytes[0], fr.depth, fr.format, fr.full_range, fr.matrix_coefficients = y.ctypes.data, 8, 8, _lib.YUV_400, 1, 6
    codes = np.zeros((2, 8, 8, 3), np.uint16)
    cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    assert L.ssimu2_hbatch_score_rgb16(None, pp, pp, 2, 8, 8, 10, out) == E
    assert L.ssimu2_hbatch_score_against_reference_rgb16(None, pp, 2, 10, out) == E
    assert L.ssimu2_hbatch_score_rgb16_device(None, 4096, 8192, 384, 2, 8, 8, 10, out) == E
    assert L.ssimu2_hbatch_score_against_reference_rgb16_device(None, 4096, 384, 2, 10, out) == E
    assert L.ssimu2_hbatch_score_against_reference_yuv(None, frames, 2, 16, 0, out) == E
    assert L.ssimu2_hbatch_convert_yuv(None, frames, 2, 8, 8, 16, 0, cp) == E
    # the null context comes before n == 0
    assert L.ssimu2_hbatch_score_rgb16(None, None, None, 0, 8, 8, 10, None) == E
    assert L.ssimu2_hbatch_score_against_reference_rgb16(None, None, 0, 10, None) == E
    assert L.ssimu2_hbatch_score_rgb16_device(None, None, None, 0, 0, 8, 8, 10, None) == E
    assert L.ssimu2_hbatch_score_against_reference_rgb16_device(None, None, 0, 0, 10, None) == E
    assert L.ssimu2_hbatch_score_against_reference_yuv(None, None, 0, 16, 0, None) == E
    assert L.ssimu2_hbatch_convert_yuv(None, None, 0, 8, 8, 16, 0, None) == E


def test_same_version_as_the_product_library(hip_lib, hbatch_lib):
    assert hbatch_lib.ssimu2_version() == hip_lib.ssimu2_version()


def test_the_flag():
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    assert Ssimu2.hbatch is False
    with pytest.raises(ValueError) as ei:
        Ssimu2(0, instrumented=True, hbatch=True)
    assert "instrumented=True and hbatch=True are different libraries" in str(ei.value)
    s = Ssimu2.__new__(Ssimu2)        # no library, no device: a context without the flag makes none of the calls
    s._L = None
    f = np.zeros((1, 8, 8, 3), np.uint16)
    for call in (lambda: s.score_batch_hbd(f, f, 10), lambda: s.score_batch_against_reference_hbd(f, 10),
                 lambda: s.score_batch_hbd_device(0, 0, 384, 1, 8, 8, 10),
                 lambda: s.score_batch_against_reference_hbd_device(0, 384, 1, 10),
                 lambda: s.score_batch_against_reference_yuv([]), lambda: s.convert_yuv_batch([])):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "hbatch=True" in str(ei.value)


def test_no_cpu_fallback_without_device(hbatch_lib):
    """Without a GPU the library refuses as the product library does; with one the flag implies every earlier one."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    if torch.cuda.is_available():
        with Ssimu2(0, hbatch=True) as s:
            assert s.hbatch and s.rbatch and s.yuva and s.chroma and s.maps and s.yuv and s.extended
        return
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, hbatch=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


def test_the_python_side_refuses_what_it_would_otherwise_do_quietly():
    """A YUV batch drops no alpha plane, and the speculative search does not fall back to single calls on a context
    without the flag: both raise before any C call (no library, no device here)."""
    from oavif_amd import Ssimu2, _lib, tq
    from oavif_amd.scorer import YuvFrame
    s = Ssimu2.__new__(Ssimu2)
    s._L, s.hbatch, s.chroma = None, True, True
    y = np.zeros((8, 8), np.uint8)
    plain, alpha = YuvFrame([y], 8, _lib.YUV_400), YuvFrame([y], 8, _lib.YUV_400, alpha=y)
    for call in (s.score_batch_against_reference_yuv, s.convert_yuv_batch):
        with pytest.raises(ValueError) as ei:
            call([plain, alpha])
        assert "frames[1] carries an alpha plane" in str(ei.value)
    s.hbatch = False
    with pytest.raises(ValueError) as ei:
        tq.search_speculative_hip_frames(s, np.zeros((8, 8, 3), np.uint8), lambda q: None)
    assert "hbatch=True" in str(ei.value)
