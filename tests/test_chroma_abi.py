"""The chroma library without a GPU (include/ssimu2_hip_chroma.h): the header against the binding
table, the library's exports (the map library's and the six new calls, nothing else), the new unit's kernels and
includes, build.py's tables (LIBRARIES and MAP_LIBRARIES as they were, the sixth library in a third table), what every new
call answers to a null context, YuvFrame's shapes for the subsampled formats, the refusal the Python side makes before
any C call, and the command line of oavif_amd.yuvscore."""
import ctypes
import os
import re

import numpy as np
import pytest

import chroma_ref
import isa_text
from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes
from test_build_units import _includes, _kernels

HEADER = "ssimu2_hip_chroma.h"
NAMES = ["ssimu2_convert_yuv_chroma", "ssimu2_score_yuv_chroma", "ssimu2_set_reference_yuv_chroma",
         "ssimu2_score_against_reference_yuv_chroma", "ssimu2_error_map_yuv_chroma",
         "ssimu2_error_map_against_reference_yuv_chroma"]
# each mirrors this call with `uint32_t chroma_upsampling` added behind rgb_depth
MIRRORED = {"ssimu2_convert_yuv_chroma": ("ssimu2_hip_yuv.h", "ssimu2_convert_yuv"),
            "ssimu2_score_yuv_chroma": ("ssimu2_hip_yuv.h", "ssimu2_score_yuv"),
            "ssimu2_set_reference_yuv_chroma": ("ssimu2_hip_yuv.h", "ssimu2_set_reference_yuv"),
            "ssimu2_score_against_reference_yuv_chroma": ("ssimu2_hip_yuv.h", "ssimu2_score_against_reference_yuv"),
            "ssimu2_error_map_yuv_chroma": ("ssimu2_hip_map.h", "ssimu2_error_map_yuv"),
            "ssimu2_error_map_against_reference_yuv_chroma": ("ssimu2_hip_map.h", "ssimu2_error_map_against_reference_yuv")}
UNIT = "ssimu2_chroma.hip"
KERNELS = {f"k_yuv_chroma_to_codes<{s}, {v}, {b}>" for s in (1, 2) for v in ("false", "true") for b in ("false", "true")}


@pytest.fixture(scope="module")
def chroma_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.chroma_lib()


def _plain(path):
    return {s for s in _exported(path) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.CHROMA_FUNCTIONS) == NAMES                          # header order
    assert _lib.CHROMA_SYMBOLS == tuple(_lib.CHROMA_FUNCTIONS)
    assert set(_declared_functions(HEADER)) == set(NAMES)
    assert list(prototypes(HEADER)) == NAMES
    others = (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS) |
              set(_lib.MAP_FUNCTIONS))
    assert not set(NAMES) & others
    with open(os.path.join(isa_text.ROOT, "include", HEADER)) as f:
        text = f.read()
    defines = dict(re.findall(r"^#define\s+(SSIMU2_\w+)\s+(\d+)", text, re.M))
    assert defines == {"SSIMU2_YUV_422": "2", "SSIMU2_YUV_420": "3", "SSIMU2_CHROMA_BILINEAR": "0", "SSIMU2_CHROMA_NEAREST": "1"}
    assert (_lib.YUV_422, _lib.YUV_420, _lib.CHROMA_BILINEAR, _lib.CHROMA_NEAREST) == (2, 3, 0, 1)
    assert (chroma_ref.YUV_422, chroma_ref.YUV_420) == (_lib.YUV_422, _lib.YUV_420)
    assert os.path.basename(_lib.CHROMA_LIB_PATH) == "liboavif_hip_chroma.so"


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header_and_the_call_it_mirrors(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.CHROMA_FUNCTIONS[name]
    ret, params = prototypes(HEADER)[name]
    check(name, (ret, params), restype, argtypes)
    for decl, ctype in zip(params, argtypes):
        is_frame = re.match(r"const\s+ssimu2_yuv_frame\s*\*", decl) is not None
        assert (ctype is ctypes.POINTER(_lib.YuvFrameC)) == is_frame, (name, decl, ctype)
    header, old = MIRRORED[name]
    old_ret, old_params = prototypes(header)[old]
    norm = lambda ds: [re.sub(r"\s+", " ", d) for d in ds]
    at = norm(params).index("uint32_t chroma_upsampling")
    assert norm(params)[at - 1] == "uint32_t rgb_depth"
    assert ret == old_ret and norm(params[:at] + params[at + 1:]) == norm(old_params), name
    old_res, old_args = (_lib.YUV_FUNCTIONS if old in _lib.YUV_FUNCTIONS else _lib.MAP_FUNCTIONS)[old]
    assert restype is old_res and argtypes[:at] + argtypes[at + 1:] == old_args and argtypes[at] is ctypes.c_uint32


def test_chroma_library_exports_the_map_library_plus_the_six_calls(chroma_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS) | set(_lib.CHROMA_SYMBOLS)
    plain, map_plain = _plain(_lib.CHROMA_LIB_PATH), _plain(_lib.MAP_LIB_PATH)
    assert plain == want, plain ^ want
    assert plain - map_plain == set(NAMES) and map_plain <= plain
    for name in want:
        assert hasattr(chroma_lib, name), name


def test_the_other_five_libraries_have_none_of_it(hip_lib):
    from oavif_amd import _lib
    for path in (_lib.LIB_PATH, _lib.INSTR_LIB_PATH, _lib.EXT_LIB_PATH, _lib.YUV_LIB_PATH, _lib.MAP_LIB_PATH):
        assert not set(_exported(path)) & set(NAMES), path


def test_the_unit_defines_its_eight_kernels_and_no_constant_block():
    assert _kernels(UNIT) == KERNELS
    assert "c_k" not in isa_text.unit_asm(UNIT)


def test_the_kernels_use_no_lds_and_no_scratch():
    asm = isa_text.unit_asm(UNIT)
    for field in ("group_segment_fixed_size", "private_segment_fixed_size"):
        values = re.findall(rf"^\s*\.amdhsa_{field}\s+(\d+)", asm, re.M)
        assert len(values) == len(KERNELS) and set(values) == {"0"}, (field, values)


def test_the_unit_reaches_the_scorer_through_the_front_end_header_alone():
    from oavif_amd import build
    inc = _includes(os.path.join(build.CSRC, UNIT))
    assert "ssimu2_host.h" in inc and HEADER in inc and "ssimu2_yuv_pixel.h" in inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_map.hip", "ssimu2_kernels.h",
                      "ssimu2_recursive.h"}
    # the shared arithmetic header holds device functions only, and both YUV units take the two halves from it
    shared = _includes(os.path.join(build.CSRC, "ssimu2_yuv_pixel.h"))
    assert not shared & {"ssimu2_kernels.h", "ssimu2_recursive.h", "ssimu2_hip.hip"}
    with open(os.path.join(build.CSRC, "ssimu2_yuv_pixel.h")) as f:
        text = re.sub(r"//.*", "", f.read())
    assert "__global__" not in text and "__constant__" not in text
    assert "ssimu2_yuv_pixel.h" in _includes(os.path.join(build.CSRC, "ssimu2_yuv.hip"))
    for unit in (UNIT, "ssimu2_yuv.hip"):
        with open(os.path.join(build.CSRC, unit)) as f:
            body = re.sub(r"//.*", "", f.read())
        assert "yuv_unorm(" in body and "yuv_codes(" in body and "div_rn" not in body, unit


def test_build_keeps_its_two_tables_and_knows_the_sixth_library_in_a_third(hip_lib):
    from oavif_amd import _lib, build
    assert list(build.LIBRARIES) == [build.LIB_PATH, build.INSTR_LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH]
    assert build.LIBRARIES == {build.LIB_PATH: build.SOURCES, build.INSTR_LIB_PATH: build.INSTR_SOURCES,
                               build.EXT_LIB_PATH: build.EXT_SOURCES, build.YUV_LIB_PATH: build.YUV_SOURCES}
    assert build.YUV_SOURCES == ["ssimu2_hip.hip", "tq.cpp", "png_ingest.cpp", "remote_client.cpp", "ssimu2_ext.hip", "ssimu2_yuv.hip"]
    assert build.MAP_LIBRARIES == {build.MAP_LIB_PATH: [*build.YUV_SOURCES, "ssimu2_map.hip"]}
    assert len(build.compile_units()) == 7 and build.map_units() == ["ssimu2_map.hip"]
    assert os.path.samefile(os.path.dirname(build.CHROMA_LIB_PATH), os.path.dirname(_lib.CHROMA_LIB_PATH))
    assert os.path.basename(build.CHROMA_LIB_PATH) == "liboavif_hip_chroma.so"
    assert build.CHROMA_LIB_PATH not in build.LIBRARIES and build.CHROMA_LIB_PATH not in build.MAP_LIBRARIES
    assert build.CHROMA_LIBRARIES == {build.CHROMA_LIB_PATH: build.CHROMA_SOURCES}
    # the map library's units plus the one new unit, compiled once
    assert build.CHROMA_SOURCES[:-1] == build.MAP_SOURCES and build.CHROMA_SOURCES[-1] == UNIT
    assert build.chroma_units() == [UNIT] and UNIT not in build.compile_units() and UNIT not in build.map_units()
    assert os.path.exists(os.path.join(build.CSRC, UNIT))
    assert os.path.exists(build.CHROMA_LIB_PATH)                          # built by build.build()
    assert build.MAX_COMPILES <= 6


def test_build_rebuilds_when_the_sixth_library_is_missing(hip_lib, monkeypatch, tmp_path):
    from oavif_amd import build
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "CHROMA_LIBRARIES", {str(tmp_path / "liboavif_hip_chroma.so"): build.CHROMA_SOURCES})
    assert build.libs_need_build()


def test_same_version_as_the_product_library(hip_lib, chroma_lib):
    assert chroma_lib.ssimu2_version() == hip_lib.ssimu2_version()


def test_null_context_is_an_invalid_argument(chroma_lib):
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    f = YuvFrame([np.full((4, 4), 100, np.uint8), np.full((2, 2), 128, np.uint8), np.full((2, 2), 128, np.uint8)],
                 format=_lib.YUV_420)
    c = f.as_c()
    px, m, out = (ctypes.c_uint16 * 48)(), (ctypes.c_float * 16)(), ctypes.c_double()
    L, E, fr, sc = chroma_lib, _lib.ERR_INVALID_ARG, ctypes.byref(c), ctypes.byref(out)
    assert L.ssimu2_convert_yuv_chroma(None, fr, 4, 4, 16, 0, px) == E
    assert L.ssimu2_score_yuv_chroma(None, fr, fr, 4, 4, 16, 0, sc) == E
    assert L.ssimu2_set_reference_yuv_chroma(None, fr, 4, 4, 16, 1) == E
    assert L.ssimu2_score_against_reference_yuv_chroma(None, fr, 16, 1, sc) == E
    assert L.ssimu2_error_map_yuv_chroma(None, fr, fr, 4, 4, 16, 0, m, sc) == E
    assert L.ssimu2_error_map_against_reference_yuv_chroma(None, fr, 16, 0, m, sc) == E


def test_no_cpu_fallback_without_device(chroma_lib):
    """Without a GPU the chroma library refuses as the product library does; with one it creates a context."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    if torch.cuda.is_available():
        with Ssimu2(0, chroma=True) as s:
            assert s.chroma and s.maps and s.yuv
        return
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, chroma=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(ValueError):
        Ssimu2(0, instrumented=True, chroma=True)


# ---- YuvFrame ------------------------------------------------------------------------------------------------------
def test_yuvframe_takes_chroma_planes_of_their_own_size():
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    for fmt in (_lib.YUV_422, _lib.YUV_420):
        for w, h in [(1, 1), (2, 1), (1, 2), (5, 4), (4, 5), (97, 53)]:
            ch, cw = chroma_ref.chroma_shape(w, h, fmt)
            y, u, v = np.zeros((h, w), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)
            f = YuvFrame([y, u, v], 8, fmt)
            assert (f.width, f.height, f.subsampled) == (w, h, True)
            assert [p.shape for p in f.planes] == [(h, w), (ch, cw), (ch, cw)]
            c = f.as_c()
            assert c.format == fmt and c.row_bytes[0] == w and c.row_bytes[1] == c.row_bytes[2] == cw
            for bad in [(ch + 1, cw), (ch, cw + 1), (h + 2, w + 2), (cw + 3, ch + 5)]:
                for k in (1, 2):
                    planes = [y, u, v]
                    planes[k] = np.zeros(bad, np.uint8)
                    with pytest.raises(ValueError):
                        YuvFrame(planes, 8, fmt)
            with pytest.raises(ValueError):
                YuvFrame([y, u.reshape(-1), v], 8, fmt)
            with pytest.raises(ValueError):
                YuvFrame([y, u], 8, fmt)
            with pytest.raises(TypeError):
                YuvFrame([y, u.astype(np.uint16), v], 8, fmt)
    # a strided view of a decoder's chroma plane goes through as it is
    buf, view = __import__("yuv_ref").laid_out(np.ones((27, 49), np.uint8), 64, 3, seed=1)
    f = YuvFrame([np.zeros((53, 97), np.uint8), view, view], 8, _lib.YUV_420)
    assert f.planes[1].ctypes.data == view.ctypes.data and f.as_c().row_bytes[1] == 64
    # 4:4:4 keeps its same-shape rule, 4:0:0 its one plane
    y = np.zeros((4, 6), np.uint8)
    assert not YuvFrame([y, y, y]).subsampled and not YuvFrame([y], format=_lib.YUV_400).subsampled
    with pytest.raises(ValueError):
        YuvFrame([y, np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8)])
    with pytest.raises(ValueError):
        YuvFrame([y, np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8)], format=_lib.YUV_444)


def _sub_frame(fmt):
    from oavif_amd.scorer import YuvFrame
    ch, cw = chroma_ref.chroma_shape(4, 4, fmt) if fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420) else (4, 4)
    return YuvFrame([np.full((4, 4), 100, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)], 8, fmt)


def test_subsampled_frames_need_the_chroma_library():
    """A context of another library refuses a subsampled frame before any C call, naming chroma=True; yuv=True and
    maps=True are not enough.  A 4:4:4 frame is not refused here."""
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    for fmt in (_lib.YUV_422, _lib.YUV_420):
        f, full = _sub_frame(fmt), _sub_frame(_lib.YUV_444)
        for yuv, maps in ((False, False), (True, False), (True, True)):
            s = Ssimu2.__new__(Ssimu2)        # no library, no device: the refusal comes first
            s._L, s._ctx, s.extended, s.yuv, s.maps = None, ctypes.c_void_p(1), False, yuv, maps
            for call in (lambda: s.convert_yuv(f), lambda: s.compute_ssimu2_yuv(f, f), lambda: s.compute_ssimu2_yuv(full, f),
                         lambda: s.compute_ssimu2_yuv(f, full, 16, "nearest"), lambda: s.set_reference_yuv(f),
                         lambda: s.score_against_reference_yuv(f), lambda: s.error_map_yuv(f, f),
                         lambda: s.error_map_yuv(f, full), lambda: s.error_map_against_reference_yuv(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED and "chroma=True" in str(ei.value)
            for call in (lambda: s.convert_yuv(f, 16, "cubic"), lambda: s.convert_yuv(full, 16, "cubic"),
                         lambda: s.score_against_reference_yuv(full, 16, None), lambda: s.error_map_yuv(f, f, 16, 0)):
                with pytest.raises(ValueError):
                    call()
            if not yuv:                       # and a 4:4:4 frame gets the refusal it always got
                with pytest.raises(Ssimu2Error) as ei:
                    s.convert_yuv(full)
                assert "yuv=True" in str(ei.value)
            s._ctx = ctypes.c_void_p()


# ---- command line --------------------------------------------------------------------------------------------------
def test_yuvscore_chroma_upsampling_option(capsys):
    from oavif_amd import yuvscore
    a = yuvscore.parse_args(["r.png", "d.avif"])
    assert a.chroma_upsampling == "bilinear"
    assert (a.ref, a.dist, a.rgb_depth, a.blur, a.compare, a.device, a.map) == ("r.png", "d.avif", 16, "fir", False, 0, None)
    for v in ("bilinear", "nearest"):
        assert yuvscore.parse_args(["r.png", "d.avif", "--chroma-upsampling", v]).chroma_upsampling == v
    a = yuvscore.parse_args(["r.avif", "d.avif", "--chroma-upsampling", "nearest", "--map", "m.pfm", "--compare", "--rgb-depth", "10"])
    assert (a.chroma_upsampling, a.map, a.compare, a.rgb_depth) == ("nearest", "m.pfm", True, 10)
    for bad in (["r.png", "d.avif", "--chroma-upsampling"], ["r.png", "d.avif", "--chroma-upsampling", "cubic"],
                ["r.png", "d.avif", "--chroma-upsampling", "1"]):
        with pytest.raises(SystemExit) as ei:
            yuvscore.parse_args(bad)
        assert ei.value.code == 2, bad
    with pytest.raises(SystemExit):
        yuvscore.parse_args(["-h"])
    assert "--chroma-upsampling" in capsys.readouterr().out


def test_yuvscore_lets_subsampled_frames_through():
    from oavif_amd import _lib, yuvscore

    class Decoded:
        has_alpha, depth, full_range, matrix_coefficients = False, 8, True, 6

    for fmt in (_lib.YUV_422, _lib.YUV_420):
        d = Decoded()
        ch, cw = chroma_ref.chroma_shape(7, 5, fmt)
        d.format, d.planes = fmt, [np.zeros((5, 7), np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)]
        f = yuvscore.frame_of(d)
        assert f.subsampled and f.format == fmt and (f.width, f.height) == (7, 5)
    d.format = 0
    with pytest.raises(ValueError):
        yuvscore.frame_of(d)
    d.format, d.matrix_coefficients = _lib.YUV_420, 0
    with pytest.raises(ValueError):
        yuvscore.frame_of(d)
