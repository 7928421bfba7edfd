"""The map library without a GPU (include/ssimu2_hip_map.h): the header against the binding
table, the library's exports (the YUV library's and the six map calls, nothing else), build.py's tables (the four
libraries and seven units of LIBRARIES as they were, the fifth library beside them), what every new call answers to a null
context, no CPU fallback, the refusals the Python side makes before any C call, and the command lines of
oavif_amd.yuvscore --map and oavif_amd.errmap --full-depth."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes

MAP_HEADER = "ssimu2_hip_map.h"
MAP_NAMES = ["ssimu2_error_map_rgb16", "ssimu2_error_map_against_reference_rgb16", "ssimu2_error_map_rgba8",
             "ssimu2_error_map_against_reference_rgba8", "ssimu2_error_map_yuv", "ssimu2_error_map_against_reference_yuv"]
UNITS = {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_instrument.hip", "tq.cpp", "png_ingest.cpp",
         "remote_client.cpp"}


@pytest.fixture(scope="module")
def map_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.map_lib()


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.MAP_FUNCTIONS) == MAP_NAMES                         # header order
    assert _lib.MAP_SYMBOLS == tuple(_lib.MAP_FUNCTIONS)
    assert set(_declared_functions(MAP_HEADER)) == set(_lib.MAP_FUNCTIONS)
    assert list(prototypes(MAP_HEADER)) == MAP_NAMES
    others = set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS)
    assert not set(_lib.MAP_FUNCTIONS) & others


@pytest.mark.parametrize("name", MAP_NAMES)
def test_signature_matches_the_header(name):
    """test_binding_signatures.check holds the count and the class of every argument; the struct pointers are held here:
    every `const ssimu2_yuv_frame*` parameter is a POINTER(YuvFrameC), nothing else is.  Every call ends in
    `float* out_map, double* out_score`."""
    from oavif_amd import _lib
    restype, argtypes = _lib.MAP_FUNCTIONS[name]
    ret, params = prototypes(MAP_HEADER)[name]
    check(name, (ret, params), restype, argtypes)
    for decl, ctype in zip(params, argtypes):
        is_frame = re.match(r"const\s+ssimu2_yuv_frame\s*\*", decl) is not None
        assert (ctype is ctypes.POINTER(_lib.YuvFrameC)) == is_frame, (name, decl, ctype)
    frames = {"ssimu2_error_map_yuv": 2, "ssimu2_error_map_against_reference_yuv": 1}.get(name, 0)
    assert sum("ssimu2_yuv_frame" in d for d in params) == frames
    assert [re.sub(r"\s+", " ", d) for d in params[-2:]] == ["float* out_map", "double* out_score"]
    assert argtypes[-2:] == [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.c_void_p


def test_map_library_exports_the_yuv_library_plus_the_six_map_calls(map_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS)
    plain = {s for s in _exported(_lib.MAP_LIB_PATH) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}
    assert plain == want, plain ^ want
    yuv_plain = {s for s in _exported(_lib.YUV_LIB_PATH) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}
    assert plain - yuv_plain == set(MAP_NAMES) and yuv_plain <= plain
    for name in want:
        assert hasattr(map_lib, name), name


def test_the_other_libraries_have_none_of_it(hip_lib):
    from oavif_amd import _lib
    for path in (_lib.LIB_PATH, _lib.INSTR_LIB_PATH, _lib.EXT_LIB_PATH, _lib.YUV_LIB_PATH):
        assert not set(_exported(path)) & set(_lib.MAP_SYMBOLS), path


def test_build_keeps_its_four_libraries_and_knows_the_fifth_beside_them(hip_lib):
    from oavif_amd import _lib, build
    assert list(build.LIBRARIES) == [build.LIB_PATH, build.INSTR_LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH]
    assert set(build.compile_units()) == UNITS and len(build.compile_units()) == 7
    assert build.MAX_COMPILES <= 6
    assert os.path.samefile(os.path.dirname(build.MAP_LIB_PATH), os.path.dirname(_lib.MAP_LIB_PATH))
    assert os.path.basename(build.MAP_LIB_PATH) == "liboavif_hip_map.so" and build.MAP_LIB_PATH not in build.LIBRARIES
    assert build.MAP_LIBRARIES == {build.MAP_LIB_PATH: build.MAP_SOURCES}
    # the YUV library's units plus the one new unit, compiled once
    assert build.MAP_SOURCES[:-1] == build.YUV_SOURCES and build.MAP_SOURCES[-1] == "ssimu2_map.hip"
    assert build.map_units() == ["ssimu2_map.hip"] and "ssimu2_map.hip" not in build.compile_units()
    assert os.path.exists(os.path.join(build.CSRC, "ssimu2_map.hip"))
    assert os.path.exists(build.MAP_LIB_PATH)                             # built by build.build()


def test_build_rebuilds_when_the_fifth_library_is_missing(hip_lib, monkeypatch, tmp_path):
    """libs_need_build walks the fifth library's table too: with its path pointing nowhere the libraries need a build."""
    from oavif_amd import build
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "MAP_LIBRARIES", {str(tmp_path / "liboavif_hip_map.so"): build.MAP_SOURCES})
    assert build.libs_need_build()


def test_the_map_unit_reaches_the_scorer_through_the_front_end_header_alone():
    from oavif_amd import build
    with open(os.path.join(build.CSRC, "ssimu2_map.hip")) as f:
        inc = {os.path.basename(m) for m in re.findall(r'^\s*#\s*include\s+[<"]([^>"]+)[>"]', f.read(), re.M)}
    assert "ssimu2_host.h" in inc and "ssimu2_hip_map.h" in inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_kernels.h", "ssimu2_recursive.h"}


def test_same_version_as_the_product_library(hip_lib, map_lib):
    assert map_lib.ssimu2_version() == hip_lib.ssimu2_version()


def _frame():
    from oavif_amd.scorer import YuvFrame
    f = YuvFrame([np.full((4, 4), v, np.uint8) for v in (100, 128, 128)])
    return f, f.as_c()


def test_null_context_is_an_invalid_argument(map_lib):
    from oavif_amd import _lib
    _f, c = _frame()
    px16, px8 = (ctypes.c_uint16 * 48)(), (ctypes.c_uint8 * 64)()
    m, out = (ctypes.c_float * 16)(), ctypes.c_double()
    L, E = map_lib, _lib.ERR_INVALID_ARG
    assert L.ssimu2_error_map_rgb16(None, px16, px16, 4, 4, 16, m, ctypes.byref(out)) == E
    assert L.ssimu2_error_map_against_reference_rgb16(None, px16, 16, m, ctypes.byref(out)) == E
    assert L.ssimu2_error_map_rgba8(None, px8, 16, px8, 16, 4, 4, 0, m, ctypes.byref(out)) == E
    assert L.ssimu2_error_map_against_reference_rgba8(None, px8, 16, m, ctypes.byref(out)) == E
    assert L.ssimu2_error_map_yuv(None, ctypes.byref(c), ctypes.byref(c), 4, 4, 16, m, ctypes.byref(out)) == E
    assert L.ssimu2_error_map_against_reference_yuv(None, ctypes.byref(c), 16, m, ctypes.byref(out)) == E


def test_no_cpu_fallback_without_device(map_lib):
    """Without a GPU the map library refuses as the product library does; with one it creates a context."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    ctx = ctypes.c_void_p()
    rc = map_lib.ssimu2_ctx_create(0, None, ctypes.byref(ctx))
    if torch.cuda.is_available():
        assert rc == _lib.OK and ctx.value
        map_lib.ssimu2_ctx_destroy(ctx)
        return
    assert rc == _lib.ERR_NO_DEVICE and not ctx.value
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, maps=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


def test_maps_and_instrumented_exclude_each_other():
    from oavif_amd import Ssimu2
    with pytest.raises(ValueError):
        Ssimu2(0, instrumented=True, maps=True)


def test_map_methods_need_the_map_library():
    """A context of another library refuses before any C call, naming maps=True; extended=True and yuv=True are not
    enough."""
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    f, _c = _frame()
    u16, rgba = np.zeros((4, 4, 3), np.uint16), np.zeros((4, 4, 4), np.uint8)
    for extended, yuv in ((False, False), (True, False), (True, True)):
        s = Ssimu2.__new__(Ssimu2)        # no library, no device: the refusal comes first
        s._L, s._ctx, s.extended, s.yuv = None, ctypes.c_void_p(1), extended, yuv
        for call in (lambda: s.error_map_hbd(u16, u16, 16), lambda: s.error_map_against_reference_hbd(u16, 16),
                     lambda: s.error_map_rgba(rgba, rgba, 0), lambda: s.error_map_against_reference_rgba(rgba),
                     lambda: s.error_map_yuv(f, f), lambda: s.error_map_against_reference_yuv(f)):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "maps=True" in str(ei.value)
        s._ctx = ctypes.c_void_p()


# ---- command lines -------------------------------------------------------------------------------------------------
def test_yuvscore_map_option():
    from oavif_amd import yuvscore
    a = yuvscore.parse_args(["r.png", "d.avif"])
    assert (a.ref, a.dist, a.rgb_depth, a.blur, a.compare, a.device, a.map) == ("r.png", "d.avif", 16, "fir", False, 0, None)
    for out in ("m.png", "m.pam", "M.PFM"):
        assert yuvscore.parse_args(["r.png", "d.avif", "--map", out]).map == out
    a = yuvscore.parse_args(["r.avif", "d.avif", "--rgb-depth", "10", "--map", "m.pfm", "--compare"])
    assert (a.rgb_depth, a.map, a.compare) == (10, "m.pfm", True)
    for bad in (["r.png", "d.avif", "--map"], ["r.png", "d.avif", "--map", "m.jpg"], ["r.png", "d.avif", "--map", "m"]):
        with pytest.raises(SystemExit) as ei:
            yuvscore.parse_args(bad)
        assert ei.value.code == 2, bad


def test_errmap_full_depth_option(capsys):
    from oavif_amd import errmap
    a = errmap.parse_args(["r.png", "d.png", "o.pfm"])
    assert (a.ref, a.dist, a.out, a.blur, a.device, a.full_depth) == ("r.png", "d.png", "o.pfm", "fir", 0, False)
    a = errmap.parse_args(["r.png", "d.png", "o.png", "--full-depth", "--blur", "recursive"])
    assert a.full_depth is True and a.blur == "recursive"
    with pytest.raises(SystemExit) as ei:
        errmap.parse_args(["r.png", "d.png", "o.png", "--full-depth", "1"])
    assert ei.value.code == 2
    with pytest.raises(SystemExit):
        errmap.parse_args(["-h"])
    assert "--full-depth" in capsys.readouterr().out


def test_errmap_full_depth_keeps_sixteen_bit_samples(tmp_path):
    """load_rgb16: a 16-bit PNG's own samples; an 8-bit image's as 257 u.  No device."""
    import struct
    import zlib
    from oavif_amd import errmap

    def png(path, arr, depth):
        h, w, _ = arr.shape
        raw = np.zeros((h, 1 + w * 3 * (depth // 8)), np.uint8)
        raw[:, 1:] = (arr.astype(">u2") if depth == 16 else arr).reshape(h, -1).view(np.uint8)

        def chunk(kind, data):
            return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
        path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 2, 0, 0, 0)) +
                         chunk(b"IDAT", zlib.compress(raw.tobytes())) + chunk(b"IEND", b""))

    rng = np.random.default_rng(3)
    a16 = rng.integers(0, 65536, (5, 7, 3)).astype(np.uint16)
    a8 = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    png(tmp_path / "a16.png", a16, 16)
    png(tmp_path / "a8.png", a8, 8)
    got16, got8 = errmap.load_rgb16(str(tmp_path / "a16.png")), errmap.load_rgb16(str(tmp_path / "a8.png"))
    assert got16.dtype == got8.dtype == np.uint16 and got16.flags.c_contiguous
    assert np.array_equal(got16, a16) and np.array_equal(got8, a8.astype(np.uint16) * 257)
