"""YUV frames with an alpha plane without a GPU (include/ssimu2_hip_yuva.h): the consequences the
header states of its definition, on the numpy restatement (tests/yuva_ref.py); the restatement against libavif's own RGBA
output where the header says the two agree; the bridge's DecodedYuv.alpha and its layout guard; the seventh library's
exports and build tables; the binding's signatures; and the argument errors YuvFrame and Ssimu2 raise before any device
is touched."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import chroma_ref
import isa_text
import yuv_ref
import yuva_ref
from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes
from test_build_units import _includes, _kernels

HEADER = "ssimu2_hip_yuva.h"
UNIT = "ssimu2_yuva.hip"
NAMES = ["ssimu2_composite_yuva", "ssimu2_score_yuva", "ssimu2_set_reference_yuva", "ssimu2_score_against_reference_yuva",
         "ssimu2_error_map_yuva", "ssimu2_error_map_against_reference_yuva"]
# each mirrors this call of ssimu2_hip_chroma.h; the first three and the pair map add `uint32_t background_rgb`
MIRRORED = {"ssimu2_composite_yuva": "ssimu2_convert_yuv_chroma", "ssimu2_score_yuva": "ssimu2_score_yuv_chroma",
            "ssimu2_set_reference_yuva": "ssimu2_set_reference_yuv_chroma",
            "ssimu2_score_against_reference_yuva": "ssimu2_score_against_reference_yuv_chroma",
            "ssimu2_error_map_yuva": "ssimu2_error_map_yuv_chroma",
            "ssimu2_error_map_against_reference_yuva": "ssimu2_error_map_against_reference_yuv_chroma"}
WITH_BACKGROUND = {"ssimu2_composite_yuva", "ssimu2_score_yuva", "ssimu2_set_reference_yuva", "ssimu2_error_map_yuva"}


# ---- the definition's consequences -----------------------------------------------------------------------------------
def test_at_depth_8_and_rgb_depth_8_the_code_is_the_rgba_composite_for_all_2_24_triples():
    a = np.arange(256, dtype=np.uint32)[:, None, None]
    c = np.arange(256, dtype=np.uint32)[None, :, None]
    b = np.arange(256, dtype=np.uint32)[None, None, :]
    got = yuva_ref.composite(c, a, 8, 8, b)
    assert got.shape == (256, 256, 256)
    assert np.array_equal(got, a * c + (255 - a) * b)


@pytest.mark.parametrize("depth,rgb_depth", yuva_ref.DEPTH_PAIRS + [(8, 8)])
def test_range_transparent_and_opaque_at_every_depth_pair(depth, rgb_depth):
    ma, mc = (1 << depth) - 1, (1 << rgb_depth) - 1
    assert (ma * mc) % 2 == 1 and ma * mc < 1 << 28 and 255 * 255 * ma * mc < 1 << 44
    rng = np.random.default_rng(depth * 100 + rgb_depth)
    every_a = np.arange(ma + 1)
    cs = np.unique(np.concatenate([[0, 1, mc // 2, mc - 1, mc], rng.integers(0, mc + 1, 40)]))
    bs = np.array([0, 1, 127, 128, 254, 255])
    n = yuva_ref.composite(cs[None, :, None], every_a[:, None, None], depth, rgb_depth, bs[None, None, :]).astype(np.int64)
    assert n.min() == 0 and n.max() == yuva_ref.TOP
    # a = 0: the background alone, whatever the colour
    assert np.array_equal(n[0], np.broadcast_to(255 * bs[None, :], n[0].shape))
    # a = ma: the colour alone, rounded to the nearest of the 65,026 codes (den is odd: no ties)
    opaque = (2 * yuva_ref.TOP * cs + mc) // (2 * mc)
    assert np.array_equal(n[ma], np.broadcast_to(opaque[:, None], n[ma].shape))
    if rgb_depth == 8:
        assert np.array_equal(opaque, 255 * cs)
    # the nearest code to the exact blend, everywhere: |n den - 255 num| <= (den - 1) / 2
    den = ma * mc
    num = every_a[:, None, None] * cs[None, :, None] * 255 + (ma - every_a[:, None, None]) * bs[None, None, :] * mc
    assert (np.abs(n * den - 255 * num) <= (den - 1) // 2).all()
    # n does not decrease in a when the colour is at least the background, nor increase when it is at most
    assert (np.diff(n[:, -1, 0]) >= 0).all() and (np.diff(n[:, 0, -1]) <= 0).all()
    # samples above ma are read as ma
    if depth > 8:
        over = np.array([ma + 1, 4095 if depth < 12 else 5000, 65535])
        assert np.array_equal(yuva_ref.composite(cs[None, :], over[:, None], depth, rgb_depth, 77),
                              np.broadcast_to(yuva_ref.composite(cs, ma, depth, rgb_depth, 77)[None, :], (3, len(cs))))


def test_opaque_codes_at_other_rgb_depths_are_quantised_to_the_tables_levels():
    """What the header says an opaque frame does not keep: at rgb_depth 16 two colour codes may share a composite code,
    at rgb_depth 10 the composite code is not a multiple that a table of depth 10 would be read at."""
    c16 = np.arange(65536)
    n16 = yuva_ref.composite(c16, 255, 8, 16, 0)
    assert len(np.unique(n16)) == yuva_ref.TOP + 1 < 65536
    n10 = yuva_ref.composite(np.arange(1024), 1023, 10, 10, 0).astype(np.int64)
    assert ((n10 * 1023) != np.arange(1024) * yuva_ref.TOP).any()


@pytest.mark.parametrize("name,fmt", list(yuva_ref.FORMATS.items()))
def test_frames_under_full_transparency_and_without_alpha(name, fmt):
    w, h, bg = 13, 7, 0x1A80E6
    for depth, rgb_depth in [(8, 8), (10, 16), (12, 12)]:
        planes, alpha = yuva_ref.random_frame(w, h, depth, fmt, seed=depth)
        other, _ = yuva_ref.random_frame(w, h, depth, fmt, seed=depth + 50)
        zero = np.zeros_like(alpha)
        a = yuva_ref.codes(planes, zero, depth, True, 6, rgb_depth, fmt, bg)
        assert np.array_equal(a, yuva_ref.codes(other, zero, depth, True, 6, rgb_depth, fmt, bg))
        assert np.array_equal(a, np.broadcast_to((255 * yuva_ref.background(bg)).astype(np.uint16), a.shape))
        full = np.full_like(alpha, (1 << depth) - 1)
        assert np.array_equal(yuva_ref.codes(planes, None, depth, True, 6, rgb_depth, fmt, bg),
                              yuva_ref.codes(planes, full, depth, True, 6, rgb_depth, fmt, bg))
    planes, alpha = yuva_ref.random_frame(w, h, 8, fmt, seed=3)
    assert np.array_equal(yuva_ref.codes(planes, None, 8, False, 1, 8, fmt, bg).astype(np.uint32),
                          255 * yuva_ref.colour_codes(planes, 8, False, 1, 8, fmt).astype(np.uint32))


# ---- against libavif -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def avif():
    from oavif_amd import avif_bridge as ab
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    return ab._lib()


def rgba_source(w, h, seed, opaque=False):
    from oavif_amd import synth
    rgb = synth.make_ref(w, h, seed=seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.clip((0.45 * min(w, h) - np.hypot(xx - w / 2.0, yy - h / 2.0)) * 40.0 + 128.0, 0, 255).astype(np.uint8)
    a[:3, :5] = np.arange(5, dtype=np.uint8) * 60          # a few odd values in a corner
    if opaque:
        return np.ascontiguousarray(rgb)
    return np.ascontiguousarray(np.concatenate([rgb, a[..., None]], -1))


def encoded(src, yuv_format, quality_alpha, q=70):
    from oavif_amd import avif_bridge as ab, cli
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.quality_alpha, o.matrix_coefficients = False, 10, quality_alpha, 6
    o.tune = "psnr"          # libaom refuses tune=ssim for the lossless alpha plane of quality_alpha 100
    return ab.encode(src, 8, o, q, yuv_format=yuv_format)


def libavif_rgba8(data):
    """libavif's own RGBA8 rows of the file, from its built-in converter (avoidLibYUV = 1)."""
    from oavif_amd import avif_bridge as ab
    L = ab._lib()
    with ab.decode_yuv(data) as d:           # keeps the decoder, and decoder->image, alive
        img = ab._ptr(d._dec, ab._DEC_IMAGE)
        rgb = ctypes.create_string_buffer(ab._RGB_SIZE)
        L.avifRGBImageSetDefaults(rgb, img)
        struct.pack_into("<I", rgb, ab._RGB_DEPTH, 8)
        struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGBA)
        struct.pack_into("<i", rgb, 24, 1)                                   # avoidLibYUV
        assert L.avifRGBImageAllocatePixels(rgb) == 0
        try:
            assert L.avifImageYUVToRGB(img, rgb) == 0
            pix, row = struct.unpack_from("<QI", rgb.raw, ab._RGB_PIXELS)
            a = np.ctypeslib.as_array((ctypes.c_uint8 * (row * d.height)).from_address(pix)).reshape(d.height, row)
            return np.array(a[:, :d.width * 4].reshape(d.height, d.width, 4), copy=True)
        finally:
            L.avifRGBImageFreePixels(rgb)


@pytest.mark.parametrize("quality_alpha", [100, 60], ids=["lossless-alpha", "lossy-alpha"])
@pytest.mark.parametrize("yuv_format", [1, 3], ids=["444", "420"])
def test_the_composite_of_the_planes_is_the_composite_of_libavifs_rgba(avif, yuv_format, quality_alpha):
    from oavif_amd import avif_bridge as ab
    w, h = 67, 41
    src = rgba_source(w, h, seed=yuv_format)
    data = encoded(src, yuv_format, quality_alpha)
    theirs = libavif_rgba8(data)
    with ab.decode_yuv(data) as d:
        assert d.format == yuv_format and d.depth == 8 and d.has_alpha and d.alpha is not None
        if quality_alpha == 100:
            assert np.array_equal(d.alpha, src[..., 3])
        else:
            assert not np.array_equal(d.alpha, src[..., 3])
        assert np.array_equal(d.alpha, theirs[..., 3])
        for bg in (0x000000, 0xFFFFFF, 0x1A80E6):
            got = yuva_ref.codes(d.planes, d.alpha, 8, d.full_range, d.matrix_coefficients, 8, d.format, bg)
            a = theirs[..., 3:4].astype(np.uint32)
            exp = a * theirs[..., :3] + (255 - a) * yuva_ref.background(bg).astype(np.uint32)
            bad = got != exp
            assert not bad.any(), (yuv_format, quality_alpha, bg, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert np.array_equal(yuva_ref.rgba8(d.planes, d.alpha, d.full_range, d.matrix_coefficients, d.format), theirs)


# ---- DecodedYuv.alpha ------------------------------------------------------------------------------------------------
def test_decoded_yuv_hands_out_the_alpha_plane(avif):
    from oavif_amd import avif_bridge as ab
    w, h = 37, 23
    src = rgba_source(w, h, seed=9)
    with ab.decode_yuv(encoded(src, 1, 100)) as d:
        assert d.has_alpha and d.alpha_premultiplied is False
        assert d.alpha.shape == (h, w) and d.alpha.dtype == np.uint8
        assert d.alpha_row_bytes >= w and d.alpha.strides == (d.alpha_row_bytes, 1)
        assert np.array_equal(d.alpha, src[..., 3])
        assert not any(np.shares_memory(d.alpha, p) for p in d.planes)
    assert d.alpha is None and d.planes is None            # closed
    with ab.decode_yuv(encoded(rgba_source(w, h, seed=9, opaque=True), 3, 100)) as d:
        assert not d.has_alpha and d.alpha is None and d.alpha_row_bytes == 0 and d.alpha_premultiplied is False


def test_the_layout_guard_covers_the_alpha_fields(avif, monkeypatch):
    from oavif_amd import avif_bridge as ab
    assert (ab._IMG_ALPHAPLANE, ab._IMG_ALPHAROWBYTES, ab._IMG_OWNSALPHA, ab._IMG_ALPHAPREMULTIPLIED) == (64, 72, 76, 80)
    assert ab._check_layout(avif) is None
    # (a wrong alphaPlane offset that lands on an allocated YUV plane is caught by the older plane check, in its words)
    for name, wrong in (("_IMG_ALPHAROWBYTES", 76), ("_IMG_ALPHAPLANE", 72), ("_IMG_OWNSALPHA", 80), ("_IMG_ALPHAPREMULTIPLIED", 76)):
        with monkeypatch.context() as m:
            m.setattr(ab, name, wrong)
            why = ab._check_layout(avif)
            assert why is not None and "alpha" in why.lower(), (name, why)
    assert ab._check_layout(avif) is None


# ---- the seventh library ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yuva_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.yuva_lib()


def _plain(path):
    return {s for s in _exported(path) if not s.startswith(("_Z", "__hip", "_init", "_fini"))}


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.YUVA_FUNCTIONS) == NAMES and _lib.YUVA_SYMBOLS == tuple(NAMES)
    assert set(_declared_functions(HEADER)) == set(NAMES) and list(prototypes(HEADER)) == NAMES
    others = (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS) |
              set(_lib.MAP_FUNCTIONS) | set(_lib.CHROMA_FUNCTIONS))
    assert not set(NAMES) & others
    assert os.path.basename(_lib.YUVA_LIB_PATH) == "liboavif_hip_yuva.so"
    # the struct: ssimu2_yuv_frame, a pointer and two words
    fields = [(n, t) for n, t in _lib.YuvaFrameC._fields_]
    assert fields == [("yuv", _lib.YuvFrameC), ("alpha", ctypes.c_void_p), ("alpha_row_bytes", ctypes.c_uint32),
                      ("alpha_premultiplied", ctypes.c_uint32)]
    assert _lib.YuvaFrameC.alpha.offset == ctypes.sizeof(_lib.YuvFrameC) == 56 and ctypes.sizeof(_lib.YuvaFrameC) == 72
    with open(os.path.join(isa_text.ROOT, "include", HEADER)) as f:
        text = f.read()
    body = re.search(r"typedef struct ssimu2_yuva_frame \{(.*?)\} ssimu2_yuva_frame;", text, re.S).group(1)
    decls = [re.sub(r"\s+", " ", d).strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")]
    assert [d for d in decls if d] == ["ssimu2_yuv_frame yuv", "const void* alpha", "uint32_t alpha_row_bytes",
                                       "uint32_t alpha_premultiplied"]
    assert '#include "ssimu2_hip_chroma.h"' in text


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header_and_the_call_it_mirrors(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.YUVA_FUNCTIONS[name]
    ret, params = prototypes(HEADER)[name]
    norm = lambda ds: [re.sub(r"\s+", " ", d) for d in ds]
    # the binding table's checker knows the frame pointers of the earlier headers; here they are checked by hand
    frames = [i for i, d in enumerate(params) if re.match(r"const\s+ssimu2_yuva_frame\s*\*", d)]
    assert frames and all(argtypes[i] is ctypes.POINTER(_lib.YuvaFrameC) for i in frames)
    assert [i for i, t in enumerate(argtypes) if t is ctypes.POINTER(_lib.YuvaFrameC)] == frames
    plain = lambda ds: [d.replace("ssimu2_yuva_frame", "ssimu2_yuv_frame") for d in ds]
    swapped = [ctypes.POINTER(_lib.YuvFrameC) if t is ctypes.POINTER(_lib.YuvaFrameC) else t for t in argtypes]
    check(name, (ret, plain(params)), restype, swapped)
    old_ret, old_params = prototypes("ssimu2_hip_chroma.h")[MIRRORED[name]]
    mine = norm(plain(params))
    if name in WITH_BACKGROUND:
        at = mine.index("uint32_t background_rgb")
        assert mine[at - 1] == "uint32_t chroma_upsampling" and argtypes[at] is ctypes.c_uint32
        mine = mine[:at] + mine[at + 1:]
        swapped = swapped[:at] + swapped[at + 1:]
    else:
        assert "uint32_t background_rgb" not in mine
    assert ret == old_ret and mine == norm(old_params), name
    assert (restype, swapped) == _lib.CHROMA_FUNCTIONS[MIRRORED[name]]


def test_yuva_library_exports_the_chroma_library_plus_the_six_calls(yuva_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = (public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS) | set(_lib.CHROMA_SYMBOLS) |
            set(_lib.YUVA_SYMBOLS))
    plain, chroma_plain = _plain(_lib.YUVA_LIB_PATH), _plain(_lib.CHROMA_LIB_PATH)
    assert plain == want, plain ^ want
    assert plain - chroma_plain == set(NAMES) and chroma_plain <= plain
    for name in want:
        assert hasattr(yuva_lib, name), name
    assert yuva_lib.ssimu2_version() == _lib.lib().ssimu2_version()


def test_the_other_six_libraries_have_none_of_it(hip_lib):
    from oavif_amd import _lib
    for path in (_lib.LIB_PATH, _lib.INSTR_LIB_PATH, _lib.EXT_LIB_PATH, _lib.YUV_LIB_PATH, _lib.MAP_LIB_PATH, _lib.CHROMA_LIB_PATH):
        assert not set(_exported(path)) & set(NAMES), path


def test_the_unit_its_kernels_and_what_it_shares():
    from oavif_amd import build
    kernels = _kernels(UNIT)
    assert kernels and all(k.startswith("k_yuva_to_codes<") for k in kernels)
    shapes = {(s, sub, v, b) for s in (1, 2) for sub, v, b in [(0, "false", "false"), (2, "false", "false"),
              (1, "false", "false"), (1, "false", "true"), (1, "true", "false"), (1, "true", "true")]}
    got = {tuple(x.strip() for x in k[len("k_yuva_to_codes<"):-1].split(",")) for k in kernels}
    assert {(int(s), int(sub), v, b) for s, sub, v, b, _div in got} == shapes
    assert {(int(s), int(div)) for s, _sub, _v, _b, div in got} == {(1, 0), (1, 1), (1, 2), (2, 1), (2, 2)}
    asm = isa_text.unit_asm(UNIT)
    assert "c_k" not in asm
    for field in ("group_segment_fixed_size", "private_segment_fixed_size"):      # no LDS, no scratch
        values = re.findall(rf"^\s*\.amdhsa_{field}\s+(\d+)", asm, re.M)
        assert len(values) == len(kernels) and set(values) == {"0"}, (field, values)
    inc = _includes(os.path.join(build.CSRC, UNIT))
    assert "ssimu2_host.h" in inc and HEADER in inc and "ssimu2_yuv_pixel.h" in inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_ext.hip", "ssimu2_yuv.hip", "ssimu2_map.hip", "ssimu2_chroma.hip",
                      "ssimu2_kernels.h", "ssimu2_recursive.h"}
    # each contract expression keeps one definition: the colour and the blend come from the shared header
    texts = {}
    for unit in (UNIT, "ssimu2_chroma.hip", "ssimu2_yuv_pixel.h"):
        with open(os.path.join(build.CSRC, unit)) as f:
            texts[unit] = re.sub(r"//.*", "", f.read())
    for unit in (UNIT, "ssimu2_chroma.hip"):
        body = texts[unit]
        assert "yuv_unorm(" in body and "yuv_codes(" in body and "chroma_blend(" in body and "div_rn" not in body, unit
        assert "0.5625f" not in body and "samples_at<" in body and "void samples_at" not in body, unit
    assert texts["ssimu2_yuv_pixel.h"].count("0.5625f") == 1 and "void samples_at" in texts["ssimu2_yuv_pixel.h"]


def test_build_knows_the_seventh_library_in_a_fourth_table(hip_lib, monkeypatch, tmp_path):
    from oavif_amd import _lib, build
    assert os.path.samefile(os.path.dirname(build.YUVA_LIB_PATH), os.path.dirname(_lib.YUVA_LIB_PATH))
    assert os.path.basename(build.YUVA_LIB_PATH) == "liboavif_hip_yuva.so"
    assert not any(build.YUVA_LIB_PATH in t for t in (build.LIBRARIES, build.MAP_LIBRARIES, build.CHROMA_LIBRARIES))
    assert build.YUVA_LIBRARIES == {build.YUVA_LIB_PATH: build.YUVA_SOURCES}
    assert build.YUVA_SOURCES[:-1] == build.CHROMA_SOURCES and build.YUVA_SOURCES[-1] == UNIT
    assert build.yuva_units() == [UNIT]
    assert UNIT not in build.compile_units() + build.map_units() + build.chroma_units()
    assert os.path.exists(build.YUVA_LIB_PATH)                            # built by build.build()
    libs = (*build.LIBRARIES, *build.MAP_LIBRARIES, *build.CHROMA_LIBRARIES, *build.YUVA_LIBRARIES)
    assert len(libs) == len(set(libs)) == 7
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "YUVA_LIBRARIES", {str(tmp_path / "liboavif_hip_yuva.so"): build.YUVA_SOURCES})
    assert build.libs_need_build()


def test_null_context_is_an_invalid_argument(yuva_lib):
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    planes, alpha = yuva_ref.random_frame(8, 8, 8, chroma_ref.YUV_420, seed=1)
    c = YuvFrame(planes, 8, chroma_ref.YUV_420, alpha=alpha).as_yuva_c()
    out = np.empty((8, 8, 3), np.uint16)
    m = np.empty((8, 8), np.float32)
    score = ctypes.c_double()
    L, fr, sc = yuva_lib, ctypes.byref(c), ctypes.byref(score)
    outp, mp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert {L.ssimu2_composite_yuva(None, fr, 8, 8, 16, 0, 0, outp), L.ssimu2_score_yuva(None, fr, fr, 8, 8, 16, 0, 0, sc),
            L.ssimu2_set_reference_yuva(None, fr, 8, 8, 16, 0, 0), L.ssimu2_score_against_reference_yuva(None, fr, 16, 0, sc),
            L.ssimu2_error_map_yuva(None, fr, fr, 8, 8, 16, 0, 0, mp, sc),
            L.ssimu2_error_map_against_reference_yuva(None, fr, 16, 0, mp, sc)} == {_lib.ERR_INVALID_ARG}


# ---- YuvFrame and Ssimu2 ---------------------------------------------------------------------------------------------
def test_yuv_frame_takes_an_alpha_plane_of_plane_0s_shape_and_dtype():
    from oavif_amd.scorer import YuvFrame
    planes, alpha = yuva_ref.random_frame(9, 6, 10, chroma_ref.YUV_420, seed=2)
    f = YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=alpha)
    assert f.alpha is alpha and f.alpha_premultiplied == 0
    c = f.as_yuva_c()
    assert (c.alpha, c.alpha_row_bytes, c.alpha_premultiplied) == (alpha.ctypes.data, 18, 0)
    assert (c.yuv.depth, c.yuv.format, c.yuv.planes[0], c.yuv.row_bytes[1]) == (10, 3, planes[0].ctypes.data, 10)
    plain = YuvFrame(planes, 10, chroma_ref.YUV_420, alpha_premultiplied=True).as_yuva_c()
    assert (plain.alpha, plain.alpha_row_bytes, plain.alpha_premultiplied) == (None, 0, 1)
    # a strided view goes through as it is; one whose samples are not adjacent is copied
    buf, view = yuv_ref.laid_out(alpha, 2 * 9 + 6, 2, seed=1)
    g = YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=view)
    assert g.alpha.ctypes.data == view.ctypes.data and g.as_yuva_c().alpha_row_bytes == 24
    wide = np.zeros((6, 18), np.uint16)
    wide[:, ::2] = alpha
    gapped = YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=wide[:, ::2])
    assert gapped.alpha.flags.c_contiguous and np.array_equal(gapped.alpha, alpha)
    one_row = YuvFrame([p[:1] for p in yuv_ref.random_planes(9, 1, 8, seed=1)], 8, alpha=np.zeros((1, 9), np.uint8))
    assert one_row.as_yuva_c().alpha_row_bytes == 9
    with pytest.raises(TypeError):
        YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=alpha.astype(np.uint8))
    with pytest.raises(ValueError):
        YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=alpha[:3])              # the chroma planes' shape is not it either
    with pytest.raises(ValueError):
        YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=alpha[:, :5])
    with pytest.raises(ValueError):
        YuvFrame(planes, 10, chroma_ref.YUV_420, alpha=alpha.reshape(-1))
    assert YuvFrame(planes, 10, chroma_ref.YUV_420).alpha is None               # as before


def test_ssimu2_flags_that_need_no_device():
    import inspect
    from oavif_amd import Ssimu2
    assert "yuva" in inspect.signature(Ssimu2.__init__).parameters and Ssimu2.yuva is False
    with pytest.raises(ValueError, match="yuva=True"):
        Ssimu2(0, instrumented=True, yuva=True)
    for name in ("composite_yuva", "compute_ssimu2_yuva", "set_reference_yuva", "score_against_reference_yuva",
                 "error_map_yuva_alpha", "error_map_against_reference_yuva_alpha"):
        params = inspect.signature(getattr(Ssimu2, name)).parameters
        assert params["rgb_depth"].default == 16 and params["chroma_upsampling"].default == "bilinear", name
        assert ("background" in params) == (name not in ("score_against_reference_yuva",
                                                          "error_map_against_reference_yuva_alpha")), name


def test_contexts_of_the_other_libraries_name_the_flag():
    """The refusal comes before any C call: a context object that never reached a device shows it."""
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    from oavif_amd.scorer import YuvFrame
    planes, alpha = yuva_ref.random_frame(8, 8, 8, yuv_ref.YUV_444, seed=1)
    f = YuvFrame(planes, 8, alpha=alpha)
    s = Ssimu2.__new__(Ssimu2)
    s.chroma = True                      # even the chroma library's context
    for call in (lambda: s.composite_yuva(f, 0), lambda: s.compute_ssimu2_yuva(f, f, 0), lambda: s.set_reference_yuva(f, 0),
                 lambda: s.score_against_reference_yuva(f), lambda: s.error_map_yuva_alpha(f, f, 0),
                 lambda: s.error_map_against_reference_yuva_alpha(f)):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "yuva=True" in str(ei.value)
    s._ctx = None                        # nothing to close


def test_yuva_methods_check_their_arguments_before_the_call():
    from oavif_amd import Ssimu2
    from oavif_amd.scorer import YuvFrame
    planes, alpha = yuva_ref.random_frame(8, 8, 8, yuv_ref.YUV_444, seed=1)
    f = YuvFrame(planes, 8, alpha=alpha)
    other = YuvFrame(yuv_ref.random_planes(10, 8, 8, seed=1), 8)
    s = Ssimu2.__new__(Ssimu2)
    s.yuva, s._ref_shape = True, (8, 10, 3)
    with pytest.raises(TypeError):
        s.composite_yuva(planes, 0)
    with pytest.raises(ValueError, match="chroma_upsampling"):
        s.composite_yuva(f, 0, 16, "bicubic")
    with pytest.raises(ValueError, match="background"):
        s.composite_yuva(f, 0x1000000)
    with pytest.raises(ValueError, match="same shape"):
        s.compute_ssimu2_yuva(f, other, 0)
    with pytest.raises(ValueError, match="same shape"):
        s.error_map_yuva_alpha(f, other, 0)
    with pytest.raises(ValueError, match="reference"):
        s.score_against_reference_yuva(f)
    with pytest.raises(ValueError, match="reference"):
        s.error_map_against_reference_yuva_alpha(f)
    s._ctx = None


def test_alpha_command_line_takes_the_new_options():
    from oavif_amd import alpha
    a = alpha.parse_args(["r.png", "d.avif"])
    assert (a.rgb_depth, a.chroma_upsampling, a.blur) == (8, "bilinear", "fir") and alpha.is_avif(a.dist) and not alpha.is_avif(a.ref)
    a = alpha.parse_args(["r.AVIF", "d.avif", "--rgb-depth", "12", "--chroma-upsampling", "nearest", "--background", "102030"])
    assert (a.rgb_depth, a.chroma_upsampling, a.background) == (12, "nearest", [0x102030]) and alpha.is_avif(a.ref)
    with pytest.raises(SystemExit):
        alpha.parse_args(["r.png", "d.avif", "--chroma-upsampling", "bicubic"])
    import inspect
    p = inspect.signature(alpha.search_rgba).parameters
    assert (p["score_yuv"].default, p["rgb_depth"].default, p["chroma_upsampling"].default) == (False, 8, "bilinear")
