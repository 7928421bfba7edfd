"""The numpy restatement of the subsampled-chroma definition (tests/chroma_ref.py, include/ssimu2_hip_chroma.h, DESIGN.md
section 16) without a GPU: against the bundled libavif's built-in converter (avifRGBImage.avoidLibYUV = 1) bit for bit
over format x depth x range x matrix x RGB depth x every chromaUpsampling value, at sizes down to 1 x 1; against
decode_common(..., rgb_depth=16) on 4:2:0 and 4:2:2 files Pillow wrote; and the identities with the 4:4:4 restatement."""
import ctypes
import io
import struct

import numpy as np
import pytest

import chroma_ref
import yuv_ref
from oavif_amd import avif_bridge as ab

SIZES = [(97, 53), (96, 52)] + chroma_ref.SMALL_SIZES
FORMATS = [chroma_ref.YUV_422, chroma_ref.YUV_420]
# avifChromaUpsampling: AUTOMATIC 0, FASTEST 1, BEST_QUALITY 2, NEAREST 3, BILINEAR 4
UPSAMPLING = {0: chroma_ref.BILINEAR, 1: chroma_ref.NEAREST, 2: chroma_ref.BILINEAR, 3: chroma_ref.NEAREST,
              4: chroma_ref.BILINEAR}
_RGB_CHROMA_UPSAMPLING, _RGB_AVOID_LIBYUV = 16, 24   # offsets in avifRGBImage


@pytest.fixture(scope="module")
def avif():
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    return ab._lib()


def libavif_codes(L, planes, depth, full_range, mc, rgb_depth, fmt, upsampling):
    """avifImageYUVToRGB with avoidLibYUV = 1 and chromaUpsampling = `upsampling` on an image built of `planes` (each
    of its own size) -> (h, w, 3) uint16 codes."""
    h, w = planes[0].shape
    im = L.avifImageCreate(w, h, depth, fmt)
    assert im
    try:
        ctypes.c_uint32.from_address(im + ab._IMG_YUVRANGE).value = 1 if full_range else 0
        ctypes.c_uint16.from_address(im + ab._IMG_MC).value = mc
        assert L.avifImageAllocatePlanes(im, ab._PLANES_YUV) == 0
        size = planes[0].itemsize
        for k in range(3):
            ph, pw = planes[k].shape
            ptr, row = ab._ptr(im, ab._IMG_YUVPLANES + 8 * k), ab._u32(im, ab._IMG_YUVROWBYTES + 4 * k)
            assert ptr and row >= pw * size
            dst = np.ctypeslib.as_array((ctypes.c_uint8 * (row * ph)).from_address(ptr)).reshape(ph, row)
            dst[:, :pw * size] = np.ascontiguousarray(planes[k]).view(np.uint8).reshape(ph, pw * size)
        rgb = ctypes.create_string_buffer(ab._RGB_SIZE)
        L.avifRGBImageSetDefaults(rgb, im)
        struct.pack_into("<I", rgb, ab._RGB_DEPTH, rgb_depth)
        struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGB)
        struct.pack_into("<I", rgb, _RGB_CHROMA_UPSAMPLING, upsampling)
        struct.pack_into("<i", rgb, _RGB_AVOID_LIBYUV, 1)
        assert L.avifRGBImageAllocatePixels(rgb) == 0
        try:
            assert L.avifImageYUVToRGB(im, rgb) == 0
            pix, row = struct.unpack_from("<QI", rgb.raw, ab._RGB_PIXELS)
            if rgb_depth == 8:
                a = np.ctypeslib.as_array((ctypes.c_uint8 * (row * h)).from_address(pix)).reshape(h, row)
            else:
                a = np.ctypeslib.as_array((ctypes.c_uint16 * (row // 2 * h)).from_address(pix)).reshape(h, row // 2)
            return a[:, :w * 3].reshape(h, w, 3).astype(np.uint16)
        finally:
            L.avifRGBImageFreePixels(rgb)
    finally:
        L.avifImageDestroy(im)


@pytest.mark.parametrize("fmt", FORMATS, ids=["422", "420"])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_the_restatement_is_libavifs_built_in_converter(avif, depth, fmt):
    k = 0
    for w, h in SIZES:
        for full_range in (True, False):
            for mc in (1, 2, 6, 9):
                # one plane set in four is made of the special codes only
                planes = chroma_ref.random_planes(w, h, depth, fmt, seed=100 * depth + k, extremes=(k % 4 == 3))
                if w >= 96:
                    for sp in yuv_ref.special_codes(depth):
                        assert all((p == sp).any() for p in planes)
                for rgb_depth in sorted({8, depth, 16}):
                    got = {u: chroma_ref.codes(*planes, depth, full_range, mc, rgb_depth, fmt, u)
                           for u in (chroma_ref.BILINEAR, chroma_ref.NEAREST)}
                    for value, name in UPSAMPLING.items():
                        exp = libavif_codes(avif, planes, depth, full_range, mc, rgb_depth, fmt, value)
                        bad = got[name] != exp
                        assert not bad.any(), (w, h, depth, full_range, mc, rgb_depth, value, int(bad.sum()),
                                               np.argwhere(bad)[:4].tolist())
                k += 1


def test_the_two_upsamplings_differ_where_chroma_varies():
    """So that the comparison above tells them apart."""
    planes = chroma_ref.random_planes(97, 53, 8, chroma_ref.YUV_420, seed=1)
    a = chroma_ref.codes(*planes, 8, True, 6, 16, chroma_ref.YUV_420, chroma_ref.BILINEAR)
    b = chroma_ref.codes(*planes, 8, True, 6, 16, chroma_ref.YUV_420, chroma_ref.NEAREST)
    assert (a != b).mean() > 0.5


# ---- real files ---------------------------------------------------------------------------------------------------
def _pillow_avif(w, h, subsampling):
    from PIL import Image
    from oavif_amd import synth
    buf = io.BytesIO()
    Image.fromarray(synth.make_ref(w, h, seed=3)).save(buf, format="AVIF", subsampling=subsampling, quality=70, speed=10)
    return buf.getvalue()


@pytest.mark.parametrize("subsampling,fmt", [("4:2:0", chroma_ref.YUV_420), ("4:2:2", chroma_ref.YUV_422)])
@pytest.mark.parametrize("size", [(67, 41), (64, 40), (33, 17)])
def test_decode_yuv_planes_through_the_restatement_are_decode_commons_samples(avif, size, subsampling, fmt):
    w, h = size
    data = _pillow_avif(w, h, subsampling)
    with ab.decode_yuv(data) as f:
        assert (f.width, f.height, f.format) == (w, h, fmt) and not f.has_alpha and len(f.planes) == 3
        ch, cw = chroma_ref.chroma_shape(w, h, fmt)
        assert f.planes[0].shape == (h, w) and f.planes[1].shape == f.planes[2].shape == (ch, cw)
        got = chroma_ref.codes(*f.planes, f.depth, f.full_range, f.matrix_coefficients, 16, fmt, chroma_ref.BILINEAR)
    with ab.decode_common(data, rgb_depth=16) as g:    # at an RGB depth other than 8 libavif uses its built-in converter
        exp = g.tight_rgb16()
    assert np.array_equal(got, exp), int((got != exp).sum())


# ---- identities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=["422", "420"])
def test_constant_chroma_gives_the_444_codes_under_both_upsamplings(fmt):
    """Nearest repeats the sample, so any constant goes through.  Bilinear blends the normalised value x of the constant
    as ((x * 0.5625f + x * 0.1875f) + x * 0.1875f) + x * 0.0625f, every product rounded: that is x exactly when x * 9/16,
    x * 3/16 and x / 16 are fp32 numbers, i.e. when x has at most 20 significant bits -- the limited-range constants
    bias + n * 7 * 2^(depth-8) (x = n / 32) below, and the mid-range code of either range (x = 0).  For other constants
    the definition, which is libavif's, does not give the 4:4:4 codes: limited-range 10-bit (U, V) = (3, 77), x =
    -509 / 896 and -435 / 896, differs from them in 0.07 % of the depth-16 codes of a 96 x 52 frame (11 of 14,976), by one code each."""
    for depth, (w, h) in zip((8, 10, 12), [(97, 53), (96, 52), (3, 3)]):
        y = yuv_ref.random_planes(w, h, depth, seed=depth)[0]
        m, mid, step = (1 << depth) - 1, 1 << (depth - 1), 7 << (depth - 8)
        exact = [(mid, mid), (mid + 16 * step, mid - 16 * step), (mid - 5 * step, mid + 13 * step), (mid + step, mid - 3 * step)]
        for u, v in exact + [(0, m), (3, 77)]:
            ch, cw = chroma_ref.chroma_shape(w, h, fmt)
            sub = [y, np.full((ch, cw), u, y.dtype), np.full((ch, cw), v, y.dtype)]
            exp = yuv_ref.codes(y, np.full_like(y, u), np.full_like(y, v), depth, False, 1, 16)
            assert np.array_equal(chroma_ref.codes(*sub, depth, False, 1, 16, fmt, chroma_ref.NEAREST), exp), (depth, u, v)
            if (u, v) in exact:
                assert np.array_equal(chroma_ref.codes(*sub, depth, False, 1, 16, fmt, chroma_ref.BILINEAR), exp), (depth, u, v)
        sub = [y, np.full((ch, cw), mid, y.dtype), np.full((ch, cw), mid, y.dtype)]       # full range: x = 0
        assert np.array_equal(chroma_ref.codes(*sub, depth, True, 9, 16, fmt, chroma_ref.BILINEAR),
                              yuv_ref.codes(y, np.full_like(y, mid), np.full_like(y, mid), depth, True, 9, 16))


@pytest.mark.parametrize("fmt", FORMATS, ids=["422", "420"])
def test_nearest_is_the_444_restatement_on_repeated_chroma(fmt):
    for depth, (w, h) in zip((8, 10, 12), [(97, 53), (96, 52), (5, 4)]):
        y, u, v = chroma_ref.random_planes(w, h, depth, fmt, seed=7 * depth)
        rows = 2 if fmt == chroma_ref.YUV_420 else 1
        full = [np.repeat(np.repeat(p, rows, 0), 2, 1)[:h, :w] for p in (u, v)]
        for full_range in (True, False):
            assert np.array_equal(chroma_ref.codes(y, u, v, depth, full_range, 9, 16, fmt, chroma_ref.NEAREST),
                                  yuv_ref.codes(y, *full, depth, full_range, 9, 16))
