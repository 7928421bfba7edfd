"""The numpy restatement of the YUV definition (tests/yuv_ref.py, include/ssimu2_hip_yuv.h) without
a GPU: against the bundled libavif's built-in converter (avifRGBImage.avoidLibYUV = 1) bit for bit over depth x range x
matrix x RGB depth, 4:4:4 and 4:0:0; the grey identity; monotonicity in Y; and the bridge's decode_yuv, whose planes
through the restatement are decode_common(..., rgb_depth=16)'s samples bit for bit."""
import ctypes
import struct

import numpy as np
import pytest

import yuv_ref
from oavif_amd import avif_bridge as ab

W, H = 97, 53


@pytest.fixture(scope="module")
def avif():
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    return ab._lib()


def libavif_codes(L, planes, depth, full_range, mc, rgb_depth, fmt):
    """avifImageYUVToRGB with avoidLibYUV = 1 on an image built of `planes` -> (h, w, 3) uint16 codes."""
    h, w = planes[0].shape
    im = L.avifImageCreate(w, h, depth, fmt)
    assert im
    try:
        ctypes.c_uint32.from_address(im + ab._IMG_YUVRANGE).value = 1 if full_range else 0
        ctypes.c_uint16.from_address(im + ab._IMG_MC).value = mc
        assert L.avifImageAllocatePlanes(im, ab._PLANES_YUV) == 0
        size = planes[0].itemsize
        for k in range(1 if fmt == yuv_ref.YUV_400 else 3):
            ptr, row = ab._ptr(im, ab._IMG_YUVPLANES + 8 * k), ab._u32(im, ab._IMG_YUVROWBYTES + 4 * k)
            assert ptr and row >= w * size
            dst = np.ctypeslib.as_array((ctypes.c_uint8 * (row * h)).from_address(ptr)).reshape(h, row)
            dst[:, :w * size] = planes[k].view(np.uint8).reshape(h, w * size)
        rgb = ctypes.create_string_buffer(ab._RGB_SIZE)
        L.avifRGBImageSetDefaults(rgb, im)
        struct.pack_into("<I", rgb, ab._RGB_DEPTH, rgb_depth)
        struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGB)
        struct.pack_into("<i", rgb, 24, 1)                                   # avoidLibYUV
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


@pytest.mark.parametrize("fmt", [yuv_ref.YUV_444, yuv_ref.YUV_400], ids=["444", "400"])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_the_restatement_is_libavifs_built_in_converter(avif, depth, fmt):
    k = 0
    for full_range in (True, False):
        for mc in (1, 2, 6, 9):
            planes = yuv_ref.random_planes(W, H, depth, seed=100 * depth + k, extremes=(k % 4 == 3))
            for sp in yuv_ref.special_codes(depth):
                assert all((p == sp).any() for p in planes)
            for rgb_depth in sorted({8, depth, 16}):
                exp = libavif_codes(avif, planes, depth, full_range, mc, rgb_depth, fmt)
                got = yuv_ref.codes(*planes, depth, full_range, mc, rgb_depth, fmt)
                bad = got != exp
                assert not bad.any(), (depth, full_range, mc, rgb_depth, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            k += 1


def test_unspecified_and_bt470bg_are_bt601():
    planes = yuv_ref.random_planes(W, H, 8, seed=5)
    ref = yuv_ref.codes(*planes, 8, False, 6, 16)
    for mc in (2, 5):
        assert np.array_equal(yuv_ref.codes(*planes, 8, False, mc, 16), ref)
    assert not np.array_equal(yuv_ref.codes(*planes, 8, False, 1, 16), ref)


def test_grey_identity():
    """Full range, 8-bit, U = V = 128: the codes are Y at rgb_depth 8 and 257 Y at rgb_depth 16, for every Y and matrix."""
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    uv = np.full_like(y, 128)
    for mc in yuv_ref.MATRICES:
        for fmt in (yuv_ref.YUV_444, yuv_ref.YUV_400):
            assert np.array_equal(yuv_ref.codes(y, uv, uv, 8, True, mc, 8, fmt), np.repeat(y[..., None], 3, -1))
            assert np.array_equal(yuv_ref.codes(y, uv, uv, 8, True, mc, 16, fmt), np.repeat(y[..., None], 3, -1).astype(np.uint16) * 257)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_do_not_decrease_in_y_at_fixed_chroma(depth):
    m = (1 << depth) - 1
    dtype = np.uint8 if depth == 8 else np.uint16
    y = np.arange(m + 1, dtype=dtype)[None, :]
    rng = np.random.default_rng(depth)
    chroma = [(1 << (depth - 1), 1 << (depth - 1)), (0, m), (m, 0)] + [tuple(rng.integers(0, m + 1, 2)) for _ in range(5)]
    for full_range in (True, False):
        for mc in (1, 6, 9):
            for u, v in chroma:
                for rgb_depth in (8, 16):
                    c = yuv_ref.codes(y, np.full_like(y, u), np.full_like(y, v), depth, full_range, mc, rgb_depth).astype(np.int64)
                    assert (np.diff(c[0], axis=0) >= 0).all(), (depth, full_range, mc, u, v, rgb_depth)


def test_samples_above_the_depth_are_read_as_its_top_code():
    planes = yuv_ref.random_planes(9, 5, 10, seed=1)
    over = [p | np.uint16(0xFC00) for p in planes]
    top = [np.full_like(p, 1023) for p in planes]
    assert np.array_equal(yuv_ref.codes(*over, 10, True, 1, 16), yuv_ref.codes(*top, 10, True, 1, 16))


# ---- decode_yuv ---------------------------------------------------------------------------------------------------
def _encoded(w, h, mc, alpha=False):
    from oavif_amd import cli, synth
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.matrix_coefficients, o.quality_alpha = False, 10, mc, 90
    src = synth.make_ref(w, h, seed=3)
    if alpha:
        src = np.concatenate([src, np.full((h, w, 1), 200, np.uint8)], -1)
    return ab.encode(np.ascontiguousarray(src), 8, o, 70)


@pytest.mark.parametrize("mc", [2, 1, 9])
def test_decode_yuv_hands_out_the_planes_decode_common_converts(avif, mc):
    w, h = 67, 41
    data = _encoded(w, h, mc)
    with ab.decode_yuv(data) as f:
        assert (f.width, f.height, f.depth, f.format, f.matrix_coefficients) == (w, h, 8, yuv_ref.YUV_444, mc)
        assert f.full_range and not f.has_alpha and len(f.planes) == 3
        for p, row in zip(f.planes, f.row_bytes):
            assert p.shape == (h, w) and p.dtype == np.uint8 and p.strides == (row, 1) and row >= w
        got = yuv_ref.codes(*f.planes, f.depth, f.full_range, f.matrix_coefficients, 16)
    assert f.planes is None
    f.close()                                          # closing twice is harmless
    with ab.decode_common(data, rgb_depth=16) as g:    # at an RGB depth other than 8 libavif uses its built-in converter
        exp = g.tight_rgb16()
    assert np.array_equal(got, exp), int((got != exp).sum())


def test_decode_yuv_reports_an_alpha_plane(avif):
    with ab.decode_yuv(_encoded(32, 24, 2, alpha=True)) as f:
        assert f.has_alpha and len(f.planes) == 3
    with pytest.raises(ab.AvifBridgeError):
        ab.decode_yuv(b"not an avif")
