"""numpy restatement of the subsampled-chroma definition of include/ssimu2_hip_chroma.h, on top
of tests/yuv_ref.py: the chroma samples normalised in fp32, blended (bilinear) or repeated (nearest) in the header's
order with every product and sum rounded once (numpy never contracts), then yuv_ref's colour matrix.  Held against
libavif's built-in converter in tests/test_chroma_ref.py and against k_yuv_chroma_to_codes in tests/test_gpu_chroma.py,
bit for bit both times.  Also: the content those two modules share."""
from __future__ import annotations

import numpy as np

import yuv_ref

F = np.float32
YUV_422, YUV_420 = 2, 3
BILINEAR, NEAREST = "bilinear", "nearest"
SMALL_SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 3)]


def chroma_shape(w: int, h: int, fmt: int):
    """(ch, cw) of a w x h frame's planes 1 and 2."""
    return ((h + 1) // 2 if fmt == YUV_420 else h), (w + 1) // 2


def upsampled(p, w: int, h: int, fmt: int, upsampling: str) -> np.ndarray:
    """C(i, j) of the header for one plane `p` of normalised fp32 chroma, (ch, cw) -> (h, w)."""
    assert p.dtype == F and p.shape == chroma_shape(w, h, fmt)
    i, j = np.arange(w), np.arange(h)
    ui, uj = i >> 1, j >> (1 if fmt == YUV_420 else 0)
    if upsampling == NEAREST:
        return p[uj[:, None], ui[None, :]]
    assert upsampling == BILINEAR
    ac = np.where((i == 0) | ((i == w - 1) & (i & 1 == 1)), 0, np.where(i & 1 == 1, 1, -1))
    ar = np.where((j == 0) | ((j == h - 1) & (j & 1 == 1)), 0, np.where(j & 1 == 1, 1, -1))
    if fmt == YUV_422:
        ar = np.zeros_like(j)
    a = p[uj[:, None], ui[None, :]]
    b = p[uj[:, None], (ui + ac)[None, :]]
    c = p[(uj + ar)[:, None], ui[None, :]]
    d = p[(uj + ar)[:, None], (ui + ac)[None, :]]
    out = ((a * F(0.5625) + b * F(0.1875)) + c * F(0.1875)) + d * F(0.0625)
    assert out.dtype == F
    return out


def codes(y, u, v, depth: int, full_range, mc: int, rgb_depth: int, fmt: int, upsampling: str = BILINEAR) -> np.ndarray:
    """(h, w, 3) uint16 RGB codes of depth `rgb_depth` of the planes y (h, w) and u, v (chroma_shape) of a 4:2:2 or 4:2:0
    frame; a 4:4:4 or 4:0:0 frame goes to yuv_ref.codes."""
    if fmt not in (YUV_422, YUV_420):
        return yuv_ref.codes(y, u, v, depth, full_range, mc, rgb_depth, fmt)
    k = yuv_ref.constants(depth, full_range, mc)
    h, w = np.asarray(y).shape

    def unorm(p, bias, rng):
        return (np.minimum(np.asarray(p).astype(np.uint32), k["max_code"]).astype(F) - bias) / rng

    Y = unorm(y, k["bias_y"], k["range_y"])
    Cb = upsampled(unorm(u, k["bias_uv"], k["range_uv"]), w, h, fmt, upsampling)
    Cr = upsampled(unorm(v, k["bias_uv"], k["range_uv"]), w, h, fmt, upsampling)
    R = Y + k["r_cr"] * Cr
    B = Y + k["b_cb"] * Cb
    G = Y - (F(2.0) * (k["g_cr"] * Cr + k["g_cb"] * Cb)) / k["kg"]
    top = F((1 << rgb_depth) - 1)
    out = np.empty((h, w, 3), np.uint16)
    for c, plane in enumerate((R, G, B)):
        assert plane.dtype == F
        out[..., c] = (F(0.5) + np.clip(plane, F(0.0), F(1.0)) * top).astype(np.uint32)   # truncation
    return out


def random_planes(w: int, h: int, depth: int, fmt: int, seed: int, extremes: bool = False):
    """yuv_ref.random_planes for a subsampled frame: Y of (h, w), U and V of chroma_shape, each with the special codes
    (when they fit)."""
    ch, cw = chroma_shape(w, h, fmt)
    y = yuv_ref.random_planes(w, h, depth, seed, extremes)[0]
    _, u, v = yuv_ref.random_planes(cw, ch, depth, seed + 1, extremes)
    return [y, u, v]


def subsample(planes, fmt: int):
    """Full-size (y, u, v) -> the frame of format `fmt` whose chroma is every second column (and row) of them: test
    content, not a definition."""
    y, u, v = planes
    step = 2 if fmt == YUV_420 else 1
    return [y, np.ascontiguousarray(u[::step, ::2]), np.ascontiguousarray(v[::step, ::2])]
