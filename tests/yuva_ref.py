"""numpy restatement of the composite definition of include/ssimu2_hip_yuva.h, on top of
tests/yuv_ref.py and tests/chroma_ref.py: their colour codes at rgb_depth, then the header's three integer lines in
uint64, with numpy's own floor division.  Held against libavif's RGBA output (where the header says they agree) in
tests/test_yuva_ref.py and against k_yuva_to_codes in tests/test_gpu_yuva.py, bit for bit both times.  Also: the content
those two modules share."""
from __future__ import annotations

import numpy as np

import chroma_ref
import yuv_ref

TOP = 65025                      # the largest composite code, 255 * 255
DEPTH_PAIRS = [(8, 16), (10, 10), (12, 16), (10, 8), (12, 12), (8, 10)]      # (depth, rgb_depth) beyond (8, 8)
FORMATS = {"444": yuv_ref.YUV_444, "422": chroma_ref.YUV_422, "420": chroma_ref.YUV_420, "400": yuv_ref.YUV_400}


def background(bg: int) -> np.ndarray:
    return np.array([(bg >> 16) & 255, (bg >> 8) & 255, bg & 255], np.uint64)


def composite(c, a, depth: int, rgb_depth: int, b) -> np.ndarray:
    """n of the header for colour codes `c` (0..mc), alpha samples `a` (any unsigned; above ma read as ma) and 8-bit
    background samples `b`, broadcast against each other -> uint32."""
    ma, mc = np.uint64((1 << depth) - 1), np.uint64((1 << rgb_depth) - 1)
    a = np.minimum(np.asarray(a).astype(np.uint64), ma)
    c, b = np.asarray(c).astype(np.uint64), np.asarray(b).astype(np.uint64)
    assert c.max(initial=0) <= mc and b.max(initial=0) <= 255
    den = ma * mc
    assert int(den) % 2 == 1 and int(den) < 1 << 28
    num = a * c * np.uint64(255) + (ma - a) * b * mc
    assert num.max(initial=0) <= np.uint64(255) * den
    n = (np.uint64(255) * num + (den - np.uint64(1)) // np.uint64(2)) // den
    assert n.max(initial=0) <= TOP
    return n.astype(np.uint32)


def colour_codes(planes, depth: int, full_range, mc: int, rgb_depth: int, fmt: int, upsampling: str = chroma_ref.BILINEAR):
    """The (h, w, 3) colour codes c of a frame of any of the four formats (`planes`: (y,) for 4:0:0, else (y, u, v))."""
    y = planes[0]
    u, v = (planes[1], planes[2]) if fmt != yuv_ref.YUV_400 else (None, None)
    return chroma_ref.codes(y, u, v, depth, full_range, mc, rgb_depth, fmt, upsampling)


def codes(planes, alpha, depth: int, full_range, mc: int, rgb_depth: int, fmt: int, bg: int,
          upsampling: str = chroma_ref.BILINEAR) -> np.ndarray:
    """(h, w, 3) uint16 composite codes of the frame over the background 0xRRGGBB; `alpha` None = opaque."""
    c = colour_codes(planes, depth, full_range, mc, rgb_depth, fmt, upsampling)
    a = np.full(c.shape[:2], (1 << depth) - 1, np.uint32) if alpha is None else np.asarray(alpha)
    assert a.shape == c.shape[:2]
    return np.ascontiguousarray(composite(c, a[..., None], depth, rgb_depth, background(bg)[None, None, :]).astype(np.uint16))


def rgba8(planes, alpha, full_range, mc: int, fmt: int, upsampling: str = chroma_ref.BILINEAR) -> np.ndarray:
    """The RGBA8 frame an 8-bit frame is compared with: its codes at rgb_depth 8 plus its alpha plane (None: 255)."""
    c = colour_codes(planes, 8, full_range, mc, 8, fmt, upsampling)
    out = np.empty(c.shape[:2] + (4,), np.uint8)
    out[..., :3] = c
    out[..., 3] = 255 if alpha is None else alpha
    return out


def random_frame(w: int, h: int, depth: int, fmt: int, seed: int, extremes: bool = False, over: bool = False):
    """-> (planes, alpha): chroma_ref / yuv_ref's random planes of the format plus an alpha plane of every kind of value
    (0, 1, ma - 1, ma and random ones; `over`: some above ma, which only 16-bit samples can hold)."""
    if fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420):
        planes = chroma_ref.random_planes(w, h, depth, fmt, seed, extremes)
    else:
        planes = yuv_ref.random_planes(w, h, depth, seed, extremes)[:1 if fmt == yuv_ref.YUV_400 else 3]
    rng = np.random.default_rng(seed + 1000)
    ma = (1 << depth) - 1
    a = rng.integers(0, ma + 1, (h, w))
    special = np.array([0, 1, ma // 2, ma - 1, ma])
    pick = rng.random((h, w)) < (0.8 if extremes else 0.3)
    a[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    if over:
        assert depth > 8
        hi = rng.random((h, w)) < 0.2
        a[hi] = rng.integers(ma + 1, 1 << 16, int(hi.sum()))
    return planes, a.astype(np.uint8 if depth == 8 else np.uint16)
