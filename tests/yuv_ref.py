"""numpy restatement of the YUV -> RGB codes definition of include/ssimu2_hip_yuv.h: fp32 arrays,
np.float32 constants, the operations in the order the header writes them, each rounded once (numpy never contracts).
Held against libavif's built-in converter in tests/test_yuv_ref.py and against k_yuv_to_codes in
tests/test_gpu_yuv.py, bit for bit both times.  Also: the content those two modules share."""
from __future__ import annotations

import numpy as np

F = np.float32
YUV_444, YUV_400 = 1, 4
MATRICES = {1: (0.2126, 0.0722), 2: (0.299, 0.114), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}


def constants(depth: int, full_range, mc: int) -> dict:
    """The per-call constants, each formed by fp32 operations as the header writes them."""
    kr, kb = (F(v) for v in MATRICES[mc])
    one = F(1.0)
    m, scale = (1 << depth) - 1, 1 << (depth - 8)
    return {"kr": kr, "kb": kb, "kg": (one - kr) - kb,
            "bias_y": F(0.0) if full_range else F(16 * scale), "range_y": F(m) if full_range else F(219 * scale),
            "bias_uv": F(1 << (depth - 1)), "range_uv": F(m) if full_range else F(224 * scale),
            "r_cr": F(2.0) * (one - kr), "b_cb": F(2.0) * (one - kb), "g_cr": kr * (one - kr), "g_cb": kb * (one - kb),
            "max_code": m}


def codes(y, u, v, depth: int, full_range, mc: int, rgb_depth: int, fmt: int = YUV_444) -> np.ndarray:
    """(h, w, 3) uint16 RGB codes of depth `rgb_depth` of the planes y, u, v ((h, w) unsigned; u and v are not looked at
    for fmt YUV_400)."""
    k = constants(depth, full_range, mc)
    y = np.minimum(np.asarray(y).astype(np.uint32), k["max_code"])
    Y = (y.astype(F) - k["bias_y"]) / k["range_y"]
    if fmt == YUV_400:
        Cb = Cr = np.zeros_like(Y)
    else:
        u = np.minimum(np.asarray(u).astype(np.uint32), k["max_code"])
        v = np.minimum(np.asarray(v).astype(np.uint32), k["max_code"])
        Cb = (u.astype(F) - k["bias_uv"]) / k["range_uv"]
        Cr = (v.astype(F) - k["bias_uv"]) / k["range_uv"]
    R = Y + k["r_cr"] * Cr
    B = Y + k["b_cb"] * Cb
    G = Y - (F(2.0) * (k["g_cr"] * Cr + k["g_cb"] * Cb)) / k["kg"]
    top = F((1 << rgb_depth) - 1)
    out = np.empty(Y.shape + (3,), np.uint16)
    for c, plane in enumerate((R, G, B)):
        assert plane.dtype == F
        out[..., c] = (F(0.5) + np.clip(plane, F(0.0), F(1.0)) * top).astype(np.uint32)   # truncation
    return out


def forward(rgb8, depth: int, full_range, mc: int):
    """(y, u, v) planes of depth `depth` of an (h, w, 3) uint8 RGB frame: the colour matrix in fp64, rounded to the
    nearest code and clipped -- test content (what a pseudo-codec's frames are handed over as), not a definition."""
    kr, kb = MATRICES[mc]
    kg = 1.0 - kr - kb
    c = np.asarray(rgb8, np.float64) / 255.0
    Y = kr * c[..., 0] + kg * c[..., 1] + kb * c[..., 2]
    Cb = (c[..., 2] - Y) / (2.0 * (1.0 - kb))
    Cr = (c[..., 0] - Y) / (2.0 * (1.0 - kr))
    m, scale = (1 << depth) - 1, 1 << (depth - 8)
    if full_range:
        by, ry, ruv = 0.0, float(m), float(m)
    else:
        by, ry, ruv = 16.0 * scale, 219.0 * scale, 224.0 * scale
    dtype = np.uint8 if depth == 8 else np.uint16
    q = lambda a, bias, rng: np.clip(np.floor(a * rng + bias + 0.5), 0, m).astype(dtype)
    return q(Y, by, ry), q(Cb, float(1 << (depth - 1)), ruv), q(Cr, float(1 << (depth - 1)), ruv)


def special_codes(depth: int):
    """0, 1, 2, mid-range, the limited-range ends of luma and chroma, and m."""
    m, scale = (1 << depth) - 1, 1 << (depth - 8)
    return [0, 1, 2, 1 << (depth - 1), 16 * scale, 235 * scale, 240 * scale, m - 1, m]


def random_planes(w: int, h: int, depth: int, seed: int, extremes: bool = False):
    """Three (h, w) planes of random codes 0..m that include special_codes (when they fit); `extremes`: made of the
    special codes only, so that most pixels of a limited-range frame lie outside the nominal range."""
    rng = np.random.default_rng(seed)
    m = (1 << depth) - 1
    dtype = np.uint8 if depth == 8 else np.uint16
    sp = np.array(special_codes(depth))
    out = []
    for _ in range(3):
        p = sp[rng.integers(0, len(sp), (h, w))] if extremes else rng.integers(0, m + 1, (h, w))
        flat = p.reshape(-1)
        n = min(len(sp), flat.size)
        flat[rng.permutation(flat.size)[:n]] = sp[:n]
        out.append(flat.reshape(h, w).astype(dtype))
    return out


def laid_out(plane, row_bytes: int, offset: int, seed: int):
    """`plane` in rows `row_bytes` apart starting `offset` bytes into a noise-filled buffer -> (buffer, (h, w) view).
    The last row is followed by nothing but the buffer's own tail of 8 noise bytes."""
    h, w = plane.shape
    size = plane.itemsize
    assert row_bytes >= w * size and row_bytes % size == 0 and offset % size == 0
    buf = np.random.default_rng(seed).integers(0, 256, offset + row_bytes * h + 8, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:offset + row_bytes * h].view(plane.dtype), (h, w), (row_bytes, size))
    view[...] = plane
    return buf, view
