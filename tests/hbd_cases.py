"""16-bit content and layouts shared by the GPU modules and tests/ctx_walk.py (8-bit ones: tests/gpu_cases.py).  Importing
this module needs no GPU.  Each generator here makes different content on purpose; what they share is `to_depth`."""
from __future__ import annotations

import numpy as np

import gpu_cases
from oavif_amd import synth


def lift(u8):
    """8-bit samples u as the 16-bit samples 257 u (the same normalised values), one allocation."""
    return np.multiply(u8, np.uint16(257), dtype=np.uint16)


def to_depth(u8, depth, rng):
    """8-bit content taken to `depth` bits with low-order noise from `rng` (a generator or a seed), so that codes that
    are no multiple of 257 / 2^(16 - depth) occur everywhere.  -> contiguous uint16 of u8's shape."""
    top = (1 << depth) - 1
    step = top // 255
    v = u8.astype(np.int64) * top // 255 + np.random.default_rng(rng).integers(-step, step + 1, u8.shape)
    return np.ascontiguousarray(np.clip(v, 0, top).astype(np.uint16))


def hbd_content(kind, w, h, depth, seed):
    """(h, w, 3) uint16 frames of `depth` bits: a smooth gradient over every code, noise, or a content kind of
    gpu_cases.content taken to `depth` bits."""
    top = (1 << depth) - 1
    if kind == "hgradient":
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([xx * top // max(w - 1, 1), yy * top // max(h - 1, 1), (xx + yy) * top // max(w + h - 2, 1)], -1)
    elif kind == "hnoise":
        img = np.random.default_rng(seed).integers(0, top + 1, (h, w, 3))
    else:
        return to_depth(gpu_cases.content(kind, w, h, seed), depth, seed)
    return np.ascontiguousarray(img.astype(np.uint16))


def hbd_distort(img, depth, seed):
    """A mild 16-bit distortion: quantise to 8 levels fewer bits and add noise (stays inside the depth's range)."""
    top = (1 << depth) - 1
    rng = np.random.default_rng(seed)
    step = 1 << (depth - 6)
    q = (img.astype(np.int64) // step) * step + step // 2
    return np.clip(q + rng.integers(-step // 4, step // 4 + 1, img.shape), 0, top).astype(np.uint16)


def content16(w, h, d, seed, distort=False):
    """(h, w, 3) uint16 frames of d bits: a natural synthetic frame (or its blockq distortion) taken to d bits."""
    u = synth.make_ref(w, h, seed)
    if distort:
        u = synth.distort(u, "blockq", 2, seed=seed)
    return to_depth(u, d, seed + d)


def rows16(img, channels, pad, seed=None, fill=None):
    """The uint16 frame `img` laid out like libavif's avifRGBImage at depth > 8: `channels` samples per pixel, rows
    `pad` samples longer than their pixels; alpha and padding are noise from `seed`, or the constant `fill`.
    -> (buffer, (h, w, channels) view)."""
    assert (seed is None) != (fill is None)
    h, w, _ = img.shape
    pitch = w * channels + pad
    if fill is None:
        buf = np.random.default_rng(seed).integers(0, 65536, (h, pitch), dtype=np.uint16)
    else:
        buf = np.full((h, pitch), fill, np.uint16)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, channels), (pitch * 2, channels * 2, 2))
    view[..., :3] = img
    return buf, view
