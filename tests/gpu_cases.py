"""Test-side helpers shared by the GPU modules: the blur-mode table (scorer mode -> the checker's mode of the same
blur), synthetic content kinds, libavif-like padded RGB(A) layouts and the error-map check against
tests/errmap_ref.py."""
from __future__ import annotations

import numpy as np

from oavif_amd import _lib
from oracle import ssimu2_oracle as orc

import errmap_ref

# mode name -> (ssimu2_ctx_set_blur mode, the checker's OR_BLUR_* of the same blur)
MODES = {"fir": (_lib.BLUR_FIR, orc.BLUR_FIR),
         "recursive": (_lib.BLUR_RECURSIVE, orc.BLUR_IIR),
         "recursive_fma": (_lib.BLUR_RECURSIVE_FMA, orc.BLUR_IIR_FMA)}

# the bounds of tests/test_gpu_recursive.py: score to 1e-4 (relative beyond 100 points), averages to rtol 2e-5
TOL_SCORE, RTOL_AVG, ATOL_AVG = 1e-4, 2e-5, 1e-9
TOL_FAR_BELOW_ZERO = 5e-4   # test_extreme_frames' bound for frames that score far below 0

# frame sizes where the kernels change shape (tests/test_gpu_mode_matrix.py, tests/test_fp64_reference.py)
SIZES = [
    (1, 1), (7, 7), (7, 100), (100, 7), (8, 8),                  # at and below 8 px: no scale, one scale
    (15, 9), (16, 16), (112, 112), (113, 113), (127, 300),       # scale-count transitions
    (119, 40), (120, 40), (121, 40), (241, 33),                  # FIR strip edges (120 columns)
    (64, 20), (65, 21), (128, 19), (129, 41),                    # recursive tile (64 columns) and batch edges
    (333, 217), (513, 259), (1921, 1083),                        # ragged
    (9, 1000), (1000, 9), (4000, 8), (8, 4000),                  # very tall, very wide
]


def score_tol(exp: float) -> float:
    return TOL_SCORE * max(1.0, abs(exp) / 100.0)


def content(kind, w, h, seed):
    """(h, w, 3) uint8 frames of five content kinds the kernels treat differently."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "gradient":
        img = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1),
                        (xx + yy) * 255 // max(w + h - 2, 1)], -1)
    elif kind == "primaries":      # saturated patches: exercises the opsin clamp / B-Y remap
        cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255],
                         [255, 0, 255], [0, 0, 0], [255, 255, 255]])
        img = cols[((xx // 16) + (yy // 16)) % 8]
    elif kind == "checker":        # 1-px checkerboard: maximal high-frequency energy
        img = np.repeat((((xx + yy) & 1) * 255)[..., None], 3, -1)
    elif kind == "text":           # thin dark strokes on light ground
        img = np.full((h, w, 3), 235)
        for _ in range(60):
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
            img[y:y + 1 + int(rng.integers(0, 2)), x:x + int(rng.integers(3, 30))] = 20
            img[y:y + int(rng.integers(3, 20)), x:x + 1] = 20
    else:                          # white noise
        img = rng.integers(0, 256, (h, w, 3))
    return np.ascontiguousarray(img.astype(np.uint8))


def decoded_like(dist, channels, pad, seed):
    """`dist` laid out like libavif's avifRGBImage: `channels` bytes per pixel (alpha random),
    rows `pad` bytes longer than their pixels, padding filled with noise."""
    h, w, _ = dist.shape
    rng = np.random.default_rng(seed)
    pitch = w * channels + pad
    buf = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, channels), (pitch, channels, 1))
    view[..., :3] = dist
    return buf, view


def check_map(oracle, m, avg, ns, ref, dist, blur, what):
    """The device map `m` of (ref, dist), whose score left averages `avg` over `ns` scales, against the numpy
    reference in the checker's mode `blur`: per pixel to PIXEL_RTOL of the map's peak, the mean to MEAN_RTOL."""
    exp, _own, ns_r = errmap_ref.reference_map(oracle, ref, dist, blur, avg=avg)
    assert ns == ns_r and m.shape == exp.shape and m.dtype == np.float32, what
    peak = float(exp.max())
    err = float(np.abs(m.astype(np.float64) - exp).max())
    mean_e = exp.mean(dtype=np.float64)
    rel_mean = abs(m.mean(dtype=np.float64) - mean_e) / max(mean_e, 1e-30)
    assert err <= errmap_ref.PIXEL_RTOL * peak, (what, err, peak)
    assert rel_mean <= errmap_ref.MEAN_RTOL, (what, rel_mean)


def pseudo_codec(ref):
    """Deterministic stand-in for encode(q) -> decode: coarser block quantisation for lower q."""
    def codec(q):
        step = 1 + (100 - q) // 3
        dec = (ref.astype(np.int32) // step) * step + step // 2
        return np.clip(dec, 0, 255).astype(np.uint8), 1000 + 10 * q
    return codec
