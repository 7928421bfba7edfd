"""CPU references for 16-bit scorer input (include/ssimu2_hip.h).

`table(d)` restates the library's sRGB -> linear table of d-bit samples.  `compute` builds the scale-0 linear planes
of two uint16 frames from it and follows tests/errmap_ref.py's route through the oracle's public helpers
(downsample2, linear_to_xyb, the blur helpers, score_from_averages): the checker's arithmetic, fed 16-bit planes.
`compute_fp64` is the counterpart in fp64 (tests/ssimu2_fp64.py's stages, linear values never rounded to fp32).
`levels` / `reference_levels` are the per-scale planes of both routes, for the instrumented build's plane downloads, and
`every_code_frame` is a frame that holds every 16-bit code once per channel."""
from __future__ import annotations

import numpy as np

import errmap_ref
import ssimu2_fp64 as ref64


def table(d: int) -> np.ndarray:
    """2^d float32 entries: (float)(v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4)), v = s / (2^d - 1)
    in fp64 (the 8-bit table's expression)."""
    v = np.arange(1 << d, dtype=np.float64) / float((1 << d) - 1)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4).astype(np.float32)


def _clamped(img: np.ndarray, d: int) -> np.ndarray:
    assert img.dtype == np.uint16 and img.ndim == 3 and img.shape[2] == 3
    return np.minimum(img, (1 << d) - 1)


def linear_planes(img: np.ndarray, d: int) -> np.ndarray:
    """(3, h, w) float32 scale-0 linear planes of a d-bit frame (samples above 2^d - 1 clamped)."""
    return table(d)[_clamped(img, d)].transpose(2, 0, 1).copy()


def every_code_frame() -> np.ndarray:
    """(256, 256, 3) uint16: each channel holds all 65,536 codes once, each channel in its own order (R in raster
    order, G and B two fixed permutations), so that a pixel's three samples differ and no channel repeats another."""
    v = np.arange(1 << 16, dtype=np.uint32)
    g = (v * 40503 + 12345) & 0xFFFF                      # odd multiplier: a bijection of Z / 2^16
    b = np.random.default_rng(1016).permutation(1 << 16)
    return np.ascontiguousarray(np.stack([v, g, b], -1).astype(np.uint16).reshape(256, 256, 3))


def _scales(orc, lin):
    out = []
    for s in range(6):
        h, w = lin.shape[1:]
        if w < 8 or h < 8:
            break
        if s:
            lin = orc.downsample2(lin)
        out.append(lin)
    return out


def levels(orc, img: np.ndarray, d: int) -> list:
    """The checker's planes of a d-bit frame at every scale: [(linear (3, h_s, w_s), positive XYB)] (scale 0's linear
    planes from `linear_planes`, then the checker's downsample2 and linear_to_xyb)."""
    return [(lin, orc.linear_to_xyb(lin)) for lin in _scales(orc, linear_planes(img, d))]


def terms(orc, lin1, lin2, blur):
    """errmap_ref.terms from linear planes instead of 8-bit frames."""
    return [np.stack([errmap_ref.channel_terms(orc, x1[c], x2[c], blur) for c in range(3)])
            for x1, x2 in ((orc.linear_to_xyb(l1), orc.linear_to_xyb(l2))
                           for l1, l2 in zip(_scales(orc, lin1), _scales(orc, lin2)))]


def compute(orc, ref: np.ndarray, dist: np.ndarray, d: int, blur: int, d_dist: int | None = None):
    """-> (score, (6, 18) averages, nscales) of two uint16 frames of d bits (`d_dist`: the distorted frame's own
    depth) in the checker's blur mode `blur`.  The averages are errmap_ref.averages(terms(...)): the fp64 means (sums
    in extended precision) of the fp32 terms in the kernels' order, i.e. the `kavg` gpu_cases.check_against_terms
    holds a device score's averages to -- a caller needs no second pass over the terms for them."""
    tm = terms(orc, linear_planes(ref, d), linear_planes(dist, d if d_dist is None else d_dist), blur)
    avg = errmap_ref.averages(tm)
    ns = len(tm)
    return (orc.score_from_averages(avg, ns) if ns else 100.0), avg, ns


def linear_planes_fp64(img: np.ndarray, d: int) -> np.ndarray:
    v = np.moveaxis(_clamped(img, d), 2, 0).astype(np.float64) / float((1 << d) - 1)
    return np.where(v <= ref64.SRGB_THRESHOLD, v / ref64.SRGB_SLOPE,
                    ((v + ref64.SRGB_A) / (1.0 + ref64.SRGB_A)) ** ref64.SRGB_GAMMA)


def reference_levels(ref: np.ndarray, dist: np.ndarray, d: int, scales, d_dist: int | None = None) -> dict:
    """fp64_checks.reference_levels for uint16 frames of d bits (`d_dist`: the distorted frame's own depth):
    -> {scale: (lin1, lin2, xyb1, xyb2)} fp64 (3, h_s, w_s) planes at the scales asked for."""
    out = {}
    lin1 = linear_planes_fp64(ref, d)
    lin2 = linear_planes_fp64(dist, d if d_dist is None else d_dist)
    for s in range(max(scales) + 1):
        if s:
            lin1, lin2 = ref64.downsample2(lin1), ref64.downsample2(lin2)
        if s in scales:
            out[s] = (lin1, lin2, ref64.to_xyb(lin1), ref64.to_xyb(lin2))
    return out


def compute_fp64(ref: np.ndarray, dist: np.ndarray, d: int, d_dist: int | None = None) -> dict:
    """ssimu2_fp64.evaluate for uint16 frames of d bits (`d_dist`: the distorted frame's own depth):
    {"score", "averages", "nscales", "weighted_sum"}."""
    h, w, _ = ref.shape
    avg = np.zeros((ref64.NUM_SCALES, 18))
    lin1, lin2 = linear_planes_fp64(ref, d), linear_planes_fp64(dist, d if d_dist is None else d_dist)
    ns = ref64.nscales_of(w, h)
    for s in range(ns):
        if s:
            lin1, lin2 = ref64.downsample2(lin1), ref64.downsample2(lin2)
        x1, x2 = ref64.to_xyb(lin1), ref64.to_xyb(lin2)
        for c in range(3):
            a, b = x1[c], x2[c]
            mu1, mu2 = ref64.blur(a), ref64.blur(b)
            s11, s22, s12 = ref64.blur(a * a), ref64.blur(b * b), ref64.blur(a * b)
            num_m = 1.0 - (mu1 - mu2) ** 2
            num_s = 2.0 * (s12 - mu1 * mu2) + ref64.C2
            den_s = (s11 - mu1 * mu1) + (s22 - mu2 * mu2) + ref64.C2
            dd = np.maximum(0.0, 1.0 - num_m * num_s / den_s)
            e = (1.0 + np.abs(b - mu2)) / (1.0 + np.abs(a - mu1)) - 1.0
            art, det = np.maximum(e, 0.0), np.maximum(-e, 0.0)
            avg[s, c * 2] = dd.mean()
            avg[s, c * 2 + 1] = np.mean(dd ** 4) ** 0.25
            avg[s, 6 + c * 4] = art.mean()
            avg[s, 6 + c * 4 + 1] = np.mean(art ** 4) ** 0.25
            avg[s, 6 + c * 4 + 2] = det.mean()
            avg[s, 6 + c * 4 + 3] = np.mean(det ** 4) ** 0.25
    ws = ref64.weighted_sum(avg, ns)
    return {"score": ref64.score_from_weighted_sum(ws), "averages": avg, "nscales": ns, "weighted_sum": ws}
