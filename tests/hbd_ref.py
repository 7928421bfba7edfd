"""CPU references for 16-bit scorer input (include/ssimu2_hip.h): the 16-bit FRONT ENDS of the two
reference routes.  The routes themselves have one owner each: tests/errmap_ref.py the fp32 checker route over linear
planes (scales, terms_lin, kernel_averages_lin, score_lin), tests/ssimu2_fp64.py the fp64 one (evaluate_linear, levels).

`table(d)` restates the library's sRGB -> linear table of d-bit samples and `linear_planes` builds the scale-0 fp32
linear planes of a uint16 frame from it; `compute`, `terms` and `levels` hand those to errmap_ref: the checker's
arithmetic, fed 16-bit planes.  `linear_planes_fp64` is the counterpart in fp64 (linear values never rounded to fp32),
which `compute_fp64`, `reference_levels` and `error_map_fp64` hand to ssimu2_fp64; `error_map_fp32` is the fp32 route's
map of the same frames.  `every_code_frame` is a frame that holds every 16-bit
code once per channel."""
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


def levels(orc, img: np.ndarray, d: int) -> list:
    """The checker's planes of a d-bit frame at every scale: [(linear (3, h_s, w_s), positive XYB)] (scale 0's linear
    planes from `linear_planes`, then the checker's downsample2 and linear_to_xyb)."""
    return [(lin, orc.linear_to_xyb(lin)) for lin in errmap_ref.scales(orc, linear_planes(img, d))]


terms = errmap_ref.terms_lin     # (orc, lin1, lin2, blur): the terms of two frames given as linear planes


def compute(orc, ref: np.ndarray, dist: np.ndarray, d: int, blur: int, d_dist: int | None = None):
    """-> (score, (6, 18) averages, nscales) of two uint16 frames of d bits (`d_dist`: the distorted frame's own
    depth) in the checker's blur mode `blur`.  The averages are errmap_ref.kernel_averages_lin's: the fp64 means (sums
    in extended precision) of the fp32 terms in the kernels' order, i.e. the `kavg` gpu_cases.check_against_terms
    holds a device score's averages to -- a caller needs no second pass over the terms for them."""
    return errmap_ref.score_lin(orc, linear_planes(ref, d), linear_planes(dist, d if d_dist is None else d_dist), blur)


def error_map_fp32(orc, ref: np.ndarray, dist: np.ndarray, d: int, blur: int):
    """The numpy fp32 map of two uint16 frames of d bits, its coefficients from the averages of its own terms (a device
    map takes the device's): -> (map (h, w) float32, the terms per scale, the (6, 18) averages).  Bit for bit the device
    map in the recursive modes, within gpu_cases.MAP_K * 2^-24 of it in FIR."""
    h, w, _ = ref.shape
    tm = errmap_ref.terms_lin(orc, linear_planes(ref, d), linear_planes(dist, d), blur)
    avg = errmap_ref.averages(tm)
    return errmap_ref.compose(tm, errmap_ref.coefficients(orc, avg, len(tm)), w, h), tm, avg


def linear_planes_fp64(img: np.ndarray, d: int) -> np.ndarray:
    v = np.moveaxis(_clamped(img, d), 2, 0).astype(np.float64) / float((1 << d) - 1)
    return np.where(v <= ref64.SRGB_THRESHOLD, v / ref64.SRGB_SLOPE,
                    ((v + ref64.SRGB_A) / (1.0 + ref64.SRGB_A)) ** ref64.SRGB_GAMMA)


def reference_levels(ref: np.ndarray, dist: np.ndarray, d: int, scales, d_dist: int | None = None) -> dict:
    """fp64_checks.reference_levels for uint16 frames of d bits (`d_dist`: the distorted frame's own depth):
    -> {scale: (lin1, lin2, xyb1, xyb2)} fp64 (3, h_s, w_s) planes at the scales asked for."""
    return ref64.levels(linear_planes_fp64(ref, d), linear_planes_fp64(dist, d if d_dist is None else d_dist), scales)


def compute_fp64(ref: np.ndarray, dist: np.ndarray, d: int, d_dist: int | None = None) -> dict:
    """ssimu2_fp64.evaluate for uint16 frames of d bits (`d_dist`: the distorted frame's own depth):
    {"score", "averages", "nscales", "weighted_sum"}."""
    return ref64.evaluate_linear(linear_planes_fp64(ref, d), linear_planes_fp64(dist, d if d_dist is None else d_dist))


def error_map_fp64(ref: np.ndarray, dist: np.ndarray, d: int):
    """ssimu2_fp64.error_map for uint16 frames of d bits: -> (map (h, w) fp64, evaluate_linear's result with planes).
    Shares no code with the kernels or the checker beyond the weight table."""
    result = ref64.evaluate_linear(linear_planes_fp64(ref, d), linear_planes_fp64(dist, d), planes=True)
    return ref64.error_map(None, None, result, size=ref.shape[:2])
