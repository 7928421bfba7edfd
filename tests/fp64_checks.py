"""How far an fp32 SSIMULACRA2 (the checker, the HIP kernels) may sit from the fp64 reference of tests/ssimu2_fp64.py,
and the measures those bounds are stated in.  Shared by tests/test_fp64_reference.py (CPU),
tests/test_gpu_fp64_reference.py (-m gpu) and tests/tools/cpu_fp64_campaign.py, which measured every bound here:
each is the campaign's maximum times a stated margin.

Why these measures: single averages near 1e-6 carry large relative rounding error that no weight makes visible, so
averages are compared in the weighted domain, term by term against the frame's own sum w_i |a_i|; and near 100 the
score polynomial's slope diverges, so there the sum itself is compared relatively instead of the score.
"""
from __future__ import annotations

import numpy as np

import ssimu2_fp64 as ref64

# ---- stage bounds (checker stage vs the reference's stage on the same input) ----------------------------------------
# linear_to_xyb, all 2^24 colours and the pyramid levels of the plane test: absolute; campaign max 8.8e-7 (X); x1.8
XYB_ABS = 1.6e-6
# downsample2 of one plane: in ulps of the fp32 result, campaign max 1.5; x1.33
DOWNSAMPLE_ULP = 2.0
# blur_plane / blur_product: max |delta| / max |input|; campaign max FIR 1.9e-7, EXACT 5.5e-8; x2
BLUR_REL = {"fir": 4e-7, "exact": 1.1e-7}
# the fp32 recursion random-walks along a line: max |delta| / max |input| <= IIR_REL_PER_SQRT_LINE * sqrt(line);
# campaign max of the ratio 5.9e-7 (lines of 16 .. 4096, both orders); x1.7
IIR_REL_PER_SQRT_LINE = 1e-6

# ---- intermediate planes of a frame (checker planes = device planes) -------------------------------------------------
# pyramid levels 1..5 in ulps, campaign max 2.76 (4K); FIR blur of ref * ref relative to the peak, max 1.32e-6 (4K)
PLANE_LIN_ULPS, PLANE_FIR_REL = 4.0, 2.5e-6
# recursive planes: max |delta| / peak <= RG_REL0 + IIR_REL_PER_SQRT_LINE * sqrt(w + h), RG_REL0 the share of the
# fp32 XYB planes' own error; campaign max of (dev - RG_REL0) / sqrt(w + h) 3.3e-7
RG_REL0 = 3e-6

# ---- scores and averages ---------------------------------------------------------------------------------------------
# "natural" frames (photographs, the golden fixtures, synth.make_ref): |score - reference| where the reference scores
# at most NEAR_100, above it |sum - reference sum| / reference sum; and every weighted term
# w_i |a_i - reference a_i| <= TERM_REL * reference sum.  Campaign max (206 cases up to 4K):
#   FIR score 8.7e-3 (4K), term 8.1e-4; EXACT score 3.9e-3, term 5.0e-4; near 100 both < 1e-6
NEAR_100 = 95.0
SCORE_ABS = {"fir": 1.1e-2, "exact": 5e-3}
TERM_REL = {"fir": 1.2e-3, "exact": 7e-4}
SUM_REL = {"fir": 1e-3, "exact": 1e-3}
# "synthetic" frames (flat areas, 1-px checkerboards, thin strokes: gpu_cases.content, extreme frames): there sigma
# is ~0 over most of a scale and fp32 cancellation noise is as large as the averages themselves (up to 7 % of the
# weight-225 term), so neither relative measure means anything.  Instead every weighted average to an absolute
# bound, and the score (<= NEAR_100) more loosely.  Campaign max: FIR |delta a| 5.0e-5, score 0.117;
# EXACT 4.7e-5, 0.021
AVG_ABS = {"fir": 1e-4, "exact": 1e-4}
SYNTH_SCORE_ABS = {"fir": 0.25, "exact": 0.05}
# the recursive modes, measured through the checker's OR_BLUR_IIR / OR_BLUR_IIR_FMA (planes bit-identical to the
# device's), frames up to IIR_MAX_PIXELS only: natural score 0.41, term 2.6e-2, near 100 1.1e-4; synthetic |delta a|
# 4.0e-3, score 2.6.  Beyond it the recursion's noise reaches 1.8 points (4K): no bound
IIR_MAX_PIXELS = 400 * 400
for _m in ("recursive", "recursive_fma"):
    SCORE_ABS[_m], TERM_REL[_m], SUM_REL[_m] = 0.6, 4e-2, 1e-3
    AVG_ABS[_m], SYNTH_SCORE_ABS[_m] = 8e-3, 4.0

# the per-pixel error map, fp32 (device / tests/errmap_ref.py) against the fp64 map of section 9: per pixel relative to
# the map's peak, campaign max FIR 2.7e-3, RECURSIVE 3.6e-2; the mean against sum w_i |a_i| where every scale tiles
# the frame, max 1.6e-5 / 4.4e-4
MAP_PIXEL_REL = {"fir": 5e-3, "recursive": 6e-2}
MAP_MEAN_REL = {"fir": 5e-5, "recursive": 1e-3}

# the same two measures for maps of 9- to 16-bit frames (hbd_cases.content16 pairs: MAP_HBD_CASES below and a dozen more
# at depths 9..16, sizes up to 640 x 352; cpu_fp64_campaign.py's "error map, 16-bit" section), fp32 (device /
# errmap_ref over hbd_ref.linear_planes) against hbd_ref.error_map_fp64.  content16's low-order noise makes these maps
# rougher than the 8-bit campaign's, so they get bounds of their own: campaign max x 2.
#   pixel: campaign max FIR 3.18e-3 (174 x 207, 12-bit), RECURSIVE 4.13e-2 (192 x 224, 9-bit);
#   mean (tiling sizes): 1.02e-4 (160 x 128, 13-bit) / 1.97e-3 (192 x 224, 9-bit)
MAP_PIXEL_REL_HBD = {"fir": 6.4e-3, "recursive": 8.3e-2}
MAP_MEAN_REL_HBD = {"fir": 2.1e-4, "recursive": 4e-3}
MAP_HBD_CASES = [(128, 96, 10), (131, 173, 12), (640, 352, 9)]   # (w, h, depth); pairs: map_hbd_pair

# a structural variant of a stage must miss at least one FIR check (natural frames) by this factor
DISCRIMINATION_FACTOR = 2.0


def map_hbd_pair(w: int, h: int, d: int, seed=None):
    """The content16 pair of a 16-bit map case: (reference, distorted), seeded by the size unless `seed` is given."""
    from hbd_cases import content16
    seed = w * h if seed is None else seed
    return content16(w, h, d, seed), content16(w, h, d, seed, distort=True)


def map_tiles(w: int, h: int, nscales: int) -> bool:
    """Every scale tiles the frame (w, h multiples of 2^(nscales - 1)): only then is the map's mean sum w_i |a_i|."""
    return nscales >= 1 and w % (1 << (nscales - 1)) == 0 and h % (1 << (nscales - 1)) == 0


def map_deviation(m, m64, e: dict) -> dict:
    """An fp32 map `m` against the fp64 map `m64` of the result `e`: -> {"pixel": max |delta| / the fp64 map's peak,
    "mean": |mean - sum w_i |a_i|| / that sum where every scale tiles the frame, else None}."""
    assert m.shape == m64.shape
    h, w = m64.shape
    out = {"pixel": float(np.abs(m - m64).max() / m64.max()), "mean": None}
    if map_tiles(w, h, e["nscales"]):
        out["mean"] = abs(float(m.mean(dtype=np.float64)) - e["weighted_sum"]) / e["weighted_sum"]
    return out


def map_deviation_text(dev: dict, pixel_bound: float, mean_bound: float) -> str:
    mean = "not measured (a scale does not tile the frame)" if dev["mean"] is None else f"{dev['mean']:.3e}"
    return f"pixel {dev['pixel']:.3e} (bound {pixel_bound:.1e}), mean {mean} (bound {mean_bound:.1e})"


def deviation(score, avg, nscales, exp: dict) -> dict:
    """One fp32 evaluation (score, (6, 18) averages, nscales) against the reference's result `exp`: -> {"nscales_ok",
    "score" |delta score|, "sum" relative delta of sum w_i |a_i|, "term" largest w_i |delta a_i| / reference sum}."""
    avg = np.asarray(avg, np.float64).reshape(6, 18)
    ws = exp["weighted_sum"]
    out = {"nscales_ok": nscales == exp["nscales"], "score": abs(score - exp["score"])}
    if not out["nscales_ok"]:
        out.update(sum=float("inf"), term=float("inf"))
        return out
    walk = ref64.weight_walk(nscales)
    got_ws = float(sum(w * abs(avg[s, st]) for w, s, st in walk))
    out["sum"] = abs(got_ws - ws) / ws if ws > 0 else abs(got_ws)
    term = max((w * abs(avg[s, st] - exp["averages"][s, st]) for w, s, st in walk), default=0.0)
    out["term"] = term / ws if ws > 0 else term
    out["avg_abs"] = max((abs(avg[s, st] - exp["averages"][s, st]) for w, s, st in walk if w > 0), default=0.0)
    return out


def ratios(dev: dict, exp: dict, mode: str, kind: str = "natural") -> dict:
    """Each check's deviation as a multiple of its bound (> 1: the check fails)."""
    if not dev["nscales_ok"]:
        return {"nscales": float("inf")}
    if kind == "synthetic":
        r = {"avg_abs": dev["avg_abs"] / AVG_ABS[mode]}
        if exp["score"] <= NEAR_100:
            r["score"] = dev["score"] / SYNTH_SCORE_ABS[mode]
        return r
    r = {"term": dev["term"] / TERM_REL[mode]}
    if exp["score"] > NEAR_100:
        r["sum"] = dev["sum"] / SUM_REL[mode]
    else:
        r["score"] = dev["score"] / SCORE_ABS[mode]
    return r


def check(score, avg, nscales, exp: dict, mode: str, what, kind: str = "natural") -> dict:
    """Assert one fp32 evaluation against the reference in the bounds of `mode` for frames of `kind`."""
    dev = deviation(score, avg, nscales, exp)
    assert dev["nscales_ok"], (what, nscales, exp["nscales"])
    r = ratios(dev, exp, mode, kind)
    assert max(r.values()) <= 1.0, (what, mode, kind, exp["score"], score, dev)
    return dev


# ---- intermediate planes (the instrumented build's debug downloads; the checker's planes are the same bits) ---------

def reference_levels(ref, dist, scales):
    """-> {scale: (lin1, lin2, xyb1, xyb2)} fp64 (3, h_s, w_s) planes of the reference at the scales asked for."""
    lin1, lin2 = ref64.srgb_to_linear(np.moveaxis(ref, 2, 0)), ref64.srgb_to_linear(np.moveaxis(dist, 2, 0))
    return ref64.levels(lin1, lin2, scales)


def lin_ulps(got, exp) -> float:
    """linear-light pyramid levels: max |delta| in ulps of the fp32 value of the reference."""
    sp = np.spacing(np.abs(exp).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - exp) / sp))


def abs_dev(got, exp) -> float:
    return float(np.max(np.abs(got - exp)))


def rel_dev(got, exp) -> float:
    """blurred planes: max |delta| relative to the plane's largest value."""
    return float(np.max(np.abs(got - exp)) / max(float(np.max(np.abs(exp))), 1e-30))


def rg_reference(xyb1, xyb2, vertical: bool):
    """The 15 planes (5 c + {x, y, xx, yy, xy}) of the recursive mode after the horizontal pass / after both."""
    out = []
    for c in range(3):
        a, b = xyb1[c], xyb2[c]
        for src in (a, b, a * a, b * b, a * b):
            out.append(ref64.blur(src) if vertical else ref64._blur_axis(src, 1))
    return out
