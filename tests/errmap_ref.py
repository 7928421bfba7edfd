"""numpy reference of the per-pixel error map (include/ssimu2_hip.h), built from the CPU
oracle's public helpers.  The per-pixel terms are evaluated in fp32 in the kernels' operation order; a fused
multiply-add of fp32 operands is correctly rounded (`_fma`), and the map's coefficients restate the host's fp64
expression (`coefficients`).  `kernel_averages` are the 108 averages of those terms in fp64: what the kernels' sums
of the same terms approach (the recursive modes exactly up to fp64 summation).  Given the
segment rows of every scale, `kernel_averages`, `averages` and `reference_map` also return, from the same terms, the
SSIM averages summed in k_march's own order (tests/fir_sums.py).

This module owns the fp32 checker route, stated once over scale-0 linear planes: the pyramid rule (`scales`), then XYB,
`channel_terms` and the averages (`terms_lin`, `kernel_averages_lin`, which streams one channel at a time, and
`score_lin`).  What makes the planes is a front end: `linear_planes` here for 8-bit frames (`terms`, `kernel_averages`,
`reference_map`), tests/hbd_ref.py for 16-bit ones, tests/test_gpu_alpha.py for a composite's codes."""
from __future__ import annotations

import numpy as np

import fir_sums

F32 = np.float32
C2 = F32(0.0009)
# a device map against reference_map: the bound on the relative error of its mean (the per-pixel bounds are
# gpu_cases.check_map's)
MEAN_RTOL = 1e-5


def _fma(a, b, c):
    """fmaf(a, b, c) of fp32 operands, correctly rounded: the fp64 product of two fp32 values is exact; the sum with
    c is taken exactly as s + err (TwoSum), s is rounded to odd in fp64 (an inexact sum keeps an odd last bit), and
    that value rounded once to fp32.  Round-to-odd in 53 bits followed by round-to-nearest in 24 bits is the correct
    rounding (53 >= 2 * 24 + 2), where rounding s itself could round twice across an fp32 halfway point."""
    p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bp = s - p
        err = (p - (s - bp)) + (c - bp)
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def linear_planes(orc, img):
    """(3, h, w) float32 scale-0 linear planes of an (h, w, 3) uint8 frame: the checker's table."""
    return orc.srgb_lut()[img].transpose(2, 0, 1).copy()


def scales(orc, lin):
    """The scorer's pyramid rule over (3, h, w) scale-0 linear planes: -> the linear planes of every scored scale.  Every
    fp32 route starts here, whatever made the planes (8-bit frames above, hbd_ref.linear_planes, a composite's)."""
    out = []
    for s in range(6):
        h, w = lin.shape[1:]
        if w < 8 or h < 8:
            break
        if s:
            lin = orc.downsample2(lin)
        out.append(lin)
    return out


def channel_terms(orc, a, b, blur):
    """-> (6, h, w) float32 terms d, d^4, art, art^4, det, det^4 of one XYB channel pair (a reference, b distorted)."""
    mu1, mu2 = orc.blur_plane(a, blur), orc.blur_plane(b, blur)
    s11, s22, s12 = orc.blur_product(a, a, blur), orc.blur_product(b, b, blur), orc.blur_product(a, b, blur)
    mu11, mu22, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    dm = mu1 - mu2
    num_m = _fma(-dm, dm, 1.0)
    num_s = _fma(F32(2.0), s12 - mu12, C2)
    denom_s = ((s11 - mu11) + (s22 - mu22)) + C2
    d = np.maximum(F32(1.0) - (num_m * num_s) / denom_s, F32(0.0))
    ea, eb = np.abs(b - mu2), np.abs(a - mu1)
    e = (ea - eb) / (F32(1.0) + eb)
    art, det = np.maximum(e, F32(0.0)), np.maximum(-e, F32(0.0))
    d2, a2, t2 = d * d, art * art, det * det
    return np.stack([d, d2 * d2, art, a2 * a2, det, t2 * t2])


def _xyb_pairs(orc, lin1, lin2):
    for l1, l2 in zip(scales(orc, lin1), scales(orc, lin2)):
        yield orc.linear_to_xyb(l1), orc.linear_to_xyb(l2)


def terms_lin(orc, lin1, lin2, blur):
    """-> per scale: (3, 6, h_s, w_s) float32 terms d, d^4, art, art^4, det, det^4 of two frames given as scale-0 linear
    planes (reference first)."""
    return [np.stack([channel_terms(orc, x1[c], x2[c], blur) for c in range(3)])
            for x1, x2 in _xyb_pairs(orc, lin1, lin2)]


def terms(orc, ref, dist, blur):
    """terms_lin of two (h, w, 3) uint8 frames."""
    return terms_lin(orc, linear_planes(orc, ref), linear_planes(orc, dist), blur)


def _put(avg, s, c, m):
    """the fp64 means m[0..5] of one channel's terms as its six averages (L4 norms: the 4th root of the mean)."""
    avg[s, c * 2], avg[s, c * 2 + 1] = m[0], m[1] ** 0.25
    for k in range(4):
        avg[s, 6 + c * 4 + k] = m[2 + k] if k % 2 == 0 else m[2 + k] ** 0.25


def _put_sums(kord, s, c, t, seg):
    """the SSIM averages of one channel's terms t (6, h, w) summed in k_march's order at `seg` rows per segment."""
    kord[s, c * 2], kord[s, c * 2 + 1] = fir_sums.means(t[0], t[1], seg)


def averages(tm, seg_rows=None):
    """-> (6, 18) float64 averages [scale][stat] of the terms (0..5 ssim c*2+n, 6..17 edge c*4+k).  With `seg_rows`
    (rows per k_march segment, by scale): -> (those, (6, 6) averages 0..5 summed in the kernel's order)."""
    avg, kord = np.zeros((6, 18)), np.zeros((6, 6))
    for s, t in enumerate(tm):
        for c in range(3):
            _put(avg, s, c, _means(t[c]))
            if seg_rows is not None:
                _put_sums(kord, s, c, t[c], seg_rows[s])
    return avg if seg_rows is None else (avg, kord)


def _means(t):
    """(6,) fp64 means of one channel's (6, h, w) terms, each sum taken in extended precision so that the reference's
    own rounding stays far below the bounds the kernels' sums are held to (tests/gpu_cases.py)."""
    n = t[0].size
    return [float(t[k].sum(dtype=np.longdouble) / n) for k in range(6)]


def kernel_averages_lin(orc, lin1, lin2, blur, seg_rows=None):
    """-> ((6, 18) float64, nscales): averages(terms_lin(orc, lin1, lin2, blur)), one channel's terms at a time (a 4K
    pair's terms would take about 1 GB at once).  With `seg_rows` (by scale): -> (those, nscales, (6, 6) averages 0..5
    in the kernel's order), from the same pass over the terms."""
    avg, kord, ns = np.zeros((6, 18)), np.zeros((6, 6)), 0
    for s, (x1, x2) in enumerate(_xyb_pairs(orc, lin1, lin2)):
        for c in range(3):
            t = channel_terms(orc, x1[c], x2[c], blur)
            _put(avg, s, c, _means(t))
            if seg_rows is not None:
                _put_sums(kord, s, c, t, seg_rows[s])
        ns = s + 1
    return (avg, ns) if seg_rows is None else (avg, ns, kord)


def kernel_averages(orc, ref, dist, blur, seg_rows=None):
    """kernel_averages_lin of two (h, w, 3) uint8 frames."""
    return kernel_averages_lin(orc, linear_planes(orc, ref), linear_planes(orc, dist), blur, seg_rows)


def score_lin(orc, lin1, lin2, blur):
    """-> (score, (6, 18) averages, nscales) of two frames given as scale-0 linear planes in the checker's blur mode
    `blur`: the checker's score of kernel_averages_lin, 100 without a scale."""
    avg, ns = kernel_averages_lin(orc, lin1, lin2, blur)
    return (orc.score_from_averages(avg, ns) if ns else 100.0), avg, ns


def weighted_terms(orc, avg, nscales):
    """The score's contiguous weight walk: -> [(weight, scale, stat)] and sum w_i * |a_i|."""
    wts = orc.weights()
    out, j = [], 0
    for c in range(3):
        for s in range(nscales):
            for n in range(2):
                for k in range(3):
                    stat = c * 2 + n if k == 0 else 6 + c * 4 + n + (2 if k == 2 else 0)
                    out.append((wts[j], s, stat))
                    j += 1
    return out, sum(w * abs(avg[s, st]) for w, s, st in out)


def coefficient(w, a, l4):
    """map_coefficients (oavif_amd/csrc/ssimu2_hip.hip) for one average: w for an L1 statistic; w / (a * a * a) in
    fp64 for an L4 one (0 when a == 0; a quotient that overflows is inf), clamped at 3e38, rounded once to fp32."""
    if not l4:
        v = np.float64(w)
    elif a > 0.0:
        a = np.float64(a)
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            v = np.float64(w) / ((a * a) * a)
    else:
        v = np.float64(0.0)
    return F32(min(v, np.float64(3.0e38)))


def coefficients(orc, avg, nscales):
    """(6, 18) float32: w for L1 statistics, w / a^3 for L4 ones (0 when a == 0), as the host computes them."""
    coef = np.zeros((6, 18), F32)
    walk, _ = weighted_terms(orc, avg, nscales)
    for w, s, st in walk:
        coef[s, st] = coefficient(w, avg[s, st], st % 2 == 1)
    return coef


def stat_of(c, k):
    return c * 2 + k if k < 2 else 6 + c * 4 + (k - 2)


def compose(tm, coef, w, h):
    m = np.zeros((h, w), F32)
    ys, xs = np.arange(h), np.arange(w)
    for s, t in enumerate(tm):
        dens = []
        for c in range(3):
            mc = [coef[s, stat_of(c, k)] for k in range(6)]
            v = mc[0] * t[c, 0]
            for k in range(1, 6):
                v = _fma(mc[k], t[c, k], v)
            dens.append(v)
        dsum = (dens[0] + dens[1]) + dens[2]
        m = m + dsum[(ys >> s)[:, None], (xs >> s)[None, :]]
    return m


def reference_map(orc, ref, dist, blur, avg=None, seg_rows=None):
    """-> (map, averages of the reference's own terms, nscales).  `avg` (e.g. the device's) overrides the
    averages the coefficients are derived from.  With `seg_rows` (by scale) a fourth value: the (6, 6) averages 0..5
    of the same terms in the kernel's order."""
    h, w, _ = ref.shape
    tm = terms(orc, ref, dist, blur)
    own = averages(tm, seg_rows)
    kord = () if seg_rows is None else (own[1],)
    own = own if seg_rows is None else own[0]
    coef = coefficients(orc, own if avg is None else avg, len(tm))
    return (compose(tm, coef, w, h), own, len(tm)) + kord
