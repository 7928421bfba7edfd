"""numpy reference of the per-pixel error map (include/ssimu2_hip.h), built from the CPU
oracle's public helpers.  The per-pixel terms are evaluated in fp32 in the kernels' operation order; a fused
multiply-add of fp32 operands is evaluated in fp64 (the product is exact there) and rounded once."""
from __future__ import annotations

import numpy as np

F32 = np.float32
C2 = F32(0.0009)
# a device map against reference_map: per-pixel bound relative to the map's maximum, and the bound on the
# relative error of the mean
PIXEL_RTOL, MEAN_RTOL = 1e-4, 1e-5


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _scales(orc, img):
    """linear-light planes (3, h, w) of every scored scale (the scorer's pyramid rule)."""
    lin = orc.srgb_lut()[img].transpose(2, 0, 1).copy()
    out = []
    for s in range(6):
        h, w = lin.shape[1:]
        if w < 8 or h < 8:
            break
        if s:
            lin = orc.downsample2(lin)
        out.append(lin)
    return out


def terms(orc, ref, dist, blur):
    """-> per scale: (3, 6, h_s, w_s) float32 terms d, d^4, art, art^4, det, det^4."""
    res = []
    for l1, l2 in zip(_scales(orc, ref), _scales(orc, dist)):
        x1, x2 = orc.linear_to_xyb(l1), orc.linear_to_xyb(l2)
        t = np.zeros((3, 6) + x1.shape[1:], F32)
        for c in range(3):
            a, b = x1[c], x2[c]
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
            t[c] = np.stack([d, d2 * d2, art, a2 * a2, det, t2 * t2])
        res.append(t)
    return res


def averages(tm):
    """-> (6, 18) float64 averages [scale][stat] of the terms (0..5 ssim c*2+n, 6..17 edge c*4+k)."""
    avg = np.zeros((6, 18))
    for s, t in enumerate(tm):
        m = t.astype(np.float64).mean(axis=(2, 3))  # (3, 6)
        for c in range(3):
            avg[s, c * 2], avg[s, c * 2 + 1] = m[c, 0], m[c, 1] ** 0.25
            for k in range(4):
                avg[s, 6 + c * 4 + k] = m[c, 2 + k] if k % 2 == 0 else m[c, 2 + k] ** 0.25
    return avg


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


def coefficients(orc, avg, nscales):
    """(6, 18) float32: w for L1 statistics, w / a^3 for L4 ones (0 when a == 0)."""
    coef = np.zeros((6, 18), np.float64)
    walk, _ = weighted_terms(orc, avg, nscales)
    for w, s, st in walk:
        a = avg[s, st]
        l4 = st % 2 == 1
        coef[s, st] = (w / a ** 3 if a > 0 else 0.0) if l4 else w
    return np.minimum(coef, 3.0e38).astype(F32)


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


def reference_map(orc, ref, dist, blur, avg=None):
    """-> (map, averages of the reference's own terms, nscales).  `avg` (e.g. the device's) overrides the
    averages the coefficients are derived from."""
    h, w, _ = ref.shape
    tm = terms(orc, ref, dist, blur)
    own = averages(tm)
    coef = coefficients(orc, own if avg is None else avg, len(tm))
    return compose(tm, coef, w, h), own, len(tm)
