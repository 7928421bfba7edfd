"""An independent fp64 statement of SSIMULACRA2 v2.1 (TEST INFRASTRUCTURE, like errmap_ref.py).

Written from the stage list of DESIGN.md section 2.1 and the map definition of section 9, not from the checker
(oracle/ssimu2_oracle.c): plain numpy, fp64 throughout, whole planes, no fp32 rounding and no fused-multiply-add
order emulated.  The only thing taken from the checker is the 108-entry weight table (`weights()`), which
tests/test_oracle.py::test_weights_table pins by checksum.  Every other constant is typed here, and the blur taps
are derived here from sigma = 1.5 by the published recursive-Gaussian construction (Charalampidis 2016, three
second-order sections, as libjxl builds it): the recursion is run in fp64 on a unit impulse and its response read
off, so the checker's closed form of the same taps is not used either.

What the checker and the kernels evaluate in fp32 this evaluates in fp64; the difference between the two is
rounding, and tests/test_fp64_reference.py bounds it stage by stage and score by score.
"""
from __future__ import annotations

import numpy as np

SIGMA = 1.5
NUM_SCALES = 6
MIN_SIZE = 8                       # a scale is scored iff the previous one is at least 8 x 8

# sRGB transfer curve (IEC 61966-2-1)
SRGB_THRESHOLD, SRGB_SLOPE, SRGB_A, SRGB_GAMMA = 0.04045, 12.92, 0.055, 2.4

# opsin absorbance (rows L, M, S; the S row is 1 - the other two columns) and bias
OPSIN = np.array([[0.30, 0.622, 0.078],
                  [0.23, 0.692, 0.078],
                  [0.24342268924547819, 0.20476744424496821, 0.55180986650955360]], np.float64)
OPSIN_BIAS = 0.0037930732552754493

# positive XYB: X * 14 + 0.42, Y + 0.01, (B - Y) + 0.55
XYB_X_SCALE, XYB_X_OFFSET, XYB_Y_OFFSET, XYB_B_OFFSET = 14.0, 0.42, 0.01, 0.55

C2 = 0.0009

# the score: sum w_i |a_i|, times 0.9562..., a cubic, then 100 - 10 p^0.6276...
SCORE_SCALE = 0.9562382616834844
POLY = (2.326765642916932, -0.020884521182843837, 6.248496625763138e-05)
EXPONENT = 0.6276336467831387


# ---- blur taps ----------------------------------------------------------------------------------------------------

def recursive_gaussian(sigma: float = SIGMA):
    """The published construction of the three undamped second-order sections: -> (radius N, n2[3], d1[3]).
    Section k has frequency omega_k = (2k + 1) pi / (2N); its gains solve the 3 x 3 system that matches the
    Gaussian's zeroth and second moments and its value at the band edge."""
    radius = float(np.round(3.2795 * sigma + 0.2546))
    omega = np.array([1.0, 3.0, 5.0]) * np.pi / (2.0 * radius)
    p = np.array([1.0, -1.0, 1.0]) / np.tan(0.5 * omega)
    r = np.array([1.0, -1.0, 1.0]) * p * p / np.sin(omega)
    rho = np.exp(-0.5 * sigma * sigma * omega * omega) / radius
    d13 = p[0] * r[1] - r[0] * p[1]
    zeta_15 = (p[1] * r[2] - r[1] * p[2]) / d13
    zeta_35 = (p[2] * r[0] - r[2] * p[0]) / d13
    a = np.array([p, r, [zeta_15, zeta_35, 1.0]])
    gamma = np.array([1.0, radius * radius - sigma * sigma, zeta_15 * rho[0] + zeta_35 * rho[1] + rho[2]])
    beta = np.linalg.solve(a, gamma)
    n2 = -beta * np.cos(omega * (radius + 1.0))
    d1 = -2.0 * np.cos(omega)
    return int(radius), n2, d1


def recursive_blur_line(x: np.ndarray, sigma: float = SIGMA) -> np.ndarray:
    """The recursion along one line in fp64 (zero outside the line): each section is fed in[n-N-1] + in[n+N-1]."""
    radius, n2, d1 = recursive_gaussian(sigma)
    n_in = len(x)
    xp = np.concatenate([np.zeros(2 * radius), np.asarray(x, np.float64), np.zeros(2 * radius)])
    out = np.zeros(n_in)
    prev = np.zeros(3)
    prev2 = np.zeros(3)
    for n in range(-radius + 1, n_in):
        s = xp[n - radius - 1 + 2 * radius] + xp[n + radius - 1 + 2 * radius]
        o = n2 * s - d1 * prev - prev2
        prev2, prev = prev, o
        if n >= 0:
            out[n] = o.sum()
    return out


def taps(sigma: float = SIGMA) -> np.ndarray:
    """-> the 9 taps (offsets -4..4) of the recursion's impulse response, in fp64."""
    n = 41
    impulse = np.zeros(n)
    impulse[n // 2] = 1.0
    resp = recursive_blur_line(impulse, sigma)
    return resp[n // 2 - 4:n // 2 + 5].copy()


_TAPS = None


def _taps():
    global _TAPS
    if _TAPS is None:
        _TAPS = taps()
    return _TAPS


# ---- stages --------------------------------------------------------------------------------------------------------

def srgb_to_linear(v) -> np.ndarray:
    """8-bit sRGB code values (any shape) -> linear light in fp64."""
    v = np.asarray(v, np.float64) / 255.0
    return np.where(v <= SRGB_THRESHOLD, v / SRGB_SLOPE, ((v + SRGB_A) / (1.0 + SRGB_A)) ** SRGB_GAMMA)


def to_xyb(lin: np.ndarray) -> np.ndarray:
    """(3, h, w) linear RGB -> (3, h, w) positive XYB, fp64."""
    lin = np.asarray(lin, np.float64)
    cb = np.cbrt(OPSIN_BIAS)
    lms = []
    for row in OPSIN:
        mix = row[0] * lin[0] + row[1] * lin[1] + row[2] * lin[2] + OPSIN_BIAS
        lms.append(np.cbrt(np.maximum(mix, 0.0)) - cb)
    l, m, s = lms
    x = 0.5 * (l - m)
    y = 0.5 * (l + m)
    return np.stack([x * XYB_X_SCALE + XYB_X_OFFSET, y + XYB_Y_OFFSET, (s - y) + XYB_B_OFFSET])


def downsample2(plane: np.ndarray) -> np.ndarray:
    """2 x 2 box average of the last two axes, ceil(w / 2) x ceil(h / 2): an odd last row / column is replicated."""
    p = np.asarray(plane, np.float64)
    h, w = p.shape[-2:]
    if h % 2:
        p = np.concatenate([p, p[..., -1:, :]], axis=-2)
    if w % 2:
        p = np.concatenate([p, p[..., :, -1:]], axis=-1)
    return 0.25 * (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2])


def _blur_axis(p: np.ndarray, axis: int) -> np.ndarray:
    t = _taps()
    n = p.shape[axis]
    pad = [(0, 0)] * p.ndim
    pad[axis] = (4, 4)
    q = np.pad(p, pad)
    out = np.zeros_like(p)
    for k in range(9):
        out += t[k] * np.take(q, np.arange(k, k + n), axis=axis)
    return out


def blur(plane: np.ndarray) -> np.ndarray:
    """sigma-1.5 blur of a (h, w) plane: the 9 taps along rows, then along columns, zero outside the plane."""
    return _blur_axis(_blur_axis(np.asarray(plane, np.float64), 1), 0)


def weights() -> np.ndarray:
    from oracle.ssimu2_oracle import weights as checker_weights
    return checker_weights()


def weight_walk(nscales: int):
    """The published running weight index: -> [(weight, scale, stat)] in walk order, `stat` in the (6, 18) layout
    (0..5 ssim c*2+n, 6..17 edge 6+c*4+k with k = 0 artifact L1, 1 artifact L4, 2 detail-lost L1, 3 detail-lost L4).
    With fewer than six scales the weights are consumed contiguously (no gaps)."""
    wts = weights()
    out, i = [], 0
    for c in range(3):
        for s in range(nscales):
            for n in range(2):
                for stat in (c * 2 + n, 6 + c * 4 + n, 6 + c * 4 + n + 2):
                    out.append((float(wts[i]), s, stat))
                    i += 1
    return out


def weighted_sum(avg: np.ndarray, nscales: int) -> float:
    """sum w_i |a_i| over the walk: the value the score formula starts from."""
    return float(sum(w * abs(avg[s, st]) for w, s, st in weight_walk(nscales)))


def score_from_weighted_sum(x: float) -> float:
    x *= SCORE_SCALE
    p = POLY[0] * x + POLY[1] * x * x + POLY[2] * x * x * x
    return 100.0 - 10.0 * p ** EXPONENT if p > 0.0 else 100.0


def score_from_averages(avg: np.ndarray, nscales: int) -> float:
    return score_from_weighted_sum(weighted_sum(np.asarray(avg, np.float64).reshape(6, 18), nscales))


# ---- the whole operation -------------------------------------------------------------------------------------------

def _linear_planes(img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8
    return srgb_to_linear(np.moveaxis(img, 2, 0))


def scale_size(w: int, h: int, scale: int):
    """The size of `scale` of a w x h frame: halved `scale` times, rounding up.  The one halving rule of tests/."""
    for _ in range(scale):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def nscales_of(w: int, h: int) -> int:
    ns = 0
    while ns < NUM_SCALES and min(scale_size(w, h, max(ns - 1, 0))) >= MIN_SIZE:
        ns += 1
    return ns


def levels(lin1: np.ndarray, lin2: np.ndarray, scales) -> dict:
    """-> {scale: (lin1, lin2, xyb1, xyb2)} fp64 (3, h_s, w_s) planes at the scales asked for, from the scale-0 linear
    planes of both frames.  The front ends: fp64_checks.reference_levels (8-bit), hbd_ref.reference_levels (16-bit)."""
    out = {}
    for s in range(max(scales) + 1):
        if s:
            lin1, lin2 = downsample2(lin1), downsample2(lin2)
        if s in scales:
            out[s] = (lin1, lin2, to_xyb(lin1), to_xyb(lin2))
    return out


def evaluate(ref: np.ndarray, dist: np.ndarray, planes: bool = False) -> dict:
    """Score `dist` ((h, w, 3) uint8) against `ref`: evaluate_linear of their linear planes."""
    assert dist.shape == ref.shape
    return evaluate_linear(_linear_planes(ref), _linear_planes(dist), planes)


def evaluate_linear(lin1: np.ndarray, lin2: np.ndarray, planes: bool = False) -> dict:
    """Score two frames given as (3, h, w) fp64 linear planes, reference first.  -> {"score", "averages" (6, 18) in
    the checker's layout, "nscales", "weighted_sum"} and, with `planes`, "planes": one dict per scale of
    (3, h_s, w_s) fp64 arrays lin1, lin2, xyb1, xyb2, mu1, mu2, s11, s22, s12 (blurred products), d, artifact,
    detail_lost.  The one body of the fp64 route; hbd_ref.compute_fp64 feeds it 16-bit frames."""
    h, w = lin1.shape[1:]
    assert lin2.shape == lin1.shape
    avg = np.zeros((NUM_SCALES, 18))
    per_scale = []
    ns = nscales_of(w, h)
    for s in range(ns):
        if s:
            lin1, lin2 = downsample2(lin1), downsample2(lin2)
        x1, x2 = to_xyb(lin1), to_xyb(lin2)
        keep = {"lin1": lin1, "lin2": lin2, "xyb1": x1, "xyb2": x2} if planes else None
        if keep is not None:
            for k in ("mu1", "mu2", "s11", "s22", "s12", "d", "artifact", "detail_lost"):
                keep[k] = np.empty_like(x1)
        for c in range(3):                                   # one channel at a time: 4K stays near 1 GB
            a, b = x1[c], x2[c]
            mu1, mu2 = blur(a), blur(b)
            s11, s22, s12 = blur(a * a), blur(b * b), blur(a * b)
            sigma11, sigma22, sigma12 = s11 - mu1 * mu1, s22 - mu2 * mu2, s12 - mu1 * mu2
            num_m = 1.0 - (mu1 - mu2) ** 2
            num_s = 2.0 * sigma12 + C2
            den_s = sigma11 + sigma22 + C2
            d = np.maximum(0.0, 1.0 - num_m * num_s / den_s)
            del sigma11, sigma22, sigma12, num_m, num_s, den_s
            e = (1.0 + np.abs(b - mu2)) / (1.0 + np.abs(a - mu1)) - 1.0
            art, det = np.maximum(e, 0.0), np.maximum(-e, 0.0)
            avg[s, c * 2] = d.mean()
            avg[s, c * 2 + 1] = np.mean(d ** 4) ** 0.25
            avg[s, 6 + c * 4] = art.mean()
            avg[s, 6 + c * 4 + 1] = np.mean(art ** 4) ** 0.25
            avg[s, 6 + c * 4 + 2] = det.mean()
            avg[s, 6 + c * 4 + 3] = np.mean(det ** 4) ** 0.25
            if keep is not None:
                for k, v in (("mu1", mu1), ("mu2", mu2), ("s11", s11), ("s22", s22), ("s12", s12), ("d", d),
                             ("artifact", art), ("detail_lost", det)):
                    keep[k][c] = v
        del x1, x2
        if keep is not None:
            per_scale.append(keep)
    ws = weighted_sum(avg, ns)
    out = {"score": score_from_weighted_sum(ws), "averages": avg, "nscales": ns, "weighted_sum": ws}
    if planes:
        out["planes"] = per_scale
    return out


def error_map(ref: np.ndarray | None, dist: np.ndarray | None, result: dict | None = None, size=None):
    """The per-pixel error map of DESIGN.md section 9 in fp64: -> (map (h, w), evaluate()'s result).  Each average
    a_i of the walk is spread over its scale as w_i t for an L1 term and w_i t^4 / a_i^3 for an L4 term (0 when
    a_i == 0); map(x, y) = sum over scales of the scale's density at (x >> s, y >> s).  Without 8-bit frames (ref and
    dist None): `result` is evaluate_linear(..., planes=True) of any front end (hbd_ref.error_map_fp64) and `size` the
    frame's (h, w), all the map needs of the frames."""
    if ref is None:
        assert result is not None and "planes" in result and size is not None
        h, w = size
    else:
        h, w, _ = ref.shape
    if result is None or "planes" not in result:
        result = evaluate(ref, dist, planes=True)
    avg, ns = result["averages"], result["nscales"]
    coef = np.zeros((NUM_SCALES, 18))
    for wt, s, st in weight_walk(ns):
        a = avg[s, st]
        coef[s, st] = wt if st % 2 == 0 else (wt / a ** 3 if a > 0 else 0.0)
    m = np.zeros((h, w))
    ys, xs = np.arange(h), np.arange(w)
    for s, pl in enumerate(result["planes"]):
        dens = np.zeros(pl["d"].shape[1:])
        for c in range(3):
            for name, l1, l4 in (("d", c * 2, c * 2 + 1), ("artifact", 6 + c * 4, 6 + c * 4 + 1),
                                 ("detail_lost", 6 + c * 4 + 2, 6 + c * 4 + 3)):
                t = pl[name][c]
                dens += coef[s, l1] * t + coef[s, l4] * t ** 4
        m += dens[(ys >> s)[:, None], (xs >> s)[None, :]]
    return m, result
