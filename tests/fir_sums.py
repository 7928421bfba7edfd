"""k_march's summing order, restated on the CPU (oavif_amd/csrc/ssimu2_kernels.h: march_v, march_body, finalize_body).

A lane owns one column of a strip and adds its fp32 term into an fp32 accumulator that starts at 0, row after row
over the rows of its segment [y0, min(y0 + seg, h)).  Everything behind that -- the wave sum, the two half-strip waves
of a channel, the tiles' partials in k_finalize -- is fp64.  So a FIR average is fixed up to the order of an fp64 sum
by the terms, the plane's size and the segment rows alone: the strip width does not enter (a strip only says WHICH
lane owns a column), and lanes outside the image add 0.0.

For d and d^4 (statistics 0..5 of a scale) the kernel's terms are the reference's bits (div_rn is IEEE division), so
`means` of errmap_ref's term planes restates those six averages of a device score to `rtol`.  The edge statistics go
through v_rcp_f32 and keep the rounding bound of gpu_cases.fir_rtol.

`rtol`, in units of u = 2^-53, for a plane of w x h terms cut into segments of `seg` rows, N = w * ceil(h / seg)
accumulators:
  * the device's fp64 sum of N non-negative doubles (the accumulators convert exactly; zeros add nothing), in any
    order: every addend passes through at most N - 1 rounded additions, (N - 1) u;
  * v *= inv_pixels: inv_pixels is a rounded quotient and the product is rounded, 2 u.  An L1 average: N + 1;
  * an L4 average takes sqrt(sqrt(v)): a square root halves the relative error it is given and adds its own rounding,
    at most 1 ulp = 2 u each: (N + 1) / 4 + 2 / 2 + 2 <= N + 1 for N >= 5 (a scored plane has at least 8 columns);
  * the reference: the sum in extended precision (N * 2^-64, nothing here), one rounded division to fp64, 1 u, and
    for an L4 average the host's pow(., 0.25) within 1 ulp, 2 u: at most 3 u.
  Together at most (N + 4) u for either kind of average; second-order terms are below N^2 u^2 < 1e-20.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def accumulators(t: np.ndarray, seg: int) -> np.ndarray:
    """(nsegs, w) float32: per segment of `seg` rows and per column, acc = acc + t[y] in row order from 0.0."""
    t = np.asarray(t)
    assert t.dtype == F32 and t.ndim == 2 and seg >= 1
    h, w = t.shape
    nsegs = (h + seg - 1) // seg
    acc = np.zeros((nsegs, w), F32)
    for r in range(min(seg, h)):
        ys = np.arange(nsegs) * seg + r
        live = ys < h                       # the last segment may be shorter
        acc[live] = acc[live] + t[ys[live]]
    return acc


def accumulators_scalar(t: np.ndarray, seg: int) -> np.ndarray:
    """`accumulators` as the plain loop a lane runs: one column at a time, one np.float32 add per row."""
    h, w = t.shape
    nsegs = (h + seg - 1) // seg
    acc = np.zeros((nsegs, w), F32)
    for x in range(w):
        for k in range(nsegs):
            a = F32(0.0)
            for y in range(k * seg, min(k * seg + seg, h)):
                a = F32(a + t[y, x])
            acc[k, x] = a
    return acc


def mean_of(acc: np.ndarray, pixels: int) -> float:
    """The fp64 mean the accumulators give: their sum in extended precision over the plane's pixel count."""
    return float(acc.astype(np.float64).sum(dtype=np.longdouble) / pixels)


def means(d: np.ndarray, d4: np.ndarray, seg: int):
    """-> (the L1 average of d, the L4 average of d^4's terms) of one channel and scale in the kernel's order."""
    n = d.size
    return mean_of(accumulators(d, seg), n), mean_of(accumulators(d4, seg), n) ** 0.25


def rtol(w: int, h: int, seg: int) -> float:
    """The bound of a device average 0..5 against `means` over a w x h plane in segments of `seg` rows (derivation in
    the module docstring)."""
    return (w * ((h + seg - 1) // seg) + 4) * 2.0 ** -53
