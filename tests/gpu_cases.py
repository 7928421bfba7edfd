"""Test-side helpers shared by the GPU modules.  This module owns:

* the blur-mode table (scorer mode -> the checker's mode of the same blur) and the per-mode context fixtures every GPU
  module builds its `ctxs` / `ictxs` / `ictx` on (mode_contexts, contexts_fixture, ictx);
* 8-bit content: the synthetic kinds, the pairs that reach the clamps and the zero paths, libavif-like padded RGB(A)
  layouts (16-bit content and layouts: tests/hbd_cases.py);
* the one hold of a score's averages to a reference (hold_averages) and the one bound of a FIR average
  (averages_rtol), with their callers: check_against_terms (averages and k_finalize against the kernel-order terms),
  check_fir_sums (the FIR d / d^4 averages against k_march's own summing order, tests/fir_sums.py) and
  check_item_against_terms (a batch item); the error-map check against tests/errmap_ref.py (check_map; the same rule
  for maps of 16-bit, RGBA and YUV frames: tests/map_cases.py);
* what the batch modules share: the batch rule's rows, seeded neighbours, the comparison of score and averages for
  bits, frames packed into one device buffer (on_device) and the golden pair's bits (golden_bits);
* what puts foreign content around a call: a stale pair score of a larger size (stale), the cached reference scored
  against itself (scrub) and device frames between margins of random bytes (in_margins).

The references themselves live elsewhere: tests/errmap_ref.py (the fp32 checker route), tests/ssimu2_fp64.py (fp64;
its scale_size is the one halving rule), tests/hbd_ref.py (their 16-bit front ends)."""
from __future__ import annotations

import numpy as np
import pytest

from oavif_amd import Ssimu2, _lib, synth
from oracle import ssimu2_oracle as orc

import errmap_ref
import fir_sums
from ssimu2_fp64 import scale_size

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
    (119, 40), (120, 40), (121, 40), (241, 33),                  # strip edges of k_ref_blur and the map kernels (120 columns;
                                                                 # the summing kernels' 128: tests/wide_cases.py and its modules)
    (64, 20), (65, 21), (128, 19), (129, 41),                    # recursive tile (64 columns) and batch edges
    (333, 217), (513, 259), (1921, 1083),                        # ragged
    (9, 1000), (1000, 9), (4000, 8), (8, 4000),                  # very tall, very wide
]


def mode_contexts(**kw):
    """Yields {mode name: Ssimu2(0, blur=that mode, **kw)} over MODES and closes the contexts afterwards."""
    out = {name: Ssimu2(0, blur=mode, **kw) for name, (mode, _) in MODES.items()}
    yield out
    for s in out.values():
        s.close()


def contexts_fixture(**kw):
    """A module-scoped fixture of mode_contexts(**kw) (plain, instrumented=True or extended=True), to be bound to the
    fixture's name in the module that uses it: `ctxs = contexts_fixture()`.  Each module gets contexts of its own."""
    @pytest.fixture(scope="module")
    def contexts(hip_lib):
        yield from mode_contexts(**kw)
    return contexts


@pytest.fixture()
def ictx(ictxs):
    """The importing module's `ictxs` (contexts_fixture(instrumented=True)) for one test: the recursive contexts' debug
    stop (rg_stop_after_scale) is cleared when the test ends, whatever its outcome, so a failure stays in its own test."""
    yield ictxs
    for m in MODES:
        if m != "fir":
            ictxs[m].rg_stop_after_scale(-1)


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


def extreme_pairs():
    h, w = 70, 90
    black = np.zeros((h, w, 3), np.uint8)
    white = np.full((h, w, 3), 255, np.uint8)
    noise = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return [(black, white), (white, black), (noise, black), (black, noise), (noise, noise[::-1].copy())]


def flat_pairs():
    out = []
    for v in (0, 255):
        flat = np.full((96, 80, 3), v, np.uint8)
        out += [(flat, flat), (flat, synth.distort(flat, "noise", 2, seed=v)),
                (synth.distort(flat, "noise", 3, seed=v + 1), flat)]
    return out


def content_pairs(kind):
    ref = content(kind, 250, 190, 5)
    return [(ref, synth.distort(ref, dk, ds, seed=3)) for dk, ds in [("blur", 0), ("band", 2), ("noise", 2)]]


def one_sample_pairs():
    """333 x 217 frames that differ in a single sample: one step, and black to white."""
    ref = synth.make_ref(333, 217, seed=9)
    out = []
    for to in (int(ref[100, 200, 1]) ^ 1, 255 if ref[100, 200, 1] < 128 else 0):
        dist = ref.copy()
        dist[100, 200, 1] = to
        out.append((ref, dist))
    return out


# content that reaches the clamps and the zero paths: most of the 108 averages exactly 0, L4 coefficients up to 3e27,
# map densities from 1e-15 to 1e3, fourth powers close to the subnormal range
HARD_GROUPS = ["extreme", "flat", "content-gradient", "content-primaries", "content-checker", "content-text",
               "content-noise", "one-sample"]


def group_pairs(group):
    fixed = {"extreme": extreme_pairs, "flat": flat_pairs, "one-sample": one_sample_pairs}
    return fixed[group]() if group in fixed else content_pairs(group[len("content-"):])


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


# ---- the averages and k_finalize against the kernel-order terms (DESIGN.md sections 2.3 and 9) --------------------
#
# errmap_ref.kernel_averages(...) are the means, in fp64, of the very fp32 terms the score kernels sum: the terms are
# computed from the checker's planes (which the kernels match bit for bit) by the kernels' expressions in their order.
# What separates a device average from it is then only how the kernels add the terms up:
#
# * k_finalize: score = the published polynomial of sum_j w_j |avg_j| (oavif_amd/csrc/ssimu2_kernels.h).  Given the
#   device's own averages, oracle.score_from_averages differs from it only in the order of that fp64 sum (a shuffle
#   tree against a running sum: ~1e-16 relative) and in device against host pow(): FINALIZE_TOL.  No scale: 100 exactly.
# * Recursive modes: k_rg_v sums each fp32 term converted to fp64 (rg_v_body, ssimu2_recursive.h), per lane,
#   then over lanes, waves and column groups, and k_finalize over the groups' partials, all in fp64; the reference
#   takes the mean in extended precision.  A sum of n non-negative values in fp64, in any order, is within (n - 1) *
#   2^-53 of the exact sum, relatively; the division by the pixel count and the two square roots of an L4 norm add a
#   few units of 2^-53 (a 4th root divides a relative error by 4).  n <= 3840 * 2160 = 8.3 M terms per average gives
#   8.3e6 * 2^-53 = 9.2e-10 < RTOL_RECURSIVE = 1e-9.  An average is 0 exactly where all its terms are.
# * FIR: k_march sums each term in fp32 per lane down the rows of its segment (at most march_seg_rows rows), then in
#   fp64 (march_body).  A sum of `seg` non-negative fp32 values is within (seg - 1) * 2^-24 of the exact one.  The
#   edge quotient is (ea - eb) * rcp(1 + eb) (march_v): rcp within 1 ulp (2^-23 relative) and the product rounded
#   (2^-24), against the correctly rounded quotient of the reference (2^-24): art and det within 4 * 2^-24, their 4th
#   powers within 4 * 4 + 3 + 3 = 22 units (two squarings on each side), 22 / 4 = 5.5 units after an L4 norm's 4th
#   root.  d and d^4 are the reference's bits.  Per average: (seg - 1 + 4) * 2^-24 for an L1 statistic,
#   (seg - 1 + 22) / 4 * 2^-24 <= (seg + 3) * 2^-24 for an L4 one (seg >= 8); plus the fp64 part, n * 2^-53.
#   That bound lets pass whatever moves a sum by less than a few 1e-6 of it -- a term lost at a strip or segment corner
#   of a large frame, say.  The d and d^4 statistics (0..5) need no rounding bound: their terms are the reference's
#   bits, so summing them in the kernel's own order (tests/fir_sums.py) leaves only the order of the fp64 part,
#   (w_s * ceil(h_s / seg) + 4) * 2^-53 (derived there): check_fir_sums.  The edge statistics share the accumulator
#   loop, the masks, the reduction and the partial index with them, and keep the bound above.
FINALIZE_TOL = 1e-11
RTOL_RECURSIVE = 1e-9
MAX_TERMS = 3840 * 2160
MW = 120        # the segment rule's column unit (kSegRuleCols) and the strip width of k_ref_blur and the map kernels
WIDE_MW = 128   # output columns per strip of the kernels that leave partial sums (ssimu2_kernels.h, MarchWide)


def march_seg_rows(w: int, h: int, scale: int) -> int:
    """Rows per k_march workgroup at `scale` of a w x h frame: march_seg_rows in oavif_amd/csrc/ssimu2_hip.hip (no
    ssimu2_instr_set_segment_rows override): ~512 workgroups at full resolution, 8..160 rows, at most 48 below it."""
    nstrips = (w + MW - 1) // MW
    nsegs = max(1, (512 + nstrips // 2) // nstrips)
    seg = min(max((h + nsegs - 1) // nsegs, 8), 160)
    return min(seg, 48) if scale > 0 else seg


def averages_rtol(w_s: int, h_s: int, rows: int) -> float:
    """The bound of a FIR average of a w_s x h_s scale whose lanes sum at most `rows` fp32 terms each (derivation
    above): (rows + 3) * 2^-24 for the fp32 part, one unit of 2^-53 per pixel for the fp64 part."""
    return (rows + 3) * 2.0 ** -24 + w_s * h_s * 2.0 ** -53


def fir_rtol(w: int, h: int, scale: int) -> float:
    """averages_rtol at `scale` of a w x h frame under the single-score rule (rows not clamped to the scale's height)."""
    return averages_rtol(*scale_size(w, h, scale), march_seg_rows(w, h, scale))


def rows_rtol(w: int, h: int, scale: int, rows: int) -> float:
    """averages_rtol for segments of `rows` rows set by hand (ssimu2_instr_set_segment_rows): a lane sums at most
    min(rows, rows of the scale) terms."""
    sw, sh = scale_size(w, h, scale)
    return averages_rtol(sw, sh, min(rows, sh))


def seg_rows(w: int, h: int, rule=march_seg_rows):
    """Rows per k_march segment at each of the six scales of a w x h frame under `rule` (march_seg_rows, batch_seg_rows;
    both take the frame's FULL size)."""
    return [rule(w, h, s) for s in range(6)]


def override_rows(rows_scale0: int, rows_other_scales: int):
    """seg_rows under ssimu2_instr_set_segment_rows(rows_scale0, rows_other_scales), neither 0."""
    return [rows_scale0] + [rows_other_scales] * 5


def hold_averages(avg, exp, ns, rtol_of, what, each_scale=False):
    """The one hold of a score's averages `avg` (6, n) to a reference's `exp` over `ns` scales: 0 exactly where the
    reference is 0 (at every scale, scored or not), and at each scored scale s the relative deviation within
    rtol_of(s).  `each_scale`: print every scale's deviation and bound before asserting it.  -> the largest deviation
    in units of its bound."""
    assert avg.shape == exp.shape and len(avg) == 6, what
    worst = 0.0
    for s in range(6):
        got, e = avg[s], exp[s]
        assert np.array_equal(got == 0, e == 0), (what, s, got, e)
        if s >= ns:
            continue
        rtol = rtol_of(s)
        dev = np.abs(got - e) / np.where(e == 0, 1.0, e)
        if each_scale:
            print(f"measured: {what} scale {s}: {float(dev.max()):.3e} (bound {rtol:.3e})")
        assert (dev <= rtol).all(), (what, s, int(np.argmax(dev)), float(dev.max()), rtol)
        worst = max(worst, float(dev.max()) / rtol)
    return worst


def check_fir_sums(avg, ns, w, h, kord, rows, what):
    """FIR averages 0..5 (the d and d^4 statistics, whose terms are the reference's bits) of every scale of a w x h
    frame against `kord`, the same terms summed in k_march's own order at `rows` rows per segment (errmap_ref's
    seg_rows results): within fir_sums.rtol, the order of an fp64 sum, and 0 exactly where the reference is 0.  The edge
    statistics stay with check_against_terms.  -> the largest deviation in units of its bound."""
    assert avg.shape == (6, 18) and kord.shape == (6, 6), what
    worst = hold_averages(avg[:, :6], kord, ns, lambda s: fir_sums.rtol(*scale_size(w, h, s), rows[s]), what)
    print(f"measured: {what}: kernel-order sums {worst:.3e} of the bound")
    return worst


def check_against_terms(oracle, score, avg, ns, ref, dist, mode, what, kavg=None, rows=None):
    """A device score of (ref, dist) in scorer mode `mode` (a key of MODES), its averages `avg` over `ns` scales:
    k_finalize against oracle.score_from_averages(avg) to FINALIZE_TOL, and every average against
    errmap_ref.kernel_averages (or `kavg`, the same computed by the caller) to RTOL_RECURSIVE in the recursive modes,
    fir_rtol in FIR (rows_rtol where `rows`, an override's segment rows by scale, are given), exactly 0 where the
    reference is 0.  -> the largest deviation of an average in units of its bound (0 without a scale)."""
    h, w, _ = ref.shape
    assert w * h <= MAX_TERMS, what
    if ns == 0:
        assert score == 100.0 and not avg.any(), what
        return 0.0
    host = oracle.score_from_averages(avg, ns)
    assert abs(score - host) <= FINALIZE_TOL, (what, score, host)
    if kavg is None:
        kavg, ns_r = errmap_ref.kernel_averages(oracle, ref, dist, MODES[mode][1])
        assert ns_r == ns, what
    assert avg.shape == kavg.shape == (6, 18), what

    def rtol_of(s):
        if mode != "fir":
            return RTOL_RECURSIVE
        return fir_rtol(w, h, s) if rows is None else rows_rtol(w, h, s, rows[s])
    worst = hold_averages(avg, kavg, ns, rtol_of, what)
    print(f"measured: {what}: averages {worst:.3e} of the bound, finalize "
          f"{abs(score - host):.1e}")
    return worst


# ---- the error map -----------------------------------------------------------------------------------------------
#
# Recursive modes: k_rg_vmap forms the reference's terms (edge_quotient<true>: div_rn for both quotients), map_density and
# k_map_compose restate compose()'s order, and the coefficients are the host's: the map equals the reference bit for
# bit.  FIR: k_march_map shares march_v's edge quotient, (ea - eb) * rcp(1 + eb).  All terms and coefficients are
# non-negative, so relative errors add without cancellation, per pixel, in units of 2^-24:
#   art, det            4   (rcp 1 ulp = 2 units, the product 1, the reference's quotient 1)
#   art^4, det^4       22   (4 * 4, and two squarings on each side)
#   density chain      12   (one product and five FMAs, 6 roundings on each side)
#   channel sum         4   ((X + Y) + B: 2 roundings on each side)
#   sum over scales    10   (up to 6 scales: 5 roundings on each side)
# K = 48: every FIR pixel within K * 2^-24 of the reference's value (2^-126 below the normal range), and 0 exactly
# where the reference is 0.
MAP_K = 48


def check_map(oracle, m, avg, ns, ref, dist, blur, what):
    """The device map `m` of (ref, dist), whose score left averages `avg` over `ns` scales, against the numpy
    reference in the checker's mode `blur`: bit for bit in the recursive modes; in FIR per pixel within
    MAP_K * 2^-24 of the reference pixel, and 0 where it is 0; the mean to MEAN_RTOL.  -> the FIR map's largest
    relative deviation in units of 2^-24 (0 in the recursive modes) and the averages of the reference's terms (those
    of errmap_ref.kernel_averages, for check_against_terms)."""
    exp, own, ns_r = errmap_ref.reference_map(oracle, ref, dist, blur, avg=avg)
    assert ns == ns_r and m.shape == exp.shape and m.dtype == np.float32, what
    mean_e = exp.mean(dtype=np.float64)
    rel_mean = abs(m.mean(dtype=np.float64) - mean_e) / max(mean_e, 1e-30)
    assert rel_mean <= errmap_ref.MEAN_RTOL, (what, rel_mean)
    if blur != oracle.BLUR_FIR:
        bad = m.view(np.uint32) != exp.view(np.uint32)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        return 0.0, own
    assert np.array_equal(m == 0, exp == 0), (what, int(np.sum((m == 0) != (exp == 0))))
    units = np.abs(m.astype(np.float64) - exp) / np.maximum(exp.astype(np.float64), 2.0 ** -126) * 2.0 ** 24
    worst = float(units.max()) if units.size else 0.0
    assert worst <= MAP_K, (what, worst, np.unravel_index(int(np.argmax(units)), units.shape))
    print(f"measured: {what}: FIR map {worst:.2f} units of 2^-24 (K = {MAP_K})")
    return worst, own


def same_bits(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32, (what, got.shape, exp.shape)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), what


# ---- batch scoring (tests/test_gpu_score_batch.py, tests/test_gpu_batch_items.py) --------------------------------
KINDS = ("gradient", "primaries", "checker", "text", "noise")


def batch_seg_rows(w, h, scale):
    """batch_seg_rows of oavif_amd/csrc/ssimu2_hip.hip: a function of the scale alone."""
    return 96 if scale == 0 else 48


def batch_rtol(w, h, scale):
    """rows_rtol at the batch rule's rows (derivation: tests/test_gpu_score_batch.py's docstring)."""
    return rows_rtol(w, h, scale, batch_seg_rows(w, h, scale))


def bits_equal(score_a, avg_a, score_b, avg_b, what):
    """Score and all 108 averages: the same bits (same_bits over the doubles' 32-bit halves)."""
    a = np.concatenate([[score_a], np.asarray(avg_a, np.float64).ravel()])
    b = np.concatenate([[score_b], np.asarray(avg_b, np.float64).ravel()])
    same_bits(np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32), what)


def damaged(ref, seed):
    kind, strength = (("blockq", 4), ("noise", 3), ("blur", 2), ("blockq", 1))[seed % 4]
    return synth.distort(ref, kind, strength, seed=seed)


def neighbours(w, h, n, seed):
    """n seeded pairs of every content kind, some identical, some heavily damaged."""
    refs, dists = [], []
    for k in range(n):
        r = content(KINDS[(k + seed) % len(KINDS)], w, h, seed * 100 + k)
        refs.append(r)
        dists.append(r.copy() if k % 5 == 4 else damaged(r, seed + k))
    if n >= 8:
        dists[0] = 255 - refs[0]   # as damaged as a frame gets
    return refs, dists


def check_item_against_terms(oracle, score, avg, ns, ref, dist, what, kavg=None):
    """A batch item's score of (ref, dist) and its averages over `ns` scales: k_finalize_batch against
    oracle.score_from_averages(avg) to FINALIZE_TOL, every average against errmap_ref.kernel_averages in FIR (or `kavg`,
    the kernel-order averages computed by the caller) to batch_rtol, exactly 0 where the reference is 0.  -> the largest
    deviation in units of its bound."""
    h, w, _ = ref.shape
    if ns == 0:
        assert score == 100.0 and not avg.any(), what
        return 0.0
    if kavg is None:
        kavg, ns_r = errmap_ref.kernel_averages(oracle, ref, dist, MODES["fir"][1])
        assert ns_r == ns, what
    host = oracle.score_from_averages(avg, ns)
    print(f"measured: {what}: finalize {abs(score - host):.1e}")
    assert abs(score - host) <= FINALIZE_TOL, (what, score, host)
    assert avg.shape == kavg.shape == (6, 18), what
    return hold_averages(avg, kavg, ns, lambda s: batch_rtol(w, h, s), what, each_scale=True)


def on_device(frames, stride):
    """The uint8 frames in one device buffer (a torch tensor), frame k at byte k * stride, zeros between them."""
    import torch
    buf = torch.zeros(len(frames) * stride, dtype=torch.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + f.size] = torch.from_numpy(f.reshape(-1))
    buf = buf.cuda()
    torch.cuda.synchronize()
    return buf


def golden_bits(s, golden):
    """(score, averages) of the golden fixture's blockq2 pair on context `s`: what a refused call must leave as it was."""
    arrays, _ = golden
    score = s.compute_ssimu2(arrays["ref"], arrays["blockq2"])
    avg, _ns = s.last_averages()
    return score, avg


def rg_planes(oracle, blur, xa, xb):
    """The 15 planes (5 * channel + {x, y, xx, yy, xy}) of the checker's recursion over two XYB plane sets."""
    out = []
    for c in range(3):
        a, b = xa[c], xb[c]
        out += [oracle.blur_plane(src, blur) for src in (a, b, a * a, b * b, a * b)]
    return out


def check_rg(s, oracle, blur, scale, w, h, xa, xb, what):
    """The instrumented build's planes after both recursive passes at `scale` (ssimu2_debug_download RG_V = 5) against
    the checker's recursion in mode `blur` over the XYB planes xa (reference) and xb, bit for bit."""
    got = s.debug_download(5, scale, w, h)
    for k, exp in enumerate(rg_planes(oracle, blur, xa, xb)):
        same_bits(got[k], exp, what + (scale, k))


# ---- foreign content around a call (tests/test_gpu_planes_grid.py, tests/test_gpu_hbd_planes.py,
# tests/test_gpu_long_frames.py) ---------------------------------------------------------------------------------------
MARGIN = 4096


def stale_pair(w, h, k):
    """Other content of a larger size than (w, h), and a noisy copy of it."""
    big = content(KINDS[(k + 2) % 5], w + 41, h + 23, 1000 + k)
    return big, synth.distort(big, "noise", 3, seed=k)


def stale(s, w, h, k, pair=None):
    """A pair score of other content at a larger size (`pair`: stale_pair(w, h, k), kept by the caller): the context's
    buffers then hold its bytes beyond any (w, h) frame and other values inside it."""
    big, noisy = pair or stale_pair(w, h, k)
    s.compute_ssimu2(big, noisy)


def scrub(s, ref, bits=None):
    """Score the cached reference against itself, so that every buffer a later pass writes (the 8-bit frame the strided
    hand-off unpacks into, the 16-bit scale-0 planes and pyramid) holds other content: a pass that skipped rows would
    then score differently instead of finding the previous call's data in place."""
    return s.score_against_reference(ref) if bits is None else s.score_against_reference_hbd(ref, bits)


def in_margins(frame, off, seed):
    """`frame` on the device inside a uint8 torch buffer: MARGIN random bytes, then `off` more, the frame, MARGIN random
    bytes.  -> (buffer, device address of the frame's first byte)."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1))
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, 256, (2 * MARGIN + off + flat.numel(),), dtype=torch.uint8, generator=g)
    buf[MARGIN + off:MARGIN + off + flat.numel()] = flat
    buf = buf.cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 4 == 0
    return buf, buf.data_ptr() + MARGIN + off


def pseudo_codec(ref):
    """Deterministic stand-in for encode(q) -> decode: coarser block quantisation for lower q."""
    def codec(q):
        step = 1 + (100 - q) // 3
        dec = (ref.astype(np.int32) // step) * step + step // 2
        return np.clip(dec, 0, 255).astype(np.uint8), 1000 + 10 * q
    return codec
