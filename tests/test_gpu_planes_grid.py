"""The 8-bit front end on the MI355X, plane by plane on the size grid (-m gpu only).

tests/test_gpu_parity.py and tests/test_gpu_recursive.py hold the 8-bit planes to the checker at a few sizes; here every
size of gpu_cases.SIZES with w, h >= 8 runs on the instrumented build in all three modes, bit for bit against the
checker: the linear pyramid of both frames (k_pyramid_bands) through the FIR pair call, the cached XYB and
blur(ref * ref) planes after set_reference and set_reference_device, the distorted frame's pyramid after each cached FIR
pass (tight, strided RGBA rows with padding, enqueued from device memory), and the recursive planes after both passes
(k_pyramid_bands_xyb, k_rg_h, k_rg_v) at every scale through the pair call and a cached strided pass.

Every call follows a score of other content of a larger size (or, against a cached reference, a pass over the reference
itself), so the buffers it writes hold foreign bytes beyond the frame and other values inside it.  Device frames lie in
a torch allocation with 4 KiB of random bytes on either side, at a base offset of 0..3 mod 4 (cycled over the grid):
scores, averages and planes are the host path's bits.  An unaligned base adds no new kind of load: in the code objects,
k_pyramid_bands(_xyb) read the frame with global_load_dwordx3 (whole 4 x 4 blocks) and global_load_ubyte / _ushort
(clamped border blocks) and k_march with global_load_dword at byte offset 3 x of a row, and rows start at 3 w y, so odd
widths of the grid already issue each of them at every address mod 4.
"""
import numpy as np
import pytest

import errmap_ref
import gpu_cases
from gpu_cases import check_rg, ictx, in_margins, same_bits, stale  # noqa: F401  (ictx: a fixture)
from oavif_amd import synth

pytestmark = pytest.mark.gpu

LIN_REF, LIN_DIST, XYB_REF, REF_BLUR = 0, 1, 2, 3
RECURSIVE = [m for m in gpu_cases.MODES if m != "fir"]
GRID = [(w, h) for w, h in gpu_cases.SIZES if w >= 8 and h >= 8]
KINDS = ["gradient", "primaries", "checker", "text", "noise"]
DISTORTIONS = [("blockq", 2), ("noise", 2), ("blur", 1), ("band", 2)]


ictxs = gpu_cases.contexts_fixture(instrumented=True)


def frames(k):
    w, h = GRID[k]
    ref = gpu_cases.content(KINDS[k % 5], w, h, seed=k)
    dk, ds = DISTORTIONS[k % 4]
    return ref, synth.distort(ref, dk, ds, seed=k + 1)


@pytest.mark.parametrize("k", range(len(GRID)), ids=[f"{w}x{h}" for w, h in GRID])
def test_8bit_planes_on_the_size_grid_are_bit_identical(ictx, oracle, k):
    w, h = GRID[k]
    ref, dist = frames(k)
    off = k % 4
    lin_r, lin_d = [errmap_ref.scales(oracle, errmap_ref.linear_planes(oracle, f)) for f in (ref, dist)]
    ns = len(lin_r)
    xyb_r, xyb_d = [oracle.linear_to_xyb(x) for x in lin_r], [oracle.linear_to_xyb(x) for x in lin_d]
    _buf, view = gpu_cases.decoded_like(dist, 4, 5 + k, seed=k)
    t_ref, p_ref = in_margins(ref, off, 2 * k)
    t_dist, p_dist = in_margins(dist, (off + 1) % 4, 2 * k + 1)
    what = (w, h, KINDS[k % 5])

    def lin_levels(s, which, how):
        for sc in range(1, ns):
            if LIN_REF in which:
                same_bits(s.debug_download(LIN_REF, sc, w, h), lin_r[sc], what + (how, "lin ref", sc))
            same_bits(s.debug_download(LIN_DIST, sc, w, h), lin_d[sc], what + (how, "lin dist", sc))

    def ref_planes(s, how):
        for sc in range(ns):
            same_bits(s.debug_download(XYB_REF, sc, w, h), xyb_r[sc], what + (how, "xyb", sc))
            got = s.debug_download(REF_BLUR, sc, w, h)
            for c in range(3):
                exp = oracle.blur_product(xyb_r[sc][c], xyb_r[sc][c], oracle.BLUR_FIR)
                same_bits(got[c], exp, what + (how, "ref blur", sc, c))

    def same(s, score, pair, how):
        avg, n = s.last_averages()
        assert score == pair[0] and n == ns, what + (how, score, pair[0])
        assert np.array_equal(avg.view(np.uint64), pair[1].view(np.uint64)), what + (how,)

    # FIR: the pair call, the cached reference (host and device), cached passes through every hand-off
    s = ictx["fir"]
    stale(s, w, h, k)
    pair = (s.compute_ssimu2(ref, dist), s.last_averages()[0])
    assert s.last_averages()[1] == ns, what
    lin_levels(s, (LIN_REF, LIN_DIST), "pair")
    stale(s, w, h, k)
    same(s, s.score_device(p_ref, p_dist, w, h), pair, "score_device")
    lin_levels(s, (LIN_REF, LIN_DIST), "score_device")
    stale(s, w, h, k)
    s.set_reference(ref)
    ref_planes(s, "set_reference")
    same(s, s.score_against_reference(dist), pair, "cached")
    lin_levels(s, (LIN_DIST,), "cached")
    s.score_against_reference(ref)
    same(s, s.score_decoded_against_reference(view), pair, "strided")
    lin_levels(s, (LIN_DIST,), "strided")
    stale(s, w, h, k)
    s.set_reference_device(p_ref, w, h)
    ref_planes(s, "set_reference_device")
    s.score_against_reference(ref)
    s.enqueue_against_reference_device(p_dist)
    same(s, s.wait(), pair, "enqueue_against_reference_device")
    lin_levels(s, (LIN_DIST,), "enqueue_against_reference_device")

    # recursive modes: the planes after both passes, every scale, pair call and cached strided pass; the device
    # pair call at scale 0
    for mode in RECURSIVE:
        r, blur = ictx[mode], gpu_cases.MODES[mode][1]
        rpair = None
        for sc in range(ns):
            r.rg_stop_after_scale(sc)
            stale(r, w, h, k)
            score = r.compute_ssimu2(ref, dist)
            rpair = rpair or (score, r.last_averages()[0])
            same(r, score, rpair, (mode, "pair", sc))
            check_rg(r, oracle, blur, sc, w, h, xyb_r[sc], xyb_d[sc], what + (mode, "pair"))
            r.set_reference(ref)
            r.score_against_reference(ref)
            same(r, r.score_decoded_against_reference(view), rpair, (mode, "strided", sc))
            check_rg(r, oracle, blur, sc, w, h, xyb_r[sc], xyb_d[sc], what + (mode, "strided"))
        r.rg_stop_after_scale(0)
        stale(r, w, h, k)
        same(r, r.score_device(p_ref, p_dist, w, h), rpair, (mode, "score_device"))
        check_rg(r, oracle, blur, 0, w, h, xyb_r[0], xyb_d[0], what + (mode, "score_device"))
    del t_ref, t_dist
