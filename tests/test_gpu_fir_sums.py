"""k_march's sums against their own order (-m gpu only; FIR mode).

gpu_cases.check_against_terms holds a FIR average to a rounding bound, (seg + 3) * 2^-24 of the exact mean of its
terms: 2.4e-6 at 1921 x 1083, which a few terms lost or counted twice at a strip or segment corner stay below
(tests/test_fir_sums.py).  The d and d^4 averages (0..5 of every scale) need no rounding bound: their terms are the
reference's bits, the kernel's order of adding them is fixed and restated in tests/fir_sums.py, and what is left is
the order of an fp64 sum, (w_s * ceil(h_s / seg) + 4) * 2^-53: gpu_cases.check_fir_sums.  The edge statistics, whose
quotient goes through v_rcp_f32, share the accumulator loop, the masks, the reduction and the partial index with them
and keep the bound they had.

Here: the size grid (k_march, and k_march_refblur by bit equality), about 500 tiles in the XCD tile order without a
large frame, content that drives most averages to exactly 0 and fourth powers towards the subnormal range, segment
rows set by hand, batch items at the batch rule's rows (k_march_batch) and the 16-bit front end (k_march_lin).  The
4K pair is test_gpu_mode_matrix.py's."""
import os
import sys

import numpy as np
import pytest

from oavif_amd import Ssimu2Error, _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import gpu_cases  # noqa: E402
import hbd_ref  # noqa: E402
from gpu_cases import MW, bits_equal, check_against_terms, check_fir_sums  # noqa: E402
from hbd_cases import hbd_content, hbd_distort  # noqa: E402

pytestmark = pytest.mark.gpu

SCORED = [s for s in gpu_cases.SIZES if min(s) >= 8]


def _hold(oracle, score, avg, ns, ref, dist, what, rows=None):
    """A FIR score of the 8-bit pair: averages 0..5 to the kernel-order sums at `rows` (default: the single-score
    rule), every average and k_finalize as check_against_terms holds them.  -> the sums' worst share of their bound."""
    h, w, _ = ref.shape
    own = rows is not None
    rows = rows if own else gpu_cases.seg_rows(w, h)
    kavg, ns_r, kord = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=rows)
    assert ns == ns_r >= 1, what
    worst = check_fir_sums(avg, ns, w, h, kord, rows, what)
    check_against_terms(oracle, score, avg, ns, ref, dist, "fir", what, kavg=kavg, rows=rows if own else None)
    return worst


def _pair_score(s, ref, dist):
    score = s.compute_ssimu2(ref, dist)
    avg, ns = s.last_averages()
    return score, avg, ns


def _against_reference_has_the_pair_s_bits(s, ref, dist, score, avg, ns, what):
    s.set_reference(ref)
    again = s.score_against_reference(dist)
    avg_r, ns_r = s.last_averages()
    assert ns_r == ns, what
    bits_equal(again, avg_r, score, avg, f"{what}: score_against_reference")


@pytest.mark.parametrize("w,h", SCORED, ids=[f"{w}x{h}" for w, h in SCORED])
def test_size_grid(scorer, oracle, w, h):
    """Every size of the grid with a scale: k_march's sums in their order; k_march_refblur returns the same bits."""
    ref = synth.make_ref(w, h, 17 * w + h)
    dist = synth.distort(ref, "noise", 2, seed=w + 3 * h)
    score, avg, ns = _pair_score(scorer, ref, dist)
    _hold(oracle, score, avg, ns, ref, dist, f"grid {w}x{h}")
    _against_reference_has_the_pair_s_bits(scorer, ref, dist, score, avg, ns, f"grid {w}x{h}")


@pytest.mark.parametrize("w,h,strips,segs,seg", [(1000, 700, 9, 54, 13), (1921, 1083, 17, 30, 37)])
def test_many_tiles_without_a_large_frame(scorer, oracle, w, h, strips, segs, seg):
    """About 500 scale-0 tiles, dealt to the XCDs in runs (march_tile_of_block): a partial that lands in another
    tile's slot or a tile computed twice moves a sum by about 1 / 500 of it."""
    assert gpu_cases.march_seg_rows(w, h, 0) == seg
    assert ((w + MW - 1) // MW, (h + seg - 1) // seg) == (strips, segs) and 450 < strips * segs < 520
    ref = synth.make_ref(w, h, seed=3)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    score, avg, ns = _pair_score(scorer, ref, dist)
    assert ns == 6
    _hold(oracle, score, avg, ns, ref, dist, f"many tiles {w}x{h}")
    _against_reference_has_the_pair_s_bits(scorer, ref, dist, score, avg, ns, f"many tiles {w}x{h}")


@pytest.mark.parametrize("group", gpu_cases.HARD_GROUPS)
def test_content_that_hits_the_clamps(scorer, oracle, group):
    """Black against white, flat against noise, saturated primaries, a 1-px checkerboard, thin text, one sample
    flipped: most averages exactly 0 (the device's must be 0 there too), d^4 close to the subnormal range."""
    worst, zeros = 0.0, 0
    for i, (ref, dist) in enumerate(gpu_cases.group_pairs(group)):
        what = f"content {group} {i}"
        score, avg, ns = _pair_score(scorer, ref, dist)
        if np.array_equal(ref, dist):
            assert score == 100.0 and not avg.any(), what
        worst = max(worst, _hold(oracle, score, avg, ns, ref, dist, what))
        if score != 100.0:
            zeros = max(zeros, int(np.sum(avg == 0)))
        _against_reference_has_the_pair_s_bits(scorer, ref, dist, score, avg, ns, what)
    print(f"measured: content {group}: kernel-order sums {worst:.3e} of the bound, up to {zeros} of the 108 averages exactly 0 on a damaged pair")


def test_identical_frames_give_100_and_zero_averages(scorer, oracle):
    ref = synth.make_ref(333, 217, seed=9)
    score, avg, ns = _pair_score(scorer, ref, ref.copy())
    assert score == 100.0 and ns == 6 and not avg.any()
    _kavg, _ns, kord = errmap_ref.kernel_averages(oracle, ref, ref, oracle.BLUR_FIR, seg_rows=gpu_cases.seg_rows(333, 217))
    assert not kord.any()


@pytest.mark.parametrize("seg,tail", [(8, 8), (13, 21), (47, 160), (160, 9), (1, 1)])
def test_segment_rows_set_by_hand(iscorer, oracle, seg, tail):
    """ssimu2_instr_set_segment_rows regroups the sums; each setting is restated with its own rows.  Rows outside
    8..160 are refused (include/ssimu2_hip_internal.h) and leave the rule in force: (1, 1) is held at the rule's rows."""
    s = iscorer
    w, h = 333, 217
    ref = synth.make_ref(w, h, seed=41)
    dist = synth.distort(ref, "blockq", 2, seed=42)
    try:
        if seg < 8 or tail < 8:
            with pytest.raises(Ssimu2Error) as ei:
                s.set_segment_rows(seg, tail)
            assert ei.value.code == _lib.ERR_INVALID_ARG
            rows = None
        else:
            s.set_segment_rows(seg, tail)
            rows = gpu_cases.override_rows(seg, tail)
        score, avg, ns = _pair_score(s, ref, dist)
        assert ns == 6
        _hold(oracle, score, avg, ns, ref, dist, f"override ({seg}, {tail}) {w}x{h}", rows=rows)
    finally:
        s.set_segment_rows(0, 0)


@pytest.mark.parametrize("w,h", [(509, 131), (121, 40), (256, 192)])
def test_batch_items_at_the_batch_rule_s_rows(scorer, oracle, w, h):
    """k_march_batch: 7 items of every content kind, one identical pair among them, each item's averages 0..5 against
    its own terms summed at 96 / 48 rows, the rest as gpu_cases.check_item_against_terms holds a batch item."""
    refs, dists = gpu_cases.neighbours(w, h, 7, seed=w)
    rows = gpu_cases.seg_rows(w, h, gpu_cases.batch_seg_rows)
    assert rows == [96] + [48] * 5
    scores = scorer.score_batch(refs, dists)
    worst = 0.0
    for k in range(7):
        what = f"batch {w}x{h} item {k}"
        avg, ns = scorer.last_batch_averages(k)
        if k == 4:
            assert np.array_equal(refs[k], dists[k]) and scores[k] == 100.0 and not avg.any(), what
        kavg, ns_r, kord = errmap_ref.kernel_averages(oracle, refs[k], dists[k], oracle.BLUR_FIR, seg_rows=rows)
        assert ns == ns_r >= 1, what
        worst = max(worst, check_fir_sums(avg, ns, w, h, kord, rows, what))
        gpu_cases.check_item_against_terms(oracle, scores[k], avg, ns, refs[k], dists[k], what, kavg=kavg)
    print(f"measured: batch {w}x{h}: kernel-order sums {worst:.3e} of the bound")


def test_the_16_bit_front_end(scorer, oracle):
    """k_march_lin: scale 0 from the linear planes of a 12-bit pair; the terms are hbd_ref's."""
    w, h, depth = 333, 217, 12
    ref = hbd_content("text", w, h, depth, seed=12)
    dist = hbd_distort(ref, depth, seed=112)
    score = scorer.compute_ssimu2_hbd(ref, dist, depth)
    avg, ns = scorer.last_averages()
    rows = gpu_cases.seg_rows(w, h)
    tm = hbd_ref.terms(oracle, hbd_ref.linear_planes(ref, depth), hbd_ref.linear_planes(dist, depth), oracle.BLUR_FIR)
    kavg, kord = errmap_ref.averages(tm, rows)
    assert ns == len(tm) == 6
    what = f"16-bit front end, {depth}-bit {w}x{h}"
    check_fir_sums(avg, ns, w, h, kord, rows, what)
    check_against_terms(oracle, score, avg, ns, ref, dist, "fir", what, kavg=kavg)
