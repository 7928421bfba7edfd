"""The wide marching geometry (-m gpu only; FIR mode): 128 output columns per strip, 136 staged, the eight columns
behind the converter lanes converted six rows at a time (oavif_amd/csrc/ssimu2_kernels.h, MarchWide and the halo pass
of march_convert_rows).  The kernels that leave partial sums march wide strips -- the pair score (k_march) and the pass
against the cached reference (k_march_refblur) both run here.

What can go wrong is local to a strip's last eight staged columns and to the six-row batches they are converted in, so
the frames are small:

* widths: the image's right edge on each of the eight halo columns and either side of them (120 .. 136), two and three
  wide strips (255 .. 264), a strip narrower than its halo (8, 9);
* heights and segment rows (ssimu2_instr_set_segment_rows): a workgroup marches rows + 8 steps, and (height, rows) =
  (8, 8), (9, 9), (13, 13), (26, 10), (41, 11) give 16, 17, 21, 18 / 14 and 19 / 16 steps -- every residue mod 6, so
  partial last groups and partial last batches, first and last segments whose halo rows lie outside the image, and
  interior segments.

Held for each: every average against the kernel-order terms and k_finalize (check_against_terms), the d / d^4 averages
against k_march's own summing order (check_fir_sums: the fp32 accumulators over exactly the segment rows, then the
order of an fp64 sum), the score against the checker's, the pass against the cached reference bit for bit (one geometry
for every kernel that sums: the grouping of the fp64 part is shared), and a second run bit for bit."""
import os
import sys

import numpy as np
import pytest

from oavif_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import gpu_cases  # noqa: E402
from gpu_cases import bits_equal, check_against_terms, check_fir_sums, in_margins  # noqa: E402
from wide_cases import HEIGHT_ROWS, TAIL_ROWS, WIDTHS, _pair, _steps  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_heights_cover_every_residue_of_the_six_row_batches():
    assert {s % 6 for h, rows in HEIGHT_ROWS for s in _steps(h, rows)} == set(range(6))


def _hold(s, oracle, ref, dist, rows, what):
    """Pair score, its averages in every order the module's docstring names, the cached pass and a second run."""
    h, w, _ = ref.shape
    score = s.compute_ssimu2(ref, dist)
    avg, ns = s.last_averages()
    kavg, ns_r, kord = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=rows)
    assert ns == ns_r >= 1, what
    check_fir_sums(avg, ns, w, h, kord, rows, what)
    check_against_terms(oracle, score, avg, ns, ref, dist, "fir", what, kavg=kavg, rows=rows)
    exp = oracle.compute_ssimu2(ref, dist, oracle.BLUR_FIR)
    print(f"measured: {what}: score {score!r}, checker {exp!r}")
    assert abs(score - exp) <= gpu_cases.score_tol(exp), (what, score, exp)
    s.set_reference(ref)
    cached = s.score_against_reference(dist)
    cavg, cns = s.last_averages()
    assert cns == ns, what
    bits_equal(cached, cavg, score, avg, f"{what}: pass against the cached reference")
    again = s.compute_ssimu2(ref, dist)
    bits_equal(again, s.last_averages()[0], score, avg, f"{what}: second run")
    return score, avg


@pytest.mark.parametrize("w", WIDTHS)
def test_right_edge_on_every_halo_column_and_every_batch_residue(iscorer, oracle, w):
    s = iscorer
    try:
        for h, seg in HEIGHT_ROWS:
            s.set_segment_rows(seg, TAIL_ROWS)
            ref, dist = _pair(w, h, 7 * w + h)
            _hold(s, oracle, ref, dist, gpu_cases.override_rows(seg, TAIL_ROWS), f"wide {w}x{h} rows {seg}")
    finally:
        s.set_segment_rows(0, 0)


def test_ragged_full_hd(scorer, oracle):
    """1921 x 1083 under the rule's own rows: 16 wide strips whose last holds one column, 30 segments of 37 rows."""
    w, h = 1921, 1083
    assert gpu_cases.march_seg_rows(w, h, 0) == 37
    ref = synth.make_ref(w, h, seed=5)
    dist = synth.distort(ref, "blockq", 2, seed=6)
    _hold(scorer, oracle, ref, dist, gpu_cases.seg_rows(w, h), f"wide {w}x{h}")


@pytest.mark.parametrize("w,h", [(136, 26), (264, 13)])
def test_frames_at_odd_byte_offsets(scorer, oracle, w, h):
    """Device frames 1 and 3 bytes off a dword, between margins of random bytes: the lane of the image's last column --
    a halo lane at these widths -- reads one byte earlier and shifts, never past the frame; same bits as the host call."""
    ref, dist = _pair(w, h, w)
    score = scorer.compute_ssimu2(ref, dist)
    avg, _ns = scorer.last_averages()
    _t_ref, p_ref = in_margins(ref, 1, w)
    _t_dist, p_dist = in_margins(dist, 3, h)
    assert p_ref % 4 == 1 and p_dist % 4 == 3
    got = scorer.score_device(p_ref, p_dist, w, h)
    bits_equal(got, scorer.last_averages()[0], score, avg, f"wide {w}x{h} at odd offsets")
    kavg, ns, kord = errmap_ref.kernel_averages(oracle, ref, dist, oracle.BLUR_FIR, seg_rows=gpu_cases.seg_rows(w, h))
    check_fir_sums(avg, ns, w, h, kord, gpu_cases.seg_rows(w, h), f"wide {w}x{h} at odd offsets")
