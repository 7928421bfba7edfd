"""The 16-bit marching kernels at the edges of the wide geometry (-m gpu only; FIR mode): k_march_lin and
k_march_refblur_lin, whose scale 0 is fp32 linear planes.  In the halo pass of march_convert_rows (ssimu2_kernels.h) a
halo pixel of theirs is three dword loads `hplane` bytes apart with no table (HN == 3, hu8 == false) -- at scale 0,
where the 8-bit kernels load one dword and go through the LUT -- and in the cached form wave 0 copies XYB planes while
wave 1 converts linear ones.  tests/test_gpu_march_wide.py holds the 8-bit kernels at these widths and rows
(tests/wide_cases.py; what the cases reach: tests/test_wide_cases.py); this module holds the 16-bit ones:

a. lifted frames (257 u): the bits of the 8-bit pair score at the same rows, so the 8-bit module's hold to the
   kernel-order terms carries over;
b. genuine 10-, 12- and 16-bit content: the d / d^4 averages against the kernel's own summing order (check_fir_sums),
   every average against the kernel-order terms and k_finalize (check_against_terms), the score against the checker's;
c. the three cached forms -- 16-bit reference and frame, 8-bit reference and 16-bit frame, 16-bit reference and 8-bit
   frame -- bit for bit the pair score of the same pixels;
d. a second run, after a pair score of other content at another size, bit for bit;
e. padded RGBA rows of a 16-bit frame (ssimu2_score_against_reference_strided16) bit for bit the tight call.

ssimu2_instr_last_march says every time which kernel ran.  The wrapper has no device-pointer form of the 16-bit calls,
so there is none to hold here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import gpu_cases  # noqa: E402
import hbd_ref  # noqa: E402
from gpu_cases import bits_equal, check_against_terms, check_fir_sums  # noqa: E402
from hbd_cases import content16, lift, rows16  # noqa: E402
from wide_cases import ALL_WIDTHS, HEIGHT_ROWS, TAIL_ROWS, _pair  # noqa: E402

pytestmark = pytest.mark.gpu

DEPTHS = (10, 12, 16)


def _scored(s, score, kernel, what):
    """(score, averages, nscales) of the call that just returned `score`, which must have launched `kernel`."""
    assert s.last_march() == kernel, (what, s.last_march())
    avg, ns = s.last_averages()
    assert ns >= 1, what
    return score, avg, ns


def _same(got, exp, what):
    assert got[2] == exp[2], what
    bits_equal(got[0], got[1], exp[0], exp[1], what)


def _lifted(s, ref, dist, k, what):
    """a, c and d on 257 u frames: every 16-bit form has the bits of the 8-bit pair score."""
    h, w, _ = ref.shape
    exp = _scored(s, s.compute_ssimu2(ref, dist), "k_march", what)
    r16, d16 = lift(ref), lift(dist)
    _same(_scored(s, s.compute_ssimu2_hbd(r16, d16, 16), "k_march_lin", what), exp, f"{what}: lifted pair")
    s.set_reference_hbd(r16, 16)
    _same(_scored(s, s.score_against_reference_hbd(d16, 16), "k_march_refblur_lin", what), exp,
          f"{what}: lifted frame against the lifted reference")
    _same(_scored(s, s.score_against_reference(dist), "k_march_refblur", what), exp,
          f"{what}: 8-bit frame against the lifted reference")
    s.set_reference(ref)
    _same(_scored(s, s.score_against_reference_hbd(d16, 16), "k_march_refblur_lin", what), exp,
          f"{what}: lifted frame against the 8-bit reference")
    gpu_cases.stale(s, w, h, k)
    _same(_scored(s, s.compute_ssimu2_hbd(r16, d16, 16), "k_march_lin", what), exp, f"{what}: lifted pair, second run")


def _genuine(s, oracle, w, h, d, rows, k, what):
    """b, c and d on d-bit content whose codes are no multiples of 257."""
    ref = content16(w, h, d, 11 * w + h)
    dist = content16(w, h, d, 11 * w + h, distort=True)
    assert (ref != dist).any() and (ref % 257 != 0).any(), what
    pair = _scored(s, s.compute_ssimu2_hbd(ref, dist, d), "k_march_lin", what)
    score, avg, ns = pair
    kavg, ns_r, kord = errmap_ref.kernel_averages_lin(oracle, hbd_ref.linear_planes(ref, d),
                                                      hbd_ref.linear_planes(dist, d), oracle.BLUR_FIR, seg_rows=rows)
    assert ns == ns_r, what
    check_fir_sums(avg, ns, w, h, kord, rows, what)
    check_against_terms(oracle, score, avg, ns, ref, dist, "fir", what, kavg=kavg, rows=rows)
    exp, _avg_r, ns_c = hbd_ref.compute(oracle, ref, dist, d, oracle.BLUR_FIR)
    print(f"measured: {what}: score {score!r}, checker {exp!r}")
    assert ns_c == ns and abs(score - exp) <= gpu_cases.score_tol(exp), (what, score, exp)
    s.set_reference_hbd(ref, d)
    _same(_scored(s, s.score_against_reference_hbd(dist, d), "k_march_refblur_lin", what), pair,
          f"{what}: pass against the cached reference")
    gpu_cases.stale(s, w, h, k + 1)
    _same(_scored(s, s.compute_ssimu2_hbd(ref, dist, d), "k_march_lin", what), pair, f"{what}: second run")
    s.set_reference_hbd(ref, d)
    _same(_scored(s, s.score_against_reference_hbd(dist, d), "k_march_refblur_lin", what), pair,
          f"{what}: pass against the cached reference, second run")
    assert score < 100.0, what


@pytest.mark.parametrize("w", ALL_WIDTHS)
def test_16bit_right_edge_on_every_halo_column_and_every_batch_residue(iscorer, oracle, w):
    s = iscorer
    try:
        for j, (h, seg) in enumerate(HEIGHT_ROWS):
            s.set_segment_rows(seg, TAIL_ROWS)
            rows = gpu_cases.override_rows(seg, TAIL_ROWS)
            k = ALL_WIDTHS.index(w) * len(HEIGHT_ROWS) + j
            d = DEPTHS[k % 3]
            ref, dist = _pair(w, h, 7 * w + h)
            _lifted(s, ref, dist, k, f"wide lifted {w}x{h} rows {seg}")
            _genuine(s, oracle, w, h, d, rows, k, f"wide {d}-bit {w}x{h} rows {seg}")
    finally:
        s.set_segment_rows(0, 0)


@pytest.mark.parametrize("w", [129, 136, 257])
def test_padded_rgba16_rows_equal_the_tight_call(iscorer, w):
    """ssimu2_score_against_reference_strided16 on RGBA rows 6 samples longer than their pixels, alpha and padding
    noise: the frame the marching kernel reads is unpacked on the device, and the score keeps the tight call's bits."""
    s = iscorer
    try:
        for j, (h, seg) in enumerate(HEIGHT_ROWS):
            s.set_segment_rows(seg, TAIL_ROWS)
            d = DEPTHS[(w + j) % 3]
            what = f"wide strided {d}-bit {w}x{h} rows {seg}"
            ref = content16(w, h, d, 13 * w + h)
            dist = content16(w, h, d, 13 * w + h, distort=True)
            s.set_reference_hbd(ref, d)
            tight = _scored(s, s.score_against_reference_hbd(dist, d), "k_march_refblur_lin", what)
            gpu_cases.scrub(s, ref, d)   # the planes a pass writes then hold the reference, not this frame
            _buf, view = rows16(dist, 4, 6, seed=w + h)
            assert view.strides[0] == (4 * w + 6) * 2
            _same(_scored(s, s.score_decoded_against_reference_hbd(view, bit_depth=d), "k_march_refblur_lin", what),
                  tight, what)
            assert tight[0] < 100.0, what
    finally:
        s.set_segment_rows(0, 0)
