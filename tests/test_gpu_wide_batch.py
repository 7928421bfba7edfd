"""The batch marching kernels at the edges of the wide geometry (-m gpu only; FIR mode): k_march_batch and
k_march_refblur_batch.  In the halo pass of march_convert_rows (ssimu2_kernels.h) the halo cursor of a batch item is a
copy of the frame cursor taken AFTER the item's byte offset was added, the clamped-row path rebuilds its address from
that base, and the item x tile maps run over the wide strips' count.  A halo column read from another item, from the
other frame's plane, at a wrongly clamped row or zero-padded a column early changes four output columns of a strip.

Everything is held as tests/test_gpu_batch_items.py holds the batch grid -- every item has the bits (score and all 108
averages) of the single score of its pair at the same rows, all items of a batch differ -- at the cases of
tests/wide_cases.py, whose reach tests/test_wide_cases.py proves on the CPU:

a. every width that puts the right edge of scale 0 or scale 1 on column 127 and on each halo column, under scale-0
   rows (ssimu2_instr_set_batch_segment_rows) that put the steps of first, interior and last segments on every residue
   of the six-row halo passes; the rule's own 96 / 48 rows are 104 and 56 steps, one residue;
b. several strips x several segments at every residue of the batch grid, at the rule's rows (WIDE_RESIDUE_SIZES);
c. the uncached-reference fallback (k_march_batch with a shared reference);
d. the device forms with an odd item stride, where the lanes of an item's last column read one byte early;
e. an 8-bit batch against a 16-bit reference (k_march_refblur_batch copying 16-bit planes' XYB)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_cases as wc  # noqa: E402
from gpu_cases import bits_equal  # noqa: E402
from test_gpu_batch_items import (FORMS, RESIDUES, batch_items, check_against_singles,  # noqa: E402
                                  device_forms_against_singles, hold_batch_against_a_16bit_reference, run_batch)

pytestmark = pytest.mark.gpu

KERNEL = {False: "k_march_batch", True: "k_march_refblur_batch"}


# ---- a. the right edge on every halo column, every pass residue -----------------------------------------------------
@FORMS
@pytest.mark.parametrize("w", wc.ALL_WIDTHS)
def test_batch_right_edge_on_every_halo_column_and_every_pass_residue(iscorer, w, cached):
    s = iscorer
    try:
        for h, rows0 in wc.BATCH_HEIGHT_ROWS:
            s.set_batch_segment_rows(rows0)
            rows = [s.batch_segment_rows(w, h, scale) for scale in range(6)]
            assert rows == wc.batch_rows(rows0), (w, h, rows0)   # what tests/test_wide_cases.py reasons about
            batches = []
            for n in (3, 5):
                refs, dists = batch_items(w, h, n, cached)
                batches.append((refs, dists, cached, run_batch(s, refs, dists, cached)))
                assert s.last_march() == KERNEL[cached], (w, h, rows0, n)
            check_against_singles(s, w, h, batches, rows=rows)
            assert any(0.0 < g[0] < 100.0 for g in batches[-1][3]), (w, h, rows0)
    finally:
        s.set_batch_segment_rows(0)


# ---- b. several strips x several segments x every residue of the batch grid ----------------------------------------
@FORMS
@pytest.mark.parametrize("w,h", wc.WIDE_RESIDUE_SIZES)
def test_every_item_at_every_residue_of_the_wide_batch_grid(iscorer, w, h, cached):
    """n = 1 .. 17, 31, 33 at the batch rule's own rows: n * nblocks takes every residue mod 8 in every scale's
    [first, end) of the batch grid, with three strips and two strips at scale 1 (wide_cases.TILES)."""
    s = iscorer
    assert [s.batch_segment_rows(w, h, scale) for scale in range(6)] == wc.batch_rows()
    batches = []
    for n in RESIDUES:
        refs, dists = batch_items(w, h, n, cached)
        batches.append((refs, dists, cached, run_batch(s, refs, dists, cached)))
        assert s.last_march() == KERNEL[cached], (w, h, n)
    check_against_singles(s, w, h, batches)
    assert any(0.0 < g[0] < 100.0 for g in batches[-1][3])


# ---- c. the uncached-reference fallback -----------------------------------------------------------------------------
@pytest.mark.parametrize("w", [129, 136, 257])
def test_uncached_reference_batch_at_the_halo(iscorer, w):
    """Without the reference's blur cache a batch against the reference runs k_march_batch with a shared reference (no
    item offset on frame 0, one on frame 1): the pair form's bits, item by item."""
    s = iscorer
    n = 5
    try:
        for h, rows0 in wc.BATCH_HEIGHT_ROWS:
            s.set_batch_segment_rows(rows0)
            refs, dists = batch_items(w, h, n, True)
            scores = s.score_batch(refs, dists)
            assert s.last_march() == "k_march_batch"
            pair = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
            s.cache_reference_blur(False)   # drops the reference: run_batch sets it
            got = run_batch(s, refs, dists, True)
            assert s.last_march() == "k_march_batch", (w, h, rows0)
            s.cache_reference_blur(True)
            with_cache = run_batch(s, refs, dists, True)
            assert s.last_march() == "k_march_refblur_batch", (w, h, rows0)
            for k in range(n):
                assert got[k][2] == pair[k][2] == with_cache[k][2] >= 1
                bits_equal(got[k][0], got[k][1], pair[k][0], pair[k][1], f"{w}x{h} rows {rows0} cache off, item {k}")
                bits_equal(with_cache[k][0], with_cache[k][1], pair[k][0], pair[k][1],
                           f"{w}x{h} rows {rows0} cache on, item {k}")
            assert any(0.0 < g[0] < 100.0 for g in got)
    finally:
        s.cache_reference_blur(True)
        s.set_batch_segment_rows(0)


# ---- d. the device forms with an odd item stride --------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(136, 26), (257, 13)])
def test_device_forms_with_an_odd_item_stride_at_the_halo(iscorer, w, h):
    """33 items, item stride = frame + 53 bytes (odd: items start at every residue mod 4), noise between frames: the
    lanes that load an item's last column -- halo lanes at these widths -- read one byte early and shift, and stay
    inside their item."""
    device_forms_against_singles(iscorer, w, h, 33, 53)


# ---- e. an 8-bit batch against a 16-bit reference -------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(136, 41), (257, 33)])
@pytest.mark.parametrize("depth", [10, 12, 16])
def test_batch_against_a_16bit_reference_at_the_halo(iscorer, oracle, depth, w, h):
    hold_batch_against_a_16bit_reference(iscorer, oracle, depth, w, h)
