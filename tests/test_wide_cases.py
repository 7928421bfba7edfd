"""What the cases of tests/wide_cases.py reach, proved on the CPU: the image's right edge on each of a wide strip's
eight halo columns at scales 0 and 1, every residue of the six-row halo passes under the single-score override and
under the batch override, and the strip x segment counts the batch sizes' comments state -- computed with 128-column
strips, so that a change of the geometry fails here instead of thinning the GPU cases unnoticed."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_cases  # noqa: E402
import wide_cases as wc  # noqa: E402
from ssimu2_fp64 import scale_size  # noqa: E402
from test_gpu_batch_items import RESIDUE_SIZES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = range(wc.HALO0, wc.STAGED)
# the widths tests/test_gpu_wide_lin.py and tests/test_gpu_wide_batch.py name themselves
FIXED_WIDTHS = [129, 136, 257]


def _source(name):
    with open(os.path.join(ROOT, "oavif_amd", "csrc", name)) as f:
        return f.read()


def test_the_sources_have_the_geometry_restated_here():
    kernels, host = _source("ssimu2_kernels.h"), _source("ssimu2_hip.hip")
    assert re.search(r"typedef MarchGeo<%d> MarchWide;" % wc.WIDE_MW, kernels)
    assert "static constexpr int MRW = W + 2 * RAD;" in kernels and "constexpr int RAD = 4;" in kernels
    assert wc.STAGED == wc.WIDE_MW + 2 * 4 and wc.HALO0 == 128 and list(HALO) == list(range(128, 136))
    assert "hcol = 128 + (col & 7)" in kernels and "constexpr int GROUP = 3;" in kernels   # eight columns, QD = 6 rows
    assert gpu_cases.WIDE_MW == 128 and gpu_cases.MW == 120
    assert re.search(r"constexpr int kBatchSegRows = %d;" % gpu_cases.batch_seg_rows(0, 0, 0), host)
    assert wc.batch_rows() == [gpu_cases.batch_seg_rows(0, 0, s) for s in range(6)] == [96, 48, 48, 48, 48, 48]
    assert wc.batch_rows(13) == [13] * 6 and wc.batch_rows(160) == [160] + [48] * 5


def test_edge_columns_by_hand():
    assert wc.edge_columns(124) == {127} and wc.edge_columns(125) == {128} and wc.edge_columns(132) == {135, 7}
    assert wc.edge_columns(133) == {8} and wc.edge_columns(253) == {128} and wc.edge_columns(8) == {11}
    assert not wc.whole_halo_inside(131) and wc.whole_halo_inside(132) and not wc.whole_halo_inside(9)


@pytest.mark.parametrize("scale,widths", [(0, wc.WIDTHS), (1, wc.ALL_WIDTHS)], ids=["scale0", "scale1_batch"])
def test_the_right_edge_lies_on_every_halo_column(scale, widths):
    """Every halo column 128 + k is the image's last column for some width, so is column 127 (the last converter lane:
    no halo column inside the image), and some width has all eight inside."""
    edges = {w: wc.edge_columns(scale_size(w, 64, scale)[0]) for w in widths}
    for col in [wc.HALO0 - 1] + list(HALO):
        assert any(col in e for e in edges.values()), (scale, col)
    assert any(wc.whole_halo_inside(scale_size(w, 64, scale)[0]) for w in widths)
    assert any(scale_size(w, 64, scale)[0] < 8 + 4 for w in widths)   # a strip that ends before its halo begins


def test_scale0_widths_also_hold_scale1_for_the_single_scores():
    """WIDTHS alone (tests/test_gpu_march_wide.py) reaches scale 1's halo only at columns 131 .. 133 and 135 (scale-1
    widths 128 .. 130 and 132); SCALE1_WIDTHS are what the 16-bit and batch modules add, and ALL_WIDTHS holds every
    width of WIDTHS."""
    at1 = set().union(*(wc.edge_columns((w + 1) // 2) for w in wc.WIDTHS))
    assert at1 & set(HALO) == {131, 132, 133, 135}
    assert set(wc.WIDTHS) <= set(wc.ALL_WIDTHS) and max(wc.ALL_WIDTHS) <= 264
    assert all(w in wc.ALL_WIDTHS for w in FIXED_WIDTHS)


def test_the_fixed_widths_sit_on_the_halo():
    """129, 136 and 257: the right edge on halo column 132 of strip 0, every halo column inside with a second strip of
    8 columns, and a third strip of one column behind two whole halos."""
    assert 132 in wc.edge_columns(129) and wc.whole_halo_inside(136) and wc.whole_halo_inside(257)
    assert [wc.wide_tiles(w, 40, wc.batch_rows())[0][0] for w in FIXED_WIDTHS] == [2, 2, 3]


def test_single_score_rows_cover_every_residue_of_the_six_row_passes():
    assert {s % 6 for h, rows in wc.HEIGHT_ROWS for s in wc._steps(h, rows)} == set(range(6))
    assert all(8 <= rows <= 160 and 8 <= wc.TAIL_ROWS <= 160 and h <= 200 for h, rows in wc.HEIGHT_ROWS)


def test_the_batch_rule_s_own_rows_reach_one_residue():
    """96 and 48 rows are 104 and 56 steps, both 2 mod 6: under the rule every full segment ends its halo passes alike."""
    full = {wc._steps(h, rows).pop() for rows in set(wc.batch_rows()) for h in (rows, 5 * rows)}
    assert full == {104, 56} and {s % 6 for s in full} == {2}


def test_batch_rows_cover_every_residue_in_first_interior_and_last_segments():
    full0, last0, at1 = set(), set(), set()
    for h, rows0 in wc.BATCH_HEIGHT_ROWS:
        assert 8 <= rows0 <= 160 and h <= 200
        rows = wc.batch_rows(rows0)
        nsegs = -(-h // rows[0])
        assert nsegs >= 3 and h % rows[0]        # a first, an interior and a shorter last segment
        full0.add((rows[0] + 8) % 6)
        last0.add((h % rows[0] + 8) % 6)
        assert wc._steps(h, rows[0]) == {rows[0] + 8, h % rows[0] + 8}
        at1 |= {s % 6 for s in wc._steps(scale_size(64, h, 1)[1], rows[1])}
    assert full0 == last0 == at1 == set(range(6))


@pytest.mark.parametrize("w,h", RESIDUE_SIZES + wc.WIDE_RESIDUE_SIZES)
def test_strips_and_segments_of_the_batch_sizes(w, h):
    """The (strips, segments) each size's comment states, under the batch rule with 128-column strips."""
    assert w <= 264 and h <= 200
    assert wc.wide_tiles(w, h, wc.batch_rows()) == wc.TILES[(w, h)]
    assert len(wc.TILES[(w, h)]) == wc.nscales(w, h)


def test_the_wide_sizes_are_what_the_old_comments_promised():
    t = {size: wc.TILES[size] for size in wc.WIDE_RESIDUE_SIZES}
    assert t[(129, 40)][0] == (2, 1)
    assert t[(257, 100)][:2] == [(3, 2), (2, 2)] and scale_size(257, 100, 1) == (129, 50)
    assert t[(264, 200)][0] == (3, 3) and t[(264, 200)][1][0] == 2
    # and what the 120-column sizes are now: one strip, two strips
    assert wc.TILES[(121, 40)][0] == (1, 1) and wc.TILES[(241, 100)][0] == (2, 2)
    # more than one tile per item somewhere, so item x tile maps are exercised at every wide size
    assert all(sum(a * b for a, b in tiles) > len(tiles) for tiles in t.values())
