"""Cases of the wide marching geometry shared by the GPU modules that hold the six summing kernels at a strip's halo
(tests/test_gpu_march_wide.py: k_march, k_march_refblur; tests/test_gpu_wide_lin.py: k_march_lin, k_march_refblur_lin;
tests/test_gpu_wide_batch.py: k_march_batch, k_march_refblur_batch), and the restated arithmetic that says what each
case reaches.  tests/test_wide_cases.py proves the coverage on the CPU; importing this module needs no GPU.

A wide strip (MarchWide, oavif_amd/csrc/ssimu2_kernels.h) starts at image column x0 = 128 * strip and stages columns
x0 - 4 .. x0 + 131: staged column j is image column x0 - 4 + j.  Staged columns 0 .. 127 belong to the converter lanes;
128 .. 135 (image columns x0 + 124 .. x0 + 131) are converted by the halo pass, six rows at a time.  The image's last
column w - 1 therefore lies on halo column 128 + k of strip 0 at w = 125 + k, of strip 1 at w = 253 + k; at scale 1
(width (w + 1) // 2) of strip 0 at w = 249 + 2 k and 250 + 2 k."""
from __future__ import annotations

import gpu_cases
from oavif_amd import synth
from ssimu2_fp64 import scale_size

WIDE_MW = gpu_cases.WIDE_MW   # 128 output columns per strip (gpu_cases.MW, 120, stays the segment rule's unit)
STAGED = WIDE_MW + 8          # staged columns of a wide strip
HALO0 = 128                   # the first staged column without a converter lane: the 128 converter lanes end here

WIDTHS = [120, 123, 124, 125, 126, 127, 128, 129, 130, 131, 132, 135, 136,   # the right edge on every halo column
          255, 256, 257, 260, 264,                                           # two and three wide strips
          8, 9]                                                              # narrower than the halo
# the 16-bit and batch modules add the widths that put SCALE 1's right edge (width (w + 1) // 2) on column 127 and on
# the halo columns that 255 .. 264 leave out: scale-1 widths 124, 125, 126, 127 and 131 beside 128, 129, 130 and 132
SCALE1_WIDTHS = [248, 249, 251, 253, 261]
ALL_WIDTHS = WIDTHS + SCALE1_WIDTHS

HEIGHT_ROWS = [(8, 8), (9, 9), (13, 13), (26, 10), (41, 11)]
TAIL_ROWS = 8

# (height, scale-0 rows of ssimu2_instr_set_batch_segment_rows): three segments each -- a first, an interior and a
# shorter last one -- with full segments of 8 .. 13 rows (16 .. 21 steps: every residue mod 6) and last segments of
# 1 .. 6 rows (9 .. 14 steps: every residue again).  Scale 1 follows with the same rows (they are below 48): heights
# 9 .. 16, one full and one shorter segment, every residue once more.
BATCH_HEIGHT_ROWS = [(17, 8), (20, 9), (23, 10), (26, 11), (29, 12), (32, 13)]

#                     (w, h)       strips x segments per item under the batch rule (96 rows at scale 0, 48 below)
WIDE_RESIDUE_SIZES = [(129, 40),   # 2 strips at scale 0, 1 block at each of scales 1 .. 3
                      (257, 100),  # 3 strips x 2 segments at scale 0, 2 x 2 at scale 1 (129 x 50)
                      (264, 200)]  # 3 strips x 3 segments at scale 0, 2 x 3 at scale 1 (132 x 100), 1 x 2 at scale 2
# what the comments above and those of test_gpu_batch_items.RESIDUE_SIZES state: (strips, segments) from scale 0 down
TILES = {(129, 40): [(2, 1), (1, 1), (1, 1), (1, 1)],
         (257, 100): [(3, 2), (2, 2), (1, 1), (1, 1), (1, 1)],
         (264, 200): [(3, 3), (2, 3), (1, 2), (1, 1), (1, 1), (1, 1)],
         (24, 17): [(1, 1), (1, 1), (1, 1)],
         (121, 40): [(1, 1), (1, 1), (1, 1), (1, 1)],
         (241, 100): [(2, 2), (1, 2), (1, 1), (1, 1), (1, 1)],
         (130, 200): [(2, 3), (1, 3), (1, 2), (1, 1), (1, 1), (1, 1)]}


def _steps(h, rows):
    """Marching steps (rows + 8 of halo) of every segment of an h-row scale cut into segments of `rows` rows."""
    return {min(rows, h - y0) + 8 for y0 in range(0, h, rows)}


def _pair(w, h, seed):
    ref = gpu_cases.content(gpu_cases.KINDS[seed % 5], w, h, seed)
    return ref, synth.distort(ref, "noise", 2, seed=seed + 1)


def nscales(w, h):
    """make_pyramid: scale s is scored iff scale s - 1 is at least 8 x 8."""
    n = 0
    while n < 6 and min(scale_size(w, h, max(n - 1, 0))) >= 8:
        n += 1
    return n


def plan(w, h, cols, rows=None):
    """build_plans for a kernel with strips of `cols` columns under march_seg_rows, or under `rows` (segment rows by
    scale): per scale (seg, nstrips, tiles) and the running block ranges."""
    out, first = [], 0
    for s in range(nscales(w, h)):
        sw, sh = scale_size(w, h, s)
        seg = gpu_cases.march_seg_rows(w, h, s) if rows is None else rows[s]
        nstrips = (sw + cols - 1) // cols
        nb = nstrips * ((sh + seg - 1) // seg)
        out.append((seg, nstrips, nb, first, first + nb))
        first += nb
    return out


def wide_tiles(w, h, rows_by_scale):
    """-> [(strips, segments)] of every scored scale of a w x h frame for a kernel that leaves partial sums."""
    return [(nstrips, nb // nstrips) for _seg, nstrips, nb, _first, _end in plan(w, h, WIDE_MW, rows_by_scale)]


def batch_rows(rows_scale0=0):
    """batch_seg_rows by scale under ssimu2_instr_set_batch_segment_rows(rows_scale0) (0: the rule's 96): the other
    scales follow with at most 48."""
    seg = rows_scale0 or gpu_cases.batch_seg_rows(0, 0, 0)
    return [seg] + [min(seg, 48)] * 5


def edge_columns(sw):
    """The staged columns the last column of a scale sw wide lies on, over the wide strips that stage it."""
    cols = {sw - 1 - (x0 - 4) for x0 in range(0, sw, WIDE_MW)}
    return {j for j in cols if 0 <= j < STAGED}


def whole_halo_inside(sw):
    """Some strip of a scale sw wide has all eight halo columns inside the image."""
    return any(x0 - 4 + STAGED <= sw for x0 in range(0, sw, WIDE_MW))
