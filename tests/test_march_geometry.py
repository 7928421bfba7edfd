"""The marching plan's arithmetic for both strip widths, restated (CPU only; oavif_amd/csrc/ssimu2_hip.hip: build_plans,
march_seg_rule, strip_cols; ssimu2_kernels.h: MarchGeo, march_tile_of_block).

The strip width of a kernel (128 output columns for the kernels that leave partial sums, 120 for the ones that write
planes) and the segment rule's column unit (120, gpu_cases.MW) are two things: the rows a lane sums in fp32 are part of
a score's bits and must not move with the strip width, while strips, tiles and the partial-sum capacity follow the
kernel."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_cases  # noqa: E402
from ssimu2_fp64 import scale_size  # noqa: E402
from wide_cases import nscales, plan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE, NARROW = 128, 120
SIZES = [s for s in gpu_cases.SIZES if min(s) >= 8] + [(3840, 2160), (7680, 4320)]
PINNED_ROWS = {(3840, 2160): 135, (1921, 1083): 37, (1000, 700): 13}


def _source(name):
    with open(os.path.join(ROOT, "oavif_amd", "csrc", name)) as f:
        return f.read()


def tile_of_block(b, first, end):
    """march_tile_of_block: each XCD phase (b % 8) takes a contiguous run of the scale's tiles."""
    x = b & 7
    before = sum((end + 7 - r) // 8 - (first + 7 - r) // 8 for r in range(x))
    return before + (b >> 3) - ((first + 7 - x) >> 3)


def test_the_sources_name_the_two_widths_and_the_rule_s_own_unit():
    kernels, host = _source("ssimu2_kernels.h"), _source("ssimu2_hip.hip")
    assert re.search(r"typedef MarchGeo<%d> MarchNarrow;" % NARROW, kernels)
    assert re.search(r"typedef MarchGeo<%d> MarchWide;" % WIDE, kernels)
    assert re.search(r"constexpr int kSegRuleCols = %d;" % gpu_cases.MW, host)
    rule = host.split("int march_seg_rule(")[1].split("\n}\n")[0]
    assert "kSegRuleCols" in rule and "MW" not in rule.replace("kSegRuleCols", "")


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_segment_rows_do_not_follow_the_strip_width(w, h):
    wide, narrow = plan(w, h, WIDE), plan(w, h, NARROW)
    assert len(wide) == len(narrow) == nscales(w, h) >= 1
    for s, (a, b) in enumerate(zip(wide, narrow)):
        assert a[0] == b[0] == gpu_cases.march_seg_rows(w, h, s)
    if (w, h) in PINNED_ROWS:
        assert wide[0][0] == PINNED_ROWS[(w, h)]


def test_pinned_rows():
    for (w, h), rows in PINNED_ROWS.items():
        assert gpu_cases.march_seg_rows(w, h, 0) == rows


@pytest.mark.parametrize("cols", [WIDE, NARROW])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_tiles_per_scale_and_the_tile_order(w, h, cols):
    """ceil(w / cols) * ceil(h / seg) tiles per scale, never more wide tiles than narrow ones (the partial sums are
    sized for the kernels that sum), and march_tile_of_block a bijection of each scale's block range onto its tiles."""
    for s, (seg, nstrips, nb, first, end) in enumerate(plan(w, h, cols)):
        sw, sh = scale_size(w, h, s)
        assert nstrips == -(-sw // cols) and nb == nstrips * -(-sh // seg)
        assert nstrips * cols >= sw > (nstrips - 1) * cols
        assert sorted(tile_of_block(b, first, end) for b in range(first, end)) == list(range(nb))
    assert sum(p[2] for p in plan(w, h, WIDE)) <= sum(p[2] for p in plan(w, h, NARROW))


def test_4k_strip_counts():
    """What the wide strips buy at 3840 x 2160: 30 strips for 32 at scale 0, 15 for 16 at scale 1, the same below."""
    assert [p[1] for p in plan(3840, 2160, NARROW)] == [32, 16, 8, 4, 2, 1]
    assert [p[1] for p in plan(3840, 2160, WIDE)] == [30, 15, 8, 4, 2, 1]
