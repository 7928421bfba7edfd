"""The shape lists of tests/rbatch_cases.py against the classes they are there for (CPU only), so that a later edit of a
list cannot quietly lose one, and its constants against the source lines they restate."""
import os

import gpu_cases
import rbatch_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every frame size an 8-bit batch is scored at in tests/test_gpu_rbatch_grid.py, both forms and both modes each
ALL_8BIT = gpu_cases.SIZES + rc.TILE_SHAPES + rc.BAND_SHAPES + rc.LONG_SHAPES


def _source(name):
    with open(os.path.join(ROOT, "oavif_amd", "csrc", name)) as f:
        return f.read()


def test_the_constants_are_the_sources():
    for name, (_value, unit, line) in rc.SOURCE_LINES.items():
        assert line in _source(unit), (name, unit, line)
    assert (rc.RG_TW, rc.RG_N, rc.RG_HL, rc.RG_VW, rc.AHEAD_REF, rc.AHEAD_PASS) == (64, 5, 20, 64, 2, 1)
    threads, tx = rc.SOURCE_LINES["PYR_THREADS"][0], rc.SOURCE_LINES["PYR_TX"][0]
    assert tx == threads // 8 and (rc.PYR_BAND_W, rc.PYR_BAND_H) == (4 * tx, 32) == (256, 32)
    # the batch kernel takes rg_h_line's AHEAD from the form as k_rg_h does, and the unit that is instantiated is BATCH's
    h = _source("ssimu2_recursive.h")
    batch = h.split("void k_rg_h_batch(RgBatchPlan bp) {")[1].split("\n}\n")[0]
    assert "constexpr int AHEAD = REF ? RG_H_AHEAD_REF : RG_H_AHEAD_PASS;" in batch
    assert batch.count("AHEAD, true>(L, ") == 3
    assert (rc.NUM_SCALES, rc.MIN_SIZE) == (6, 8)


def test_the_restated_geometry_on_known_widths():
    assert rc.h_tiles(1) == (1, 1) and rc.h_tiles(60) == (1, 1) and rc.h_tiles(61) == (1, 2)
    assert rc.h_tiles(64) == (1, 2) and rc.h_tiles(124) == (1, 2) and rc.h_tiles(125) == (1, 3)
    assert rc.h_tiles(128) == (2, 3) and rc.h_tiles(188) == (2, 3) and rc.h_tiles(189) == (2, 4)
    assert rc.h_tiles(241) == (3, 4) and rc.h_tiles(257) == (4, 5) and rc.h_tiles(320) == (5, 6)
    # every column of the row and the three behind it are stepped over: 64 * ntiles >= w + 4 > 64 * (ntiles - 1)
    for w in range(1, 1200):
        nmain, ntiles = rc.h_tiles(w)
        assert 64 * ntiles >= w + 4 > 64 * (ntiles - 1) and 0 <= ntiles - nmain <= 2 and (nmain == 1 or 64 * nmain <= w)
    assert [rc.pair_loop(64 * k) for k in range(1, 8)] == [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True),
                                                           (3, False)]
    assert rc.bands(256, 32) == (1, 1) and rc.bands(257, 33) == (2, 2) and rc.bands(513, 65) == (3, 3)
    assert rc.nscales(7, 9) == 0 and rc.nscales(8, 8) == 2 and rc.nscales(112, 112) == 5 and rc.nscales(113, 113) == 6
    assert rc.column_groups(121, 40) == [2, 1, 1, 1] and rc.row_groups(121, 40) == [2, 1, 1, 1]
    assert rc.column_groups(1921, 1083)[0] == 31 and rc.row_groups(1921, 1083)[0] == 55


def test_the_issue_s_shapes_are_all_there():
    assert rc.TILE_WIDTHS[:11] == [61, 63, 125, 127, 191, 253, 320, 383, 384, 447, 448] and rc.TILE_HEIGHT == 21
    assert rc.BAND_SHAPES[:5] == [(255, 31), (256, 32), (257, 33), (512, 64), (513, 65)]
    assert rc.LONG_SHAPES == [(65_600, 9), (9, 65_600)]
    assert sorted(rc.FRONT_END_SHAPES) == [(333, 217), (513, 65)]
    assert rc.SEVEN_ITEMS_UP_TO == 333 * 217
    assert {(333, 217), (513, 259), (1921, 1083), (1000, 9), (9, 1000), (4000, 8), (8, 4000)} <= set(gpu_cases.SIZES)
    # height 21: a second row group with a single real row
    assert rc.row_groups(61, rc.TILE_HEIGHT)[0] == 2 and rc.TILE_HEIGHT - rc.RG_HL == 1


def test_every_tile_class_of_the_horizontal_pass_is_met():
    """Every (min(nmain, 7), ntiles - nmain) that exists: no edge tile behind the main loop only below 61 columns."""
    exists = {rc.tile_class(w) for w in range(1, 64 * 9)}
    assert exists == {(1, 0), (1, 1), (1, 2)} | {(q, d) for q in range(2, 8) for d in (1, 2)}
    met = {rc.tile_class(w) for w, _h in ALL_8BIT}
    assert met == exists, sorted(exists - met)
    # two edge tiles behind the main loop come from the tile list alone, at every count of main tiles
    assert {rc.tile_class(w) for w in rc.TILE_WIDTHS} >= {(q, 2) for q in range(1, 8)}


def test_every_class_of_the_two_tile_loop_is_met():
    """0, 1 and >= 2 trips, each with and without a leftover tile, in the tile list itself."""
    met = {rc.loop_class(w) for w in rc.TILE_WIDTHS}
    assert met == {(t, left) for t in (0, 1, 2) for left in (False, True)}, met
    # ... and a first edge tile on the even register set behind a leftover, above 188 columns, with two edge tiles
    assert any(rc.pair_loop(w)[1] and w > 188 and rc.tile_class(w)[1] == 2 for w in rc.TILE_WIDTHS)
    # the slack behind the batch's planes (kRgBatchTail) is met at more than five tiles
    assert max(rc.h_tiles(w)[1] for w in rc.TILE_WIDTHS) > 5


def test_every_band_count_is_met():
    """1 x 1, 2 x 2 and 3 x 3 bands exactly, from the band list itself; every pair of counts (three standing for three
    or more) from all the shapes together."""
    met = {rc.bands(w, h) for w, h in rc.BAND_SHAPES}
    assert met >= {(1, 1), (2, 2), (3, 3)}, met
    # ragged and exact: a last band of one column and one row, and full last bands
    assert {(w % rc.PYR_BAND_W, h % rc.PYR_BAND_H) for w, h in rc.BAND_SHAPES} >= {(0, 0), (1, 1), (255, 31)}
    both = {(min(x, 3), min(y, 3)) for x, y in (rc.bands(w, h) for w, h in ALL_8BIT)}
    assert both == {(x, y) for x in (1, 2, 3) for y in (1, 2, 3)}, both
    assert all(rc.bands(w, h)[0] > 1 and rc.bands(w, h)[1] > 1 for w, h in rc.FRONT_END_SHAPES)


def test_scales_column_groups_and_row_groups():
    assert any(rc.nscales(w, h) == 6 for w, h in gpu_cases.SIZES)
    assert {rc.nscales(w, h) for w, h in gpu_cases.SIZES} == {0, 2, 3, 4, 5, 6}   # 8 x 8 has a 4 x 4 scale behind it
    assert any(rc.column_groups(w, h)[0] >= 30 for w, h in gpu_cases.SIZES if rc.nscales(w, h))
    assert any(rc.row_groups(w, h)[0] >= 50 for w, h in gpu_cases.SIZES if rc.nscales(w, h))
    for w, h in rc.LONG_SHAPES:
        assert max(w, h) > 65_535 and rc.nscales(w, h) == 2
    assert rc.column_groups(65_600, 9) == [1025, 513] and rc.row_groups(9, 65_600) == [3280, 1640]


def test_describe_names_what_a_shape_is_there_for():
    assert rc.describe(383, 21).startswith("383x21: (nmain, ntiles) = (5, 7), two-tile trips 2, bands 2 x 1, 3 scales")
    assert "trips 1 + a leftover" in rc.describe(319, 21)
    for w, h in ALL_8BIT:
        print(rc.describe(w, h))
