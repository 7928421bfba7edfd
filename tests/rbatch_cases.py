"""Shapes for the batches of the recursive blur modes (tests/test_gpu_rbatch_grid.py) and a plain restatement of the
geometry they are chosen by.  Importable without a GPU; tests/test_rbatch_cases.py holds the lists to the classes they
are here for and the constants below to the source lines they restate.

The batch kernels have text of their own (k_pyramid_bands_xyb_batch, k_pyramid_bands_xyb16_batch<3>, k_rg_h_batch with its
own instantiations of rg_h_line, k_rg_v_emit_batch, k_rg_v_batch), so what the single scores meet on gpu_cases.SIZES
says nothing about them.  What can go wrong in a batch is placement -- an item, a band, a tile's register set, a job or
a partial sum in the wrong place -- and placement follows the counts restated here."""
from ssimu2_fp64 import scale_size

# each constant with the line it restates: name -> (value, file under oavif_amd/csrc, the line's text)
SOURCE_LINES = {
    "RG_TW": (64, "ssimu2_recursive.h", "constexpr int RG_TW = 64;          // columns per staged tile"),
    "RG_N": (5, "ssimu2_recursive.h", "constexpr int RG_N = 5;         // radius of the sigma-1.5 recursion"),
    "RG_HL": (20, "ssimu2_recursive.h", "constexpr int RG_HL = 20;       // image rows per wave of the horizontal pass"),
    "RG_VW": (64, "ssimu2_recursive.h", "constexpr int RG_VW = 64;       // columns per workgroup of the vertical pass"),
    "RG_H_AHEAD_REF": (2, "ssimu2_recursive.h", "constexpr int RG_H_AHEAD_REF = 2;"),
    "RG_H_AHEAD_PASS": (1, "ssimu2_recursive.h", "constexpr int RG_H_AHEAD_PASS = 1;"),
    "PYR_THREADS": (512, "ssimu2_kernels.h", "constexpr int PYR_THREADS = 512;"),
    "PYR_TX": (64, "ssimu2_kernels.h", "constexpr int PYR_TX = PYR_THREADS / 8;"),
    "PYR_BAND": ((256, 32), "ssimu2_kernels.h", "constexpr int PYR_BAND_W = 4 * PYR_TX, PYR_BAND_H = 32;"),
    # the expressions of rg_h_line and of the host's plans that the functions below restate
    "ntiles": (None, "ssimu2_recursive.h", "const int ntiles = (w + (RG_N - 1) + RG_TW - 1) / RG_TW;"),
    "nmain": (None, "ssimu2_recursive.h", "const int nmain = max(1, w / RG_TW);"),
    "pair loop": (None, "ssimu2_recursive.h", "for (; T + 1 < nmain; T += 2) {"),
    "leftover": (None, "ssimu2_recursive.h", "if (T < nmain) {"),
    "bands": (None, "ssimu2_hip.hip", "return (long long)((w + PYR_BAND_W - 1) / PYR_BAND_W) * ((h + PYR_BAND_H - 1) / PYR_BAND_H);"),
    "vgroups": (None, "ssimu2_hip.hip", "rp->vgroups[s] = (p.w[s] + RG_VW - 1) / RG_VW;"),
    "hblk_end": (None, "ssimu2_hip.hip", "rp->hblk_end[s] = n.hblocks += 3 * ((p.h[s] + RG_HL - 1) / RG_HL);"),
}
RG_TW, RG_N, RG_HL, RG_VW = (SOURCE_LINES[k][0] for k in ("RG_TW", "RG_N", "RG_HL", "RG_VW"))
AHEAD_REF, AHEAD_PASS = SOURCE_LINES["RG_H_AHEAD_REF"][0], SOURCE_LINES["RG_H_AHEAD_PASS"][0]
PYR_BAND_W, PYR_BAND_H = SOURCE_LINES["PYR_BAND"][0]
NUM_SCALES, MIN_SIZE = 6, 8


# ---- the geometry ------------------------------------------------------------------------------------------------------
def h_tiles(w):
    """(nmain, ntiles) of rg_h_line over a row of w columns: tile 0 and the tiles nmain .. ntiles - 1 are EDGE tiles (they
    zero what lies outside the row), tiles 1 .. nmain - 1 lie inside it.  The steps run to column w + 3."""
    return max(1, w // RG_TW), (w + (RG_N - 1) + RG_TW - 1) // RG_TW


def tile_class(w):
    """(min(nmain, 7), ntiles - nmain): how many tiles the main loop takes, capped, and how many edge tiles follow it."""
    nmain, ntiles = h_tiles(w)
    return min(nmain, 7), ntiles - nmain


def pair_loop(w):
    """The AHEAD = 2 path of rg_h_line (the reference's pass of the pair form, two register sets): -> (trips of the
    two-tile loop `for (; T + 1 < nmain; T += 2)` from T = 1, whether a leftover main tile follows it)."""
    nmain, _ = h_tiles(w)
    t, trips = 1, 0
    while t + 1 < nmain:
        t, trips = t + 2, trips + 1
    return trips, t < nmain


def loop_class(w):
    trips, leftover = pair_loop(w)
    return min(trips, 2), leftover


def nscales(w, h):
    """make_pyramid: scale s is scored iff scale s - 1 is at least 8 x 8."""
    n = 0
    while n < NUM_SCALES and min(scale_size(w, h, max(n - 1, 0))) >= MIN_SIZE:
        n += 1
    return n


def bands(w, h):
    """(bands across, bands down) of the conversion launch: PYR_BAND_W x PYR_BAND_H pixels of the frame each."""
    return -(-w // PYR_BAND_W), -(-h // PYR_BAND_H)


def column_groups(w, h):
    """ceil(w_s / 64) per scored scale: jobs per channel of the vertical pass, and partial sums per statistic."""
    return [-(-scale_size(w, h, s)[0] // RG_VW) for s in range(nscales(w, h))]


def row_groups(w, h):
    """ceil(h_s / 20) per scored scale: workgroups per channel of the horizontal pass."""
    return [-(-scale_size(w, h, s)[1] // RG_HL) for s in range(nscales(w, h))]


def describe(w, h):
    nmain, ntiles = h_tiles(w)
    trips, leftover = pair_loop(w)
    bx, by = bands(w, h)
    return (f"{w}x{h}: (nmain, ntiles) = ({nmain}, {ntiles}), two-tile trips {trips}{' + a leftover' if leftover else ''}, "
            f"bands {bx} x {by}, {nscales(w, h)} scales, column groups {column_groups(w, h)}, row groups {row_groups(w, h)}")


# ---- the shapes --------------------------------------------------------------------------------------------------------
# (b) horizontal-pass tile classes.  Height 21: two row groups, the second with one real row, so lanes shadow the last
# row.  61 .. 448: one edge tile or two after 1, 2, 3, 5, 6 and 7 main tiles; 0, 1, 2 and 3 trips of the two-tile loop,
# with a leftover (191, 384, 447) and without.  319 and 511 complete the classes: two edge tiles after four main tiles
# (one trip and a leftover, the first edge tile on the even register set) and after seven.
TILE_WIDTHS = [61, 63, 125, 127, 191, 253, 320, 383, 384, 447, 448, 319, 511]
TILE_HEIGHT = 21
TILE_SHAPES = [(w, TILE_HEIGHT) for w in TILE_WIDTHS]

# (c) conversion band edges: 1 x 1, 2 x 2 and 3 x 3 bands, ragged and exact; 513 x 33 is three bands across and two down,
# the one pair of counts up to three that neither these nor the size grid and the tile shapes have
BAND_SHAPES = [(255, 31), (256, 32), (257, 33), (512, 64), (513, 65), (513, 33)]

# (d) just past 2^16 in either direction (the smaller of the lengths of tests/test_gpu_long_frames.py)
LONG_SHAPES = [(65_600, 9), (9, 65_600)]

# (f) more than one band, ragged: the other front ends and the anchor that is not the device's own single score
FRONT_END_SHAPES = [(513, 65), (333, 217)]

# (a) N = 7 as well as N = 3 for frames of at most this many pixels
SEVEN_ITEMS_UP_TO = 333 * 217
