"""Full-depth error maps (include/ssimu2_hip_map.h) on the size grid, on hard content and on frames
65,600 to 100,000 px long, in all three blur modes (-m gpu only).

tests/test_gpu_map_hbd.py holds the 16-bit, RGBA and YUV maps at eight sizes up to 250 x 130; this module takes
k_march_map_lin (march_body<MARCH_MAP, true>), k_lin0_of_u8, k_rg_vmap / k_map_compose over the planes a 16-bit score
leaves, and map_against's ref.lin0 bookkeeping to where the 8-bit map is already held:

1. the 16-bit pair map against numpy (map_cases.check_pair_hbd, unchanged) at the sizes of GRID, one depth per size
   cycling 9..16; every map call follows, on the same context, a map of other content at a strictly larger size, so that
   map_ensure's replace-on-different-size path and foreign bytes in map.dens / hbd.lin0_* are part of every case; a
   repeated map has the first one's bits;
2. every pair of gpu_cases.HARD_GROUPS: (a) lifted to the codes 257 u at depth 16 the score, averages and map have the
   bits of the 8-bit error_map of the same pair on the same context (itself held to numpy by test_gpu_error_map.py),
   (b) brought to 10 bits the pair is held to numpy by check_pair_hbd, finite, and identical pairs score 100 with an
   all-zero map;
3. W1 = 65,600 x 9 (all modes) and T1 = 9 x 100,000 (fir, recursive) on 10-bit content: the pair map against numpy;
   the map against a 16-bit reference; the map against an 8-bit reference (k_lin0_of_u8 at n = 590,400 and 900,000,
   twice: the second call finds the planes the first one made, and a later score is what it was before the maps); the
   YUV and the opaque RGBA map of W1 (fir).

The rule is map_cases.hold_map's and nothing else: recursive modes bit for bit; FIR per pixel within gpu_cases.MAP_K *
2^-24 and 0 exactly where the reference is 0; the mean to errmap_ref.MEAN_RTOL.  Identities between two device results are
held bit for bit.  The CPU reference of a long frame is computed once per (shape, mode), where its pair map is held, and
the device results it was held with are kept for the identities."""
import numpy as np
import pytest

import gpu_cases
import hbd_cases
import yuv_ref
from gpu_cases import MW, same_bits, scale_size
from map_cases import assert_bits, check_pair_hbd, results
from oavif_amd import synth
from ssimu2_fp64 import nscales_of
from test_gpu_alpha import laid_out, rgba_of
from test_gpu_yuv import frame_of, yuv_pair

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
RG_VW = 64                       # columns per vertical job (oavif_amd/csrc/ssimu2_recursive.h)
BAND_W, BAND_H = 256, 32         # k_pyramid_bands' band (oavif_amd/csrc/ssimu2_kernels.h)

# size -> what it reaches that 121 x 9 and 129 x 67 (tests/test_gpu_map_hbd.py) do not
GRID = [
    (119, 40), (120, 40), (241, 33),     # FIR strip edges (MW = 120): one short of a strip, a whole one, one past two
    (65, 21), (129, 41),                 # 64-column recursive tile / batch edges
    (257, 33), (259, 35),                # one and three pixels past the 256 x 32 pyramid band (k_pyramid_bands16's lin0)
    (513, 259),                          # three bands across, nine down; six scales, all ragged (257, 129, 65, 33, 17)
    (1000, 9), (9, 1000),                # one segment row of strips; one strip of segments
    (4160, 75),                          # 387 vertical jobs > CUs: a second job per k_rg_vmap workgroup
]

mctxs = gpu_cases.contexts_fixture(maps=True, extended=True, yuv=True)


def vertical_jobs(w, h):
    ns = nscales_of(w, h)
    return 3 * sum(-(-scale_size(w, h, s)[0] // RG_VW) for s in range(ns)), ns


def foreign_map(s, w, h, k):
    """A 16-bit map of other content (noise against noise, another depth) at a strictly larger size: the map buffers
    are replaced before and after it, and map.dens, map.out and hbd.lin0_* hold its values afterwards."""
    d = 9 + (k + 3) % 8
    big = hbd_cases.hbd_content("hnoise", w + 41, h + 23, d, 1000 + k)
    other = hbd_cases.hbd_content("hnoise", w + 41, h + 23, d, 2000 + k)
    score, m = s.error_map_hbd(big, other, d)
    assert m.shape == (h + 23, w + 41) and score < 100.0 and m.any()


# ---- 1. the size grid ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", GRID, ids=[f"{w}x{h}" for w, h in GRID])
@pytest.mark.parametrize("mode", MODES)
def test_pair_map_on_the_size_grid(mctxs, oracle, mode, size):
    w, h = size
    s = mctxs[mode]
    k = GRID.index(size)
    d = 9 + k % 8
    jobs, ns = vertical_jobs(w, h)
    if size == (4160, 75):
        assert ns == 5 and jobs == 387 and jobs > s.device_info()["compute_units"], (jobs, s.device_info())
    if size == (513, 259):
        assert ns == 6 and -(-w // BAND_W) == 3 and -(-h // BAND_H) == 9
    if size in ((257, 33), (259, 35)):
        assert -(-w // BAND_W) == 2 and -(-h // BAND_H) == 2
    if size == (241, 33):
        assert -(-w // MW) == 3 and w - 2 * MW == 1
    ref = hbd_cases.content16(w, h, d, seed=w + h)
    dist = hbd_cases.content16(w, h, d, seed=w + h, distort=True)
    what = f"{mode} {w}x{h} depth {d}"
    foreign_map(s, w, h, k)
    _worst, score, m = check_pair_hbd(oracle, s, mode, ref, dist, d, what)
    first = results(s, score)
    assert first[2] == ns and 0.0 < score < 100.0, what
    score2, m2 = s.error_map_hbd(ref, dist, d)                  # the same size: the buffers stay
    assert_bits(results(s, score2), first, what + " second map")
    same_bits(m2, m, what + " second map")
    foreign_map(s, w, h, k + 1)
    score3, m3 = s.error_map_hbd(ref, dist, d)                  # behind another larger frame: replaced again
    assert_bits(results(s, score3), first, what + " map after a larger frame")
    same_bits(m3, m, what + " map after a larger frame")


# ---- 2. hard content -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", gpu_cases.HARD_GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_hard_content_through_the_full_depth_path(mctxs, oracle, mode, group):
    """Black against white, flat against noise, saturated primaries, a 1-px checkerboard, thin text and frames that
    differ in one sample (L4 coefficients up to 3e27, densities down to the subnormal edge) through k_march_map_lin and
    the 16-bit recursive route."""
    s = mctxs[mode]
    for i, (ref, dist) in enumerate(gpu_cases.group_pairs(group)):
        what = f"{mode} {group} {i}"
        score8, m8 = s.error_map(ref, dist)
        exp = results(s, score8)
        score, m = s.error_map_hbd(hbd_cases.lift(ref), hbd_cases.lift(dist), 16)
        assert_bits(results(s, score), exp, what + " 257 u")
        same_bits(m, m8, what + " 257 u")
        # one seed for both frames: what the pair shares it still shares at 10 bits, identical pairs stay identical
        r10, d10 = hbd_cases.to_depth(ref, 10, 77 + i), hbd_cases.to_depth(dist, 10, 77 + i)
        _worst, score10, m10 = check_pair_hbd(oracle, s, mode, r10, d10, 10, what + " 10-bit")
        assert np.isfinite(m10).all(), what
        if np.array_equal(ref, dist):
            assert np.array_equal(r10, d10) and score10 == 100.0 and not m10.any(), what


# ---- 3. long frames ----------------------------------------------------------------------------------------------------
SHAPES = {"W1": (65_600, 9), "T1": (9, 100_000)}
LONG_CASES = [("W1", "fir"), ("W1", "recursive"), ("W1", "recursive_fma"), ("T1", "fir"), ("T1", "recursive")]
_FRAMES10 = {}    # shape -> (ref, dist) of 10 bits
_FRAMES8 = {}     # shape -> (rgb8 reference, its distortion)
_PAIR = {}        # (shape, mode) -> (results, map) of the pair map, held to numpy once


def frames10(shape):
    if shape not in _FRAMES10:
        w, h = SHAPES[shape]
        _FRAMES10[shape] = (hbd_cases.content16(w, h, 10, w + 2), hbd_cases.content16(w, h, 10, w + 2, distort=True))
    return _FRAMES10[shape]


def frames8(shape):
    if shape not in _FRAMES8:
        w, h = SHAPES[shape]
        ref = synth.make_ref(w, h, 17 * w + h)
        _FRAMES8[shape] = (ref, synth.distort(ref, "noise", 2, seed=w + 3 * h))
    return _FRAMES8[shape]


def held_pair(oracle, s, mode, shape):
    """The 10-bit pair map of a long shape, held to numpy by check_pair_hbd the first time it is asked for."""
    if (shape, mode) not in _PAIR:
        w, h = SHAPES[shape]
        r10, d10 = frames10(shape)
        foreign_map(s, w, h, 5)
        _worst, score, m = check_pair_hbd(oracle, s, mode, r10, d10, 10, f"{mode} {shape} {w}x{h} 10-bit")
        assert m.shape == (h, w) and 0.0 < score < 100.0 and s.last_averages()[1] == 2
        _PAIR[shape, mode] = (results(s, score), m)
    return _PAIR[shape, mode]


@pytest.mark.parametrize("shape,mode", LONG_CASES)
def test_long_frame_pair_map_and_the_map_against_a_16_bit_reference(mctxs, oracle, shape, mode):
    s = mctxs[mode]
    w, h = SHAPES[shape]
    r10, d10 = frames10(shape)
    pair, pair_map = held_pair(oracle, s, mode, shape)
    what = f"{mode} {shape}"
    foreign_map(s, w, h, 6)
    s.set_reference_hbd(r10, 10)
    assert gpu_cases.scrub(s, r10, 10) == 100.0
    for rep in range(2):
        score, m = s.error_map_against_reference_hbd(d10, 10)
        assert_bits(results(s, score), pair, f"{what} against a 16-bit reference, call {rep}")
        same_bits(m, pair_map, f"{what} against a 16-bit reference, call {rep}")


@pytest.mark.parametrize("shape,mode", LONG_CASES)
def test_long_frame_map_against_an_8_bit_reference(mctxs, shape, mode):
    """k_lin0_of_u8 over w * h = 590,400 (W1) and 900,000 (T1) pixels in FIR; map_against's bookkeeping in every mode."""
    s = mctxs[mode]
    w, h = SHAPES[shape]
    assert w * h == {"W1": 590_400, "T1": 900_000}[shape]
    rgb8, drgb = frames8(shape)
    d16 = hbd_cases.to_depth(drgb, 16, 3)
    what = f"{mode} {shape} 8-bit reference"
    foreign_map(s, w, h, 7)
    exp_score, exp_map = s.error_map_hbd(hbd_cases.lift(rgb8), d16, 16)
    exp = results(s, exp_score)
    assert 0.0 < exp_score < 100.0 and exp_map.any()
    foreign_map(s, w, h, 8)                                      # hbd.lin0_ref holds a larger frame's planes
    s.set_reference(rgb8)
    before = results(s, s.score_against_reference_hbd(d16, 16))
    assert_bits(before, exp, what + " score")
    for rep in range(2):                                         # the second call finds the planes the first one made
        score, m = s.error_map_against_reference_hbd(d16, 16)
        assert_bits(results(s, score), exp, f"{what} call {rep}")
        same_bits(m, exp_map, f"{what} call {rep}")
    assert_bits(results(s, s.score_against_reference_hbd(d16, 16)), before, what + " the score after the maps")


def test_long_yuv_frame_map_is_the_rgb16_map_of_its_codes(mctxs):
    s = mctxs["fir"]
    w, h = SHAPES["W1"]
    rp, dp = yuv_pair(w, h, 10, False, 1, 3)
    rf, _rb = frame_of(rp, 10, False, 1, yuv_ref.YUV_444, 3)
    df, _db = frame_of(dp, 10, False, 1, yuv_ref.YUV_444, 4)
    cr, cd = s.convert_yuv(rf, 10), s.convert_yuv(df, 10)
    assert np.array_equal(cr, yuv_ref.codes(*rp, 10, False, 1, 10)) and np.array_equal(cd, yuv_ref.codes(*dp, 10, False, 1, 10))
    exp_score, exp_map = s.error_map_hbd(cr, cd, 10)
    exp = results(s, exp_score)
    assert 0.0 < exp_score < 100.0
    foreign_map(s, w, h, 9)
    score, m = s.error_map_yuv(rf, df, 10)
    assert_bits(results(s, score), exp, "W1 YUV map")
    same_bits(m, exp_map, "W1 YUV map")


def test_long_opaque_rgba_frame_map_is_the_8_bit_map(mctxs):
    s = mctxs["fir"]
    w, h = SHAPES["W1"]
    rgb, drgb = frames8("W1")
    score8, m8 = s.error_map(rgb, drgb)
    exp = results(s, score8)
    assert 0.0 < score8 < 100.0
    _br, r4 = laid_out(rgba_of(rgb, 255), 4 * w + 5, 1, seed=1)
    _bd, d4 = laid_out(rgba_of(drgb, 255), 4 * w + 12, 2, seed=2)
    foreign_map(s, w, h, 10)
    score, m = s.error_map_rgba(r4, d4, 0xE680FF)
    assert_bits(results(s, score), exp, "W1 opaque RGBA map")
    same_bits(m, m8, "W1 opaque RGBA map")
