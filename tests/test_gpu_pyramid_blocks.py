"""The band pyramid of the pair score (k_pyramid_bands, k_pyramid_bands_batch) on the MI355X at sizes that cross every
branch of the kernel, bit for bit against the CPU checker's downsample2 chained from the table planes:

  (8, 8)      one level; a single whole 4 x 4 block row and column
  (9, 11)     clamped blocks in x and y, odd width and height, odd w1 = 5 (no 8-byte level-1 stores)
  (257, 33)   one pixel past the 256-column and the 32-row band edge: bands that hold a single clamped block
  (259, 35)   the same with three pixels past; w1 = 130 is even, so whole blocks pair their level-1 stores
  (515, 67)   three bands across and down; w1 = 258 even, w2 = 129 odd, clamped level-2 and LDS-level sources
  (1021, 31)  four bands across, one short band down; odd w1 = 511: every level-1 row starts 4 bytes off 8

A wave of the kernel is one thread row and forms its row addresses on the scalar unit; a lane adds a 32-bit offset.
The sizes put a row's first and last lane, the first and last thread row and the first and last band on either side
of every such address."""
import numpy as np
import pytest

from oavif_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 11), (257, 33), (259, 35), (515, 67), (1021, 31)]
BATCH_LIN_REF, BATCH_LIN_DIST, BATCH_ITEM = 6, 7, 8   # SSIMU2_DEBUG_BATCH_* (include/ssimu2_hip_internal.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("w,h", SIZES)
def test_every_level_of_both_frames_is_bit_identical(iscorer, oracle, w, h):
    ref = synth.make_ref(w, h, 11 * w + h)
    dist = synth.distort(ref, "noise", 2, seed=1)
    lut = oracle.srgb_lut()
    lin = [np.ascontiguousarray(lut[f].transpose(2, 0, 1)) for f in (ref, dist)]
    iscorer.compute_ssimu2(ref, dist)
    _, ns = iscorer.last_averages()
    assert ns >= 2
    for s in range(1, ns):
        lin = [oracle.downsample2(a) for a in lin]
        for what in (0, 1):
            got = iscorer.debug_download(what, s, w, h)
            assert got.shape == lin[what].shape, (s, what)
            assert np.array_equal(bits(got), bits(lin[what])), (s, what)


def test_every_item_of_a_batch_has_the_single_calls_planes(iscorer):
    """k_pyramid_bands_batch: the item's share of blockIdx and its input / output strides move no bit of any level."""
    w, h, n = 259, 35, 3
    refs = [synth.make_ref(w, h, 500 + k) for k in range(n)]
    dists = [synth.distort(r, "noise", 1 + k, seed=k) for k, r in enumerate(refs)]
    singles = []
    for r, d in zip(refs, dists):
        iscorer.compute_ssimu2(r, d)
        _, ns = iscorer.last_averages()
        singles.append([[iscorer.debug_download(what, s, w, h) for what in (0, 1)] for s in range(1, ns)])
    assert not np.array_equal(singles[0][-1][1], singles[1][-1][1])   # items differ down to the last level
    iscorer.score_batch(refs, dists)
    for k in range(n):
        for s in range(1, ns):
            for what, code in ((0, BATCH_LIN_REF), (1, BATCH_LIN_DIST)):
                got = iscorer.debug_download(code + BATCH_ITEM * k, s, w, h)
                assert np.array_equal(bits(got), bits(singles[k][s - 1][what])), (k, s, what)
