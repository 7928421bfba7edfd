"""Batches of the recursive blur modes on the size grid and at tile and band edges (MI355X; DESIGN.md sections 18 to 20).

The contract is the one tests/test_gpu_rbatch.py, test_gpu_hbatch.py and test_gpu_abatch.py state: the score and all 108
averages of every item of a batch have the BITS of the item's single score in the same mode on a fresh plain context.
Every item of every batch is compared, the batch runs behind a larger batch of other content on the same context, and
there is no tolerance anywhere but in the one anchor of section (f).  The items of a batch differ in content wherever the
section makes them (seeded noise); section (e) takes the hard pairs as they are, and some of those share a frame.

What is new is where the batches run (tests/rbatch_cases.py names the counts; tests/test_rbatch_cases.py holds the lists to
them).  The batch kernels have text of their own, so none of this was reached through the single scores:

(a) 8-bit batches at every size of gpu_cases.SIZES: six scales, up to 31 column groups and 55 row groups at scale 0 (the
    items-fastest job numbering of the against-reference form, all of hblk_end[] / vblk_end[]), 200 row groups and 401
    ten-row batches per column job at 8 x 4000, 63 tiles per row at 4000 x 8, no scale at all below 8 px.
(b) the horizontal pass at every (main tiles, edge tiles behind them) and every trip count of the two-tile loop of the
    pair form's reference pass (two register sets), at height 21.
(c) the conversion at 1 x 1, 2 x 2, 3 x 3 and 3 x 2 bands, ragged and exact, 8-bit with 3 and 5 items and 16-bit at depths
    10 and 16, and device frames a stride apart at 3 x 3 bands.
(d) 65,600 columns and 65,600 rows: the block counts of a frame past 2^16, times the items.
(e) the pairs that reach the clamps and the zero paths (gpu_cases.HARD_GROUPS), a group a batch.
(f) the YUV, YUV-with-alpha and RGBA front ends at more than one band across and down; and two items of a pair batch
    against the kernel-order terms of the CPU checker (gpu_cases.check_against_terms at RTOL_RECURSIVE and FINALIZE_TOL,
    whose derivation covers every frame of at most MAX_TERMS pixels): the one hold that does not rest on the device's own
    single score."""
import numpy as np
import pytest

import chroma_ref
import gpu_cases
import rbatch_cases as rc
import yuva_ref
from oavif_amd import Ssimu2, synth
from test_gpu_abatch import (batch_results, item_alpha, single_result, yuva_items, make_stale as make_stale_rgba,
                             pool as pool_rgba, same_bits as same_result, set_reference as set_reference_alpha)
from test_gpu_chroma import frame_of
from test_gpu_hbatch import (damaged_planes, pool16, make_stale as make_stale16, hold_items as hold_items16,
                             run_both_forms as run_both_forms16)
from test_gpu_rbatch import hold_items, make_stale, pool, run_both_forms, singles
from test_gpu_yuva import alpha_of

pytestmark = pytest.mark.gpu

RECURSIVE = ("recursive", "recursive_fma")


def _contexts(**flag):
    @pytest.fixture(scope="module")
    def contexts(hip_lib):
        out = {mode: Ssimu2(0, blur=gpu_cases.MODES[mode][0], **flag) for mode in RECURSIVE}
        yield out
        for s in out.values():
            s.close()
    return contexts


ctxs = _contexts(rbatch=True)     # the 8-bit calls
hctxs = _contexts(hbatch=True)    # the 16-bit and YUV calls
actxs = _contexts(abatch=True)    # the RGBA and YUV-with-alpha calls

_frames = {}


def frames(w, h, n):
    """test_gpu_rbatch.pool(w, h, n), made once per size (a longer pool starts with a shorter one)."""
    have = _frames.get((w, h))
    if have is None or len(have[0]) < n:
        have = _frames[(w, h)] = pool(w, h, n)
    return have[0][:n], have[1][:n]


def ids(shapes):
    return [f"{w}x{h}" for w, h in shapes]


def hold_8bit(s, mode, w, h, counts):
    print("shape:", rc.describe(w, h))
    refs, dists = frames(w, h, max(counts))
    for n in counts:
        run_both_forms(s, mode, w, h, n, refs, dists)
    pair, against = singles(mode, w, h, max(counts))
    if rc.nscales(w, h) == 0:
        assert all(sc == 100.0 and ns == 0 and not avg.any() for sc, avg, ns in pair + against)
    else:
        assert pair[0][2] == against[0][2] == rc.nscales(w, h) and pair[0][0] < 100.0
        assert len({sc for sc, _avg, _ns in pair[:3]}) == min(3, len(pair))   # the items differ: a misplaced one is seen


# ---- (a) the size grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", gpu_cases.SIZES, ids=ids(gpu_cases.SIZES))
def test_a_8bit_batches_on_the_size_grid(ctxs, mode, w, h):
    hold_8bit(ctxs[mode], mode, w, h, (3, 7) if w * h <= rc.SEVEN_ITEMS_UP_TO else (3,))


# ---- (b) tile classes of the horizontal pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.TILE_SHAPES, ids=ids(rc.TILE_SHAPES))
def test_b_tile_classes_of_the_horizontal_pass(ctxs, mode, w, h):
    print(f"{w}x{h}: (nmain, ntiles) = {rc.h_tiles(w)}, two-tile loop (trips, leftover) = {rc.pair_loop(w)}")
    hold_8bit(ctxs[mode], mode, w, h, (3,))   # the pair form is the one that runs k_rg_h_batch<., true> (AHEAD = 2)


# ---- (c) band edges of the conversion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.BAND_SHAPES, ids=ids(rc.BAND_SHAPES))
def test_c_8bit_batches_at_the_band_edges(ctxs, mode, w, h):
    print(f"{w}x{h}: bands {rc.bands(w, h)}")
    hold_8bit(ctxs[mode], mode, w, h, (3, 5))   # 5: per_item * item is odd against every band count


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("depth", [10, 16])
@pytest.mark.parametrize("w,h", rc.BAND_SHAPES, ids=ids(rc.BAND_SHAPES))
def test_c_16bit_batches_at_the_band_edges(hctxs, mode, w, h, depth):
    print(f"{w}x{h}: bands {rc.bands(w, h)}")
    refs, dists = pool16(w, h, 3, depth)
    run_both_forms16(hctxs[mode], mode, w, h, depth, 3, refs, dists)


@pytest.mark.parametrize("mode", RECURSIVE)
def test_c_device_frames_a_stride_apart_at_three_bands_by_three(ctxs, mode):
    """Both device forms at 513 x 65 with in_stride not the frame's own size and noise between the frames (as
    tests/test_gpu_rbatch.py does at 121 x 40, where a frame is one band)."""
    import torch
    s, (w, h), n = ctxs[mode], (513, 65), 3
    assert rc.bands(w, h) == (3, 3)
    refs, dists = frames(w, h, n)
    pair, against = singles(mode, w, h, n)
    stride = w * h * 3 + 52
    bufs = []
    for k, side in enumerate((refs, dists)):
        g = torch.Generator().manual_seed(k)
        buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, generator=g)
        for i, f in enumerate(side):
            buf[i * stride:i * stride + f.size] = torch.from_numpy(f.reshape(-1))
        bufs.append(buf.cuda())
    torch.cuda.synchronize()
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_device(bufs[0].data_ptr(), bufs[1].data_ptr(), stride, n, w, h), pair, f"{mode} device pairs")
    s.set_reference_device(bufs[0].data_ptr(), w, h)
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_against_reference_device(bufs[1].data_ptr(), stride, n), against, f"{mode} device against")


# ---- (d) frames past 2^16 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.LONG_SHAPES, ids=ids(rc.LONG_SHAPES))
def test_d_8bit_batches_of_long_frames(ctxs, mode, w, h):
    hold_8bit(ctxs[mode], mode, w, h, (2,))


def test_d_a_12bit_batch_of_tall_frames(hctxs):
    mode, (w, h), depth = "recursive_fma", (9, 65_600), 12
    refs, dists = pool16(w, h, 2, depth)
    run_both_forms16(hctxs[mode], mode, w, h, depth, 2, refs, dists)


# ---- (e) hard content --------------------------------------------------------------------------------------------------
_hard = {}


def hard_pairs(group):
    if group not in _hard:
        _hard[group] = [(np.ascontiguousarray(r), np.ascontiguousarray(d)) for r, d in gpu_cases.group_pairs(group)]
    return _hard[group]


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("group", gpu_cases.HARD_GROUPS)
def test_e_hard_content_a_group_a_batch(ctxs, mode, group):
    """The group's pairs as one pair batch; against the group's first reference, all its distorted frames and the
    reference itself as one against-reference batch.  An item whose single score is exactly 100 with every average 0 has
    those bits too: bits_equal compares all of them."""
    s = ctxs[mode]
    pairs = hard_pairs(group)
    refs, dists = [r for r, _d in pairs], [d for _r, d in pairs]
    h, w, _ = refs[0].shape
    assert all(f.shape == (h, w, 3) for f in refs + dists)
    items = dists + [refs[0]]
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as one:
        pair = [(one.compute_ssimu2(r, d), *one.last_averages()) for r, d in pairs]
        one.set_reference(refs[0])
        against = [(one.score_against_reference(d), *one.last_averages()) for d in items]
    zeros = [int((avg[:ns] == 0).sum()) for _sc, avg, ns in pair]
    print(f"{mode} {group} {w}x{h}: {len(pairs)} pairs, scores {[sc for sc, _a, _n in pair]}, averages exactly 0: {zeros}")
    make_stale(s, w, h, len(pairs))
    hold_items(s, s.score_batch(refs, dists), pair, f"{mode} {group} pairs")
    s.set_reference(refs[0])
    make_stale(s, w, h, len(items))
    hold_items(s, s.score_batch_against_reference(items), against, f"{mode} {group} against")


# ---- (f) the other front ends at more than one band, and an independent anchor -----------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("fmt,depth", [(chroma_ref.YUV_420, 10), (chroma_ref.YUV_422, 8)], ids=["420-10", "422-8"])
@pytest.mark.parametrize("w,h", rc.FRONT_END_SHAPES, ids=ids(rc.FRONT_END_SHAPES))
def test_f_yuv_batches(hctxs, mode, w, h, fmt, depth):
    s, n, up = hctxs[mode], 3, chroma_ref.BILINEAR
    full_range, mc = depth == 10, (6, 1)[depth == 8]
    ref = synth.make_ref(w, h, seed=31)
    planes = [damaged_planes(w, h, depth, full_range, mc, fmt, i) for i in range(n)]
    laid = [frame_of(p, depth, full_range, mc, fmt, i) for i, p in enumerate(planes)]   # (frame, the buffers it views)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], chroma=True) as one:
        one.set_reference(ref)
        exp = [(one.score_against_reference_yuv(f, 16, up), *one.last_averages()) for f, _bufs in laid]
    assert len({sc for sc, _avg, _ns in exp}) == n and all(sc < 100.0 for sc, _avg, _ns in exp)
    s.set_reference(ref)
    make_stale16(s, w, h, n)
    scores = s.score_batch_against_reference_yuv([f for f, _bufs in laid], 16, up)
    hold_items16(s, scores, exp, f"{mode} {w}x{h} YUV format {fmt} depth {depth}")


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.FRONT_END_SHAPES, ids=ids(rc.FRONT_END_SHAPES))
def test_f_yuva_batches(actxs, mode, w, h):
    s, n, depth, fmt, up = actxs[mode], 3, 8, yuva_ref.FORMATS["420"], chroma_ref.BILINEAR
    how = (w, h, "yuva", depth, fmt, True, 6, 0x1A80E6, 16, up)
    items = yuva_items(w, h, n, depth, fmt, True, 6)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], yuva=True) as one:
        set_reference_alpha(one, *how)
        exp = [single_result(one, one.score_against_reference_yuva(f, 16, up)) for f in items]
    assert len({r[0] for r in exp}) == n and all(r[0] < 100.0 for r in exp)
    make_stale_rgba(s, w, h, n)
    set_reference_alpha(s, *how)
    got = batch_results(s, s.score_batch_against_reference_yuva(items, 16, up))
    for i in range(n):
        same_result(got[i], exp[i], (mode, w, h, "yuva", i))


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.FRONT_END_SHAPES, ids=ids(rc.FRONT_END_SHAPES))
def test_f_rgba_batches_in_both_forms(actxs, mode, w, h):
    s, n, bg = actxs[mode], 3, 0x7B3FC2
    rgb, dists = pool_rgba(w, h, n)
    ref = np.dstack([rgb, alpha_of(w, h, 8, 0)])
    items = [np.dstack([d, item_alpha(w, h, 8, i)]) for i, d in enumerate(dists)]
    refs = [items[(i + 1) % n] for i in range(n)]     # the pair form: item i against the next item's frame
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], yuva=True) as one:
        one.set_reference_rgba(ref, bg)
        against = [single_result(one, one.score_against_reference_rgba(f)) for f in items]
        pair = [single_result(one, one.compute_ssimu2_rgba(r, d, bg)) for r, d in zip(refs, items)]
    assert len({r[0] for r in against}) == n and len({r[0] for r in pair}) == n
    make_stale_rgba(s, w, h, n)
    s.set_reference_rgba(ref, bg)
    got = batch_results(s, s.score_batch_against_reference_rgba(items))
    for i in range(n):
        same_result(got[i], against[i], (mode, w, h, "rgba against", i))
    make_stale_rgba(s, w, h, n)
    got = batch_results(s, s.score_batch_rgba(refs, items, bg))
    for i in range(n):
        same_result(got[i], pair[i], (mode, w, h, "rgba pair", i))


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", rc.FRONT_END_SHAPES, ids=ids(rc.FRONT_END_SHAPES))
def test_f_two_items_of_a_pair_batch_against_the_kernel_order_terms(ctxs, oracle, mode, w, h):
    s, n = ctxs[mode], 3
    assert w * h <= gpu_cases.MAX_TERMS
    refs, dists = frames(w, h, n)
    make_stale(s, w, h, n)
    scores = s.score_batch(refs, dists)
    for k in (0, 2):
        avg, ns = s.last_batch_averages(k)
        assert ns == rc.nscales(w, h)
        gpu_cases.check_against_terms(oracle, scores[k], avg, ns, refs[k], dists[k], mode, f"{mode} {w}x{h} item {k}")
