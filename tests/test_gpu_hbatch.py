"""Batches of 16-bit and YUV frames in the recursive blur modes on the MI355X (ssimu2_hbatch_*,
include/ssimu2_hip_hbatch.h).

The contract under test: in SSIMU2_BLUR_RECURSIVE / _FMA an item's score and its 108 averages have the BITS of its single
score in that mode -- ssimu2_score_rgb16 for the rgb16 pair form, ssimu2_score_against_reference_rgb16 for the rgb16
against-reference forms, ssimu2_score_against_reference_yuv_chroma for the YUV form -- whatever the batch's size, the
item's place and its neighbours, and item i's block of ssimu2_hbatch_convert_yuv has the bits of
ssimu2_convert_yuv_chroma on frame i and of the numpy restatement (tests/chroma_ref.py, tests/yuv_ref.py).  Every
comparison is bit for bit, every item of every batch is compared, all items of a batch differ in content (an over-read
into a neighbour's planes, a misplaced item or job changes bits), the single scores come from a fresh context without
the flag, and each batch runs behind a larger batch of other content on the same context, so the batch's scratch is stale
and larger than needed.

Shapes: the recursion's edges as in tests/test_gpu_rbatch.py, and 257 x 33, which has two pyramid bands across (256
columns each) and two down (32 rows each), so the [item][frame][band] split of the conversion launch is exercised.  The
conversion runs at tests/test_gpu_chroma.py's sizes, pitches and alignments.  The one anchor that is not the device's own
single score is the CPU checker on the restated codes, at the bounds tests/test_gpu_hbd.py holds single 16-bit scores to
(gpu_cases.score_tol, RTOL_AVG, ATOL_AVG, check_against_terms)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth, tq
from oavif_amd.scorer import YuvFrame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref  # noqa: E402
import gpu_cases  # noqa: E402
import hbd_ref  # noqa: E402
import yuv_ref  # noqa: E402
from gpu_cases import bits_equal, damaged, neighbours, on_device  # noqa: E402
from test_gpu_chroma import MATRIX_CODES, SIZES, TALL, UPSAMPLINGS, frame_of  # noqa: E402
from test_gpu_yuv import _Handed, same_codes  # noqa: E402

pytestmark = pytest.mark.gpu

RECURSIVE = ("recursive", "recursive_fma")
DEPTHS = (8, 10, 12, 16)
COUNTS = (1, 2, 3, 5, 17)
# (w, h) -> the batch sizes scored at it
SHAPES = {
    (24, 17): COUNTS,            # w < 64, h < 20: one row group, one column group at each of its three scales
    (64, 20): (3,),              # exactly RG_VW columns and RG_HL rows
    (65, 21): (3,),              # one past both
    (121, 40): COUNTS,           # two column groups, two row groups
    (241, 100): (3,),            # four column groups, five row groups
    (130, 200): (3,),            # 20 ten-row batches + 1
    (257, 33): (3,),             # two pyramid bands across and two down
    (16, 16): (3,),              # one scale
    (8, 8): (3,),                # one scale, the smallest
    (7, 9): (3,),                # no scale: every score exactly 100
}
FORMATS = {"444": yuv_ref.YUV_444, "400": yuv_ref.YUV_400, "422": chroma_ref.YUV_422, "420": chroma_ref.YUV_420}

ctxs = gpu_cases.contexts_fixture(hbatch=True)


# ---- content ---------------------------------------------------------------------------------------------------------
def pool16(w, h, n, depth, seed=0):
    """n pairs of w x h uint16 frames of `depth` bits, every frame of its own content (seeded noise: no two items
    alike).  Item k is a function of (w, h, depth, seed, k) alone, so a shorter pool is a prefix of a longer one."""
    top = (1 << depth) - 1
    refs, dists = [], []
    for k in range(n):
        rng = np.random.default_rng([w, h, depth, seed, k])
        r = rng.integers(0, top + 1, (h, w, 3), dtype=np.int64)
        d = np.clip(r + rng.integers(-(top // 6), top // 6 + 1, (h, w, 3)) * (k % 4 != 3), 0, top)
        d[::3, ::2] = r[::3, ::2]   # part of every frame undamaged (item 3, 7, ...: all of it)
        refs.append(r.astype(np.uint16))
        dists.append(d.astype(np.uint16))
    return refs, dists


_singles = {}


def singles16(mode, w, h, depth, n):
    """[(score, averages, nscales)] of the first n pairs of pool16(w, h, ., depth): the pair form's singles and, against
    the pool's reference 0, the against form's; on a fresh plain context in `mode`, computed once and kept."""
    key = (mode, w, h, depth)
    have = _singles.get(key)
    if have is None or len(have[0]) < n:
        refs, dists = pool16(w, h, n, depth)
        pair, against = [], []
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as s:
            for r, d in zip(refs, dists):
                sc = s.compute_ssimu2_hbd(r, d, depth)
                pair.append((sc, *s.last_averages()))
            s.set_reference_hbd(refs[0], depth)
            for d in dists:
                sc = s.score_against_reference_hbd(d, depth)
                against.append((sc, *s.last_averages()))
        have = _singles[key] = (pair, against)
    return have[0][:n], have[1][:n]


def make_stale(s, w, h, n):
    """A larger batch of other content on the same context: more items (up to the maximum) of a larger frame."""
    m = min(n + 3, _lib.MAX_BATCH)
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 1 << 16, (2, h + 8, w + 8, 3), dtype=np.uint16)
    s.score_batch_hbd([frames[0]] * m, [frames[1]] * m, 16)


def hold_items(s, scores, exp, what):
    assert len(scores) == len(exp), what
    for k, (sc, avg, ns) in enumerate(exp):
        got_avg, got_ns = s.last_batch_averages(k)
        assert got_ns == ns, (what, k)
        bits_equal(scores[k], got_avg, sc, avg, f"{what}: item {k}")


def run_both_forms(s, mode, w, h, depth, n, refs, dists):
    pair, against = singles16(mode, w, h, depth, n)
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_hbd(refs[:n], dists[:n], depth), pair, f"{mode} {w}x{h} depth {depth} pairs, n = {n}")
    s.set_reference_hbd(refs[0], depth)
    make_stale(s, w, h, n)   # a pair batch: it keeps the reference
    hold_items(s, s.score_batch_against_reference_hbd(dists[:n], depth), against,
               f"{mode} {w}x{h} depth {depth} against, n = {n}")


def yuv_planes(w, h, depth, fmt, seed, extremes=False):
    """Random planes of a frame of any of the four formats: [y] for 4:0:0, else [y, u, v]."""
    if fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420):
        return chroma_ref.random_planes(w, h, depth, fmt, seed, extremes)
    planes = yuv_ref.random_planes(w, h, depth, seed, extremes)
    return planes[:1] if fmt == yuv_ref.YUV_400 else planes


def yuv_codes(planes, depth, full_range, mc, rgb_depth, fmt, up):
    y, u, v = (list(planes) + [None, None])[:3]
    return chroma_ref.codes(y, u, v, depth, full_range, mc, rgb_depth, fmt, up)


def damaged_planes(w, h, depth, full_range, mc, fmt, k):
    """The planes of a damaged natural frame (item k of a wave of decodes of one image), in format `fmt`."""
    rgb = synth.make_ref(w, h, seed=31)
    dist = damaged(rgb, k) if min(w, h) >= 8 else gpu_cases.content("noise", w, h, seed=k)
    dist = dist ^ np.random.default_rng([w, h, k]).integers(0, 4, dist.shape, dtype=np.uint8)   # no two items alike
    planes = yuv_ref.forward(dist, depth, full_range, mc)
    if fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420):
        return chroma_ref.subsample(planes, fmt)
    return list(planes[:1] if fmt == yuv_ref.YUV_400 else planes)


# ---- (a) the conversion, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_of_every_item_at_every_size_pitch_and_alignment(ctxs, depth, fmt):
    n = 3
    for k, (w, h) in enumerate(SIZES):
        s = ctxs[list(gpu_cases.MODES)[k % 3]]   # the conversion works in every blur mode, FIR included
        full_range, mc = bool(k & 1), MATRIX_CODES[k % 5]
        items = [yuv_planes(w, h, depth, fmt, seed=77 * depth + 10 * k + i, extremes=(i == 1)) for i in range(n)]
        frames = [frame_of(p, depth, full_range, mc, fmt, k + i) for i, p in enumerate(items)]   # (frame, its buffers)
        big = [yuv_planes(w + 40, h + 9, depth, fmt, seed=k + i) for i in range(n + 1)]
        for up in UPSAMPLINGS:
            s.convert_yuv_batch([YuvFrame(p, depth, fmt, full_range, mc) for p in big], 16, up)   # stale and larger
            for rgb_depth in (16, depth):
                got = s.convert_yuv_batch([f for f, _ in frames], rgb_depth, up)
                assert got.shape == (n, h, w, 3) and got.dtype == np.uint16
                for i in range(n):
                    what = (w, h, depth, fmt, up, rgb_depth, i)
                    same_codes(got[i], yuv_codes(items[i], depth, full_range, mc, rgb_depth, fmt, up), what)
                    same_codes(got[i], s.convert_yuv(frames[i][0], rgb_depth, up), what + ("single",))


@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_range_matrix_and_rgb_depth(ctxs, depth, fmt):
    s, (w, h), n = ctxs["recursive"], (129, 67), 3
    k = 0
    for full_range in (True, False):
        for mc in MATRIX_CODES:
            items = [yuv_planes(w, h, depth, fmt, seed=1000 * depth + 10 * k + i, extremes=(i == 1)) for i in range(n)]
            frames = [frame_of(p, depth, full_range, mc, fmt, k + i) for i, p in enumerate(items)]
            for rgb_depth in sorted({8, depth, 16}):
                for up in UPSAMPLINGS:
                    got = s.convert_yuv_batch([f for f, _ in frames], rgb_depth, up)
                    for i in range(n):
                        same_codes(got[i], yuv_codes(items[i], depth, full_range, mc, rgb_depth, fmt, up),
                                   (depth, full_range, mc, fmt, rgb_depth, up, i))
            k += 1


@pytest.mark.parametrize("fmt", [chroma_ref.YUV_422, chroma_ref.YUV_420], ids=["422", "420"])
def test_two_tall_frames_take_a_second_round_of_rows(ctxs, fmt):
    s, (w, h), depth = ctxs["recursive_fma"], TALL[fmt], 8
    assert (h if fmt == chroma_ref.YUV_422 else (h + 1) // 2) > 65535   # more chroma rows than gridDim.y holds
    items = [yuv_planes(w, h, depth, fmt, seed=5 + i) for i in range(2)]
    # item 0 at a padded pitch off alignment (staged row by row: 2D copies), item 1 with tight rows (one copy per plane)
    frames = [frame_of(items[0], depth, True, 6, fmt, 0), (YuvFrame(items[1], depth, fmt, True, 6), None)]
    for up in UPSAMPLINGS:
        got = s.convert_yuv_batch([f for f, _ in frames], 16, up)
        for i in range(2):
            same_codes(got[i], yuv_codes(items[i], depth, True, 6, 16, fmt, up), (w, h, fmt, up, i))


# ---- (b) rgb16 batches, bit for bit against single scores ------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", list(SHAPES))
def test_every_rgb16_item_has_the_bits_of_its_single_score(ctxs, mode, w, h):
    counts = SHAPES[(w, h)]
    for depth in DEPTHS:
        refs, dists = pool16(w, h, max(counts), depth)
        for n in counts:
            run_both_forms(ctxs[mode], mode, w, h, depth, n, refs, dists)
        pair, _ = singles16(mode, w, h, depth, 1)
        if min(w, h) < 8:
            assert pair[0][0] == 100.0 and pair[0][2] == 0 and not pair[0][1].any()
        else:
            assert pair[0][2] >= 1 and pair[0][0] < 100.0


@pytest.mark.parametrize("mode", RECURSIVE)
def test_257_items_of_one_scale(ctxs, mode):
    (w, h), depth, n = (16, 16), 12, 257
    refs, dists = pool16(w, h, n, depth)
    run_both_forms(ctxs[mode], mode, w, h, depth, n, refs, dists)


@pytest.mark.parametrize("mode,depth", [("recursive", 10), ("recursive_fma", 16)])
def test_the_largest_batch(ctxs, mode, depth):
    s, (w, h), n = ctxs[mode], (8, 8), _lib.MAX_BATCH
    refs, dists = pool16(w, h, n, depth)
    run_both_forms(s, mode, w, h, depth, n, refs, dists)
    with pytest.raises(Ssimu2Error) as ei:
        s.last_batch_averages(n)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    out = (ctypes.c_double * 1)()
    assert s._L.ssimu2_hbatch_score_rgb16_device(s._ctx, 4096, 8192, w * h * 6, n + 1, w, h, depth, out) == _lib.ERR_INVALID_ARG
    assert "SSIMU2_MAX_BATCH" in s._L.ssimu2_last_error(s._ctx).decode()


@pytest.mark.parametrize("mode", RECURSIVE)
def test_device_forms_at_an_even_stride_with_noise_between_the_frames(ctxs, mode):
    import torch
    s, (w, h), depth, n = ctxs[mode], (121, 40), 10, 17
    refs, dists = pool16(w, h, n, depth)
    pair, against = singles16(mode, w, h, depth, n)
    stride = w * h * 6 + 54
    assert stride % 2 == 0 and stride % 4 == 2   # odd items start 2-byte aligned only
    bufs = []
    for k, frames in enumerate((refs, dists)):
        g = torch.Generator().manual_seed(k)
        buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, generator=g)
        for i, f in enumerate(frames):
            buf[i * stride:i * stride + f.nbytes] = torch.from_numpy(f.reshape(-1).view(np.uint8))
        bufs.append(buf.cuda())
    torch.cuda.synchronize()
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_hbd_device(bufs[0].data_ptr(), bufs[1].data_ptr(), stride, n, w, h, depth), pair,
               f"{mode} device pairs")
    s.set_reference_hbd(refs[0], depth)
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_against_reference_hbd_device(bufs[1].data_ptr(), stride, n, depth), against,
               f"{mode} device against")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_samples_above_the_depth_are_clamped(ctxs, mode):
    s, (w, h), n = ctxs[mode], (65, 21), 3
    for depth in (8, 10, 12):
        top = (1 << depth) - 1
        refs, dists = pool16(w, h, n, depth, seed=9)
        rng = np.random.default_rng(depth)
        over_r = [np.where(rng.random(f.shape) < 0.3, f | np.uint16(0xFFFF ^ top), f).astype(np.uint16) for f in refs]
        over_d = [np.where(rng.random(f.shape) < 0.3, f | np.uint16(0xFFFF ^ top), f).astype(np.uint16) for f in dists]
        assert all((f > top).any() for f in over_r + over_d)
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as plain:
            exp = [(plain.compute_ssimu2_hbd(np.minimum(r, top), np.minimum(d, top), depth), *plain.last_averages())
                   for r, d in zip(over_r, over_d)]
            single = [(plain.compute_ssimu2_hbd(r, d, depth), *plain.last_averages()) for r, d in zip(over_r, over_d)]
        make_stale(s, w, h, n)
        hold_items(s, s.score_batch_hbd(over_r, over_d, depth), exp, f"{mode} depth {depth}: read as the top code")
        hold_items(s, s.score_batch_hbd(over_r, over_d, depth), single, f"{mode} depth {depth}: as the single call reads them")
        s.set_reference_hbd(over_r[0], depth)
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as plain:
            plain.set_reference_hbd(np.minimum(over_r[0], top), depth)
            exp = [(plain.score_against_reference_hbd(np.minimum(d, top), depth), *plain.last_averages()) for d in over_d]
        hold_items(s, s.score_batch_against_reference_hbd(over_d, depth), exp, f"{mode} depth {depth}: against, clamped")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_an_items_bits_do_not_depend_on_its_place_or_its_neighbours(ctxs, mode):
    s, (w, h), depth = ctxs[mode], (121, 40), 10
    ref, dist = (f[0] for f in pool16(w, h, 1, depth, seed=77))
    for against in (False, True):
        got = []
        if against:
            s.set_reference_hbd(ref, depth)
        for at, n in ((0, 1), (3, 7), (16, 17)):
            refs, dists = pool16(w, h, n, depth, seed=at + n)
            refs[at], dists[at] = ref, dist
            make_stale(s, w, h, n)
            scores = s.score_batch_against_reference_hbd(dists, depth) if against else s.score_batch_hbd(refs, dists, depth)
            got.append((scores[at], *s.last_batch_averages(at)))
        for sc, avg, ns in got[1:]:
            assert ns == got[0][2]
            bits_equal(sc, avg, got[0][0], got[0][1], f"{mode} against={against}")
        assert 0.0 < got[0][0] < 100.0


# ---- (c) YUV batches, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))
def test_every_yuv_item_has_the_bits_of_its_single_score_and_of_the_rgb16_batch_on_its_codes(ctxs, mode, fmt):
    s = ctxs[mode]
    subsampled = fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420)
    k = 0
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], chroma=True) as plain:   # the single calls: a fresh context without the flag
        for (w, h), counts in (((9, 8), (1, 2, 5)), ((17, 33), (1, 2, 5, 17)), ((129, 67), (1, 2, 5)), ((1027, 9), (1, 2, 5))):
            ref = synth.make_ref(w, h, seed=31)
            plain.set_reference(ref)
            s.set_reference(ref)
            for depth in (8, 10):
                full_range, mc = bool(k & 1), MATRIX_CODES[k % 5]
                items = [damaged_planes(w, h, depth, full_range, mc, fmt, i) for i in range(max(counts))]
                frames = [frame_of(p, depth, full_range, mc, fmt, k + i) for i, p in enumerate(items)]
                for rgb_depth in sorted({8, depth, 16}):
                    for up in (UPSAMPLINGS if subsampled else UPSAMPLINGS[k % 2:k % 2 + 1]):
                        what = f"{mode} fmt {fmt} {w}x{h} depth {depth} rgb_depth {rgb_depth} {up}"
                        exp = [(plain.score_against_reference_yuv(f, rgb_depth, up), *plain.last_averages()) for f, _ in frames]
                        codes = [yuv_codes(p, depth, full_range, mc, rgb_depth, fmt, up) for p in items]
                        for n in counts:
                            make_stale(s, w, h, n)
                            scores = s.score_batch_against_reference_yuv([f for f, _ in frames[:n]], rgb_depth, up)
                            hold_items(s, scores, exp[:n], f"{what}, n = {n}")
                            hold_items(s, s.score_batch_against_reference_hbd(codes[:n], rgb_depth), exp[:n],
                                       f"{what}, codes, n = {n}")
                k += 1


@pytest.mark.parametrize("mode", RECURSIVE)
def test_yuv_batches_against_references_set_by_every_call(ctxs, mode):
    s, (w, h), n, depth, fmt = ctxs[mode], (129, 67), 5, 10, chroma_ref.YUV_420
    rgb = synth.make_ref(w, h, seed=12)
    rgba = np.dstack([rgb, np.random.default_rng(3).integers(0, 256, (h, w, 1), dtype=np.uint8)])
    ref_planes = chroma_ref.subsample(yuv_ref.forward(rgb, depth, False, 1), fmt)
    setters = {
        "8-bit": lambda c: c.set_reference(rgb),
        "16-bit": lambda c: c.set_reference_hbd(hbd_ref_lift(rgb), 16),
        "RGBA": lambda c: c.set_reference_rgba(rgba, (10, 200, 30)),
        "YUV": lambda c: c.set_reference_yuv(YuvFrame(ref_planes, depth, fmt, False, 1), 16, "bilinear"),
    }
    items = [damaged_planes(w, h, depth, False, 1, fmt, i) for i in range(n)]
    frames = [frame_of(p, depth, False, 1, fmt, i) for i, p in enumerate(items)]
    for name, set_ref in setters.items():
        for up in UPSAMPLINGS:
            with Ssimu2(0, blur=gpu_cases.MODES[mode][0], chroma=True, extended=True) as plain:
                set_ref(plain)
                exp = [(plain.score_against_reference_yuv(f, 16, up), *plain.last_averages()) for f, _ in frames]
            set_ref(s)
            make_stale(s, w, h, n)
            hold_items(s, s.score_batch_against_reference_yuv([f for f, _ in frames], 16, up), exp, f"{mode} {name} reference, {up}")


def hbd_ref_lift(u8):
    return np.multiply(u8, np.uint16(257), dtype=np.uint16)


# ---- (d) one independent hold: the CPU checker on the restated codes ---------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", [(121, 40), (241, 100)])
def test_a_batch_of_five_10bit_420_items_against_the_checker(ctxs, oracle, mode, w, h):
    s, depth, fmt, n = ctxs[mode], 10, chroma_ref.YUV_420, 5
    blur = gpu_cases.MODES[mode][1]
    rgb = synth.make_ref(w, h, seed=31)
    ref_planes = chroma_ref.subsample(yuv_ref.forward(rgb, depth, True, 6), fmt)
    cr = yuv_codes(ref_planes, depth, True, 6, 16, fmt, "bilinear")
    items = [damaged_planes(w, h, depth, True, 6, fmt, i) for i in range(n)]
    s.set_reference_hbd(cr, 16)
    make_stale(s, w, h, n)
    scores = s.score_batch_against_reference_yuv([YuvFrame(p, depth, fmt, True, 6) for p in items], 16, "bilinear")
    for i in range(n):
        cd = yuv_codes(items[i], depth, True, 6, 16, fmt, "bilinear")
        exp, avg_r, ns_r = hbd_ref.compute(oracle, cr, cd, 16, blur)
        avg, ns = s.last_batch_averages(i)
        what = f"{mode} {w}x{h} item {i}"
        print(f"measured: {what}: score {scores[i]!r}, checker {exp!r}, |d| {abs(scores[i] - exp):.2e}")
        assert ns == ns_r, what
        assert abs(scores[i] - exp) <= gpu_cases.score_tol(exp), (what, scores[i], exp)
        assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), what
        gpu_cases.check_against_terms(oracle, scores[i], avg, ns, cr, cd, mode, what, kavg=avg_r)


# ---- (e) lifecycle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
def test_a_pair_batch_leaves_the_cached_reference_its_pass_and_its_map_alone(hip_lib, mode):
    w, h, depth = 121, 40, 10
    ref = synth.make_ref(w, h, seed=3)
    dist = damaged(ref, 1)
    r16, d16 = pool16(w, h, 1, depth, seed=5)
    refs, dists = pool16(w + 8, h + 8, 9, depth, seed=2)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], hbatch=True) as s:
        for hbd in (False, True):
            if hbd:
                s.set_reference_hbd(r16[0], depth)
                single = lambda: s.score_against_reference_hbd(d16[0], depth)          # noqa: E731
                emap = lambda: s.error_map_against_reference_hbd(d16[0], depth)        # noqa: E731
            else:
                s.set_reference(ref)
                single = lambda: s.score_against_reference(dist)                       # noqa: E731
                emap = lambda: s.error_map_against_reference(dist)                     # noqa: E731
            cached = single()
            cavg, _ = s.last_averages()
            mscore, m = emap()
            s.score_batch_hbd(refs, dists, depth)
            aavg, _ = s.last_averages()
            bits_equal(mscore, aavg, mscore, cavg, "last_averages after a pair batch")
            again = single()   # no set_reference in between
            aavg, _ = s.last_averages()
            bits_equal(again, aavg, cached, cavg, f"cached pass after a pair batch (hbd={hbd})")
            s.score_batch_hbd(refs, dists, depth)
            mscore2, m2 = emap()
            assert mscore2 == mscore
            gpu_cases.same_bits(m2, m, "recursive error map after a pair batch")
            s.score_batch_against_reference_hbd([f for f in pool16(w, h, 4, depth, seed=8)[1]], depth)
            again = single()
            aavg, _ = s.last_averages()
            bits_equal(again, aavg, cached, cavg, f"cached pass after an against-reference batch (hbd={hbd})")


def test_set_blur_drops_the_reference_and_a_pending_enqueue_survives(hip_lib):
    w, h, n, depth = 64, 20, 3, 12
    refs8, dists8 = neighbours(w, h, n, seed=6)
    refs, dists = pool16(w, h, n, depth)
    planes = [damaged_planes(w, h, 8, True, 6, chroma_ref.YUV_420, i) for i in range(n)]
    frames = [YuvFrame(p, 8, chroma_ref.YUV_420, True, 6) for p in planes]
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, hbatch=True) as s:
        s.set_reference_hbd(refs[0], depth)
        s.score_batch_against_reference_hbd(dists, depth)
        s.score_batch_against_reference_yuv(frames)
        s.set_blur(_lib.BLUR_RECURSIVE_FMA)
        for call in (lambda: s.score_batch_against_reference_hbd(dists, depth),
                     lambda: s.score_batch_against_reference_hbd_device(4096, w * h * 6, n, depth),
                     lambda: s.score_batch_against_reference_yuv(frames)):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_NO_REFERENCE
        # a pending enqueue: the batch runs behind it on the stream and leaves its result for ssimu2_wait
        dev = on_device([refs8[0], dists8[0]], refs8[0].size)
        s.set_reference_device(dev.data_ptr(), w, h)
        single = s.score_against_reference(dists8[0])
        savg, _ = s.last_averages()
        s.enqueue_against_reference_device(dev.data_ptr() + refs8[0].size)
        scores = s.score_batch_hbd(refs, dists, depth)
        yscores = s.score_batch_against_reference_yuv(frames)
        got = s.wait()
        gavg, _ = s.last_averages()
        bits_equal(got, gavg, single, savg, "the enqueued pass, waited for behind two batches")
        again = s.score_batch_hbd(refs, dists, depth)
        assert np.array_equal(scores.view(np.uint64), again.view(np.uint64))
        assert np.array_equal(yscores.view(np.uint64), s.score_batch_against_reference_yuv(frames).view(np.uint64))


def test_a_context_that_never_batches_allocates_nothing_for_it(hip_lib):
    import torch
    w, h, n, depth = 512, 384, 8, 10
    ref = synth.make_ref(w, h, seed=4)
    r16 = hbd_ref_lift(ref) >> 6
    d16 = [hbd_ref_lift(damaged(ref, k)) >> 6 for k in range(n)]
    frame = YuvFrame(chroma_ref.subsample(yuv_ref.forward(damaged(ref, 1), 10, True, 6), chroma_ref.YUV_420), 10,
                     chroma_ref.YUV_420, True, 6)
    torch.cuda.synchronize()
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, hbatch=True) as s:
        def work():
            s.set_reference_hbd(r16, depth)
            for d in d16:
                s.score_against_reference_hbd(d, depth)
            s.score_against_reference_yuv(frame)
            s.compute_ssimu2_hbd(r16, d16[0], depth)
            s.score_batch([ref] * n, [damaged(ref, k) for k in range(n)])   # an 8-bit batch of the recursive modes
        work()
        free_plain, _ = torch.cuda.mem_get_info(0)
        work()
        assert torch.cuda.mem_get_info(0)[0] == free_plain   # no 16-bit batch: nothing allocated for one
        s.set_reference_hbd(r16, depth)
        s.score_batch_against_reference_yuv([frame] * n)     # codes and staged planes: 8 items x 1.7 MB
        assert torch.cuda.mem_get_info(0)[0] < free_plain    # ... the first one does


@pytest.mark.parametrize("mode", RECURSIVE)
def test_8bit_batches_before_and_after_keep_their_bits(hip_lib, mode):
    w, h, n, depth = 121, 40, 5, 10
    refs8, dists8 = neighbours(w, h, n, seed=4)
    refs, dists = pool16(w + 16, h + 3, n + 2, depth)
    blur = gpu_cases.MODES[mode][0]
    with Ssimu2(0, blur=blur, rbatch=True) as r:
        exp = r.score_batch(refs8, dists8)
        exp = [(exp[k], *r.last_batch_averages(k)) for k in range(n)]
        r.set_reference(refs8[0])
        exp_a = r.score_batch_against_reference(dists8)
        exp_a = [(exp_a[k], *r.last_batch_averages(k)) for k in range(n)]
    with Ssimu2(0, blur=blur, hbatch=True) as s:
        for _ in range(2):   # before the first 16-bit batch, and after it
            hold_items(s, s.score_batch(refs8, dists8), exp, f"{mode}: 8-bit pairs")
            s.set_reference(refs8[0])
            hold_items(s, s.score_batch_against_reference(dists8), exp_a, f"{mode}: 8-bit against")
            s.score_batch_hbd(refs, dists, depth)


# ---- (f) refusals ----------------------------------------------------------------------------------------------------
def _u16pp(frames):
    return (ctypes.POINTER(ctypes.c_uint16) * len(frames))(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)) if f is not None
                                                              else None for f in frames])


def _yuv_array(frames, edits=None):
    """The C array of `frames` with field `name` of frame i set to edits[(i, name)]."""
    arr = (_lib.YuvFrameC * len(frames))(*[f.as_c() for f in frames])
    for (i, name), v in (edits or {}).items():
        setattr(arr[i], name, v)
    return arr


@pytest.mark.parametrize("mode", list(gpu_cases.MODES))
def test_refusals(hip_lib, golden, mode):
    import torch
    w, h, depth = 64, 40, 10
    refs, dists = pool16(w, h, 3, depth)
    planes = [damaged_planes(w, h, 8, True, 6, chroma_ref.YUV_420, i) for i in range(3)]
    frames = [YuvFrame(p, 8, chroma_ref.YUV_420, True, 6) for p in planes]
    E, U = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    fir = mode == "fir"
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], hbatch=True) as s:
        L, c = s._L, s._ctx
        before = gpu_cases.golden_bits(s, golden)
        out = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
        codes = np.zeros((3, h, w, 3), np.uint16)
        cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
        err = lambda: L.ssimu2_last_error(c).decode()   # noqa: E731
        stride = w * h * 6
        # 1. a null context; n == 0: OK, nothing read; no reference; too many items
        assert L.ssimu2_hbatch_score_rgb16(None, _u16pp(refs), _u16pp(dists), 3, w, h, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_yuv(None, _yuv_array(frames), 3, 16, 0, out) == E
        assert L.ssimu2_hbatch_score_rgb16(c, None, None, 0, w, h, depth, None) == _lib.OK
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, None, 0, depth, None) == _lib.OK
        assert L.ssimu2_hbatch_score_rgb16_device(c, None, None, 0, 0, w, h, depth, None) == _lib.OK
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, None, 0, 0, depth, None) == _lib.OK
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, None, 0, 16, 0, None) == _lib.OK
        assert L.ssimu2_hbatch_convert_yuv(c, None, 0, w, h, 16, 0, None) == _lib.OK
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), 3, depth, out) == _lib.ERR_NO_REFERENCE
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, stride, 3, depth, out) == _lib.ERR_NO_REFERENCE
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 16, 0, out) == _lib.ERR_NO_REFERENCE
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), _lib.MAX_BATCH + 1, w, h, depth, out) == E
        assert "SSIMU2_MAX_BATCH" in err()
        assert L.ssimu2_hbatch_convert_yuv(c, _yuv_array(frames), _lib.MAX_BATCH + 1, w, h, 16, 0, cp) == E
        if fir:
            # the five scoring calls: 16-bit batches run in the recursive modes only; the conversion works
            s.set_reference_hbd(refs[0], depth)
            for rc in (L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, w, h, depth, out),
                       L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), 3, depth, out),
                       L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride, 3, w, h, depth, out),
                       L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, stride, 3, depth, out),
                       L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 16, 0, out)):
                assert rc == U and "16-bit batches run in the recursive modes only" in err()
            assert list(out) == [-1.0] * 4
            got = s.convert_yuv_batch(frames)
            for i in range(3):
                same_codes(got[i], yuv_codes(planes[i], 8, True, 6, 16, chroma_ref.YUV_420, "bilinear"), ("fir", i))
            after = gpu_cases.golden_bits(s, golden)
            bits_equal(after[0], after[1], before[0], before[1], "after the refusals")
            return
        # 2. null arrays, null and odd items, null out_scores, a zero dimension, the depth, the stride
        assert L.ssimu2_hbatch_score_rgb16(c, None, _u16pp(dists), 3, w, h, depth, out) == E and "null" in err()
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), None, 3, w, h, depth, out) == E
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp([dists[0], None, dists[2]]), 3, w, h, depth, out) == E
        assert "null image pointer in the batch" in err()
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, w, h, depth, None) == E
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, 0, h, depth, out) == E
        assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, w, 0, depth, out) == E
        for bad in (7, 17):
            assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, w, h, bad, out) == U and "8..16" in err()
            assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride, 3, w, h, bad, out) == U
        assert L.ssimu2_hbatch_score_rgb16_device(c, None, 8192, stride, 3, w, h, depth, out) == E
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, None, stride, 3, w, h, depth, out) == E
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride, 3, w, h, depth, None) == E
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride, 3, 0, h, depth, out) == E
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4097, 8192, stride, 3, w, h, depth, out) == E and "aligned" in err()
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride - 2, 3, w, h, depth, out) == E
        assert "item_stride_bytes" in err()
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, stride + 1, 3, w, h, depth, out) == E and "odd" in err()
        # 3. an item above 2^28 pixels: refused before anything is allocated or read
        free0, _ = torch.cuda.mem_get_info(0)
        bw, bh = 16385, 16384
        assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, bw * bh * 6, 2, bw, bh, depth, out) == E and "2^28" in err()
        assert torch.cuda.mem_get_info(0)[0] == free0
        # the against-reference forms, with a reference
        s.set_reference_hbd(refs[0], depth)
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, None, 3, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp([dists[0], None, dists[2]]), 3, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), 3, depth, None) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), 3, 17, out) == U
        assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), _lib.MAX_BATCH + 1, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, None, stride, 3, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, stride, 3, depth, None) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, stride - 2, 3, depth, out) == E
        assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, stride + 1, 3, depth, out) == E
        # the YUV forms: null pointers, check_chroma's refusals per frame, the mixed-frame refusal
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, None, 3, 16, 0, out) == E
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 16, 0, None) == E
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 17, 0, out) == U
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 16, 2, out) == E
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames, {(2, "depth"): 9}), 3, 16, 0, out) == U
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames, {(1, "matrix_coefficients"): 0}), 3, 16, 0, out) == U
        bad = _yuv_array(frames)
        bad[2].planes[1] = None
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, bad, 3, 16, 0, out) == E and "null plane" in err()
        bad = _yuv_array(frames)
        bad[1].row_bytes[2] = (w + 1) // 2 - 1
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, bad, 3, 16, 0, out) == E and "row_bytes" in err()
        for field, v in (("full_range", 0), ("matrix_coefficients", 1), ("format", _lib.YUV_422)):
            mixed = _yuv_array(frames, {(1, field): v})
            assert L.ssimu2_hbatch_score_against_reference_yuv(c, mixed, 3, 16, 0, out) == E, field
            assert "score mixed frames one by one" in err()
            assert L.ssimu2_hbatch_convert_yuv(c, mixed, 3, w, h, 16, 0, cp) == E and "mixed" in err()
        ten = YuvFrame([p.astype(np.uint16) for p in planes[1]], 10, chroma_ref.YUV_420, True, 6)   # another depth
        assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array([frames[0], ten, frames[2]]), 3, 16, 0, out) == E
        assert "score mixed frames one by one" in err()
        assert L.ssimu2_hbatch_convert_yuv(c, None, 3, w, h, 16, 0, cp) == E
        assert L.ssimu2_hbatch_convert_yuv(c, _yuv_array(frames), 3, w, h, 16, 0, None) == E
        assert L.ssimu2_hbatch_convert_yuv(c, _yuv_array(frames), 3, 0, h, 16, 0, cp) == E
        assert L.ssimu2_hbatch_convert_yuv(c, _yuv_array(frames), 3, w, h, 7, 0, cp) == U
        assert list(out) == [-1.0] * 4 and not codes.any()
        after = gpu_cases.golden_bits(s, golden)
        bits_equal(after[0], after[1], before[0], before[1], "after the refusals")
        assert s.score_batch_hbd(refs, dists, depth).shape == (3,)   # and the context batches
        s.set_reference_hbd(refs[0], depth)
        assert s.score_batch_against_reference_yuv(frames).shape == (3,)


def _same_u16pp(frame, n):
    """n pointers to one small frame: for calls that must refuse before they read any item."""
    return (ctypes.POINTER(ctypes.c_uint16) * n)(*[frame.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))] * n)


def _still_scores(s, mode, golden, before, what):
    """After a refusal: the golden pair's bits as before, and a following batch with the bits of its single scores."""
    after = gpu_cases.golden_bits(s, golden)
    bits_equal(after[0], after[1], before[0], before[1], what)
    (w, h), depth, n = (24, 17), 10, 3
    refs, dists = pool16(w, h, n, depth)
    pair, against = singles16(mode, w, h, depth, n)
    hold_items(s, s.score_batch_hbd(refs, dists, depth), pair, f"{what}: a following pair batch")
    s.set_reference_hbd(refs[0], depth)
    hold_items(s, s.score_batch_against_reference_hbd(dists, depth), against, f"{what}: a following against batch")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_a_batch_too_large_for_one_launch_is_refused_before_anything_is_allocated(hip_lib, golden, mode):
    """Refusal 4 of the contract.  4,096 items of 8 x 2^25 (2^28 pixels each: the size limit lets them through) are
    3 * ceil(2^25 / 20) * 4,096 = 2.1e10 workgroups of the horizontal pass and 8.6e9 of the conversion: beyond
    2^31 - 1.  The device form gets there without touching a frame; the host form must get there before it grows its
    staging buffers (6.6 TB: SSIMU2_ERR_OOM otherwise) or copies an item.  The against-reference and YUV forms make the
    same check through the same function, but need a cached reference of 2^28 pixels (tens of GB of planes) to reach
    it: not run."""
    import torch
    w, h, n, depth = 8, 1 << 25, _lib.MAX_BATCH, 10
    small = np.zeros((8, 8, 3), np.uint16)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], hbatch=True) as s:
        L, c = s._L, s._ctx
        before = gpu_cases.golden_bits(s, golden)
        out = (ctypes.c_double * 1)(-1.0)
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info(0)
        rc = L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, w * h * 6, n, w, h, depth, out)
        assert rc == _lib.ERR_INVALID_ARG and "fewer items per call" in L.ssimu2_last_error(c).decode()
        assert torch.cuda.mem_get_info(0)[0] == free0
        rc = L.ssimu2_hbatch_score_rgb16(c, _same_u16pp(small, n), _same_u16pp(small, n), n, w, h, depth, out)
        assert rc == _lib.ERR_INVALID_ARG and "fewer items per call" in L.ssimu2_last_error(c).decode()
        assert torch.cuda.mem_get_info(0)[0] == free0 and out[0] == -1.0
        _still_scores(s, mode, golden, before, f"{mode}: after the launch-size refusal")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_out_of_memory_is_refused_and_the_context_goes_on_scoring(hip_lib, golden, mode):
    """Refusal 5 of the contract.  4,096 pairs of 2048 x 1536 pass every check before it (1.9e6 workgroups of the
    horizontal pass, 3.1e6 of the conversion) and need 21 planes of 1.33 x 3.1 M floats per item: 1.4 TB of batch planes,
    more than the device has, so the allocation is refused -- before any launch, and in the device form without a frame
    being touched.  The host forms are not run: their staging buffers (77 GB a side here) fit the device, so the call
    would go on to read 4,096 real frames of 19 MB each."""
    w, h, n, depth = 2048, 1536, _lib.MAX_BATCH, 12
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], hbatch=True) as s:
        L, c = s._L, s._ctx
        before = gpu_cases.golden_bits(s, golden)
        s.score_batch_hbd(*pool16(24, 17, 3, 10), 10)          # the batch's buffers exist: a failed grow releases one
        out = (ctypes.c_double * 1)(-1.0)
        rc = L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, w * h * 6, n, w, h, depth, out)
        assert rc == _lib.ERR_OOM and "hipMalloc(recursive batch planes" in L.ssimu2_last_error(c).decode()
        assert out[0] == -1.0
        _still_scores(s, mode, golden, before, f"{mode}: after the refused planes")


def test_a_context_without_the_flag_makes_none_of_the_calls(hip_lib):
    refs, dists = pool16(64, 20, 3, 10)
    frame = YuvFrame(damaged_planes(64, 20, 8, True, 6, chroma_ref.YUV_420, 0), 8, chroma_ref.YUV_420, True, 6)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, rbatch=True) as s:
        assert not s.hbatch
        for name in _lib.HBATCH_SYMBOLS:
            assert not hasattr(s._L, name), name
        for call in (lambda: s.score_batch_hbd(refs, dists, 10), lambda: s.score_batch_against_reference_hbd(dists, 10),
                     lambda: s.score_batch_hbd_device(4096, 8192, 64 * 20 * 6, 3, 64, 20, 10),
                     lambda: s.score_batch_against_reference_hbd_device(4096, 64 * 20 * 6, 3, 10),
                     lambda: s.score_batch_against_reference_yuv([frame]), lambda: s.convert_yuv_batch([frame])):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "hbatch=True" in str(ei.value)


def test_a_service_context_refuses_and_goes_on_scoring(hip_lib):
    from oavif_amd import service
    w, h, depth = 64, 40, 10
    refs8, dists8 = neighbours(w, h, 3, seed=1)
    refs, dists = pool16(w, h, 3, depth)
    frames = [YuvFrame(damaged_planes(w, h, 8, True, 6, chroma_ref.YUV_420, i), 8, chroma_ref.YUV_420, True, 6) for i in range(3)]
    svc = service.start(max_lifetime=120)
    try:
        with Ssimu2(0, service=svc.socket, hbatch=True) as s:
            exp = s.compute_ssimu2(refs8[0], dists8[0])
            out = (ctypes.c_double * 3)()
            codes = np.zeros((3, h, w, 3), np.uint16)
            L, c, U = s._L, s._ctx, _lib.ERR_UNSUPPORTED
            assert L.ssimu2_hbatch_score_rgb16(c, _u16pp(refs), _u16pp(dists), 3, w, h, depth, out) == U
            assert L.ssimu2_hbatch_score_against_reference_rgb16(c, _u16pp(dists), 3, depth, out) == U
            assert L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, w * h * 6, 3, w, h, depth, out) == U
            assert L.ssimu2_hbatch_score_against_reference_rgb16_device(c, 4096, w * h * 6, 3, depth, out) == U
            assert L.ssimu2_hbatch_score_against_reference_yuv(c, _yuv_array(frames), 3, 16, 0, out) == U
            assert L.ssimu2_hbatch_convert_yuv(c, _yuv_array(frames), 3, w, h, 16, 0,
                                               codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))) == U
            assert s.compute_ssimu2(refs8[0], dists8[0]) == exp
    finally:
        assert svc.stop(timeout=30) == 0


# ---- (g) the search --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
def test_the_speculative_search_over_420_frames_is_the_sequential_one(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 67
    ref = synth.make_ref(w, h, seed=21)
    codec = gpu_cases.pseudo_codec(ref)
    handed = []

    def codec_yuv(q):
        dec, size = codec(q)
        planes = chroma_ref.subsample(yuv_ref.forward(dec, 8, True, 6), chroma_ref.YUV_420)
        f = _Handed(planes=planes, depth=8, format=chroma_ref.YUV_420, full_range=True, matrix_coefficients=6, width=w, height=h)
        handed.append(f)   # list.append is atomic: the codec runs on several threads
        return f, size

    how = dict(score_tgt=80.0, tolerance=0.5, max_pass=6)
    a = tq.search_hip_frames(s, ref, codec_yuv, **how)
    assert a.num_pass >= 2, a           # the target is chosen so that the sequential search takes at least two passes
    bits = lambda r: np.array([sc for _q, sc in r.history] + [r.score]).view(np.uint64)   # noqa: E731
    assert len(handed) == a.num_pass and all(f.closed for f in handed)
    widest = 0
    calls = []
    real = s.score_batch_against_reference_yuv
    s.score_batch_against_reference_yuv = lambda frames, *args: (calls.append(len(frames)), real(frames, *args))[1]
    try:
        for fan in (1, 2, 4):
            for first in (1, 4):
                del handed[:], calls[:]
                b, stats, sizes = tq.search_speculative_hip_frames(s, ref, codec_yuv, max_fanout=fan, first_wave_fanout=first, **how)
                what = (mode, fan, first, a, b, stats)
                assert (b.q, b.num_pass, b.last_avif_size) == (a.q, a.num_pass, a.last_avif_size), what
                assert [q for q, _ in b.history] == [q for q, _ in a.history], what
                assert np.array_equal(bits(a), bits(b)), what
                assert all(sizes[q] == codec(q)[1] for q in sizes) and b.buf_q in sizes, what
                assert len(handed) == stats.probes_issued >= b.num_pass and all(f.closed for f in handed), what
                assert all(n >= tq.MIN_BATCHED_WAVE for n in calls) and (fan > 1 or not calls), what
                assert sum(calls) <= stats.probes_issued
                if fan > 1:
                    assert stats.probes_issued > stats.waves and calls, what   # a wave of two or more, scored by one call
                widest = max(widest, *calls, 0)
    finally:
        del s.score_batch_against_reference_yuv
    assert widest >= 2
