"""Every item of a batch, the uncached-reference fallbacks and batches against a 16-bit reference on the MI355X
(ssimu2_score_batch_*, DESIGN.md sections 10 and 11).

A. Every item of every batch below has the bits (score and all 108 averages) of a single score of its pair taken on
   the instrumented context at the batch rule's rows (ssimu2_instr_set_segment_rows): the batch grid's own index
   arithmetic -- march_batch_body's (scale, item, tile) maps, march_tile_of_block over ranges of n_items * nblocks,
   the item strides, k_pyramid_bands_batch's blockIdx / per_item, k_finalize_batch's block of the results -- moves no
   bit.  All items of a batch differ (asserted), so an item or tile that lands in another item's slot changes bits.
B. With the reference's blur cache off (ssimu2_instr_cache_reference_blur; the state a failed hipMalloc leaves) a pass
   against the reference runs k_march and a batch k_march_batch with a shared reference: same bits as with the cache,
   and as the pair forms; ssimu2_instr_last_march says which kernel ran.  16-bit references and frames need the cache:
   those calls refuse with SSIMU2_ERR_OOM and leave the context scoring as before.
C. A batch of 8-bit frames against a 16-bit reference: the bits of the single scores at the same rows, and the
   kernel-order terms of (16-bit reference, 257 u) within gpu_cases.batch_rtol."""
import os
import sys

import numpy as np
import pytest

from oavif_amd import Ssimu2Error, _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import gpu_cases  # noqa: E402
import hbd_ref  # noqa: E402
from gpu_cases import KINDS, bits_equal, damaged, golden_bits, on_device  # noqa: E402
from hbd_cases import lift, to_depth  # noqa: E402

pytestmark = pytest.mark.gpu

RESIDUES = list(range(1, 18)) + [31, 33]
#                (w, h)      scales and blocks per item (batch rule: 96 rows at scale 0, 48 below; strips of 128 columns:
#                            tests/test_wide_cases.py asserts these counts, tests/wide_cases.py::TILES; the sizes with
#                            three strips and with two strips at scale 1: WIDE_RESIDUE_SIZES, tests/test_gpu_wide_batch.py)
RESIDUE_SIZES = [(24, 17),   # 3 scales of 1 block
                 (121, 40),  # 1 strip: 4 scales of 1 block
                 (241, 100),  # 2 strips x 2 segments at scale 0, 1 x 2 at scale 1 (50 rows)
                 (130, 200)]  # 2 strips x 3 segments at scale 0, 1 x 3 at scale 1, 1 x 2 at scale 2


def seed_of(w, h, n, k):
    return ((w * 4099 + h) * 4099 + n) * 4099 + k


def distinct(frames):
    return len({f.tobytes() for f in frames}) == len(frames)


def batch_items(w, h, n, cached):
    """n pairs of distinct content with seeds from (w, h, n, k): every content kind with seeded noise on top (three of
    the kinds do not depend on their seed), damaged by seeded noise of four strengths, every third one on top of block
    quantisation; item n // 2 of three or more is left undamaged.  `cached`: one reference for all items."""
    refs, dists = [], []
    for k in range(n):
        sd = seed_of(w, h, n, k)
        if cached and k:
            r = refs[0]
        else:
            r = synth.distort(gpu_cases.content(KINDS[(k + n) % len(KINDS)], w, h, sd), "noise", k % 2, seed=sd)
        base = synth.distort(r, "blockq", 2) if k % 3 == 1 else r
        d = r.copy() if n >= 3 and k == n // 2 else synth.distort(base, "noise", 1 + k % 4, seed=sd + 1)
        refs.append(r)
        dists.append(d)
    assert distinct(dists) and (cached or distinct(refs)), (w, h, n)
    return refs, dists


def stale_batch(s, w, h, n):
    """A pair batch of other content, of more items (as many at the limit) and of larger frames, on the same context:
    the batch scratch then holds its values and is larger than the next batch needs."""
    pool = [gpu_cases.content(KINDS[k], w + 9, h + 6, 7000 + k) for k in range(5)]
    m = min(n + 5, _lib.MAX_BATCH)
    s.score_batch([pool[k % 5] for k in range(m)], [pool[(k + 1 + k // 5) % 5] for k in range(m)])


def run_batch(s, refs, dists, cached):
    """-> [(score, averages, nscales)] of every item."""
    if cached:
        s.set_reference(refs[0])
        stale_batch(s, refs[0].shape[1], refs[0].shape[0], len(dists))
        scores = s.score_batch_against_reference(dists)
    else:
        stale_batch(s, refs[0].shape[1], refs[0].shape[0], len(dists))
        scores = s.score_batch(refs, dists)
    assert scores.shape == (len(dists),)
    return [(scores[k],) + s.last_batch_averages(k) for k in range(len(dists))]


def check_against_singles(s, w, h, batches, rows=None):
    """`batches`: [(refs, dists, cached, results of run_batch)].  Every item of every batch against the single score of
    its pair on `s` at the batch rule's rows (`rows`: the rows by scale that an override of
    ssimu2_instr_set_batch_segment_rows must give instead).  -> the single scores of the last batch."""
    rule = [s.batch_segment_rows(w, h, 0), s.batch_segment_rows(w, h, 1)]
    assert rule == (list(rows[:2]) if rows else [gpu_cases.batch_seg_rows(w, h, 0), gpu_cases.batch_seg_rows(w, h, 1)])
    singles = []
    try:
        s.set_segment_rows(rule[0], rule[1])
        for refs, dists, cached, got in batches:
            n = len(dists)
            assert len(got) == n
            if cached:
                s.set_reference(refs[0])
            singles = []
            for k in range(n):
                single = s.score_against_reference(dists[k]) if cached else s.compute_ssimu2(refs[k], dists[k])
                avg1, ns1 = s.last_averages()
                assert got[k][2] == ns1, (w, h, n, k)
                bits_equal(got[k][0], got[k][1], single, avg1, f"{w}x{h} n={n} cached={cached} item {k}")
                singles.append((single, avg1, ns1))
    finally:
        s.set_segment_rows(0, 0)
    return singles


FORMS = pytest.mark.parametrize("cached", [False, True], ids=["pairs", "cached_reference"])


# ---- A. every item, bit for bit -----------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("w,h", RESIDUE_SIZES)
def test_every_item_at_every_residue_of_the_batch_grid(iscorer, w, h, cached):
    """n = 1 .. 17, 31, 33: n * nblocks takes every residue mod 8 in every scale's [first, end) of the batch grid."""
    s = iscorer
    batches = []
    for n in RESIDUES:
        refs, dists = batch_items(w, h, n, cached)
        batches.append((refs, dists, cached, run_batch(s, refs, dists, cached)))
    check_against_singles(s, w, h, batches)
    assert any(0.0 < g[0] < 100.0 for g in batches[-1][3])


@FORMS
@pytest.mark.parametrize("w,h", [(16, 16), (121, 40)])
def test_every_item_of_a_wide_grid(iscorer, w, h, cached):
    """n = 255 and 257: ranges far from a multiple of 8, many more items than tiles."""
    s = iscorer
    batches = []
    for n in (255, 257):
        refs, dists = batch_items(w, h, n, cached)
        batches.append((refs, dists, cached, run_batch(s, refs, dists, cached)))
    check_against_singles(s, w, h, batches)


@FORMS
@pytest.mark.parametrize("w,h", [(16, 16), (8, 8)])
def test_every_item_of_the_largest_batch(iscorer, w, h, cached):
    """n = SSIMU2_MAX_BATCH: blk_end, off_part and k_finalize_batch's block of the results at their largest item."""
    s = iscorer
    n = _lib.MAX_BATCH
    assert n == 4096
    refs, dists = batch_items(w, h, n, cached)
    got = run_batch(s, refs, dists, cached)
    avg_last, ns_last = s.last_batch_averages(n - 1)
    with pytest.raises(Ssimu2Error) as ei:
        s.last_batch_averages(n)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    singles = check_against_singles(s, w, h, [(refs, dists, cached, got)])
    assert ns_last == singles[-1][2] >= 1
    bits_equal(got[-1][0], avg_last, singles[-1][0], singles[-1][1], f"{w}x{h} item {n - 1} read again")


def device_forms_against_singles(s, w, h, n, gap):
    """n items of w x h on the device, item stride = frame + `gap` bytes, noise between frames: both device forms
    against the single scores."""
    import torch
    frame = w * h * 3
    stride = frame + gap
    for cached in (False, True):
        refs, dists = batch_items(w, h, n, cached)
        g = torch.Generator().manual_seed(seed_of(w, h, n, int(cached)))
        bufs = []
        for frames in (refs, dists):
            buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, generator=g)
            for k in range(n):
                buf[k * stride:k * stride + frame] = torch.from_numpy(frames[k].reshape(-1))
            bufs.append(buf.cuda())
        torch.cuda.synchronize()
        if cached:
            s.set_reference_device(bufs[0].data_ptr(), w, h)
            scores = s.score_batch_against_reference_device(bufs[1].data_ptr(), stride, n)
        else:
            scores = s.score_batch_device(bufs[0].data_ptr(), bufs[1].data_ptr(), stride, n, w, h)
        got = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
        check_against_singles(s, w, h, [(refs, dists, cached, got)])


def test_every_item_of_the_device_forms_with_an_odd_item_stride(iscorer):
    """33 items of 121 x 40 on the device, item stride = frame + 52 bytes (no multiple of 16), noise between frames."""
    device_forms_against_singles(iscorer, 121, 40, 33, 52)


# ---- B. the uncached-reference fallbacks --------------------------------------------------------------------------
def many_dists(ref, n):
    """n distinct damaged frames of `ref` from four distortions (rolled copies: cheap at full HD)."""
    base = [damaged(ref, k) for k in range(min(n, 4))]
    out = [np.ascontiguousarray(np.roll(base[k % 4], k // 4, axis=1)) for k in range(n)]
    assert distinct(out)
    return out


def against_reference_family(s, ref, dist, dists, expect):
    """Every call that scores against a cached 8-bit reference, on the context as it is.  `expect`: the marching
    kernels (single pass, batch) each must have launched, by ssimu2_instr_last_march.
    -> {"pass": [(score, averages)] of the three single-pass calls, "map": (score, map), "batch": {(form, n): items}}"""
    h, w, _ = ref.shape
    out = {"pass": [], "batch": {}}
    s.set_reference(ref)
    out["pass"].append((s.score_against_reference(dist), s.last_averages()[0]))
    assert s.last_march() == expect[0], (w, h)
    _buf, view = gpu_cases.decoded_like(dist, 4, 12, seed=w)
    out["pass"].append((s.score_decoded_against_reference(view), s.last_averages()[0]))
    assert s.last_march() == expect[0], (w, h)
    dev = on_device([ref, dist], ref.size)
    s.set_reference_device(dev.data_ptr(), w, h)
    s.enqueue_against_reference_device(dev.data_ptr() + ref.size)
    out["pass"].append((s.wait(), s.last_averages()[0]))
    assert s.last_march() == expect[0], (w, h)
    out["map"] = s.error_map_against_reference(dist)
    stride = ref.size + 20
    ddev = on_device(dists, stride)
    for n in (1, 7, 16):
        scores = s.score_batch_against_reference(dists[:n])
        out["batch"]["host", n] = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
        assert s.last_march() == expect[1], (w, h, n)
        scores = s.score_batch_against_reference_device(ddev.data_ptr(), stride, n)
        out["batch"]["device", n] = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
        assert s.last_march() == expect[1], (w, h, n)
    return out


def same_family(a, b, what):
    for k, (x, y) in enumerate(zip(a["pass"], b["pass"])):
        bits_equal(x[0], x[1], y[0], y[1], f"{what}: pass {k}")
    assert a["map"][0] == b["map"][0], what
    gpu_cases.same_bits(a["map"][1], b["map"][1], f"{what}: map")
    assert a["batch"].keys() == b["batch"].keys()
    for key in a["batch"]:
        for k, (x, y) in enumerate(zip(a["batch"][key], b["batch"][key])):
            assert x[2] == y[2], (what, key, k)
            bits_equal(x[0], x[1], y[0], y[1], f"{what}: batch {key} item {k}")


CACHED_KERNELS = ("k_march_refblur", "k_march_refblur_batch")
FALLBACK_KERNELS = ("k_march", "k_march_batch")


@pytest.mark.parametrize("w,h", [(64, 20), (121, 41), (333, 217), (1921, 1083)])
def test_uncached_reference_fallbacks_keep_the_bits(iscorer, w, h):
    s = iscorer
    ref = synth.make_ref(w, h, seed=w + h) if w * h > 4096 else gpu_cases.content("noise", w, h, w + h)
    dists = many_dists(ref, 16)
    dist = dists[3]
    # the pair forms: what every call against the reference must equal
    pair = (s.compute_ssimu2(ref, dist), s.last_averages()[0])
    assert s.last_march() == "k_march"
    pair_map = s.error_map(ref, dist)
    pair_batch = {}
    for n in (1, 7, 16):
        scores = s.score_batch([ref] * n, dists[:n])
        pair_batch[n] = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
        assert s.last_march() == "k_march_batch"
    try:
        on = against_reference_family(s, ref, dist, dists, CACHED_KERNELS)
        s.cache_reference_blur(False)   # drops the reference: the family sets it again
        off = against_reference_family(s, ref, dist, dists, FALLBACK_KERNELS)
        s.cache_reference_blur(True)
        on2 = against_reference_family(s, ref, dist, dists, CACHED_KERNELS)
    finally:
        s.cache_reference_blur(True)
    same_family(off, on, f"{w}x{h} cache off against on")
    same_family(on2, on, f"{w}x{h} cache on again")
    for name, fam in (("on", on), ("off", off)):
        for k, (score, avg) in enumerate(fam["pass"]):
            bits_equal(score, avg, pair[0], pair[1], f"{w}x{h} cache {name}: pass {k} against the pair score")
        assert fam["map"][0] == pair_map[0]
        gpu_cases.same_bits(fam["map"][1], pair_map[1], f"{w}x{h} cache {name}: map against the pair map")
        for (form, n), items in fam["batch"].items():
            for k in range(n):
                assert items[k][2] == pair_batch[n][k][2]
                bits_equal(items[k][0], items[k][1], pair_batch[n][k][0], pair_batch[n][k][1],
                           f"{w}x{h} cache {name}: {form} batch of {n}, item {k} against the pair batch")
    assert 0.0 < pair[0] < 100.0


def test_time_kernels_takes_the_fallback_too(iscorer):
    """ssimu2_time_kernels enqueues through the product's path: k_march_refblur with the cache, k_march without (the
    launch NAMES it returns follow its arguments, so ssimu2_instr_last_march is what tells the two apart)."""
    s = iscorer
    w, h = 121, 41
    ref = synth.make_ref(w, h, seed=5)
    dev = on_device([ref, damaged(ref, 1)], ref.size)
    try:
        names, _, _ = s.time_kernels(w, h, [dev.data_ptr() + ref.size], 2, d_ref=dev.data_ptr())
        assert "march_refblur" in names and s.last_march() == "k_march_refblur"
        s.cache_reference_blur(False)
        names, _, _ = s.time_kernels(w, h, [dev.data_ptr() + ref.size], 2, d_ref=dev.data_ptr())
        assert len(names) == 3 and s.last_march() == "k_march"
        names, _, _ = s.time_kernels(w, h, [dev.data_ptr() + ref.size], 2, d_refs=[dev.data_ptr()])
        assert "march" in names and "march_refblur" not in names and s.last_march() == "k_march"
    finally:
        s.cache_reference_blur(True)


def test_uncached_reference_of_a_frame_without_a_scale(iscorer):
    s = iscorer
    ref = gpu_cases.content("noise", 7, 7, 1)
    dists = many_dists(ref, 7)
    try:
        for enabled in (True, False, True):
            s.cache_reference_blur(enabled)
            s.set_reference(ref)
            assert s.score_against_reference(dists[0]) == 100.0 and s.last_march() is None
            avg, ns = s.last_averages()
            assert ns == 0 and not avg.any()
            score, m = s.error_map_against_reference(dists[1])
            assert score == 100.0 and m.shape == (7, 7) and not m.any()
            scores = s.score_batch_against_reference(dists)
            assert (scores == 100.0).all() and s.last_march() is None
            for k in range(7):
                avg, ns = s.last_batch_averages(k)
                assert ns == 0 and not avg.any()
    finally:
        s.cache_reference_blur(True)


def test_16bit_calls_refuse_without_the_cache_and_leave_the_context_scoring(iscorer, golden):
    """16-bit scale 0 cannot be paired with an 8-bit reference frame in one marching kernel, so without the cached
    planes ssimu2_set_reference_rgb16 (cache_reference_fir(required)) and ssimu2_score_against_reference_rgb16
    (enqueue_score16) refuse with SSIMU2_ERR_OOM.  The third such refusal, batch_run's for a batch against a 16-bit
    reference, cannot be reached with the hook: setting a 16-bit reference is what refuses first, so no 16-bit reference
    exists for the batch to meet, and the batch reports that there is none."""
    s = iscorer
    w, h = 121, 41
    r8 = synth.make_ref(w, h, seed=9)
    d8 = many_dists(r8, 3)
    before = golden_bits(s, golden)
    s.set_reference(r8)
    cached = (s.score_against_reference(d8[0]), s.last_averages()[0])

    def unchanged(what):
        after = golden_bits(s, golden)
        bits_equal(after[0], after[1], before[0], before[1], what)

    try:
        s.cache_reference_blur(False)
        with pytest.raises(Ssimu2Error) as ei:
            s.set_reference_hbd(lift(r8), 16)
        assert ei.value.code == _lib.ERR_OOM
        with pytest.raises(Ssimu2Error) as ei:   # the refused call left no reference behind, 8- or 16-bit
            s.score_batch_against_reference(d8)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        with pytest.raises(Ssimu2Error) as ei:
            s.score_against_reference(d8[0])
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        unchanged("after the refused 16-bit reference")
        s.set_reference(r8)
        with pytest.raises(Ssimu2Error) as ei:
            s.score_against_reference_hbd(lift(d8[0]), 16)
        assert ei.value.code == _lib.ERR_OOM
        again = (s.score_against_reference(d8[0]), s.last_averages()[0])   # the 8-bit reference is still set
        assert s.last_march() == "k_march"
        bits_equal(again[0], again[1], cached[0], cached[1], "8-bit pass after the refused 16-bit pass")
        scores = s.score_batch_against_reference(d8)
        bits_equal(scores[0], s.last_batch_averages(0)[0], *batch_single(s, w, h, r8, d8[0]), "batch after the refusals")
        unchanged("after the refused 16-bit pass")
    finally:
        s.cache_reference_blur(True)
    s.set_reference_hbd(lift(r8), 16)   # with the cache the same calls score
    got = (s.score_against_reference_hbd(lift(d8[0]), 16), s.last_averages()[0])
    assert s.last_march() == "k_march_refblur_lin"
    bits_equal(got[0], got[1], cached[0], cached[1], "16-bit pass of 257 u with the cache")
    unchanged("after switching the cache back on")


def batch_single(s, w, h, ref, dist):
    """(score, averages) of the pair's single score at the batch rule's rows (the context loses its reference)."""
    try:
        s.set_segment_rows(gpu_cases.batch_seg_rows(w, h, 0), gpu_cases.batch_seg_rows(w, h, 1))
        return s.compute_ssimu2(ref, dist), s.last_averages()[0]
    finally:
        s.set_segment_rows(0, 0)


# ---- C. a batch against a 16-bit reference ------------------------------------------------------------------------
def hbd_reference(w, h, depth, seed):
    """A genuine `depth`-bit frame: 8-bit content scaled to the depth with low-order detail added."""
    return to_depth(synth.make_ref(w, h, seed=seed), depth, seed)


def to_8bit(img16, depth):
    return np.ascontiguousarray((img16.astype(np.int64) * 255 // ((1 << depth) - 1)).astype(np.uint8))


def hold_batch_against_a_16bit_reference(s, oracle, depth, w, h):
    """Part C at one size and depth, on the instrumented context `s`."""
    n = 9
    r16 = hbd_reference(w, h, depth, seed=seed_of(w, h, n, depth))
    low = to_8bit(r16, depth)
    d8 = [synth.distort(synth.distort(low, "blockq", 2) if k % 3 == 1 else low, "noise", 1 + k % 4,
                        seed=seed_of(w, h, n, k)) for k in range(n)]
    assert distinct(d8)
    # the 8-bit frame buffer of the context holds a frame that is not the reference
    other = gpu_cases.content("text", w, h, 77)
    s.compute_ssimu2(other, damaged(other, 2))
    s.set_reference_hbd(r16, depth)
    scores = s.score_batch_against_reference(d8)
    assert s.last_march() == "k_march_refblur_batch"
    got = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
    try:
        s.set_segment_rows(gpu_cases.batch_seg_rows(w, h, 0), gpu_cases.batch_seg_rows(w, h, 1))
        s.compute_ssimu2(other, damaged(other, 2))
        s.set_reference_hbd(r16, depth)
        for k in range(n):
            single = s.score_against_reference(d8[k])
            avg1, ns1 = s.last_averages()
            assert ns1 == got[k][2]
            bits_equal(got[k][0], got[k][1], single, avg1, f"{depth}-bit reference {w}x{h} item {k}")
    finally:
        s.set_segment_rows(0, 0)
    lin_ref = hbd_ref.linear_planes(r16, depth)
    worst = 0.0
    for k in range(n):
        tm = hbd_ref.terms(oracle, lin_ref, hbd_ref.linear_planes(lift(d8[k]), 16), oracle.BLUR_FIR)
        assert len(tm) == got[k][2]
        worst = max(worst, gpu_cases.check_item_against_terms(oracle, got[k][0], got[k][1], got[k][2], r16, d8[k],
                                                              f"{depth}-bit reference {w}x{h} item {k}",
                                                              kavg=errmap_ref.averages(tm)))
    print(f"measured: batch against a {depth}-bit reference {w}x{h}: averages {worst:.3f} of batch_rtol")
    assert all(g[0] < 100.0 for g in got)


@pytest.mark.parametrize("w,h", [(333, 217), (121, 40)])
@pytest.mark.parametrize("depth", [10, 12, 16])
def test_batch_against_a_16bit_reference(iscorer, oracle, depth, w, h):
    hold_batch_against_a_16bit_reference(iscorer, oracle, depth, w, h)


def test_an_8bit_reference_after_a_16bit_one(scorer):
    w, h, n = 121, 40, 9
    ref = synth.make_ref(w, h, seed=3)
    dists = many_dists(ref, n)
    pair = scorer.score_batch([ref] * n, dists)
    pavg = [scorer.last_batch_averages(k) for k in range(n)]
    scorer.set_reference_hbd(hbd_reference(w, h, 12, seed=4), 12)
    scorer.score_batch_against_reference(dists)
    scorer.set_reference(ref)
    scores = scorer.score_batch_against_reference(dists)
    for k in range(n):
        avg, ns = scorer.last_batch_averages(k)
        assert ns == pavg[k][1]
        bits_equal(scores[k], avg, pair[k], pavg[k][0], f"item {k}")


def test_a_pair_batch_leaves_a_16bit_reference_alone(scorer):
    w, h = 333, 217
    r16 = hbd_reference(w, h, 16, seed=6)
    d16 = np.clip(r16.astype(np.int64) + np.random.default_rng(7).integers(-600, 601, r16.shape), 0, 65535).astype(np.uint16)
    scorer.set_reference_hbd(r16, 16)
    first = (scorer.score_against_reference_hbd(d16, 16), scorer.last_averages()[0])
    scorer.set_reference_hbd(r16, 16)
    refs, dists = gpu_cases.neighbours(w, h, 6, seed=5)
    scorer.score_batch(refs, dists)                       # between setting the reference and scoring against it
    again = (scorer.score_against_reference_hbd(d16, 16), scorer.last_averages()[0])
    bits_equal(again[0], again[1], first[0], first[1], "16-bit cached score after a pair batch")
    assert first[0] < 100.0
