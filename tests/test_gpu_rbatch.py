"""Batches in every blur mode on the MI355X (ssimu2_rbatch_*, include/ssimu2_hip_rbatch.h).

The contract under test: in SSIMU2_BLUR_RECURSIVE / _FMA an item's score and its 108 averages have the BITS of the
single score of its pair in that mode -- ssimu2_score_rgb8 for the pair form, ssimu2_set_reference +
ssimu2_score_against_reference for the against-reference form -- whatever the batch's size, the item's place and its
neighbours; in SSIMU2_BLUR_FIR the calls are the batch of ssimu2_score_batch_*.  Every comparison is bit for bit on the
score and all 108 averages, every item of every batch is compared (none is sampled), all items of a batch differ in
content (a misplaced item or job changes bits), the single scores come from a fresh context in the same mode, and each
batch runs behind a larger batch of other content on the same context, so the batch's scratch is stale and larger
than needed.

Shapes sit at the kernels' edges (oavif_amd/csrc/ssimu2_recursive.h): RG_HL = 20 rows per workgroup of the horizontal
pass, RG_VW = 64 columns per job of the vertical pass, batches of ten rows rounded up to RG_PF = 6 of them, the number of
scales.  Counts meet every residue of n_items x blocks at two shapes and make the persistent vertical pass pull many jobs
per workgroup (N = 257).  The one anchor that is not the device's own single score is gpu_cases.check_against_terms at the
project's RTOL_RECURSIVE and FINALIZE_TOL (derived in tests/gpu_cases.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_cases  # noqa: E402
from gpu_cases import bits_equal, damaged, neighbours, on_device  # noqa: E402

pytestmark = pytest.mark.gpu

RECURSIVE = ("recursive", "recursive_fma")
ALL_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33)
# (w, h) -> the batch sizes scored at it
SHAPES = {
    (24, 17): ALL_COUNTS,        # w < 64, h < 20: one row group, one column group at each of its three scales
    (64, 20): (3, 7),            # exactly RG_VW columns and RG_HL rows
    (65, 21): (3, 7),            # one past both
    (121, 40): ALL_COUNTS,       # two column groups, two row groups
    (241, 100): (3, 7),          # four column groups, five row groups
    (130, 200): (3, 7),          # 20 ten-row batches + 1, rounded up to RG_PF
    (16, 16): (3, 7),            # one scale
    (8, 8): (3, 7),              # one scale, the smallest
    (7, 9): (3, 7),              # no scale: every score exactly 100
}


@pytest.fixture(scope="module")
def ctxs(hip_lib):
    """One rbatch=True context per blur mode: the one the batches run on."""
    out = {name: Ssimu2(0, blur=mode, rbatch=True) for name, (mode, _) in gpu_cases.MODES.items()}
    yield out
    for s in out.values():
        s.close()


def pool(w, h, n, seed=0):
    """n pairs of w x h, every frame of its own content (seeded noise: no two items alike, at any size).  Item k is a
    function of (w, h, seed, k) alone, so a shorter pool is a prefix of a longer one."""
    refs, dists = [], []
    for k in range(n):
        rng = np.random.default_rng([w, h, seed, k])
        r = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        d = np.clip(r.astype(np.int64) + rng.integers(-40, 41, (h, w, 3)) * (k % 4 != 3), 0, 255).astype(np.uint8)
        d[::3, ::2] = r[::3, ::2]   # part of every frame undamaged (item 3, 7, ...: all of it)
        refs.append(r)
        dists.append(d)
    return refs, dists


_singles = {}


def singles(mode, w, h, n):
    """[(score, averages, nscales)] of the first n pairs of pool(w, h): the pair form's singles and, against
    pool's reference 0, the against form's; on a fresh plain context in `mode`, computed once and kept."""
    key = (mode, w, h)
    have = _singles.get(key)
    if have is None or len(have[0]) < n:
        refs, dists = pool(w, h, n)
        pair, against = [], []
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as s:
            for r, d in zip(refs, dists):
                sc = s.compute_ssimu2(r, d)
                pair.append((sc, *s.last_averages()))
            s.set_reference(refs[0])
            for d in dists:
                sc = s.score_against_reference(d)
                against.append((sc, *s.last_averages()))
        have = _singles[key] = (pair, against)
    return have[0][:n], have[1][:n]


def make_stale(s, w, h, n):
    """A larger batch of other content on the same context: more items (up to the maximum) of a larger frame."""
    m = min(n + 3, _lib.MAX_BATCH)
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, (2, h + 8, w + 8, 3), dtype=np.uint8)
    s.score_batch([frames[0]] * m, [frames[1]] * m)


def hold_items(s, scores, exp, what):
    assert len(scores) == len(exp), what
    for k, (sc, avg, ns) in enumerate(exp):
        got_avg, got_ns = s.last_batch_averages(k)
        assert got_ns == ns, (what, k)
        bits_equal(scores[k], got_avg, sc, avg, f"{what}: item {k}")


def run_both_forms(s, mode, w, h, n, refs, dists):
    pair, against = singles(mode, w, h, n)
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch(refs[:n], dists[:n]), pair, f"{mode} {w}x{h} pairs, n = {n}")
    s.set_reference(refs[0])
    make_stale(s, w, h, n)   # a pair batch: it keeps the reference
    hold_items(s, s.score_batch_against_reference(dists[:n]), against, f"{mode} {w}x{h} against, n = {n}")


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", list(SHAPES))
def test_every_item_has_the_bits_of_its_single_score(ctxs, mode, w, h):
    counts = SHAPES[(w, h)]
    refs, dists = pool(w, h, max(counts))
    for n in counts:
        run_both_forms(ctxs[mode], mode, w, h, n, refs, dists)
    pair, _ = singles(mode, w, h, 1)
    if min(w, h) < 8:
        assert pair[0][0] == 100.0 and pair[0][2] == 0 and not pair[0][1].any()
    else:
        assert pair[0][2] >= 1 and pair[0][0] < 100.0


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", [(16, 16), (121, 40)])
def test_257_items_keep_the_persistent_pass_pulling(ctxs, mode, w, h):
    import torch
    n = 257
    if (w, h) == (121, 40):
        # vertical jobs of one item: 3 channels x ceil(w_s / 64) column groups over its four scales (121 x 40, 61 x 20,
        # 31 x 10, 16 x 5): 3 * (2 + 1 + 1 + 1)
        vjobs = 3 * sum(-(-ws // 64) for ws in (121, 61, 31, 16))
        assert vjobs == 15 and n * vjobs == 3855
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert n * vjobs >= 8 * cus, (n * vjobs, cus)   # one workgroup per CU: each pulls many jobs
    refs, dists = pool(w, h, n)
    run_both_forms(ctxs[mode], mode, w, h, n, refs, dists)


@pytest.mark.parametrize("mode", RECURSIVE)
def test_the_largest_batch(ctxs, mode):
    s, (w, h), n = ctxs[mode], (8, 8), _lib.MAX_BATCH
    refs, dists = pool(w, h, n)
    run_both_forms(s, mode, w, h, n, refs, dists)
    _, against = singles(mode, w, h, n)
    avg, ns = s.last_batch_averages(n - 1)
    bits_equal(0.0, avg, 0.0, against[n - 1][1], "the last item's averages")
    with pytest.raises(Ssimu2Error) as ei:
        s.last_batch_averages(n)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    out = (ctypes.c_double * 1)()
    assert s._L.ssimu2_rbatch_score_rgb8_device(s._ctx, 4096, 8192, w * h * 3, n + 1, w, h, out) == _lib.ERR_INVALID_ARG
    assert "SSIMU2_MAX_BATCH" in s._L.ssimu2_last_error(s._ctx).decode()


@pytest.mark.parametrize("mode", RECURSIVE)
def test_device_forms_with_a_stride_and_noise_between_the_frames(ctxs, mode):
    import torch
    s, (w, h), n = ctxs[mode], (121, 40), 33
    refs, dists = pool(w, h, n)
    pair, against = singles(mode, w, h, n)
    stride = w * h * 3 + 52
    bufs = []
    for k, frames in enumerate((refs, dists)):
        g = torch.Generator().manual_seed(k)
        buf = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, generator=g)
        for i, f in enumerate(frames):
            buf[i * stride:i * stride + f.size] = torch.from_numpy(f.reshape(-1))
        bufs.append(buf.cuda())
    torch.cuda.synchronize()
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_device(bufs[0].data_ptr(), bufs[1].data_ptr(), stride, n, w, h), pair, f"{mode} device pairs")
    s.set_reference_device(bufs[0].data_ptr(), w, h)
    make_stale(s, w, h, n)
    hold_items(s, s.score_batch_against_reference_device(bufs[1].data_ptr(), stride, n), against, f"{mode} device against")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_an_items_bits_do_not_depend_on_its_place_or_its_neighbours(ctxs, mode):
    s, (w, h) = ctxs[mode], (121, 40)
    ref = synth.make_ref(w, h, seed=21)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    for against in (False, True):
        got = []
        if against:
            s.set_reference(ref)
        for at, n in ((0, 1), (3, 7), (31, 32)):
            refs, dists = neighbours(w, h, n, seed=at + n)
            refs[at], dists[at] = ref, dist
            make_stale(s, w, h, n)
            scores = s.score_batch_against_reference(dists) if against else s.score_batch(refs, dists)
            got.append((scores[at], *s.last_batch_averages(at)))
        for sc, avg, ns in got[1:]:
            assert ns == got[0][2]
            bits_equal(sc, avg, got[0][0], got[0][1], f"{mode} against={against}")
        assert 0.0 < got[0][0] < 100.0


def test_fir_through_the_new_calls_is_the_existing_batch(ctxs):
    s, (w, h), n = ctxs["fir"], (121, 40), 7
    refs, dists = neighbours(w, h, n, seed=5)
    out = (ctypes.c_double * n)()
    u8pp = lambda fr: (ctypes.POINTER(ctypes.c_uint8) * n)(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) for f in fr])  # noqa: E731
    for against in (False, True):
        if against:
            s.set_reference(refs[0])
            rc = s._L.ssimu2_score_batch_against_reference(s._ctx, u8pp(dists), n, out)
        else:
            rc = s._L.ssimu2_score_batch_rgb8(s._ctx, u8pp(refs), u8pp(dists), n, w, h, out)
        assert rc == _lib.OK
        old = [(out[k], *s.last_batch_averages(k)) for k in range(n)]
        new = s.score_batch_against_reference(dists) if against else s.score_batch(refs, dists)   # the rbatch calls
        hold_items(s, new, old, f"fir against={against}")


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("w,h", [(121, 40), (241, 100)])
def test_a_batch_of_five_against_the_kernel_order_terms(ctxs, oracle, mode, w, h):
    s = ctxs[mode]
    refs, dists = neighbours(w, h, 5, seed=w)
    scores = s.score_batch(refs, dists)
    for k in range(5):
        avg, ns = s.last_batch_averages(k)
        gpu_cases.check_against_terms(oracle, scores[k], avg, ns, refs[k], dists[k], mode, f"{mode} {w}x{h} item {k}")
    s.set_reference(refs[0])
    ds = [damaged(refs[0], k) for k in range(5)]
    scores = s.score_batch_against_reference(ds)
    for k in range(5):
        avg, ns = s.last_batch_averages(k)
        gpu_cases.check_against_terms(oracle, scores[k], avg, ns, refs[0], ds[k], mode, f"{mode} {w}x{h} against, item {k}")


# ---- lifecycle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RECURSIVE)
def test_a_pair_batch_leaves_the_cached_reference_its_pass_and_its_map_alone(hip_lib, mode):
    w, h = 121, 40
    ref = synth.make_ref(w, h, seed=3)
    dist = damaged(ref, 1)
    refs, dists = neighbours(w + 8, h + 8, 9, seed=2)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], rbatch=True) as s:
        s.set_reference(ref)
        cached = s.score_against_reference(dist)
        cavg, _ = s.last_averages()
        mscore, m = s.error_map_against_reference(dist)
        s.score_batch(refs, dists)
        aavg, _ = s.last_averages()
        bits_equal(mscore, aavg, mscore, cavg, "last_averages after a pair batch")
        again = s.score_against_reference(dist)   # no set_reference in between
        aavg, _ = s.last_averages()
        bits_equal(again, aavg, cached, cavg, "cached pass after a pair batch")
        s.score_batch(refs, dists)
        mscore2, m2 = s.error_map_against_reference(dist)
        assert mscore2 == mscore
        gpu_cases.same_bits(m2, m, "recursive error map after a pair batch")
        s.score_batch_against_reference([damaged(ref, k) for k in range(4)])
        again = s.score_against_reference(dist)
        aavg, _ = s.last_averages()
        bits_equal(again, aavg, cached, cavg, "cached pass after an against-reference batch")


@pytest.mark.parametrize("mode", RECURSIVE)
def test_8bit_batch_against_a_16bit_reference(hip_lib, mode):
    w, h, n = 65, 21, 5
    ref = synth.make_ref(w, h, seed=8)
    r16 = ref.astype(np.uint16) * 257
    dists = [damaged(ref, k) for k in range(n)]
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as s:
        s.set_reference_hbd(r16, 16)
        exp = [(s.score_against_reference(d), *s.last_averages()) for d in dists]
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], rbatch=True) as s:
        s.set_reference_hbd(r16, 16)
        hold_items(s, s.score_batch_against_reference(dists), exp, f"{mode}: 8-bit batch, 16-bit reference")


def test_set_blur_drops_the_reference_and_a_pending_enqueue_survives(hip_lib):
    w, h, n = 64, 20, 3
    refs, dists = neighbours(w, h, n, seed=6)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, rbatch=True) as s:
        s.set_reference(refs[0])
        s.score_batch_against_reference(dists)
        s.set_blur(_lib.BLUR_RECURSIVE_FMA)
        with pytest.raises(Ssimu2Error) as ei:
            s.score_batch_against_reference(dists)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        with pytest.raises(Ssimu2Error) as ei:
            s.score_batch_against_reference_device(4096, w * h * 3, n)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        # a pending enqueue: the batch runs behind it on the stream and leaves its result for ssimu2_wait
        dev = on_device([refs[0], dists[0]], refs[0].size)
        s.set_reference_device(dev.data_ptr(), w, h)
        single = s.score_against_reference(dists[0])
        savg, _ = s.last_averages()
        s.enqueue_against_reference_device(dev.data_ptr() + refs[0].size)
        scores = s.score_batch(refs, dists)
        got = s.wait()
        gavg, _ = s.last_averages()
        bits_equal(got, gavg, single, savg, "the enqueued pass, waited for behind a batch")
        again = s.score_batch(refs, dists)
        assert np.array_equal(scores.view(np.uint64), again.view(np.uint64))


def test_a_context_without_a_recursive_batch_allocates_nothing_for_it(hip_lib):
    import torch
    w, h, n = 512, 384, 8
    ref = synth.make_ref(w, h, seed=4)
    dists = [damaged(ref, k) for k in range(n)]
    torch.cuda.synchronize()
    with Ssimu2(0, rbatch=True) as s:
        def work():
            s.set_blur(_lib.BLUR_FIR)
            s.score_batch([ref] * n, dists)   # the FIR batch through the new calls
            s.set_blur(_lib.BLUR_RECURSIVE)
            s.set_reference(ref)
            for d in dists:
                s.score_against_reference(d)
            s.compute_ssimu2(ref, dists[0])
        work()
        free_plain, _ = torch.cuda.mem_get_info(0)
        work()
        assert torch.cuda.mem_get_info(0)[0] == free_plain   # no recursive batch: nothing allocated for one
        s.set_reference(ref)
        s.score_batch_against_reference(dists)
        assert torch.cuda.mem_get_info(0)[0] < free_plain    # ... the first one does


# ---- refusals ------------------------------------------------------------------------------------------------------
def _u8pp(frames):
    return (ctypes.POINTER(ctypes.c_uint8) * len(frames))(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if f is not None
                                                             else None for f in frames])


@pytest.mark.parametrize("mode", list(gpu_cases.MODES))
def test_refusals(hip_lib, golden, mode):
    import torch
    w, h = 64, 40
    refs, dists = neighbours(w, h, 3, seed=1)
    E = _lib.ERR_INVALID_ARG
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], rbatch=True) as s:
        L, c = s._L, s._ctx
        before = gpu_cases.golden_bits(s, golden)
        out = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
        err = lambda: L.ssimu2_last_error(c).decode()   # noqa: E731
        # a null context; n == 0: OK, nothing read
        assert L.ssimu2_rbatch_score_rgb8(None, _u8pp(refs), _u8pp(dists), 3, w, h, out) == E
        assert L.ssimu2_rbatch_score_against_reference(None, _u8pp(dists), 3, out) == E
        assert L.ssimu2_rbatch_score_rgb8_device(None, 4096, 8192, w * h * 3, 3, w, h, out) == E
        assert L.ssimu2_rbatch_score_against_reference_device(None, 4096, w * h * 3, 3, out) == E
        assert L.ssimu2_rbatch_score_rgb8(c, None, None, 0, w, h, None) == _lib.OK
        assert L.ssimu2_rbatch_score_against_reference(c, None, 0, None) == _lib.OK
        assert L.ssimu2_rbatch_score_rgb8_device(c, None, None, 0, 0, w, h, None) == _lib.OK
        assert L.ssimu2_rbatch_score_against_reference_device(c, None, 0, 0, None) == _lib.OK
        # null arrays, a null item, null out_scores, a zero dimension, too many items
        assert L.ssimu2_rbatch_score_rgb8(c, None, _u8pp(dists), 3, w, h, out) == E and "null" in err()
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), None, 3, w, h, out) == E
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp([dists[0], None, dists[2]]), 3, w, h, out) == E
        assert "null image pointer in the batch" in err()
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp(dists), 3, w, h, None) == E
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp(dists), 3, 0, h, out) == E
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp(dists), 3, w, 0, out) == E
        assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp(dists), _lib.MAX_BATCH + 1, w, h, out) == E
        assert "SSIMU2_MAX_BATCH" in err()
        assert L.ssimu2_rbatch_score_rgb8_device(c, None, 8192, w * h * 3, 3, w, h, out) == E
        assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, None, w * h * 3, 3, w, h, out) == E
        assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, 8192, w * h * 3, 3, w, h, None) == E
        assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, 8192, w * h * 3, 3, 0, h, out) == E
        assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, 8192, w * h * 3 - 1, 3, w, h, out) == E
        assert "item_stride_bytes" in err()
        # an item above 2^28 pixels: refused by the recursive modes before anything is allocated or read
        free0, _ = torch.cuda.mem_get_info(0)
        bw, bh = 16385, 16384
        if mode != "fir":   # (FIR has no such limit and would score the frames: not called with these pointers)
            assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, 8192, bw * bh * 3, 2, bw, bh, out) == E and "2^28" in err()
            assert torch.cuda.mem_get_info(0)[0] == free0
        # no reference
        assert L.ssimu2_rbatch_score_against_reference(c, _u8pp(dists), 3, out) == _lib.ERR_NO_REFERENCE
        assert L.ssimu2_rbatch_score_against_reference_device(c, 4096, w * h * 3, 3, out) == _lib.ERR_NO_REFERENCE
        s.set_reference(refs[0])
        assert L.ssimu2_rbatch_score_against_reference(c, None, 3, out) == E
        assert L.ssimu2_rbatch_score_against_reference(c, _u8pp([dists[0], None, dists[2]]), 3, out) == E
        assert L.ssimu2_rbatch_score_against_reference(c, _u8pp(dists), 3, None) == E
        assert L.ssimu2_rbatch_score_against_reference(c, _u8pp(dists), _lib.MAX_BATCH + 1, out) == E
        assert L.ssimu2_rbatch_score_against_reference_device(c, None, w * h * 3, 3, out) == E
        assert L.ssimu2_rbatch_score_against_reference_device(c, 4096, w * h * 3, 3, None) == E
        assert L.ssimu2_rbatch_score_against_reference_device(c, 4096, w * h * 3 - 1, 3, out) == E
        assert "item_stride_bytes" in err()
        assert list(out) == [-1.0] * 4
        # the four calls of ssimu2_hip.h are what they were, in this library too
        if mode != "fir":
            assert L.ssimu2_score_batch_rgb8(c, _u8pp(refs), _u8pp(dists), 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert "ssimu2_ctx_set_blur" in err()
            assert L.ssimu2_score_batch_against_reference(c, _u8pp(dists), 3, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_score_batch_rgb8_device(c, 4096, 8192, w * h * 3, 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_score_batch_against_reference_device(c, 4096, w * h * 3, 3, out) == _lib.ERR_UNSUPPORTED
            assert list(out) == [-1.0] * 4
        after = gpu_cases.golden_bits(s, golden)
        bits_equal(after[0], after[1], before[0], before[1], "after the refusals")
        assert s.score_batch(refs, dists).shape == (3,)   # and the context batches


def test_a_context_without_the_flag_refuses_as_before(hip_lib):
    refs, dists = neighbours(64, 20, 3, seed=1)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE) as s:
        assert not s.rbatch
        with pytest.raises(Ssimu2Error) as ei:
            s.score_batch(refs, dists)
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "ssimu2_ctx_set_blur" in str(ei.value)


def test_a_service_context_refuses_and_goes_on_scoring(hip_lib):
    from oavif_amd import service
    w, h = 64, 40
    refs, dists = neighbours(w, h, 3, seed=1)
    svc = service.start(max_lifetime=120)
    try:
        with Ssimu2(0, service=svc.socket, rbatch=True) as s:
            exp = s.compute_ssimu2(refs[0], dists[0])
            out = (ctypes.c_double * 3)()
            L, c = s._L, s._ctx
            assert L.ssimu2_rbatch_score_rgb8(c, _u8pp(refs), _u8pp(dists), 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_rbatch_score_against_reference(c, _u8pp(dists), 3, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_rbatch_score_rgb8_device(c, 4096, 8192, w * h * 3, 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_rbatch_score_against_reference_device(c, 4096, w * h * 3, 3, out) == _lib.ERR_UNSUPPORTED
            assert s.compute_ssimu2(refs[0], dists[0]) == exp
    finally:
        assert svc.stop(timeout=30) == 0
