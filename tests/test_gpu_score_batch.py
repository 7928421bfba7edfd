"""Batch scoring on the MI355X (ssimu2_score_batch_*): an item's score is a property of its pair
(independent of the batch), has the bits of a single score taken at the same segment rows, is the same in the pair and
the cached-reference form, and holds to the checker's kernel-order terms; the contract of include/ssimu2_hip.h.

The bound against the kernel-order terms (test 7) is gpu_cases.fir_rtol's formula evaluated at the BATCH rule's segment
rows.  Derivation (tests/gpu_cases.py, "FIR"): k_march sums each fp32 term per lane down the rows of its segment, then in
fp64.  A lane of a batch item sums at most R = min(batch rule rows, rows of the scale) non-negative fp32 terms: within
(R - 1) * 2^-24 of the exact sum; the edge quotient adds 4 units to an L1 statistic and 22 / 4 to an L4 one, so every
average is within (R + 3) * 2^-24, plus n * 2^-53 for the fp64 part over the scale's n pixels.  The batch rule is 96
rows at full resolution and at most 48 below it (ssimu2_hip.hip: batch_seg_rows), whatever the frame size."""
import ctypes
import os
import struct
import sys
import threading
import zlib

import numpy as np
import pytest

from oavif_amd import _lib, pam, scorepairs, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_cases  # noqa: E402

pytestmark = pytest.mark.gpu

from gpu_cases import (KINDS, batch_rtol, batch_seg_rows, bits_equal, check_item_against_terms, damaged,  # noqa: E402
                       golden_bits, neighbours)


def item_in_batches(s, ref, dist, cached, placements=((0, 1), (3, 7), (31, 32), (5, 64))):
    """(score, averages) of the pair as item `at` of `n`, among different neighbours each time."""
    h, w, _ = ref.shape
    out = []
    if cached:
        s.set_reference(ref)
    for at, n in placements:
        refs, dists = neighbours(w, h, n, seed=at + n)
        refs[at], dists[at] = ref, dist
        if cached:
            dists = [dist if k == at else damaged(ref, 7 * n + k) for k in range(n)]
            scores = s.score_batch_against_reference(dists)
        else:
            scores = s.score_batch(refs, dists)
        avg, ns = s.last_batch_averages(at)
        out.append((scores[at], avg, ns))
    return out


def assert_independent(results, what):
    s0, a0, n0 = results[0]
    for k, (sc, avg, ns) in enumerate(results[1:], 1):
        assert ns == n0, what
        bits_equal(sc, avg, s0, a0, f"{what}: placement {k}")


@pytest.mark.parametrize("cached", [False, True], ids=["pairs", "cached_reference"])
def test_an_items_score_does_not_depend_on_its_batch(scorer, cached):
    ref = synth.make_ref(320, 200, seed=21)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    res = item_in_batches(scorer, ref, dist, cached)
    assert res[0][2] == 6 and 0.0 < res[0][0] < 100.0
    assert_independent(res, "cached" if cached else "pairs")


@pytest.mark.parametrize("w,h", [s for s in gpu_cases.SIZES if min(s) >= 8])
def test_batch_item_has_the_bits_of_a_single_score_at_the_same_rows(iscorer, w, h):
    s = iscorer
    rule = [s.batch_segment_rows(w, h, sc) for sc in (0, 1)]
    assert rule == [batch_seg_rows(w, h, 0), batch_seg_rows(w, h, 1)]
    assert all(s.batch_segment_rows(w, h, sc) == rule[1] for sc in range(1, 6))
    ref = gpu_cases.content("noise", w, h, w * 31 + h) if w * h < 4096 else synth.make_ref(w, h, seed=w + h)
    dist = damaged(ref, w)
    refs, dists = neighbours(w, h, 3, seed=w ^ h)
    refs[1], dists[1] = ref, dist
    scores = s.score_batch(refs, dists)
    avg, ns = s.last_batch_averages(1)
    try:
        s.set_segment_rows(rule[0], rule[1])
        single = s.compute_ssimu2(ref, dist)
        avg1, ns1 = s.last_averages()
    finally:
        s.set_segment_rows(0, 0)
    assert ns == ns1
    bits_equal(scores[1], avg, single, avg1, f"{w}x{h}")


def test_frames_without_a_scale_score_100(scorer):
    for w, h in [s for s in gpu_cases.SIZES if min(s) < 8]:
        refs, dists = neighbours(w, h, 3, seed=w + h)
        scores = scorer.score_batch(refs, dists)
        assert (scores == 100.0).all(), (w, h, scores)
        avg, ns = scorer.last_batch_averages(2)
        assert ns == 0 and not avg.any()


@pytest.mark.parametrize("w,h", [(256, 192), (509, 131), (121, 40)])
def test_pair_form_equals_cached_reference_form(scorer, w, h):
    ref = synth.make_ref(w, h, seed=w)
    dists = [damaged(ref, k) for k in range(5)] + [ref.copy()]
    pair = scorer.score_batch([ref] * len(dists), dists)
    pavg = [scorer.last_batch_averages(k) for k in range(len(dists))]
    scorer.set_reference(ref)
    cached = scorer.score_batch_against_reference(dists)
    for k in range(len(dists)):
        avg, ns = scorer.last_batch_averages(k)
        assert ns == pavg[k][1]
        bits_equal(cached[k], avg, pair[k], pavg[k][0], f"{w}x{h} item {k}")
    assert pair[-1] == 100.0 and not pavg[-1][0].any()


def test_golden_pairs_in_one_batch_against_the_kernel_order_terms(scorer, oracle, golden):
    arrays, _meta = golden
    ref = arrays["ref"]
    keys = ("avif_q20", "avif_q65", "blockq2", "noise1", "blur1")
    scores = scorer.score_batch([ref] * len(keys), [arrays[k] for k in keys])
    for i, k in enumerate(keys):
        avg, ns = scorer.last_batch_averages(i)
        check_item_against_terms(oracle, scores[i], avg, ns, ref, arrays[k], f"golden {k}")
    scores = scorer.score_batch([arrays["odd_ref"]], [arrays["odd_dist"]])
    avg, ns = scorer.last_batch_averages(0)
    check_item_against_terms(oracle, scores[0], avg, ns, arrays["odd_ref"], arrays["odd_dist"], "golden odd")


@pytest.mark.parametrize("w,h", [(256, 192), (509, 131)])
def test_sixteen_seeded_frames_against_the_kernel_order_terms(scorer, oracle, w, h):
    refs, dists = neighbours(w, h, 16, seed=w)
    scores = scorer.score_batch(refs, dists)
    assert {KINDS[(k + w) % 5] for k in range(16)} == set(KINDS)
    for k in range(16):
        avg, ns = scorer.last_batch_averages(k)
        if k % 5 == 4:   # identical pair, next to damaged ones
            assert scores[k] == 100.0 and not avg.any(), k
        check_item_against_terms(oracle, scores[k], avg, ns, refs[k], dists[k], f"{w}x{h} item {k}")
    print(f"measured: {w}x{h}: scores {np.round(scores, 2).tolist()}")
    assert scores[0] < 30.0   # the inverted frame: heavily damaged, next to identical pairs


# ---- contract ----------------------------------------------------------------------------------------------------
def _u8pp(frames):
    return (ctypes.POINTER(ctypes.c_uint8) * len(frames))(*[f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if f is not None
                                                             else None for f in frames])


def test_refusals_leave_the_context_as_it_was(hip_lib, golden):
    from oavif_amd import Ssimu2
    L = hip_lib
    s = Ssimu2(0)
    try:
        before = golden_bits(s, golden)
        w, h = 64, 40
        refs, dists = neighbours(w, h, 3, seed=1)
        out = (ctypes.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
        err = lambda: L.ssimu2_last_error(s._ctx).decode()   # noqa: E731

        def unchanged(what):
            after = golden_bits(s, golden)
            bits_equal(after[0], after[1], before[0], before[1], what)

        # n == 0: OK, nothing read, nothing written
        assert L.ssimu2_score_batch_rgb8(s._ctx, None, None, 0, w, h, None) == _lib.OK
        assert L.ssimu2_score_batch_against_reference(s._ctx, None, 0, None) == _lib.OK
        assert L.ssimu2_score_batch_rgb8_device(s._ctx, None, None, 0, 0, w, h, None) == _lib.OK
        assert L.ssimu2_score_batch_against_reference_device(s._ctx, None, 0, 0, None) == _lib.OK
        unchanged("n == 0")
        # null arrays, a null item, null out_scores, zero size, too many items
        assert L.ssimu2_score_batch_rgb8(s._ctx, None, _u8pp(dists), 3, w, h, out) == _lib.ERR_INVALID_ARG and "null" in err()
        assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), None, 3, w, h, out) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), _u8pp([dists[0], None, dists[2]]), 3, w, h, out) == _lib.ERR_INVALID_ARG
        assert "null image pointer in the batch" in err()
        assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), _u8pp(dists), 3, w, h, None) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), _u8pp(dists), 3, 0, h, out) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), _u8pp(dists), _lib.MAX_BATCH + 1, w, h, out) == _lib.ERR_INVALID_ARG
        assert "SSIMU2_MAX_BATCH" in err()
        # the device forms: null pointers and a stride below one frame (refused before any pointer is read)
        assert L.ssimu2_score_batch_rgb8_device(s._ctx, None, None, w * h * 3, 3, w, h, out) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_score_batch_rgb8_device(s._ctx, 4096, 8192, w * h * 3 - 1, 3, w, h, out) == _lib.ERR_INVALID_ARG
        assert "item_stride_bytes" in err()
        assert list(out) == [-1.0] * 4
        unchanged("invalid arguments")
        # no reference
        assert L.ssimu2_score_batch_against_reference(s._ctx, _u8pp(dists), 3, out) == _lib.ERR_NO_REFERENCE
        assert L.ssimu2_score_batch_against_reference_device(s._ctx, 4096, w * h * 3, 3, out) == _lib.ERR_NO_REFERENCE
        s.set_reference(refs[0])
        assert L.ssimu2_score_batch_against_reference(s._ctx, None, 3, out) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_score_batch_against_reference_device(s._ctx, 4096, w * h * 3 - 1, 3, out) == _lib.ERR_INVALID_ARG
        assert L.ssimu2_last_batch_averages(s._ctx, 0, (ctypes.c_double * 108)(), None) == _lib.ERR_INVALID_ARG  # no batch yet
        unchanged("no reference")
        # the recursive modes refuse, name the way out, and keep their mode
        for mode in (_lib.BLUR_RECURSIVE, _lib.BLUR_RECURSIVE_FMA):
            s.set_blur(mode)
            rec = s.compute_ssimu2(refs[0], dists[0])
            assert L.ssimu2_score_batch_rgb8(s._ctx, _u8pp(refs), _u8pp(dists), 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert "ssimu2_ctx_set_blur" in err()
            assert L.ssimu2_score_batch_against_reference(s._ctx, _u8pp(dists), 3, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_score_batch_rgb8_device(s._ctx, 4096, 8192, w * h * 3, 3, w, h, out) == _lib.ERR_UNSUPPORTED
            assert L.ssimu2_score_batch_against_reference_device(s._ctx, 4096, w * h * 3, 3, out) == _lib.ERR_UNSUPPORTED
            assert s.compute_ssimu2(refs[0], dists[0]) == rec   # still the recursive mode
        s.set_blur(_lib.BLUR_FIR)
        assert list(out) == [-1.0] * 4
        unchanged("recursive modes")
        scores = s.score_batch(refs, dists)   # and the context batches
        assert scores.shape == (3,) and L.ssimu2_last_batch_averages(s._ctx, 3, (ctypes.c_double * 108)(), None) == _lib.ERR_INVALID_ARG
        unchanged("after a batch")
    finally:
        s.close()


def test_a_batch_leaves_single_scores_maps_and_the_cached_reference_alone(hip_lib, golden):
    from oavif_amd import Ssimu2
    arrays, _ = golden
    ref, dist = arrays["ref"], arrays["avif_q20"]
    h, w, _c = ref.shape
    s = Ssimu2(0)
    try:
        single = s.compute_ssimu2(ref, dist)
        savg, _ = s.last_averages()
        mscore, m = s.error_map(ref, dist)
        s.set_reference(ref)
        cached = s.score_against_reference(dist)
        cavg, _ = s.last_averages()
        refs, dists = neighbours(w, h, 6, seed=3)
        s.score_batch(refs, dists)                    # a pair batch keeps the cached reference
        again = s.score_against_reference(dist)       # no set_reference in between
        aavg, _ = s.last_averages()
        bits_equal(again, aavg, cached, cavg, "cached score after a pair batch")
        s.score_batch_against_reference([damaged(ref, k) for k in range(5)])
        aavg, _ = s.last_averages()
        bits_equal(again, aavg, cached, cavg, "last_averages after an against-reference batch")
        again = s.score_against_reference(dist)
        aavg, _ = s.last_averages()
        bits_equal(again, aavg, cached, cavg, "cached score after an against-reference batch")
        _sc, m_ref = s.error_map_against_reference(dist)
        gpu_cases.same_bits(m_ref, m, "map against the kept reference")
        s.score_batch(refs, dists)
        single2 = s.compute_ssimu2(ref, dist)
        savg2, _ = s.last_averages()
        bits_equal(single2, savg2, single, savg, "single score after a pair batch")
        mscore2, m2 = s.error_map(ref, dist)
        assert mscore2 == mscore
        gpu_cases.same_bits(m2, m, "error map after a pair batch")
    finally:
        s.close()


def test_scratch_growth_then_a_smaller_batch(hip_lib):
    from oavif_amd import Ssimu2
    ref = synth.make_ref(200, 150, seed=5)
    dist = synth.distort(ref, "blockq", 3, seed=6)
    s = Ssimu2(0)
    try:
        for cached in (False, True):
            res = item_in_batches(s, ref, dist, cached, placements=((0, 1), (1, 4), (11, 12), (2, 3)))
            assert_independent(res, f"growth cached={cached}")
        big = synth.make_ref(700, 500, seed=9)        # a larger frame grows every buffer again
        res = item_in_batches(s, big, damaged(big, 2), False, placements=((0, 1), (4, 5), (1, 2)))
        assert_independent(res, "growth, larger frame")
    finally:
        s.close()


def test_two_contexts_batch_concurrently_from_two_threads(hip_lib):
    from oavif_amd import Ssimu2
    ref = synth.make_ref(320, 200, seed=21)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    ctxs = [Ssimu2(0), Ssimu2(0)]
    results, errors = [None, None], []

    def work(i):
        try:
            rounds = [item_in_batches(ctxs[i], ref, dist, cached=bool(i)) for _ in range(3)]
            results[i] = [r for rnd in rounds for r in rnd]
        except BaseException as e:   # surfaced on the main thread
            errors.append(e)
    try:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert_independent(results[0], "thread 0 (pairs)")
        assert_independent(results[1], "thread 1 (cached reference)")
        bits_equal(results[0][0][0], results[0][0][1], results[1][0][0], results[1][0][1], "pair form == cached form across contexts")
    finally:
        for c in ctxs:
            c.close()


def test_device_forms_equal_the_host_forms(scorer):
    import torch
    w, h, n = 256, 192, 5
    refs, dists = neighbours(w, h, n, seed=8)
    host = scorer.score_batch(refs, dists)
    havg = [scorer.last_batch_averages(k)[0] for k in range(n)]
    stride = w * h * 3 + 48    # items need not be tightly packed
    dr = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    dd = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    for k in range(n):
        dr[k * stride:k * stride + w * h * 3] = torch.from_numpy(refs[k].ravel()).cuda()
        dd[k * stride:k * stride + w * h * 3] = torch.from_numpy(dists[k].ravel()).cuda()
    torch.cuda.synchronize()
    dev = scorer.score_batch_device(dr.data_ptr(), dd.data_ptr(), stride, n, w, h)
    for k in range(n):
        bits_equal(dev[k], scorer.last_batch_averages(k)[0], host[k], havg[k], f"device item {k}")
    scorer.set_reference_device(dr.data_ptr(), w, h)
    same_ref = scorer.score_batch_against_reference_device(dd.data_ptr(), stride, n)
    pair = scorer.score_batch([refs[0]] * n, dists)
    assert np.array_equal(same_ref.view(np.uint64), pair.view(np.uint64))


# ---- scorepairs end to end ---------------------------------------------------------------------------------------
def _png(rgb):
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_scorepairs_end_to_end(scorer, oracle, tmp_path):
    specs = [(96, 64, "png"), (160, 120, "pam"), (96, 64, "pam"), (160, 120, "png"), (96, 64, "png"), (160, 120, "pam")]
    frames, lines = [], []
    for k, (w, h, fmt) in enumerate(specs):
        ref = synth.make_ref(w, h, seed=40 + k)
        dist = damaged(ref, k)
        frames.append((ref, dist))
        for name, a in ((f"r{k}.{fmt}", ref), (f"d{k}.{fmt}", dist)):
            (tmp_path / name).write_bytes(_png(a) if fmt == "png" else pam.write_pam(a))
        lines.append(f"r{k}.{fmt}\td{k}.{fmt}")
    (tmp_path / "pairs.tsv").write_text("\n".join(lines) + "\n")
    assert scorepairs.main([str(tmp_path / "pairs.tsv"), str(tmp_path / "out.csv"), "--batch", "2"], scorer=scorer) == 0
    rows = [ln.split(",") for ln in open(tmp_path / "out.csv").read().splitlines()[1:]]
    assert [int(r[0]) for r in rows] == list(range(1, len(specs) + 1))
    for k, (ref, dist) in enumerate(frames):
        h, w, _ = ref.shape
        single = scorer.compute_ssimu2(ref, dist)
        avg, ns = scorer.last_averages()
        # both scores' averages are within their bounds of the same exact means: the weighted sum moves by at most
        # r = the two bounds added, relatively, and the score by what the published polynomial makes of that
        r = max(batch_rtol(w, h, s) + gpu_cases.fir_rtol(w, h, s) for s in range(ns))
        f = lambda a: oracle.score_from_averages(a, ns)   # noqa: E731
        bound = max(abs(f(avg * (1 + r)) - f(avg)), abs(f(avg * (1 - r)) - f(avg))) + 2 * gpu_cases.FINALIZE_TOL
        got = float(rows[k][5])
        print(f"measured: scorepairs pair {k}: |batch - single| = {abs(got - single):.3e} (bound {bound:.3e})")
        assert (int(rows[k][3]), int(rows[k][4])) == (w, h) and abs(got - single) <= bound, (k, got, single, bound)
