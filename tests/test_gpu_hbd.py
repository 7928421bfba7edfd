"""16-bit scorer input on the MI355X (ssimu2_*_rgb16 / _strided16), in all three blur modes:
bit identity with the 8-bit path on 257*u frames, mixed depths against a cached reference, the strided hand-off,
clamping, genuine 10/12/16-bit content against tests/hbd_ref.py and the fp64 counterpart, and the context lifecycle.

Genuine 16-bit content is also held to the kernel-order terms (gpu_cases.check_against_terms): hbd_ref.compute's
averages ARE errmap_ref.averages(hbd_ref.terms(...)), the fp64 means of the fp32 terms k_march_lin /
k_march_refblur_lin sum, so the derived bounds of tests/gpu_cases.py apply unchanged -- RTOL_RECURSIVE in the recursive
modes, fir_rtol in FIR (k_march_lin shares march_v and the segment rule with k_march), FINALIZE_TOL for k_finalize."""
import numpy as np
import pytest

import fp64_checks
import gpu_cases
import hbd_ref
from hbd_cases import hbd_content, hbd_distort, lift, rows16
from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
KINDS = ["gradient", "primaries", "checker", "text", "noise"]


ctxs = gpu_cases.contexts_fixture()


def pair_8(s, ref, dist):
    score = s.compute_ssimu2(ref, dist)
    return score, s.last_averages()


def assert_same(s, score, exp, what):
    avg, ns = s.last_averages()
    assert score == exp[0], (what, score, exp[0])
    assert ns == exp[1][1] and np.array_equal(avg, exp[1][0]), what


@pytest.mark.parametrize("mode", MODES)
def test_bit_identity_with_the_8bit_path(ctxs, mode):
    s = ctxs[mode]
    sizes = gpu_cases.SIZES + [(1920, 1080), (3840, 2160)]
    for k, (w, h) in enumerate(sizes):
        kind = KINDS[k % len(KINDS)]
        ref = gpu_cases.content(kind, w, h, seed=k) if w * h < 10**6 else synth.make_ref(w, h, seed=k)
        dist = synth.distort(ref, "blockq", 2) if w >= 8 and h >= 8 else gpu_cases.content("noise", w, h, seed=k + 50)
        exp = pair_8(s, ref, dist)
        what = (mode, w, h, kind)
        assert_same(s, s.compute_ssimu2_hbd(lift(ref), lift(dist), 16), exp, what + ("rgb16 257u",))
        assert_same(s, s.compute_ssimu2_hbd(ref.astype(np.uint16), dist.astype(np.uint16), 8), exp, what + ("rgb16 d8",))
        # cached reference: 8-bit reference, 8-bit pass; then the 16-bit reference and 16-bit passes, tight and strided
        s.set_reference(ref)
        exp_c = (s.score_against_reference(dist), s.last_averages())
        s.set_reference_hbd(lift(ref), 16)
        assert_same(s, s.score_against_reference_hbd(lift(dist), 16), exp_c, what + ("cached 16/16",))
        assert_same(s, s.score_against_reference_hbd(dist.astype(np.uint16), 8), exp_c, what + ("cached 16/d8",))
        buf, view = rows16(lift(dist), 4, 6, seed=k)
        assert_same(s, s.score_decoded_against_reference_hbd(view, bit_depth=16), exp_c, what + ("strided16",))


@pytest.mark.parametrize("mode", MODES)
def test_genuine_high_bit_depth_content_against_the_checker(ctxs, oracle, mode):
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    k, worst = 0, 0.0
    for depth in (10, 12, 16):
        for kind in ["hgradient", "hnoise"] + KINDS:
            w, h = [(256, 192), (333, 217), (129, 41)][k % 3]
            ref = hbd_content(kind, w, h, depth, seed=k)
            dist = hbd_distort(ref, depth, seed=k + 100)
            got = s.compute_ssimu2_hbd(ref, dist, depth)
            avg, ns = s.last_averages()
            exp, avg_r, ns_r = hbd_ref.compute(oracle, ref, dist, depth, blur)
            assert ns == ns_r, (mode, depth, kind)
            assert abs(got - exp) <= gpu_cases.score_tol(exp), (mode, depth, kind, got, exp)
            assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), (mode, depth, kind)
            exp64 = hbd_ref.compute_fp64(ref, dist, depth)
            # white noise and flat or saturated content: fp32 cancellation noise is as large as the averages there,
            # so fp64_checks' "synthetic" bounds (every weighted average absolutely, the score loosely) apply
            fp64_checks.check(got, avg, ns, exp64, mode, (mode, depth, kind), "synthetic")
            worst = max(worst, gpu_cases.check_against_terms(oracle, got, avg, ns, ref, dist, mode,
                                                             f"{mode} {depth}-bit {kind} {w}x{h}", kavg=avg_r))
            k += 1
    print(f"measured: genuine 16-bit content, {mode}: worst average {worst:.3e} of its bound")


@pytest.mark.parametrize("mode", MODES)
def test_mixed_depths(ctxs, oracle, mode):
    s = ctxs[mode]
    w, h = 333, 217
    ref8 = gpu_cases.content("text", w, h, seed=3)
    d16 = hbd_distort(hbd_content("text", w, h, 16, seed=4), 16, seed=5)
    d8 = synth.distort(ref8, "blockq", 3)
    # 8-bit reference, 16-bit frames: the pair score of the lifted reference and the frame
    exp = (s.compute_ssimu2_hbd(lift(ref8), d16, 16), s.last_averages())
    s.set_reference(ref8)
    assert_same(s, s.score_against_reference_hbd(d16, 16), exp, (mode, "8-bit ref, 16-bit frame"))
    buf, view = rows16(d16, 3, 5, seed=1)
    assert_same(s, s.score_decoded_against_reference_hbd(view, bit_depth=16), exp, (mode, "8-bit ref, strided"))
    # 16-bit reference, 8-bit frames: the pair score with the 8-bit frame as 257 u
    r16 = hbd_content("gradient", w, h, 16, seed=6)
    exp = (s.compute_ssimu2_hbd(r16, lift(d8), 16), s.last_averages())
    s.set_reference_hbd(r16, 16)
    assert_same(s, s.score_against_reference(d8), exp, (mode, "16-bit ref, 8-bit frame"))
    for ch, pad in ((3, 0), (4, 8)):
        buf8, view8 = gpu_cases.decoded_like(d8, ch, pad, seed=2)
        assert_same(s, s.score_decoded_against_reference(view8), exp, (mode, "16-bit ref, 8-bit strided", ch))
    # a 10-bit frame against a 12-bit reference: the checker and the fp64 counterpart read each frame at its own depth
    r12 = hbd_content("text", w, h, 12, seed=7)
    d10 = hbd_distort(hbd_content("text", w, h, 10, seed=7), 10, seed=8)
    s.set_reference_hbd(r12, 12)
    got = s.score_against_reference_hbd(d10, 10)
    avg, ns = s.last_averages()
    exp, avg_r, ns_r = hbd_ref.compute(oracle, r12, d10, 12, gpu_cases.MODES[mode][1], d_dist=10)
    assert ns == ns_r and abs(got - exp) <= gpu_cases.score_tol(exp), (mode, got, exp)
    assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), mode
    fp64_checks.check(got, avg, ns, hbd_ref.compute_fp64(r12, d10, 12, d_dist=10), mode, (mode, "12/10"), "synthetic")
    gpu_cases.check_against_terms(oracle, got, avg, ns, r12, d10, mode, f"{mode} 10-bit frame, 12-bit reference", kavg=avg_r)
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(d8)
    assert ei.value.code == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("mode", MODES)
def test_strided_hand_off_equals_the_tight_call(ctxs, oracle, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate([(333, 217), (120, 40), (121, 41), (1921, 1083), (8, 8)]):
        ref = hbd_content("text", w, h, 10, seed=k)
        dist = hbd_distort(ref, 10, seed=k + 1)
        s.set_reference_hbd(ref, 10)
        exp = (s.score_against_reference_hbd(dist, 10), s.last_averages())
        if k == 0:   # the hand-offs below equal the tight call in bits: one value check anchors them all
            _score, kavg, ns_r = hbd_ref.compute(oracle, ref, dist, 10, gpu_cases.MODES[mode][1])
            assert ns_r == exp[1][1]
            gpu_cases.check_against_terms(oracle, exp[0], exp[1][0], ns_r, ref, dist, mode,
                                          f"{mode} tight 10-bit call {w}x{h}", kavg=kavg)
        for ch, pad in ((3, 0), (3, 7), (4, 0), (4, 12)):
            buf, view = rows16(dist, ch, pad, seed=k + ch)
            assert_same(s, s.score_decoded_against_reference_hbd(view, bit_depth=10), exp, (mode, w, h, ch, pad))
            flat = buf.reshape(-1)
            assert_same(s, s.score_decoded_against_reference_hbd(flat, row_bytes=buf.strides[0], channels=ch,
                                                                 bit_depth=10), exp, (mode, w, h, ch, pad, "flat"))


@pytest.mark.parametrize("mode", MODES)
def test_samples_above_the_depth_are_clamped(ctxs, mode):
    s = ctxs[mode]
    w, h = 257, 131
    ref = hbd_content("gradient", w, h, 10, seed=1)
    dist = hbd_distort(ref, 10, seed=2)
    rng = np.random.default_rng(3)
    wild = dist.copy()
    mask = rng.random(dist.shape) < 0.2
    wild[mask] = rng.integers(1024, 65536, int(mask.sum()))
    clamped = np.minimum(wild, 1023).astype(np.uint16)
    exp = (s.compute_ssimu2_hbd(ref, clamped, 10), s.last_averages())
    assert_same(s, s.compute_ssimu2_hbd(ref, wild, 10), exp, (mode, "pair"))
    s.set_reference_hbd(ref, 10)
    assert_same(s, s.score_against_reference_hbd(wild, 10), exp, (mode, "cached"))


def test_lifecycle_memory_interleaving_and_repeats(hip_lib):
    import torch
    w, h = 1920, 1080
    ref = synth.make_ref(w, h, seed=4)
    dist = synth.distort(ref, "blockq", 2)
    r16, d16 = lift(ref), hbd_distort(lift(ref), 16, seed=9)
    torch.cuda.synchronize()
    with Ssimu2(0) as s:
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)
        free_plain, _ = torch.cuda.mem_get_info(0)
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)
        assert torch.cuda.mem_get_info(0)[0] == free_plain   # an 8-bit-only context allocates nothing for 16 bits
        exp8 = s.compute_ssimu2(ref, dist)
        exp16 = s.compute_ssimu2_hbd(r16, d16, 16)
        assert torch.cuda.mem_get_info(0)[0] < free_plain    # ... the first 16-bit call does
        for mode in (_lib.BLUR_RECURSIVE, _lib.BLUR_FIR, _lib.BLUR_RECURSIVE_FMA, _lib.BLUR_FIR):
            s.set_blur(mode)
            a8, a16 = s.compute_ssimu2(ref, dist), s.compute_ssimu2_hbd(r16, d16, 16)
            assert s.compute_ssimu2(ref, dist) == a8 and s.compute_ssimu2_hbd(r16, d16, 16) == a16
            s.set_reference_hbd(r16, 16)
            c16 = s.score_against_reference_hbd(d16, 16)
            assert c16 == a16 and s.score_against_reference_hbd(d16, 16) == c16
            assert s.score_against_reference(dist) == s.score_against_reference(dist)
            if mode == _lib.BLUR_FIR:
                assert (a8, a16) == (exp8, exp16)
    with Ssimu2(0) as s:   # the 16-bit buffers went with the context: the same 8-bit work holds what it held
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)
        assert abs(torch.cuda.mem_get_info(0)[0] - free_plain) <= (8 << 20)


def test_argument_errors_on_the_device(ctxs):
    s = ctxs["fir"]
    a = np.zeros((16, 16, 3), np.uint16)
    for bad in (7, 17, 0):
        with pytest.raises(Ssimu2Error) as ei:
            s.compute_ssimu2_hbd(a, a, bad)
        assert ei.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(TypeError):
        s.compute_ssimu2_hbd(a.astype(np.uint8), a.astype(np.uint8), 8)
    with pytest.raises(ValueError):
        s.compute_ssimu2_hbd(a[..., :2], a[..., :2], 8)


@pytest.mark.parametrize("mode", MODES)
def test_search_with_16bit_decodes_end_to_end(ctxs, mode):
    from oavif_amd import avif_bridge as ab, cli, tq
    if not ab.available():
        pytest.fail(f"libavif bridge unavailable: {ab.why_unavailable()}")
    s = ctxs[mode]
    ref = synth.make_ref(333, 211, 21)
    o = cli.AvifEncOptions()
    o.tenbit = False
    data, seen = {}, []

    def codec_frame(q):
        if q not in data:
            data[q] = ab.encode(ref, 8, o, q)
        f = ab.decode_common(data[q], rgb_depth=16)
        seen.append((q, f.tight_rgb16()))
        return f, len(data[q])

    r = tq.search_hip_frames(s, ref, codec_frame, score_tgt=84.0, tolerance=1.0, max_pass=5)
    assert 1 <= r.num_pass == len(seen)
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0]) as pair:
        for (q, score), (q2, px) in zip(r.history, seen):
            assert q == q2
            assert score == pair.compute_ssimu2_hbd(lift(ref), px, 16), (mode, q)
    # the same search with the source as 16-bit samples
    r16 = tq.search_hip_frames(s, lift(ref), codec_frame, score_tgt=84.0, tolerance=1.0, max_pass=5, ref_bit_depth=16)
    assert r16.history == r.history and r16.q == r.q
