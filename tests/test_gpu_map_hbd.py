"""Error maps of 16-bit, RGBA and YUV frames on the MI355X (include/ssimu2_hip_map.h), in all
three blur modes.

The reference is numpy alone, built from the helpers the 8-bit map is held with: scale-0 linear planes
(hbd_ref.linear_planes, or the composite table for RGBA codes) -> errmap_ref.terms_lin -> errmap_ref.coefficients of the
DEVICE's averages (as gpu_cases.check_map takes them) -> errmap_ref.compose.  The comparison rule is check_map's, restated
in map_cases.hold_map because check_map itself builds its reference from 8-bit frames: the recursive modes bit for bit;
FIR per pixel within gpu_cases.MAP_K * 2^-24 of the reference pixel and 0 exactly where the reference is 0; the mean to
errmap_ref.MEAN_RTOL.  MAP_K counts the roundings after the blur, which k_march_map_lin shares with k_march_map (the two
differ in where a converter lane takes its linear value from, a load instead of a table read), so the bound is the 8-bit
map's, unchanged.  Everything else here is an identity between two device results and is held bit for bit."""
import ctypes

import numpy as np
import pytest

import gpu_cases
import hbd_cases
import yuv_ref
from map_cases import assert_bits, check_pair_hbd, hold_map, reference_map, results
from oavif_amd import Ssimu2, Ssimu2Error, _lib, scorer as scorer_mod, synth
from test_gpu_alpha import alpha_plane, codes_of, laid_out, rgba_of
from test_gpu_yuv import frame_of, yuv_pair

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
# no scale (zero map, score 100); one scale; ragged; across the 120-column strip; several scales; 40 x 41: six row
# segments of eight rows at scale 0, the last one ragged (the smallest sizes already have two or three)
SIZES = [(1, 1), (7, 7), (8, 8), (9, 17), (121, 9), (129, 67), (250, 130), (40, 41)]
DEPTHS = (8, 10, 12, 16)

mctxs = gpu_cases.contexts_fixture(maps=True, extended=True, yuv=True)


# ---- 1. the pair map against the numpy reference -----------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("mode", MODES)
def test_pair_map_matches_the_reference(mctxs, oracle, mode, size):
    w, h = size
    if (w, h) == (40, 41):
        assert h > 5 * gpu_cases.march_seg_rows(w, h, 0)
    if (w, h) == (121, 9):
        assert w > gpu_cases.MW
    s = mctxs[mode]
    for d in DEPTHS:
        ref = hbd_cases.content16(w, h, d, seed=w + h)
        dist = hbd_cases.content16(w, h, d, seed=w + h, distort=True)
        check_pair_hbd(oracle, s, mode, ref, dist, d, f"{mode} {w}x{h} depth {d}")


@pytest.mark.parametrize("mode", MODES)
def test_all_zero_against_all_maximum_reaches_the_coefficient_clamp(mctxs, oracle, mode):
    w, h = 90, 70
    zero, top = np.zeros((h, w, 3), np.uint16), np.full((h, w, 3), 65535, np.uint16)
    for ref, dist, name in ((zero, top, "0 / max"), (top, zero, "max / 0")):
        _worst, score, m = check_pair_hbd(oracle, mctxs[mode], mode, ref, dist, 16, f"{mode} {name}")
        assert score < 0.0 and m.any()


# ---- 2. codes 257 u at depth 16 are the 8-bit frames ---------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_depth_16_map_of_lifted_frames_is_the_8_bit_map(mctxs, mode):
    s = mctxs[mode]
    for k, (w, h) in enumerate([(9, 17), (121, 9), (129, 67), (250, 130), (40, 41)]):
        ref = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
        dist = synth.distort(ref, "blockq", 2, seed=k)
        score8, m8 = s.error_map(ref, dist)
        exp = results(s, score8)
        score, m = s.error_map_hbd(hbd_cases.lift(ref), hbd_cases.lift(dist), 16)
        assert_bits(results(s, score), exp, (mode, w, h))
        gpu_cases.same_bits(m, m8, (mode, w, h, "257 u"))


# ---- 3. the against-reference map is the pair map, whichever call set the reference --------------------------------
def _reference_cases(w, h, k):
    """name -> (pair map call, set-reference call, against-reference map call, a later score call)."""
    rgb = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
    drgb = synth.distort(rgb, "blockq", 2, seed=k)
    d16 = hbd_cases.to_depth(drgb, 16, k)
    r10, d10 = hbd_cases.content16(w, h, 10, k), hbd_cases.content16(w, h, 10, k, distort=True)
    bg = 0x1A80E6
    _b1, r4 = laid_out(rgba_of(rgb, alpha_plane("disc", w, h, k)), 4 * w + 3, 1, seed=k)
    _b2, d4 = laid_out(rgba_of(drgb, alpha_plane("noise", w, h, k)), 4 * w + 12, 2, seed=k + 1)
    rp, dp = yuv_pair(w, h, 10, False, 1, k)
    rf, _rb = frame_of(rp, 10, False, 1, yuv_ref.YUV_444, k)
    df, _db = frame_of(dp, 10, False, 1, yuv_ref.YUV_444, k + 1)
    keep = (_b1, _b2, _rb, _db)
    return keep, {
        "set_reference, 16-bit frame": (lambda s: s.error_map_hbd(hbd_cases.lift(rgb), d16, 16), lambda s: s.set_reference(rgb),
                                        lambda s: s.error_map_against_reference_hbd(d16, 16),
                                        lambda s: s.score_against_reference_hbd(d16, 16)),
        "set_reference, YUV frame": (lambda s: s.error_map_hbd(hbd_cases.lift(rgb), s.convert_yuv(df, 16), 16),
                                     lambda s: s.set_reference(rgb), lambda s: s.error_map_against_reference_yuv(df, 16),
                                     lambda s: s.score_against_reference_yuv(df, 16)),
        "set_reference_hbd": (lambda s: s.error_map_hbd(r10, d10, 10), lambda s: s.set_reference_hbd(r10, 10),
                              lambda s: s.error_map_against_reference_hbd(d10, 10),
                              lambda s: s.score_against_reference_hbd(d10, 10)),
        "set_reference_rgba": (lambda s: s.error_map_rgba(r4, d4, bg), lambda s: s.set_reference_rgba(r4, bg),
                               lambda s: s.error_map_against_reference_rgba(d4), lambda s: s.score_against_reference_rgba(d4)),
        "set_reference_yuv": (lambda s: s.error_map_yuv(rf, df, 12), lambda s: s.set_reference_yuv(rf, 12),
                              lambda s: s.error_map_against_reference_yuv(df, 12),
                              lambda s: s.score_against_reference_yuv(df, 12)),
        "set_reference_yuv, 16-bit frame": (lambda s: s.error_map_hbd(s.convert_yuv(rf, 16), d16, 16),
                                            lambda s: s.set_reference_yuv(rf, 16),
                                            lambda s: s.error_map_against_reference_hbd(d16, 16),
                                            lambda s: s.score_against_reference_hbd(d16, 16)),
    }


@pytest.mark.parametrize("mode", MODES)
def test_against_reference_map_is_the_pair_map_for_every_kind_of_reference(mctxs, mode):
    s = mctxs[mode]
    for k, (w, h) in enumerate([(129, 67), (250, 130)]):
        _keep, cases = _reference_cases(w, h, k)
        for name, (pair, set_ref, against, later) in cases.items():
            what = (mode, w, h, name)
            pair_score, pair_map = pair(s)
            pair_res = results(s, pair_score)
            set_ref(s)
            before = results(s, later(s))
            for rep in range(2):                       # the second call finds the planes the first one made
                score, m = against(s)
                assert_bits(results(s, score), pair_res, what + (rep,))
                gpu_cases.same_bits(m, pair_map, what + (rep,))
            assert_bits(results(s, later(s)), before, what + ("the score after the map",))


# ---- 4. the YUV map is the rgb16 map of the converted codes --------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_yuv_map_is_the_rgb16_map_of_its_codes(mctxs, mode):
    s = mctxs[mode]
    k = 0
    for w, h in [(9, 17), (129, 67)]:
        for depth, full_range, mc, fmt in [(8, True, 6, yuv_ref.YUV_444), (10, False, 1, yuv_ref.YUV_444),
                                            (12, True, 9, yuv_ref.YUV_444), (8, False, 2, yuv_ref.YUV_400),
                                            (10, True, 5, yuv_ref.YUV_400)]:
            rp, dp = yuv_pair(w, h, depth, full_range, mc, k)
            rf, _rb = frame_of(rp, depth, full_range, mc, fmt, k)
            df, _db = frame_of(dp, depth, full_range, mc, fmt, k + 1)
            for rgb_depth in sorted({8, depth, 16}):
                what = (mode, w, h, depth, full_range, mc, fmt, rgb_depth)
                cr, cd = s.convert_yuv(rf, rgb_depth), s.convert_yuv(df, rgb_depth)
                exp_score, exp_map = s.error_map_hbd(cr, cd, rgb_depth)
                exp = results(s, exp_score)
                score, m = s.error_map_yuv(rf, df, rgb_depth)
                assert_bits(results(s, score), exp, what)
                gpu_cases.same_bits(m, exp_map, what)
                assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, rgb_depth)), exp, what + ("score call",))
            k += 1


# ---- 5. the RGBA map is the 16-bit pipeline's map of the composite codes -------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_opaque_rgba_map_is_the_8_bit_map(mctxs, mode):
    """An opaque frame's codes are 255 u, whose table entry is the 8-bit entry u: the map of the RGB frames, bit for bit."""
    s = mctxs[mode]
    for k, (w, h) in enumerate([(9, 17), (121, 9), (129, 67)]):
        rgb = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
        drgb = synth.distort(rgb, "blockq", 2, seed=k)
        score8, m8 = s.error_map(rgb, drgb)
        exp = results(s, score8)
        _br, r4 = laid_out(rgba_of(rgb, 255), 4 * w + 5, 1, seed=k)
        _bd, d4 = laid_out(rgba_of(drgb, 255), 4 * w + 12, 2, seed=k + 1)
        score, m = s.error_map_rgba(r4, d4, 0xE680FF)
        assert_bits(results(s, score), exp, (mode, w, h))
        gpu_cases.same_bits(m, m8, (mode, w, h, "opaque"))


@pytest.mark.parametrize("mode", MODES)
def test_rgba_map_matches_the_reference_through_the_composite_table(mctxs, oracle, mode):
    """Genuine alpha: codes n = a c + (255 - a) b (numpy's integers, which composite_rgba hands out) -> T[n] as scale-0
    linear planes, as tests/test_gpu_alpha.py relates the RGBA score to the 16-bit pipeline -> the numpy map."""
    s = mctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    table = scorer_mod.alpha_table()
    for k, (w, h, akind) in enumerate([(129, 67, "disc"), (250, 130, "noise"), (121, 9, "binary")]):
        bg = (0x000000, 0xFFFFFF, 0x1A80E6)[k]
        rgb = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
        alpha = alpha_plane(akind, w, h, k)
        ref = rgba_of(rgb, alpha)
        dalpha = np.clip(alpha.astype(np.int64) + np.random.default_rng(k + 9).integers(-3, 4, (h, w)), 0, 255)
        dist = rgba_of(synth.distort(rgb, "blockq", 2), dalpha.astype(np.uint8))
        _br, rv = laid_out(ref, 4 * w + 3, 3, seed=k)
        _bd, dv = laid_out(dist, 4 * w + 64, 1, seed=k + 1)
        what = f"{mode} {akind} alpha {w}x{h} over {bg:06X}"
        plain = results(s, s.compute_ssimu2_rgba(rv, dv, bg))
        score, m = s.error_map_rgba(rv, dv, bg)
        got = results(s, score)
        assert_bits(got, plain, what)
        cr, cd = s.composite_rgba(rv, bg), s.composite_rgba(dv, bg)
        assert np.array_equal(cr, codes_of(ref, bg)) and np.array_equal(cd, codes_of(dist, bg))
        lin_r, lin_d = (np.ascontiguousarray(table[c].transpose(2, 0, 1)) for c in (cr, cd))
        exp, ns = reference_map(oracle, lin_r, lin_d, blur, got[1])
        assert ns == got[2]
        hold_map(oracle, m, exp, blur, what)


# ---- 6. 8-bit and 16-bit maps of different sizes on one context ----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_interleaved_8_bit_and_16_bit_maps_equal_fresh_contexts(mctxs, mode):
    r8 = gpu_cases.content("text", 129, 67, seed=1)
    d8 = synth.distort(r8, "blockq", 3)
    r16, d16 = hbd_cases.content16(250, 130, 12, 2), hbd_cases.content16(250, 130, 12, 2, distort=True)
    small16, small16d = hbd_cases.content16(40, 41, 16, 3), hbd_cases.content16(40, 41, 16, 3, distort=True)
    ops = {"8-bit 129x67": lambda s: s.error_map(r8, d8), "12-bit 250x130": lambda s: s.error_map_hbd(r16, d16, 12),
           "16-bit 40x41": lambda s: s.error_map_hbd(small16, small16d, 16)}
    fresh = {}
    for name, op in ops.items():
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0], maps=True) as t:
            score, m = op(t)
            fresh[name] = (results(t, score), m)
    s = mctxs[mode]
    for i, name in enumerate(["8-bit 129x67", "12-bit 250x130", "8-bit 129x67", "16-bit 40x41", "12-bit 250x130",
                              "8-bit 129x67"]):
        score, m = ops[name](s)
        assert_bits(results(s, score), fresh[name][0], (mode, i, name))
        gpu_cases.same_bits(m, fresh[name][1], (mode, i, name))


# ---- 7. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_identical_calls_give_identical_bits(mctxs, mode):
    s = mctxs[mode]
    ref, dist = hbd_cases.content16(250, 130, 10, 7), hbd_cases.content16(250, 130, 10, 7, distort=True)
    score, m = s.error_map_hbd(ref, dist, 10)
    first = results(s, score)
    score2, m2 = s.error_map_hbd(ref, dist, 10)
    assert_bits(results(s, score2), first, mode)
    gpu_cases.same_bits(m2, m, mode)
    score3, m3 = s.error_map_hbd(ref, ref, 10)
    assert score3 == 100.0 and not m3.any()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(mctxs):
    s = mctxs["fir"]
    w, h = 40, 41
    ref, dist = hbd_cases.content16(w, h, 10, 1), hbd_cases.content16(w, h, 10, 1, distort=True)
    rp, dp = yuv_pair(w, h, 8, True, 6, 0)
    rf, df = scorer_mod.YuvFrame(rp, 8), scorer_mod.YuvFrame(dp, 8)
    for bits in (7, 17):
        for call in (lambda: s.error_map_hbd(ref, dist, bits), lambda: s.error_map_yuv(rf, df, bits)):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED, bits
    with Ssimu2(0, maps=True, extended=True, yuv=True) as t:          # no reference
        for call in (lambda: t.error_map_against_reference_hbd(dist, 10), lambda: t.error_map_against_reference_yuv(df),
                     lambda: t.error_map_against_reference_rgba(np.zeros((h, w, 4), np.uint8))):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_NO_REFERENCE
    s.set_reference_hbd(ref, 10)
    for bits in (7, 17):
        with pytest.raises(Ssimu2Error) as ei:
            s.error_map_against_reference_hbd(dist, bits)
        assert ei.value.code == _lib.ERR_UNSUPPORTED
        with pytest.raises(Ssimu2Error) as ei:
            s.error_map_against_reference_yuv(df, bits)
        assert ei.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):                                   # a size mismatch, caught by the Python side
        s.error_map_against_reference_hbd(hbd_cases.content16(w + 1, h, 10, 1), 10)
    with pytest.raises(ValueError):
        s.error_map_hbd(ref, hbd_cases.content16(w, h + 1, 10, 1), 10)
    with pytest.raises(Ssimu2Error) as ei:                            # a reference that recorded no background
        s.error_map_against_reference_rgba(np.zeros((h, w, 4), np.uint8))
    assert ei.value.code == _lib.ERR_INVALID_ARG and "background" in str(ei.value)
    # null map / score pointers: the C checks themselves
    L, p16 = s._L, scorer_mod._u16p
    m, out = np.empty((h, w), np.float32), ctypes.c_double()
    mp, op = scorer_mod._f32p(m), ctypes.byref(out)
    fr, fd = rf.as_c(), df.as_c()
    px4 = np.zeros((h, w, 4), np.uint8)
    for rc in (L.ssimu2_error_map_rgb16(s._ctx, p16(ref), p16(dist), w, h, 10, None, op),
               L.ssimu2_error_map_rgb16(s._ctx, p16(ref), p16(dist), w, h, 10, mp, None),
               L.ssimu2_error_map_rgb16(s._ctx, None, p16(dist), w, h, 10, mp, op),
               L.ssimu2_error_map_rgba8(s._ctx, scorer_mod._u8p(px4), 4 * w, scorer_mod._u8p(px4), 4 * w, w, h, 0, None, op),
               L.ssimu2_error_map_rgba8(s._ctx, scorer_mod._u8p(px4), 4 * w, scorer_mod._u8p(px4), 4 * w, w, h, 0, mp, None),
               L.ssimu2_error_map_yuv(s._ctx, ctypes.byref(fr), ctypes.byref(fd), w, h, 16, None, op),
               L.ssimu2_error_map_yuv(s._ctx, ctypes.byref(fr), ctypes.byref(fd), w, h, 16, mp, None)):
        assert rc == _lib.ERR_INVALID_ARG
    s.set_reference_hbd(ref, 10)
    for rc in (L.ssimu2_error_map_against_reference_rgb16(s._ctx, p16(dist), 10, None, op),
               L.ssimu2_error_map_against_reference_rgb16(s._ctx, p16(dist), 10, mp, None),
               L.ssimu2_error_map_against_reference_yuv(s._ctx, ctypes.byref(fd), 16, None, op),
               L.ssimu2_error_map_against_reference_yuv(s._ctx, ctypes.byref(fd), 16, mp, None),
               L.ssimu2_error_map_against_reference_rgba8(s._ctx, scorer_mod._u8p(px4), 4 * w, None, op)):
        assert rc == _lib.ERR_INVALID_ARG
    score, _m = s.error_map_against_reference_hbd(dist, 10)           # and the reference is still cached
    assert score == s.score_against_reference_hbd(dist, 10)
    # the 8-bit call keeps its refusal of a 16-bit reference in this library too
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(np.zeros((h, w, 3), np.uint8))
    assert ei.value.code == _lib.ERR_UNSUPPORTED


def test_a_service_context_refuses_the_map_calls_and_scores_on(hip_lib):
    from oavif_amd import service
    w, h = 40, 41
    ref, dist = hbd_cases.content16(w, h, 10, 1), hbd_cases.content16(w, h, 10, 1, distort=True)
    px4 = np.zeros((h, w, 4), np.uint8)
    rp, _dp = yuv_pair(w, h, 8, True, 6, 0)
    f = scorer_mod.YuvFrame(rp, 8)
    svc = service.start(max_lifetime=600)
    try:
        with Ssimu2(0, maps=True, extended=True, yuv=True, service=svc.socket) as remote:
            before = remote.compute_ssimu2_hbd(ref, dist, 10)
            remote.set_reference_hbd(ref, 10)
            for call in (lambda: remote.error_map_hbd(ref, dist, 10), lambda: remote.error_map_against_reference_hbd(dist, 10),
                         lambda: remote.error_map_rgba(px4, px4, 0), lambda: remote.error_map_against_reference_rgba(px4),
                         lambda: remote.error_map_yuv(f, f), lambda: remote.error_map_against_reference_yuv(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert remote.score_against_reference_hbd(dist, 10) == before
    finally:
        assert svc.stop(timeout=30) == 0
