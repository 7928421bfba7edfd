"""Subsampled YUV input on the MI355X (include/ssimu2_hip_chroma.h): the codes of
k_yuv_chroma_to_codes against the numpy restatement (tests/chroma_ref.py, itself held to libavif's built-in converter in
tests/test_chroma_ref.py) bit for bit in both formats, both upsamplings and every depth, at the sizes, pitches and
alignments where the kernel changes path; bit identity of every new call with the 16-bit call on the restated codes in
all three blur modes, maps included; formats 4:4:4 and 4:0:0 through the new calls against the old calls; state,
refusals, memory and the scoring service's refusal; and one 4:2:0 file Pillow wrote, end to end against the checker.

Only the last test reads libavif: everywhere else the planes are numpy's."""
import ctypes
import io

import numpy as np
import pytest

import chroma_ref
import gpu_cases
import hbd_ref
import yuv_ref
from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth, tq
from oavif_amd.scorer import YuvFrame
from test_gpu_yuv import _Handed, assert_bits, results, same_codes, yuv_pair

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
FORMATS = [chroma_ref.YUV_422, chroma_ref.YUV_420]
IDS = ["422", "420"]
UPSAMPLINGS = (chroma_ref.BILINEAR, chroma_ref.NEAREST)
# A lane takes four luma columns and a workgroup 256 lanes: below four columns (the tail path alone), one group, groups
# plus a tail of 1, 2 and 3, both parities of the last row and column, one width just past one workgroup's 1024 columns
# and one past two workgroups' 2048
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 3), (4, 4), (5, 3), (7, 9), (8, 8), (9, 8), (17, 33), (129, 67), (1027, 5),
         (2051, 4)]
# ... and 8 columns of more rows than gridDim.y (65,535) holds, so that the row loop takes a second round: a 4:2:2 lane
# takes one luma row per round, a 4:2:0 lane the two luma rows of one chroma row, so twice the height
TALL = {chroma_ref.YUV_422: (8, 65_600), chroma_ref.YUV_420: (8, 131_080)}
MATRIX_CODES = (1, 2, 5, 6, 9)

ctxs = gpu_cases.contexts_fixture(chroma=True)


def frame_of(planes, depth, full_range, mc, fmt, k=0):
    """A YuvFrame of `planes` (each of its own size) laid out as a decoder might: a pitch of its own per plane, padded
    by 0, 1, 3, 64 or 5 samples (odd byte pitches at depth 8), plane starts 1..3 bytes (depth 8) or 2 bytes (deeper)
    off alignment, noise around every plane.  -> (frame, the buffers it views)."""
    size = planes[0].itemsize
    bufs, views = [], []
    for p, plane in enumerate(planes):
        pad = (0, 1, 3, 64, 5)[(k + p) % 5] * size if size == 1 else (0, 2, 6, 64, 10)[(k + p) % 5]
        off = 1 + (k + p) % 3 if size == 1 else 2
        buf, view = yuv_ref.laid_out(plane, plane.shape[1] * size + pad, off, seed=10 * k + p)
        bufs.append(buf)
        views.append(view)
    f = YuvFrame(views, depth, fmt, full_range, mc)
    assert all(a.ctypes.data == v.ctypes.data for a, v in zip(f.planes, views))     # views went through as they are
    return f, bufs


# ---- (a) the codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_size_pitch_and_alignment(ctxs, depth, fmt):
    # the tall frame at depths 8 and 10: one-byte and two-byte samples are the kernel's two forms, 12 is 10's
    for k, (w, h) in enumerate(SIZES + [TALL[fmt]] * (depth < 12)):
        s = ctxs[MODES[k % 3]]       # the kernel does not depend on the blur mode; every context has its own buffers
        planes = chroma_ref.random_planes(w, h, depth, fmt, seed=77 * depth + k, extremes=(k % 4 == 1))
        full_range, mc = bool(k & 1), MATRIX_CODES[k % 5]
        f, _bufs = frame_of(planes, depth, full_range, mc, fmt, k)
        tight = YuvFrame(planes, depth, fmt, full_range, mc)                          # tight rows, aligned starts
        for up in UPSAMPLINGS:
            same_codes(s.convert_yuv(f, 16, up), chroma_ref.codes(*planes, depth, full_range, mc, 16, fmt, up), (w, h, depth, up))
            if (w, h) != TALL[fmt]:
                same_codes(s.convert_yuv(tight, depth, up), chroma_ref.codes(*planes, depth, full_range, mc, depth, fmt, up),
                           (w, h, depth, up, "tight"))


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_range_matrix_and_rgb_depth(ctxs, depth, fmt):
    s = ctxs["fir"]
    w, h = 129, 67
    k = 0
    for full_range in (True, False):
        for mc in MATRIX_CODES:
            planes = chroma_ref.random_planes(w, h, depth, fmt, seed=1000 * depth + k, extremes=(k % 3 == 2))
            f, _bufs = frame_of(planes, depth, full_range, mc, fmt, k)
            for rgb_depth in sorted({8, depth, 16}):
                for up in UPSAMPLINGS:
                    exp = chroma_ref.codes(*planes, depth, full_range, mc, rgb_depth, fmt, up)
                    same_codes(s.convert_yuv(f, rgb_depth, up), exp, (depth, full_range, mc, fmt, rgb_depth, up))
            k += 1


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_every_chroma_sample_value_and_codes_above_the_depth(ctxs, fmt):
    s = ctxs["fir"]
    for depth in (8, 10, 12):
        n = 1 << depth
        side = 1 << (depth // 2)
        dtype = np.uint8 if depth == 8 else np.uint16
        u = np.arange(n, dtype=dtype).reshape(side, side)                 # every U and V, each beside and above others
        v = np.ascontiguousarray(u[::-1].T)
        w, h = 2 * side - 1, (2 * side - 1 if fmt == chroma_ref.YUV_420 else side)
        assert chroma_ref.chroma_shape(w, h, fmt) == (side, side)
        planes = [yuv_ref.random_planes(w, h, depth, seed=depth)[0], u, v]
        for full_range in (True, False):
            for up in UPSAMPLINGS:
                same_codes(s.convert_yuv(YuvFrame(planes, depth, fmt, full_range, 9), 16, up),
                           chroma_ref.codes(*planes, depth, full_range, 9, 16, fmt, up), (depth, full_range, up))
    planes = chroma_ref.random_planes(9, 5, 10, fmt, seed=1)
    over = [p | np.uint16(0xFC00) for p in planes]
    top = [np.full_like(p, 1023) for p in planes]
    for up in UPSAMPLINGS:
        exp = chroma_ref.codes(*top, 10, True, 1, 16, fmt, up)
        assert np.array_equal(exp, chroma_ref.codes(*over, 10, True, 1, 16, fmt, up))
        same_codes(s.convert_yuv(YuvFrame(over, 10, fmt, True, 1), 16, up), exp, ("above the depth", up))
        # 12-bit samples in a 10-bit frame: above m, below 2^12, each read as m
        some = [np.minimum(p | np.uint16(0x0400), 4095).astype(np.uint16) for p in planes]
        same_codes(s.convert_yuv(YuvFrame(some, 10, fmt, False, 6), 12, up),
                   chroma_ref.codes(*some, 10, False, 6, 12, fmt, up), ("some above the depth", up))


@pytest.mark.parametrize("mode", MODES)
def test_a_conversion_leaves_the_reference_and_the_averages(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 67
    ref = gpu_cases.content("text", w, h, seed=1)
    dist = synth.distort(ref, "blockq", 2)
    s.set_reference(ref)
    exp = results(s, s.score_against_reference(dist))
    for k, fmt in enumerate(FORMATS):
        big = chroma_ref.random_planes(w + 40, h + 9, 8, fmt, seed=3 + k)     # a larger frame first: the staging buffer
        same_codes(s.convert_yuv(YuvFrame(big, 8, fmt, True, 6), 16),         # then holds its bytes beyond the next one
                   chroma_ref.codes(*big, 8, True, 6, 16, fmt), (mode, fmt, "larger"))
        assert np.array_equal(s.last_averages()[0], exp[1])
        planes = chroma_ref.random_planes(w, h, 10, fmt, seed=2 + k)
        for up in UPSAMPLINGS:
            same_codes(s.convert_yuv(YuvFrame(planes, 10, fmt, False, 1), 12, up),
                       chroma_ref.codes(*planes, 10, False, 1, 12, fmt, up), (mode, fmt, up))
        assert np.array_equal(s.last_averages()[0], exp[1])
    assert_bits(results(s, s.score_against_reference(dist)), exp, (mode, "reference still cached"))


# ---- (b) every new call is the 16-bit call on the restated codes ---------------------------------------------------
def sub_pair(w, h, depth, full_range, mc, k, fmt_r, fmt_d):
    """yuv_pair's reference and damaged frame, each subsampled to its own format (4:4:4: left as it is)."""
    rp, dp = yuv_pair(w, h, depth, full_range, mc, k)
    sub = lambda planes, fmt: list(planes) if fmt == yuv_ref.YUV_444 else chroma_ref.subsample(planes, fmt)
    return sub(rp, fmt_r), sub(dp, fmt_d)


def same_map(got, exp, what):
    assert got.dtype == exp.dtype == np.float32 and got.shape == exp.shape, what
    bad = got.view(np.uint32) != exp.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def raw_set_reference_yuv(s, frame, rgb_depth):
    """ssimu2_set_reference_yuv itself (ssimu2_hip_yuv.h), which a chroma=True context's methods do not call."""
    c = frame.as_c()
    assert s._L.ssimu2_set_reference_yuv(s._ctx, ctypes.byref(c), frame.width, frame.height, rgb_depth) == _lib.OK
    s._ref_shape = (frame.height, frame.width, 3)


CONFIGS = [(8, True, 6, chroma_ref.YUV_420, chroma_ref.YUV_420), (10, False, 1, chroma_ref.YUV_422, chroma_ref.YUV_422),
           (12, True, 9, chroma_ref.YUV_420, chroma_ref.YUV_422), (8, False, 2, yuv_ref.YUV_444, chroma_ref.YUV_420)]


@pytest.mark.parametrize("mode", MODES)
def test_scores_equal_the_16bit_calls_on_the_restated_codes(ctxs, mode):
    s = ctxs[mode]
    k = 0
    for w, h in [(9, 8), (17, 33), (129, 67)]:
        for depth, full_range, mc, fmt_r, fmt_d in CONFIGS:
            rp, dp = sub_pair(w, h, depth, full_range, mc, k, fmt_r, fmt_d)
            rf, _rb = frame_of(rp, depth, full_range, mc, fmt_r, k)
            df, _db = frame_of(dp, depth, full_range, mc, fmt_d, k + 1)
            up = UPSAMPLINGS[k % 2]
            for rgb_depth in sorted({depth, 16}):
                what = (mode, w, h, depth, full_range, mc, fmt_r, fmt_d, rgb_depth, up)
                cr = chroma_ref.codes(*rp, depth, full_range, mc, rgb_depth, fmt_r, up)
                cd = chroma_ref.codes(*dp, depth, full_range, mc, rgb_depth, fmt_d, up)
                exp = results(s, s.compute_ssimu2_hbd(cr, cd, rgb_depth))
                assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, rgb_depth, up)), exp, what + ("pair",))
                s.set_reference_hbd(cr, rgb_depth)
                exp_c = results(s, s.score_against_reference_hbd(cd, rgb_depth))
                assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth, up)), exp_c, what + ("16-bit reference",))
                s.set_reference_yuv(rf, rgb_depth, up)
                assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth, up)), exp_c, what + ("cached",))
                assert_bits(results(s, s.score_against_reference_hbd(cd, rgb_depth)), exp_c, what + ("its reference, 16-bit frame",))
            rgb8 = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)              # a reference set by the 8-bit call
            s.set_reference(rgb8)
            exp_8 = results(s, s.score_against_reference_hbd(cd, 16))
            assert_bits(results(s, s.score_against_reference_yuv(df, 16, up)), exp_8, (mode, w, h, depth, "8-bit reference"))
            full = yuv_pair(w, h, depth, full_range, mc, k)[0]                          # ... and by the 4:4:4 YUV call
            s.set_reference_hbd(yuv_ref.codes(*full, depth, full_range, mc, 16), 16)
            exp_y = results(s, s.score_against_reference_hbd(cd, 16))
            raw_set_reference_yuv(s, YuvFrame(full, depth, yuv_ref.YUV_444, full_range, mc), 16)
            assert_bits(results(s, s.score_against_reference_yuv(df, 16, up)), exp_y, (mode, w, h, depth, "4:4:4 reference"))
            k += 1


@pytest.mark.parametrize("mode", MODES)
def test_maps_equal_the_16bit_maps_of_the_restated_codes(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate([(17, 33), (129, 67)]):
        depth, full_range, mc, fmt_r, fmt_d = CONFIGS[(k + 2) % 4]
        rp, dp = sub_pair(w, h, depth, full_range, mc, k + 7, fmt_r, fmt_d)
        rf, _rb = frame_of(rp, depth, full_range, mc, fmt_r, k)
        df, _db = frame_of(dp, depth, full_range, mc, fmt_d, k + 1)
        for up in UPSAMPLINGS:
            what = (mode, w, h, depth, up)
            cr = chroma_ref.codes(*rp, depth, full_range, mc, 16, fmt_r, up)
            cd = chroma_ref.codes(*dp, depth, full_range, mc, 16, fmt_d, up)
            score, m = s.error_map_hbd(cr, cd, 16)
            exp = results(s, score)
            got_score, got = s.error_map_yuv(rf, df, 16, up)
            assert_bits(results(s, got_score), exp, what + ("pair map",))
            same_map(got, m, what + ("pair map",))
            s.set_reference_hbd(cr, 16)
            score, m = s.error_map_against_reference_hbd(cd, 16)
            exp = results(s, score)
            s.set_reference_yuv(rf, 16, up)
            got_score, got = s.error_map_against_reference_yuv(df, 16, up)
            assert_bits(results(s, got_score), exp, what + ("map against the reference",))
            same_map(got, m, what + ("map against the reference",))


@pytest.mark.parametrize("mode", MODES)
def test_full_resolution_and_grey_frames_have_the_bits_of_the_old_calls(ctxs, mode):
    """Formats 4:4:4 and 4:0:0 through the new calls, whatever the upsampling, against the calls of ssimu2_hip_yuv.h and
    ssimu2_hip_map.h on a context of the map library."""
    s = ctxs[mode]
    w, h = 129, 67
    with Ssimu2(0, maps=True, yuv=True, blur=gpu_cases.MODES[mode][0]) as old:
        for k, (depth, fmt) in enumerate([(8, yuv_ref.YUV_444), (10, yuv_ref.YUV_400), (12, yuv_ref.YUV_444)]):
            rp, dp = yuv_pair(w, h, depth, bool(k & 1), MATRIX_CODES[k], k)
            keep = 1 if fmt == yuv_ref.YUV_400 else 3
            rf = YuvFrame(rp[:keep], depth, fmt, bool(k & 1), MATRIX_CODES[k])
            df = YuvFrame(dp[:keep], depth, fmt, bool(k & 1), MATRIX_CODES[k])
            exp_codes = old.convert_yuv(df, 16)
            score, exp_pair_map = old.error_map_yuv(rf, df, 16)
            exp = results(old, score)
            assert_bits(results(old, old.compute_ssimu2_yuv(rf, df, 16)), exp, (mode, depth, fmt, "the old calls agree"))
            old.set_reference_yuv(rf, 16)
            score, exp_map = old.error_map_against_reference_yuv(df, 16)
            exp_c = results(old, score)
            for up in UPSAMPLINGS:
                what = (mode, depth, fmt, up)
                same_codes(s.convert_yuv(df, 16, up), exp_codes, what)
                assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, 16, up)), exp, what + ("pair",))
                score, m = s.error_map_yuv(rf, df, 16, up)
                assert_bits(results(s, score), exp, what + ("pair map",))
                same_map(m, exp_pair_map, what + ("pair map",))
                s.set_reference_yuv(rf, 16, up)
                assert_bits(results(s, s.score_against_reference_yuv(df, 16, up)), exp_c, what + ("cached",))
                score, m = s.error_map_against_reference_yuv(df, 16, up)
                assert_bits(results(s, score), exp_c, what + ("map against the reference",))
                same_map(m, exp_map, what + ("map against the reference",))


def test_search_over_subsampled_frames_is_the_search_over_their_codes(ctxs):
    """tq.search_hip_frames hands a decoder's frame to score_against_reference_yuv as it is: 4:2:0 frames work unchanged."""
    s = ctxs["fir"]
    w, h = 129, 67
    ref = synth.make_ref(w, h, seed=21)
    codec = gpu_cases.pseudo_codec(ref)
    handed = []

    def planes_of(q):
        dec, size = codec(q)
        return chroma_ref.subsample(yuv_ref.forward(dec, 8, True, 6), chroma_ref.YUV_420), size

    def codec_yuv(q):
        planes, size = planes_of(q)
        handed.append(_Handed(planes=planes, depth=8, format=chroma_ref.YUV_420, full_range=True, matrix_coefficients=6,
                              width=w, height=h))
        return handed[-1], size

    def codec_codes(q):
        planes, size = planes_of(q)
        c = chroma_ref.codes(*planes, 8, True, 6, 16, chroma_ref.YUV_420)
        handed.append(_Handed(rows=c.reshape(h, w * 3), row_bytes=w * 6, channels=3, rgb_depth=16, width=w, height=h))
        return handed[-1], size

    how = dict(score_tgt=80.0, tolerance=2.0, max_pass=6)
    a = tq.search_hip_frames(s, ref, codec_yuv, **how)
    b = tq.search_hip_frames(s, ref, codec_codes, **how)
    assert a.num_pass == b.num_pass >= 1 and a.q == b.q and a.last_avif_size == b.last_avif_size
    sa, sb = (np.array([sc for _q, sc in r.history] + [r.score]) for r in (a, b))
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)), (a.history, b.history)
    assert len(handed) == 2 * a.num_pass and all(f.closed for f in handed)


# ---- (c) refusals, memory, the service ------------------------------------------------------------------------------
def _c_frame(planes, fmt, **kw):
    """A frame of `planes` (full range, BT.601) and its C struct with the fields of `kw` overwritten."""
    f = YuvFrame(planes, 8 if planes[0].dtype == np.uint8 else 10, fmt, True, 6)
    c = f.as_c()
    for name, v in kw.items():
        if name == "row_bytes":
            c.row_bytes[v[0]] = v[1]
        elif name == "null_plane":
            c.planes[v] = None
        else:
            setattr(c, name, v)
    return f, c


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_refusals_that_need_a_context(ctxs, fmt):
    s = ctxs["fir"]
    L = s._L
    w, h = 15, 12
    cw = 8
    planes = chroma_ref.random_planes(w, h, 8, fmt, seed=1)
    planes16 = chroma_ref.random_planes(w, h, 10, fmt, seed=1)
    out = np.empty((h, w, 3), np.uint16)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    m = np.empty((h, w), np.float32)
    mp = m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    score = ctypes.c_double()
    sc = ctypes.byref(score)
    with Ssimu2(0, chroma=True) as t:
        with pytest.raises(Ssimu2Error) as ei:
            t.score_against_reference_yuv(YuvFrame(planes, 8, fmt))
        assert ei.value.code == _lib.ERR_NO_REFERENCE
    rgb = gpu_cases.content("noise", w, h, seed=2)
    s.set_reference(rgb)
    kept = results(s, s.score_against_reference_yuv(YuvFrame(planes, 8, fmt)))

    def every_call(c, up=0):
        """The codes of all six calls for one frame."""
        fr = ctypes.byref(c)
        return {L.ssimu2_convert_yuv_chroma(s._ctx, fr, w, h, 16, up, outp),
                L.ssimu2_set_reference_yuv_chroma(s._ctx, fr, w, h, 16, up),
                L.ssimu2_score_against_reference_yuv_chroma(s._ctx, fr, 16, up, sc),
                L.ssimu2_score_yuv_chroma(s._ctx, fr, fr, w, h, 16, up, sc),
                L.ssimu2_error_map_yuv_chroma(s._ctx, fr, fr, w, h, 16, up, mp, sc),
                L.ssimu2_error_map_against_reference_yuv_chroma(s._ctx, fr, 16, up, mp, sc)}

    cases = [(dict(depth=9), _lib.ERR_UNSUPPORTED), (dict(depth=16), _lib.ERR_UNSUPPORTED),
             (dict(format=0), _lib.ERR_UNSUPPORTED), (dict(format=5), _lib.ERR_UNSUPPORTED),
             (dict(matrix_coefficients=0), _lib.ERR_UNSUPPORTED), (dict(matrix_coefficients=8), _lib.ERR_UNSUPPORTED),
             (dict(matrix_coefficients=7), _lib.ERR_UNSUPPORTED),
             (dict(full_range=2), _lib.ERR_INVALID_ARG), (dict(row_bytes=(0, w - 1)), _lib.ERR_INVALID_ARG),
             (dict(row_bytes=(1, cw - 1)), _lib.ERR_INVALID_ARG), (dict(row_bytes=(2, cw - 1)), _lib.ERR_INVALID_ARG),
             (dict(null_plane=0), _lib.ERR_INVALID_ARG), (dict(null_plane=1), _lib.ERR_INVALID_ARG),
             (dict(null_plane=2), _lib.ERR_INVALID_ARG)]
    for kw, code in cases:
        _f, c = _c_frame(planes, fmt, **kw)
        assert every_call(c) == {code}, kw
    _f, c = _c_frame(planes, fmt)
    for up in (2, 3, 0xFFFFFFFF):
        assert every_call(c, up) == {_lib.ERR_INVALID_ARG}, up
    fr = ctypes.byref(c)
    for rgb_depth in (7, 17, 0):
        assert L.ssimu2_convert_yuv_chroma(s._ctx, fr, w, h, rgb_depth, 0, outp) == _lib.ERR_UNSUPPORTED
        assert L.ssimu2_score_against_reference_yuv_chroma(s._ctx, fr, rgb_depth, 0, sc) == _lib.ERR_UNSUPPORTED
    assert L.ssimu2_convert_yuv_chroma(s._ctx, fr, 0, h, 16, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_convert_yuv_chroma(s._ctx, fr, w, 0, 16, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_convert_yuv_chroma(s._ctx, fr, w, h, 16, 0, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_convert_yuv_chroma(s._ctx, None, w, h, 16, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuv_chroma(s._ctx, fr, 16, 0, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuv_chroma(s._ctx, None, 16, 0, sc) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_error_map_against_reference_yuv_chroma(s._ctx, fr, 16, 0, None, sc) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_error_map_yuv_chroma(s._ctx, fr, fr, w, h, 16, 0, None, sc) == _lib.ERR_INVALID_ARG
    # chroma rows of exactly cw samples are enough, whatever the luma pitch
    _f, c = _c_frame(planes, fmt)
    assert (c.row_bytes[1], c.row_bytes[2]) == (cw, cw)
    assert L.ssimu2_convert_yuv_chroma(s._ctx, ctypes.byref(c), w, h, 16, 0, outp) == _lib.OK
    same_codes(out, chroma_ref.codes(*planes, 8, True, 6, 16, fmt), "tight chroma rows")
    # 16-bit samples: odd chroma row_bytes, an odd chroma pointer
    _f16, c16 = _c_frame(planes16, fmt, depth=10, row_bytes=(1, 2 * cw + 1))
    assert L.ssimu2_convert_yuv_chroma(s._ctx, ctypes.byref(c16), w, h, 16, 0, outp) == _lib.ERR_INVALID_ARG
    _f16, c16 = _c_frame(planes16, fmt, depth=10)
    c16.planes[2] = c16.planes[2] + 1
    assert L.ssimu2_score_against_reference_yuv_chroma(s._ctx, ctypes.byref(c16), 16, 1, sc) == _lib.ERR_INVALID_ARG
    # the calls of ssimu2_hip_yuv.h and ssimu2_hip_map.h in this library go on refusing the subsampled formats
    _f, c = _c_frame(planes, fmt)
    assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), w, h, 16, outp) == _lib.ERR_UNSUPPORTED
    assert L.ssimu2_error_map_against_reference_yuv(s._ctx, ctypes.byref(c), 16, mp, sc) == _lib.ERR_UNSUPPORTED
    # after all of it the reference is the one that was set, and a frame of another size is refused before any C call
    assert_bits(results(s, s.score_against_reference_yuv(YuvFrame(planes, 8, fmt))), kept, "reference usable after refusals")
    with pytest.raises(ValueError):
        s.score_against_reference_yuv(YuvFrame(chroma_ref.random_planes(w + 2, h, 8, fmt, seed=1), 8, fmt))
    with pytest.raises(ValueError):
        s.convert_yuv(YuvFrame(planes, 8, fmt), 16, "bicubic")
    s.set_reference_yuv(YuvFrame(planes, 8, fmt))
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(rgb)
    assert ei.value.code == _lib.ERR_UNSUPPORTED          # a reference set from subsampled YUV is a high-bit-depth reference
    assert s.score_against_reference_hbd(chroma_ref.codes(*planes, 8, True, 6, 16, fmt), 16) == 100.0


def test_contexts_of_the_other_libraries_refuse_subsampled_frames(hip_lib, scorer):
    planes = chroma_ref.random_planes(16, 12, 8, chroma_ref.YUV_420, seed=1)
    f = YuvFrame(planes, 8, chroma_ref.YUV_420)
    with Ssimu2(0, yuv=True, maps=True) as m:
        for s in (scorer, m):
            for call in (lambda: s.convert_yuv(f), lambda: s.compute_ssimu2_yuv(f, f), lambda: s.set_reference_yuv(f),
                         lambda: s.score_against_reference_yuv(f), lambda: s.error_map_yuv(f, f),
                         lambda: s.error_map_against_reference_yuv(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED and "chroma=True" in str(ei.value)
        full = yuv_ref.random_planes(16, 12, 8, seed=1)
        same_codes(m.convert_yuv(YuvFrame(full), 16, "nearest"), yuv_ref.codes(*full, 8, True, 6, 16), "4:4:4 as before")


def test_a_context_without_these_calls_allocates_nothing_new(hip_lib):
    import torch
    w, h = 1920, 1080
    ref = synth.make_ref(w, h, seed=4)
    dist = synth.distort(ref, "blockq", 2)
    torch.cuda.synchronize()

    def work(s):
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)

    for chroma in (False, True):        # each library's code object is on the device before anything is measured
        with Ssimu2(0, chroma=chroma) as s:
            s.compute_ssimu2(ref[:16, :16].copy(), dist[:16, :16].copy())
    with Ssimu2(0) as s:
        work(s)
        work(s)
        free_plain = torch.cuda.mem_get_info(0)[0]
    with Ssimu2(0, chroma=True) as s:
        work(s)
        work(s)
        assert abs(torch.cuda.mem_get_info(0)[0] - free_plain) <= (8 << 20)
        before = torch.cuda.mem_get_info(0)[0]
        planes = chroma_ref.subsample(yuv_ref.forward(dist, 8, True, 6), chroma_ref.YUV_420)
        s.set_reference(ref)
        assert s.score_against_reference_yuv(YuvFrame(planes, 8, chroma_ref.YUV_420)) < 100.0
        assert torch.cuda.mem_get_info(0)[0] < before       # ... the first such call does


def test_a_service_context_refuses_the_new_calls_and_scores_on(hip_lib):
    from oavif_amd import service
    w, h = 121, 41
    rgb = gpu_cases.content("text", w, h, seed=2)
    dist = synth.distort(rgb, "blockq", 2)
    f = YuvFrame(chroma_ref.subsample(yuv_ref.forward(rgb, 8, True, 6), chroma_ref.YUV_420), 8, chroma_ref.YUV_420)
    svc = service.start(max_lifetime=600)
    try:
        with Ssimu2(0, chroma=True, service=svc.socket) as remote:
            before = remote.compute_ssimu2(rgb, dist)
            for call in (lambda: remote.convert_yuv(f), lambda: remote.compute_ssimu2_yuv(f, f),
                         lambda: remote.set_reference_yuv(f), lambda: remote.score_against_reference_yuv(f),
                         lambda: remote.error_map_yuv(f, f), lambda: remote.error_map_against_reference_yuv(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert remote.compute_ssimu2(rgb, dist) == before
            remote.set_reference(rgb)
            assert remote.score_against_reference(rgb) == 100.0
    finally:
        assert svc.stop(timeout=30) == 0


# ---- (d) end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_a_420_file_scores_against_the_checker(ctxs, oracle, mode):
    """A 4:2:0 AVIF Pillow wrote -> decode_yuv -> score_against_reference_yuv against a reference set from the 8-bit
    source, within tests/test_gpu_yuv.py::test_scores_against_the_checker's 1e-4 of the checker on the samples
    decode_common(rgb_depth=16) makes of the same file."""
    from PIL import Image
    from oavif_amd import avif_bridge as ab
    if not ab.available():
        pytest.fail(f"libavif bridge unavailable: {ab.why_unavailable()}")
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    w, h = 131, 67
    src = synth.make_ref(w, h, seed=5)
    buf = io.BytesIO()
    Image.fromarray(src).save(buf, format="AVIF", subsampling="4:2:0", quality=60, speed=10)
    data = buf.getvalue()
    with ab.decode_common(data, rgb_depth=16) as g:
        cd = g.tight_rgb16()
    exp, avg_r, ns_r = hbd_ref.compute(oracle, src.astype(np.uint16) * 257, cd, 16, blur)
    s.set_reference(src)
    with ab.decode_yuv(data) as d:
        assert d.format == chroma_ref.YUV_420 and (d.width, d.height) == (w, h)
        f = YuvFrame(d.planes, d.depth, d.format, d.full_range, d.matrix_coefficients)
        same_codes(s.convert_yuv(f, 16), cd, (mode, "codes of the file"))
        score, avg, ns = results(s, s.score_against_reference_yuv(f, 16))
    print(f"measured: {mode} {w}x{h} 4:2:0 file: score {score!r}, checker {exp!r}, |d| {abs(score - exp):.2e}")
    assert ns == ns_r and 0.0 < score < 100.0
    assert abs(score - exp) <= gpu_cases.score_tol(exp), (mode, score, exp)
    assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), mode
