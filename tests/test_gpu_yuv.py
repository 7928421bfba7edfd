"""YUV input on the MI355X (include/ssimu2_hip_yuv.h): the codes of k_yuv_to_codes against the numpy
restatement (tests/yuv_ref.py, itself held to libavif's built-in converter in tests/test_yuv_ref.py) bit for bit at
every depth, range, matrix, format and RGB depth, at the sizes, pitches and alignments where the kernel changes path;
bit identity of every YUV call with the 16-bit call on the restated codes in all three blur modes; the grey identity
with the 8-bit path; the checker; the search; the refusals; memory; the scoring service's refusal.

Nothing here reads libavif: the planes are numpy's."""
import numpy as np
import pytest

import gpu_cases
import hbd_ref
import yuv_ref
from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth, tq
from oavif_amd.scorer import YuvFrame

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
# 1 x 1 up: below four pixels (the tail path alone), exactly one group, groups plus a tail of 1, 2 and 3, more than one
# 256-lane block of groups (1027 = 4 * 256 + 3), and more rows than gridDim.y can hold (conversion only)
SIZES = [(1, 1), (3, 1), (4, 4), (5, 3), (7, 9), (8, 8), (9, 8), (17, 33), (129, 67), (1027, 5), (8, 65600)]
MATRIX_CODES = (1, 2, 5, 6, 9)

ctxs = gpu_cases.contexts_fixture(yuv=True)


def frame_of(planes, depth, full_range, mc, fmt=yuv_ref.YUV_444, k=0):
    """A YuvFrame of `planes` laid out as a decoder might: padded pitches (odd ones at depth 8), every plane with a pitch
    of its own, plane starts 1..3 bytes (depth 8) or 2 bytes (deeper) off alignment.  -> (frame, the buffers it views)."""
    size = planes[0].itemsize
    h, w = planes[0].shape
    bufs, views = [], []
    for p, plane in enumerate(planes[:1 if fmt == yuv_ref.YUV_400 else 3]):
        pad = ((0, 1, 3, 64, 5)[(k + p) % 5]) * size if size == 1 else ((0, 2, 6, 64, 10)[(k + p) % 5])
        off = 1 + (k + p) % 3 if size == 1 else 2
        buf, view = yuv_ref.laid_out(plane, w * size + pad, off, seed=10 * k + p)
        bufs.append(buf)
        views.append(view)
    f = YuvFrame(views, depth, fmt, full_range, mc)
    assert all(a.ctypes.data == v.ctypes.data for a, v in zip(f.planes, views))     # views went through as they are
    return f, bufs


def results(s, score):
    avg, ns = s.last_averages()
    return score, avg, ns


def assert_bits(got, exp, what):
    assert got[2] == exp[2], (what, got[2], exp[2])
    gpu_cases.bits_equal(got[0], got[1], exp[0], exp[1], what)


def same_codes(got, exp, what):
    assert got.dtype == np.uint16 and got.shape == exp.shape, what
    bad = got != exp
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- (a) the codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [yuv_ref.YUV_444, yuv_ref.YUV_400], ids=["444", "400"])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_range_matrix_and_rgb_depth(ctxs, depth, fmt):
    s = ctxs["fir"]
    k = 0
    for w, h in [(5, 3), (17, 33), (129, 67)]:
        for full_range in (True, False):
            for mc in MATRIX_CODES:
                planes = yuv_ref.random_planes(w, h, depth, seed=1000 * depth + k, extremes=(k % 3 == 2))
                f, _bufs = frame_of(planes, depth, full_range, mc, fmt, k)
                for rgb_depth in sorted({8, depth, 16}):
                    exp = yuv_ref.codes(*planes, depth, full_range, mc, rgb_depth, fmt)
                    same_codes(s.convert_yuv(f, rgb_depth), exp, (w, h, depth, full_range, mc, fmt, rgb_depth))
                k += 1


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_size_pitch_and_alignment(ctxs, depth):
    for k, (w, h) in enumerate(SIZES):
        s = ctxs[MODES[k % 3]]       # the kernel does not depend on the blur mode; every context has its own buffers
        planes = yuv_ref.random_planes(w, h, depth, seed=77 * depth + k, extremes=(k % 4 == 1))
        full_range, mc = bool(k & 1), MATRIX_CODES[k % 5]
        f, _bufs = frame_of(planes, depth, full_range, mc, k=k)
        same_codes(s.convert_yuv(f, 16), yuv_ref.codes(*planes, depth, full_range, mc, 16), (w, h, depth))
        tight = YuvFrame(planes, depth, yuv_ref.YUV_444, full_range, mc)             # tight rows, aligned starts
        same_codes(s.convert_yuv(tight, depth), yuv_ref.codes(*planes, depth, full_range, mc, depth), (w, h, depth, "tight"))


def test_every_sample_value_and_codes_above_the_depth(ctxs):
    s = ctxs["fir"]
    for depth in (8, 10, 12):
        n = 1 << depth
        side = 1 << (depth // 2)
        dtype = np.uint8 if depth == 8 else np.uint16
        y = np.arange(n, dtype=dtype).reshape(side, side)                 # every Y, over three chroma pairs
        for u, v in ((n // 2, n // 2), (0, n - 1), (n - 1, 3)):
            planes = [y, np.full_like(y, u), np.full_like(y, v)]
            for full_range in (True, False):
                same_codes(s.convert_yuv(YuvFrame(planes, depth, yuv_ref.YUV_444, full_range, 1), 16),
                           yuv_ref.codes(*planes, depth, full_range, 1, 16), (depth, u, v, full_range))
        planes = [np.ascontiguousarray(y.T), y, y[::-1].copy()]           # every U and V
        same_codes(s.convert_yuv(YuvFrame(planes, depth, yuv_ref.YUV_444, False, 9), 16),
                   yuv_ref.codes(*planes, depth, False, 9, 16), (depth, "chroma"))
    planes = yuv_ref.random_planes(9, 5, 10, seed=1)
    over = [p | np.uint16(0xFC00) for p in planes]
    same_codes(s.convert_yuv(YuvFrame(over, 10, yuv_ref.YUV_444, True, 1), 16),
               yuv_ref.codes(*[np.full_like(p, 1023) for p in planes], 10, True, 1, 16), "above the depth")


@pytest.mark.parametrize("mode", MODES)
def test_a_conversion_leaves_the_reference_and_the_averages(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 67
    ref = gpu_cases.content("text", w, h, seed=1)
    dist = synth.distort(ref, "blockq", 2)
    s.set_reference(ref)
    exp = results(s, s.score_against_reference(dist))
    planes = yuv_ref.random_planes(w, h, 10, seed=2)
    same_codes(s.convert_yuv(YuvFrame(planes, 10, yuv_ref.YUV_444, False, 1), 12), yuv_ref.codes(*planes, 10, False, 1, 12), mode)
    assert np.array_equal(s.last_averages()[0], exp[1])
    big = yuv_ref.random_planes(w + 40, h + 9, 8, seed=3)                 # another size: the staging buffer grows
    same_codes(s.convert_yuv(YuvFrame(big, 8, yuv_ref.YUV_444, True, 6), 16), yuv_ref.codes(*big, 8, True, 6, 16), mode)
    assert np.array_equal(s.last_averages()[0], exp[1])
    assert_bits(results(s, s.score_against_reference(dist)), exp, (mode, "reference still cached"))


# ---- (b) every YUV call is the 16-bit call on the restated codes ---------------------------------------------------
def yuv_pair(w, h, depth, full_range, mc, k):
    """A reference and a damaged frame as YUV planes of `depth`, and nothing else: ((ref planes), (dist planes))."""
    rgb = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
    dist = synth.distort(rgb, "blockq", 2) if w >= 8 and h >= 8 else gpu_cases.content("noise", w, h, seed=k + 50)
    return yuv_ref.forward(rgb, depth, full_range, mc), yuv_ref.forward(dist, depth, full_range, mc)


@pytest.mark.parametrize("mode", MODES)
def test_scores_equal_the_16bit_calls_on_the_restated_codes(ctxs, mode):
    s = ctxs[mode]
    k = 0
    for w, h in [(9, 8), (17, 33), (129, 67)]:
        for depth, full_range, mc, fmt in [(8, True, 6, yuv_ref.YUV_444), (10, False, 1, yuv_ref.YUV_444),
                                            (12, True, 9, yuv_ref.YUV_444), (8, False, 2, yuv_ref.YUV_400)]:
            rp, dp = yuv_pair(w, h, depth, full_range, mc, k)
            rf, _rb = frame_of(rp, depth, full_range, mc, fmt, k)
            df, _db = frame_of(dp, depth, full_range, mc, fmt, k + 1)
            for rgb_depth in sorted({depth, 16}):
                what = (mode, w, h, depth, full_range, mc, fmt, rgb_depth)
                cr = yuv_ref.codes(*rp, depth, full_range, mc, rgb_depth, fmt)
                cd = yuv_ref.codes(*dp, depth, full_range, mc, rgb_depth, fmt)
                exp = results(s, s.compute_ssimu2_hbd(cr, cd, rgb_depth))
                assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, rgb_depth)), exp, what + ("pair",))
                s.set_reference_hbd(cr, rgb_depth)
                exp_c = results(s, s.score_against_reference_hbd(cd, rgb_depth))
                assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth)), exp_c, what + ("16-bit reference",))
                s.set_reference_yuv(rf, rgb_depth)
                assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth)), exp_c, what + ("cached",))
                assert_bits(results(s, s.score_against_reference_hbd(cd, rgb_depth)), exp_c, what + ("YUV reference, 16-bit frame",))
            rgb8 = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)              # a reference set by the 8-bit call
            s.set_reference(rgb8)
            exp_8 = results(s, s.score_against_reference_hbd(cd, 16))
            assert_bits(results(s, s.score_against_reference_yuv(df, 16)), exp_8, (mode, w, h, depth, "8-bit reference"))
            k += 1


def test_frame_of_65600_rows_scores_as_the_16bit_calls_on_the_restated_codes(ctxs):
    """9 x 65,600 (FIR): k_yuv_to_codes' second row round (gridDim.y ends at 65,535) in front of the pair score and the
    cached score, which (8, 65600) of SIZES holds as codes only."""
    s = ctxs["fir"]
    w, h, depth, full_range, mc = 9, 65_600, 10, False, 1
    rp, dp = yuv_pair(w, h, depth, full_range, mc, 4)
    rf, _rb = frame_of(rp, depth, full_range, mc, yuv_ref.YUV_444, 4)
    df, _db = frame_of(dp, depth, full_range, mc, yuv_ref.YUV_444, 5)
    for rgb_depth in (depth, 16):
        what = (w, h, depth, rgb_depth)
        cr = yuv_ref.codes(*rp, depth, full_range, mc, rgb_depth)
        cd = yuv_ref.codes(*dp, depth, full_range, mc, rgb_depth)
        exp = results(s, s.compute_ssimu2_hbd(cr, cd, rgb_depth))
        assert 0.0 < exp[0] < 100.0 and exp[2] == 2, what
        s.set_reference_hbd(cr, rgb_depth)
        exp_c = results(s, s.score_against_reference_hbd(cd, rgb_depth))
        gpu_cases.stale(s, w, h, 2)
        assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, rgb_depth)), exp, what + ("pair",))
        s.set_reference_yuv(rf, rgb_depth)
        assert s.score_against_reference_yuv(rf, rgb_depth) == 100.0, what
        assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth)), exp_c, what + ("cached",))


@pytest.mark.parametrize("mode", MODES)
def test_grey_frames_score_as_their_rgb8_bit_for_bit(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate([(8, 8), (17, 33), (129, 67)]):
        grey_r = gpu_cases.content("gradient", w, h, seed=k)[..., 1]
        grey_d = synth.distort(np.repeat(grey_r[..., None], 3, -1), "noise", 2, seed=k)[..., 0]
        assert (grey_r != grey_d).any()
        rgb_r, rgb_d = (np.ascontiguousarray(np.repeat(g[..., None], 3, -1)) for g in (grey_r, grey_d))
        exp = results(s, s.compute_ssimu2(rgb_r, rgb_d))
        s.set_reference(rgb_r)
        exp_c = results(s, s.score_against_reference(rgb_d))
        mid = np.full_like(grey_r, 128)
        for mc in (1, 6, 9):
            rf, _rb = frame_of([grey_r, mid, mid], 8, True, mc, k=k)
            df, _db = frame_of([grey_d, mid, mid], 8, True, mc, k=k + 1)
            for rgb_depth in (8, 16):
                what = (mode, w, h, mc, rgb_depth)
                assert_bits(results(s, s.compute_ssimu2_yuv(rf, df, rgb_depth)), exp, what + ("pair",))
                s.set_reference_yuv(rf, rgb_depth)
                assert_bits(results(s, s.score_against_reference_yuv(df, rgb_depth)), exp_c, what + ("cached",))
        mono_r, mono_d = YuvFrame([grey_r], 8, yuv_ref.YUV_400, True, 2), YuvFrame([grey_d], 8, yuv_ref.YUV_400, True, 2)
        assert_bits(results(s, s.compute_ssimu2_yuv(mono_r, mono_d, 16)), exp, (mode, w, h, "4:0:0"))


# ---- (c) the checker -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scores_against_the_checker(ctxs, oracle, mode):
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    for k, (w, h) in enumerate([(17, 33), (129, 67)]):
        for depth, full_range, mc in [(8, True, 6), (10, False, 1)]:
            rp, dp = yuv_pair(w, h, depth, full_range, mc, k + 3)
            cr, cd = yuv_ref.codes(*rp, depth, full_range, mc, 16), yuv_ref.codes(*dp, depth, full_range, mc, 16)
            exp, avg_r, ns_r = hbd_ref.compute(oracle, cr, cd, 16, blur)
            rf, _rb = frame_of(rp, depth, full_range, mc, k=k)
            df, _db = frame_of(dp, depth, full_range, mc, k=k + 2)
            for name, got in (("pair", lambda: s.compute_ssimu2_yuv(rf, df, 16)),
                              ("cached", lambda: (s.set_reference_yuv(rf, 16), s.score_against_reference_yuv(df, 16))[1])):
                score, avg, ns = results(s, got())
                what = f"{mode} {w}x{h} depth {depth} {name}"
                print(f"measured: {what}: score {score!r}, checker {exp!r}, |d| {abs(score - exp):.2e}")
                assert ns == ns_r, what
                assert abs(score - exp) <= gpu_cases.score_tol(exp), (what, score, exp)
                assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), what


# ---- (d) the search ------------------------------------------------------------------------------------------------
class _Handed:
    """A decoded frame as search_hip_frames takes it, closed by the search."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.closed = False

    def close(self):
        self.closed = True


def test_search_over_yuv_frames_is_the_search_over_their_codes(ctxs):
    s = ctxs["fir"]
    w, h = 129, 67
    ref = synth.make_ref(w, h, seed=21)
    codec = gpu_cases.pseudo_codec(ref)
    handed = []

    def planes_of(q):
        dec, size = codec(q)
        return yuv_ref.forward(dec, 8, True, 6), size

    def codec_yuv(q):
        planes, size = planes_of(q)
        handed.append(_Handed(planes=planes, depth=8, format=yuv_ref.YUV_444, full_range=True, matrix_coefficients=6,
                              width=w, height=h))
        return handed[-1], size

    def codec_codes(q):
        planes, size = planes_of(q)
        c = yuv_ref.codes(*planes, 8, True, 6, 16)
        handed.append(_Handed(rows=c.reshape(h, w * 3), row_bytes=w * 6, channels=3, rgb_depth=16, width=w, height=h))
        return handed[-1], size

    how = dict(score_tgt=80.0, tolerance=2.0, max_pass=6)
    a = tq.search_hip_frames(s, ref, codec_yuv, **how)
    b = tq.search_hip_frames(s, ref, codec_codes, **how)
    assert a.num_pass == b.num_pass >= 1 and a.q == b.q and a.last_avif_size == b.last_avif_size
    assert [q for q, _ in a.history] == [q for q, _ in b.history]
    sa, sb = (np.array([sc for _q, sc in r.history] + [r.score]) for r in (a, b))
    assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)), (a.history, b.history)
    assert len(handed) == 2 * a.num_pass and all(f.closed for f in handed)


# ---- (e) refusals, memory, the service ------------------------------------------------------------------------------
def _c_frame(planes, **kw):
    """A frame of `planes` (full range, BT.601) and its C struct with the fields of `kw` overwritten."""
    f = YuvFrame(planes, 8 if planes[0].dtype == np.uint8 else 10, yuv_ref.YUV_444, True, 6)
    c = f.as_c()
    for name, v in kw.items():
        if name == "row_bytes":
            for p in range(3):
                c.row_bytes[p] = v
        elif name == "null_plane":
            c.planes[v] = None
        else:
            setattr(c, name, v)
    return f, c


def test_refusals_that_need_a_context(ctxs, scorer):
    import ctypes
    s = ctxs["fir"]
    L = s._L
    w, h = 16, 12
    planes = yuv_ref.random_planes(w, h, 8, seed=1)
    planes16 = yuv_ref.random_planes(w, h, 10, seed=1)
    out = np.empty((h, w, 3), np.uint16)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    score = ctypes.c_double()
    with Ssimu2(0, yuv=True) as t:
        with pytest.raises(Ssimu2Error) as ei:
            t.score_against_reference_yuv(YuvFrame(planes))
        assert ei.value.code == _lib.ERR_NO_REFERENCE
    rgb = gpu_cases.content("noise", w, h, seed=2)
    s.set_reference(rgb)
    kept = results(s, s.score_against_reference_yuv(YuvFrame(planes)))
    cases = [(dict(depth=9), _lib.ERR_UNSUPPORTED), (dict(depth=16), _lib.ERR_UNSUPPORTED),
             (dict(format=2), _lib.ERR_UNSUPPORTED), (dict(format=3), _lib.ERR_UNSUPPORTED), (dict(format=0), _lib.ERR_UNSUPPORTED),
             (dict(matrix_coefficients=0), _lib.ERR_UNSUPPORTED), (dict(matrix_coefficients=8), _lib.ERR_UNSUPPORTED),
             (dict(matrix_coefficients=7), _lib.ERR_UNSUPPORTED),
             (dict(full_range=2), _lib.ERR_INVALID_ARG), (dict(row_bytes=w - 1), _lib.ERR_INVALID_ARG),
             (dict(null_plane=0), _lib.ERR_INVALID_ARG), (dict(null_plane=2), _lib.ERR_INVALID_ARG)]
    for kw, code in cases:
        _f, c = _c_frame(planes, **kw)
        assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), w, h, 16, outp) == code, kw
        assert L.ssimu2_set_reference_yuv(s._ctx, ctypes.byref(c), w, h, 16) == code, kw
        assert L.ssimu2_score_against_reference_yuv(s._ctx, ctypes.byref(c), 16, ctypes.byref(score)) == code, kw
        assert L.ssimu2_score_yuv(s._ctx, ctypes.byref(c), ctypes.byref(c), w, h, 16, ctypes.byref(score)) == code, kw
    _f, c = _c_frame(planes)
    for rgb_depth in (7, 17, 0):
        assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), w, h, rgb_depth, outp) == _lib.ERR_UNSUPPORTED
        assert L.ssimu2_score_against_reference_yuv(s._ctx, ctypes.byref(c), rgb_depth, ctypes.byref(score)) == _lib.ERR_UNSUPPORTED
    assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), 0, h, 16, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), w, h, 16, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_convert_yuv(s._ctx, None, w, h, 16, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuv(s._ctx, ctypes.byref(c), 16, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuv(s._ctx, None, 16, ctypes.byref(score)) == _lib.ERR_INVALID_ARG
    # 16-bit samples: odd row_bytes, an odd pointer
    _f16, c16 = _c_frame(planes16, depth=10, row_bytes=2 * w + 1)
    assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c16), w, h, 16, outp) == _lib.ERR_INVALID_ARG
    _f16, c16 = _c_frame(planes16, depth=10)
    c16.planes[1] = c16.planes[1] + 1
    assert L.ssimu2_score_against_reference_yuv(s._ctx, ctypes.byref(c16), 16, ctypes.byref(score)) == _lib.ERR_INVALID_ARG
    # 4:0:0 does not look at planes 1 and 2
    _f, c = _c_frame(planes, format=yuv_ref.YUV_400, null_plane=1)
    c.planes[2], c.row_bytes[1], c.row_bytes[2] = None, 0, 0
    assert L.ssimu2_convert_yuv(s._ctx, ctypes.byref(c), w, h, 8, outp) == _lib.OK
    same_codes(out, yuv_ref.codes(*planes, 8, True, 6, 8, yuv_ref.YUV_400), "4:0:0 with null chroma")
    # after all of it the reference is the one that was set, and a frame of another size is refused before any C call
    assert_bits(results(s, s.score_against_reference_yuv(YuvFrame(planes))), kept, "reference usable after refusals")
    with pytest.raises(ValueError):
        s.score_against_reference_yuv(YuvFrame(yuv_ref.random_planes(w + 1, h, 8, seed=1)))
    with pytest.raises(TypeError):
        YuvFrame(planes, depth=10)
    with pytest.raises(TypeError):
        s.convert_yuv(planes)
    s.set_reference_yuv(YuvFrame(planes))
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(rgb)
    assert ei.value.code == _lib.ERR_UNSUPPORTED          # a YUV reference is a high-bit-depth reference
    # a context of the product library has none of it
    f = YuvFrame(planes)
    for call in (lambda: scorer.convert_yuv(f), lambda: scorer.compute_ssimu2_yuv(f, f),
                 lambda: scorer.set_reference_yuv(f), lambda: scorer.score_against_reference_yuv(f)):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "yuv=True" in str(ei.value)


def test_rgba_calls_work_on_a_yuv_context(hip_lib):
    """The YUV library has the RGBA calls: yuv=True with extended=True is one context for both."""
    rgba = np.random.default_rng(1).integers(0, 256, (12, 16, 4), dtype=np.uint8)
    with Ssimu2(0, yuv=True, extended=True) as s, Ssimu2(0, extended=True) as e:
        assert np.array_equal(s.composite_rgba(rgba, 0x1A80E6), e.composite_rgba(rgba, 0x1A80E6))
        assert s.compute_ssimu2_rgba(rgba, rgba, 0) == 100.0
        planes = yuv_ref.random_planes(16, 12, 8, seed=1)
        same_codes(s.convert_yuv(YuvFrame(planes), 16), yuv_ref.codes(*planes, 8, True, 6, 16), "after RGBA calls")


def test_a_context_without_yuv_calls_allocates_nothing_new(hip_lib):
    import torch
    w, h = 1920, 1080
    ref = synth.make_ref(w, h, seed=4)
    dist = synth.distort(ref, "blockq", 2)
    torch.cuda.synchronize()

    def work(s):
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)

    for yuv in (False, True):           # each library's code object is on the device before anything is measured
        with Ssimu2(0, yuv=yuv) as s:
            s.compute_ssimu2(ref[:16, :16].copy(), dist[:16, :16].copy())
    with Ssimu2(0) as s:
        work(s)
        work(s)
        free_plain = torch.cuda.mem_get_info(0)[0]
    with Ssimu2(0, yuv=True) as s:
        work(s)
        work(s)
        assert abs(torch.cuda.mem_get_info(0)[0] - free_plain) <= (8 << 20)
        before = torch.cuda.mem_get_info(0)[0]
        planes = yuv_ref.forward(dist, 8, True, 6)
        s.set_reference(ref)
        assert s.score_against_reference_yuv(YuvFrame(planes)) < 100.0
        assert torch.cuda.mem_get_info(0)[0] < before       # ... the first YUV call does


def test_a_service_context_refuses_yuv_and_scores_on(hip_lib):
    from oavif_amd import service
    w, h = 121, 41
    rgb = gpu_cases.content("text", w, h, seed=2)
    dist = synth.distort(rgb, "blockq", 2)
    f = YuvFrame(yuv_ref.forward(rgb, 8, True, 6))
    svc = service.start(max_lifetime=600)
    try:
        with Ssimu2(0, yuv=True, service=svc.socket) as remote:
            before = remote.compute_ssimu2(rgb, dist)
            for call in (lambda: remote.convert_yuv(f), lambda: remote.compute_ssimu2_yuv(f, f),
                         lambda: remote.set_reference_yuv(f), lambda: remote.score_against_reference_yuv(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert remote.compute_ssimu2(rgb, dist) == before
            remote.set_reference(rgb)
            assert remote.score_against_reference(rgb) == 100.0
    finally:
        assert svc.stop(timeout=30) == 0
