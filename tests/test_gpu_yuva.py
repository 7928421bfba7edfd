"""YUV frames with an alpha plane on the MI355X (include/ssimu2_hip_yuva.h): the composite codes
of k_yuva_to_codes against the numpy restatement (tests/yuva_ref.py, itself held to libavif's RGBA output in
tests/test_yuva_ref.py) bit for bit in every format, depth, upsampling and RGB depth, at the sizes, pitches and
alignments where the kernel changes path, for every alpha value at the extremes of colour and background, and past the
grid's rows; bit identity of every new call with the RGBA calls at depth 8 and rgb_depth 8 in all three blur modes, maps
included; deeper frames against the checker; the properties the header states; state, refusals, memory and the scoring
service's refusal; and the search of an RGBA source scored from the decoder's planes.

Only the last test reads libavif: everywhere else the planes are numpy's."""
import ctypes
import os

import numpy as np
import pytest

import chroma_ref
import gpu_cases
import yuv_ref
import yuva_ref
from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth
from oavif_amd.scorer import YuvFrame
from test_gpu_alpha import alpha_plane, expected, held_to_the_checker, table  # noqa: F401  (table: a fixture)
from test_gpu_chroma import same_map
from test_gpu_yuv import assert_bits, results, same_codes, yuv_pair

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
FORMATS = list(yuva_ref.FORMATS.values())
IDS = list(yuva_ref.FORMATS)
UPSAMPLINGS = (chroma_ref.BILINEAR, chroma_ref.NEAREST)
RGB_DEPTHS = (8, 10, 12, 16)
MATRIX_CODES = (1, 2, 5, 6, 9)
BACKGROUNDS = [0x000000, 0xFFFFFF, 0x1A80E6, int(np.random.default_rng(78).integers(0, 1 << 24))]
# A lane takes four luma columns and a workgroup 256 lanes: widths below four (the tail alone), one and two groups with
# every tail, and one block of 1,024 columns less one, exactly, plus one (a second block that is a tail alone) and plus
# three; heights with both parities of the last chroma row of a 4:2:0 frame, and a single row
WIDTHS = list(range(1, 10)) + [1023, 1024, 1025, 1027]
HEIGHTS = [1, 2, 3, 5]
# more rows than gridDim.y (65,535) holds: a 4:2:0 lane takes the two luma rows of one chroma row, so twice the height
TALL = {"444": (4, 65_600), "422": (4, 65_600), "420": (6, 131_100)}

ctxs = gpu_cases.contexts_fixture(yuva=True)


def frame_of(planes, alpha, depth, full_range, mc, fmt, k=0):
    """A YuvFrame of `planes` and `alpha` laid out as tests/test_gpu_chroma.py's frame_of lays planes out -- a pitch of
    its own per plane, padded by 0, 1, 3, 64 or 5 samples, starts 1..3 bytes (depth 8) or 2 bytes off alignment, noise
    around every plane -- the alpha plane included, as the plane behind the others.  -> (frame, the buffers it views)."""
    size = planes[0].itemsize
    bufs, views = [], []
    for p, plane in enumerate(list(planes) + ([alpha] if alpha is not None else [])):
        pad = (0, 1, 3, 64, 5)[(k + p) % 5] * size if size == 1 else (0, 2, 6, 64, 10)[(k + p) % 5]
        off = 1 + (k + p) % 3 if size == 1 else 2
        buf, view = yuv_ref.laid_out(plane, plane.shape[1] * size + pad, off, seed=10 * k + p)
        bufs.append(buf)
        views.append(view)
    a = views.pop() if alpha is not None else None
    f = YuvFrame(views, depth, fmt, full_range, mc, alpha=a)
    assert all(x.ctypes.data == v.ctypes.data for x, v in zip(f.planes, views))         # views went through as they are
    assert a is None or f.alpha.ctypes.data == a.ctypes.data
    return f, bufs


# ---- (a) the codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_codes_at_every_size_pitch_alignment_and_rgb_depth(ctxs, depth, fmt):
    k = 0
    for h in HEIGHTS:
        for w in WIDTHS:
            s = ctxs[MODES[k % 3]]       # the kernel does not depend on the blur mode; every context has its own buffers
            planes, alpha = yuva_ref.random_frame(w, h, depth, fmt, seed=91 * depth + k, extremes=(k % 4 == 1),
                                                  over=(depth > 8 and k % 3 == 0))
            if k % 5 == 4:
                alpha = None             # a null alpha plane: opaque
            full_range, mc, bg = bool(k & 1), MATRIX_CODES[k % 5], BACKGROUNDS[k % 4]
            f, _bufs = frame_of(planes, alpha, depth, full_range, mc, fmt, k)
            # two RGB depths per frame, all four over any four consecutive frames; both upsamplings
            for rgb_depth in (RGB_DEPTHS[k % 4], RGB_DEPTHS[(k + 2) % 4]):
                for up in UPSAMPLINGS:
                    exp = yuva_ref.codes(planes, alpha, depth, full_range, mc, rgb_depth, fmt, bg, up)
                    same_codes(s.composite_yuva(f, bg, rgb_depth, up), exp, (w, h, depth, fmt, rgb_depth, up, alpha is None))
            k += 1


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_codes_at_every_range_matrix_and_rgb_depth(ctxs, fmt):
    s = ctxs["fir"]
    w, h = 131, 35
    k = 0
    for depth in (8, 10, 12):
        for full_range in (True, False):
            for mc in MATRIX_CODES:
                planes, alpha = yuva_ref.random_frame(w, h, depth, fmt, seed=1000 * depth + k, extremes=(k % 3 == 2),
                                                      over=(depth > 8 and k % 2 == 0))
                f, _bufs = frame_of(planes, alpha, depth, full_range, mc, fmt, k)
                tight = YuvFrame(planes, depth, fmt, full_range, mc, alpha=alpha)         # tight rows, aligned starts
                bg = BACKGROUNDS[k % 4]
                for rgb_depth in RGB_DEPTHS:
                    up = UPSAMPLINGS[(k + rgb_depth) % 2]
                    exp = yuva_ref.codes(planes, alpha, depth, full_range, mc, rgb_depth, fmt, bg, up)
                    same_codes(s.composite_yuva(f, bg, rgb_depth, up), exp, (depth, full_range, mc, fmt, rgb_depth, up))
                    same_codes(s.composite_yuva(tight, bg, rgb_depth, up), exp, (depth, full_range, mc, fmt, rgb_depth, up, "tight"))
                k += 1


def samples_for(depth, rgb_depth, target):
    """(y, u, v, channel) of a full-range BT.601 4:4:4 pixel whose colour code of that channel at rgb_depth is `target`:
    found by looking through the restated codes of a (y, v) grid, u at mid-range."""
    m = (1 << depth) - 1
    dtype = np.uint8 if depth == 8 else np.uint16
    Y, V = np.meshgrid(np.arange(m + 1, dtype=dtype), np.arange(0, m + 1, max(1, (m + 1) // 512), dtype=dtype))
    U = np.full_like(Y, 1 << (depth - 1))
    c = yuv_ref.codes(Y, U, V, depth, True, 6, rgb_depth)
    for ch in (0, 1):
        hit = np.argwhere(c[..., ch] == target)
        if len(hit):
            i, j = hit[0]
            return int(Y[i, j]), int(U[i, j]), int(V[i, j]), ch
    raise AssertionError(f"no sample gives code {target} at depth {depth} -> {rgb_depth}")


# (8, 8) is the form without a division; the others hold the division at every alpha value, at the ends of the colour
# range and of the background's, where num and the remainder reach their extremes
@pytest.mark.parametrize("depth,rgb_depth", [(8, 8), (8, 10), (8, 16), (10, 8), (10, 10), (12, 12), (12, 16)])
def test_every_alpha_value_at_the_extremes_of_colour_and_background(ctxs, depth, rgb_depth):
    s = ctxs["fir"]
    ma, mc = (1 << depth) - 1, (1 << rgb_depth) - 1
    dtype = np.uint8 if depth == 8 else np.uint16
    w, h = 9, ma + 1                                            # two whole lanes and a tail of one; row j has alpha j
    alpha = np.ascontiguousarray(np.broadcast_to(np.arange(h, dtype=dtype)[:, None], (h, w)))
    for target in (0, 1, mc // 2, mc - 1, mc):
        y, u, v, ch = samples_for(depth, rgb_depth, target)
        planes = [np.full((h, w), x, dtype) for x in (y, u, v)]
        assert (yuva_ref.colour_codes(planes, depth, True, 6, rgb_depth, yuv_ref.YUV_444)[..., ch] == target).all()
        f = YuvFrame(planes, depth, yuv_ref.YUV_444, True, 6, alpha=alpha)
        for b in (0, 1, 127, 254, 255):
            bg = b << 16 | b << 8 | b
            exp = yuva_ref.codes(planes, alpha, depth, True, 6, rgb_depth, yuv_ref.YUV_444, bg)
            assert exp[0, 0, ch] == 255 * b and exp[-1, 0, ch] == (2 * yuva_ref.TOP * target + mc) // (2 * mc)
            same_codes(s.composite_yuva(f, bg, rgb_depth), exp, (depth, rgb_depth, target, b))


@pytest.mark.parametrize("bg", [0x1A80E6, 0xFF0001], ids=["1A80E6", "FF0001"])
def test_every_alpha_colour_pair_at_depth_8_and_rgb_depth_8(ctxs, bg):
    """256 x 256, 4:0:0 full range (c = Y exactly): a = row, c = column -- all 2^16 pairs in each channel."""
    yy, xx = np.mgrid[0:256, 0:256]
    y, alpha = np.ascontiguousarray(xx.astype(np.uint8)), np.ascontiguousarray(yy.astype(np.uint8))
    c = yuva_ref.colour_codes([y], 8, True, 6, 8, yuv_ref.YUV_400)
    assert np.array_equal(c, np.repeat(xx[..., None], 3, -1))
    b = yuva_ref.background(bg).astype(np.int64)
    exp = (yy[..., None] * xx[..., None] + (255 - yy[..., None]) * b).astype(np.uint16)
    assert np.array_equal(yuva_ref.codes([y], alpha, 8, True, 6, 8, yuv_ref.YUV_400, bg), exp)
    f = YuvFrame([y], 8, yuv_ref.YUV_400, True, 6, alpha=alpha)
    for mode in MODES:
        same_codes(ctxs[mode].composite_yuva(f, bg, 8), exp, (mode, bg))


def test_all_three_forms_of_the_division_give_the_same_codes(ctxs, monkeypatch):
    """OAVIF_YUVA_DIVISION (the measurement's switch) forces umul64hi with one correction, or the plain 64-bit division,
    where the rule would take the other or none: the codes do not depend on it."""
    s = ctxs["fir"]
    for k, (depth, rgb_depth) in enumerate([(8, 8), (8, 16), (10, 10), (12, 16)]):
        fmt = FORMATS[k % 4]
        planes, alpha = yuva_ref.random_frame(131, 35, depth, fmt, seed=k, extremes=True)
        f = YuvFrame(planes, depth, fmt, False, 9, alpha=alpha)
        exp = yuva_ref.codes(planes, alpha, depth, False, 9, rgb_depth, fmt, BACKGROUNDS[k])
        for how in ("mulhi", "plain"):
            with monkeypatch.context() as m:
                m.setenv("OAVIF_YUVA_DIVISION", how)
                same_codes(s.composite_yuva(f, BACKGROUNDS[k], rgb_depth), exp, (depth, rgb_depth, how))
        assert "OAVIF_YUVA_DIVISION" not in os.environ
        same_codes(s.composite_yuva(f, BACKGROUNDS[k], rgb_depth), exp, (depth, rgb_depth, "the rule"))


@pytest.mark.parametrize("name", list(TALL))
def test_codes_past_the_grids_rows(ctxs, name):
    """gridDim.y ends at 65,535: the last rows are taken in the kernel's second round (r += gridDim.y).  4 x 65,600 for
    4:4:4 and 4:2:2; 6 x 131,100 for 4:2:0, whose 65,550 chroma rows exceed it.  The composite call only."""
    s = ctxs["fir"]
    fmt = yuva_ref.FORMATS[name]
    w, h = TALL[name]
    assert chroma_ref.chroma_shape(w, h, fmt)[0] > 65_535 if fmt != yuv_ref.YUV_444 else h > 65_535
    for k, (depth, rgb_depth) in enumerate([(8, 8), (10, 16)]):
        planes, alpha = yuva_ref.random_frame(w, h, depth, fmt, seed=5 + k)
        f, _bufs = frame_of(planes, alpha, depth, True, 6, fmt, k)
        exp = yuva_ref.codes(planes, alpha, depth, True, 6, rgb_depth, fmt, BACKGROUNDS[2])
        same_codes(s.composite_yuva(f, BACKGROUNDS[2], rgb_depth), exp, (name, depth, rgb_depth))


# ---- (b) scores and maps ---------------------------------------------------------------------------------------------
def alpha_of(w, h, depth, k):
    """test_gpu_alpha's alpha planes (a disc with a soft edge, noise, blocks of 0 and 255), rescaled to the depth."""
    a = alpha_plane(("disc", "noise", "binary")[k % 3], w, h, k).astype(np.uint32)
    if depth == 8:
        return a.astype(np.uint8)
    ma = (1 << depth) - 1
    return ((a * ma + 127) // 255).astype(np.uint16)


def sub_frames(w, h, depth, full_range, mc, k, fmt_r, fmt_d):
    """A reference and a damaged frame, each in its own format, with alpha planes that differ a little too."""
    rp, dp = yuv_pair(w, h, depth, full_range, mc, k)

    def sub(planes, fmt):
        if fmt == yuv_ref.YUV_400:
            return [planes[0]]
        return list(planes) if fmt == yuv_ref.YUV_444 else chroma_ref.subsample(planes, fmt)

    ar = alpha_of(w, h, depth, k)
    ad = ar.copy()
    ad[h // 3:h // 3 + 4, w // 4:w // 4 + 6] //= 2              # a dent in the distorted frame's alpha plane
    return sub(rp, fmt_r), ar, sub(dp, fmt_d), ad


SIZES = [(65, 21), (129, 41), (35, 27)]                         # two of the project's list; 35 x 27: odd x odd 4:2:0
CONFIGS_8 = [(True, 6, yuva_ref.FORMATS["420"], yuva_ref.FORMATS["420"]), (False, 1, yuva_ref.FORMATS["422"], yuva_ref.FORMATS["444"]),
             (True, 9, yuva_ref.FORMATS["444"], yuva_ref.FORMATS["400"])]


@pytest.mark.parametrize("mode", MODES)
def test_depth_8_at_rgb_depth_8_is_the_rgba_calls_bit_for_bit(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate(SIZES):
        full_range, mc, fmt_r, fmt_d = CONFIGS_8[(k + 1) % 3]           # (35, 27), the last: 4:2:0 both
        rp, ar, dp, ad = sub_frames(w, h, 8, full_range, mc, k, fmt_r, fmt_d)
        if k == 1:
            ar = None                                           # the reference has no alpha plane: opaque
        up, bg = UPSAMPLINGS[k % 2], BACKGROUNDS[(k + 2) % 4]
        rf, _rb = frame_of(rp, ar, 8, full_range, mc, fmt_r, k)
        df, _db = frame_of(dp, ad, 8, full_range, mc, fmt_d, k + 1)
        r4 = yuva_ref.rgba8(rp, ar, full_range, mc, fmt_r, up)
        d4 = yuva_ref.rgba8(dp, ad, full_range, mc, fmt_d, up)
        what = (mode, w, h, fmt_r, fmt_d, up)
        # the pair, and its map
        exp = results(s, s.compute_ssimu2_rgba(r4, d4, bg))
        assert exp[0] < 100.0
        assert_bits(results(s, s.compute_ssimu2_yuva(rf, df, bg, 8, up)), exp, what + ("pair",))
        score, exp_map = s.error_map_rgba(r4, d4, bg)
        assert_bits(results(s, score), exp, what + ("the RGBA map's score",))
        score, m = s.error_map_yuva_alpha(rf, df, bg, 8, up)
        assert_bits(results(s, score), exp, what + ("pair map",))
        same_map(m, exp_map, what + ("pair map",))
        # set / against, and the map against the reference: a reference of either kind, a probe of either kind
        s.set_reference_rgba(r4, bg)
        exp_c = results(s, s.score_against_reference_rgba(d4))
        score, exp_map_c = s.error_map_against_reference_rgba(d4)
        assert_bits(results(s, score), exp_c, what + ("the RGBA map's score against the reference",))
        assert_bits(results(s, s.score_against_reference_yuva(df, 8, up)), exp_c, what + ("RGBA reference, YUVA probe",))
        score, m = s.error_map_against_reference_yuva_alpha(df, 8, up)
        assert_bits(results(s, score), exp_c, what + ("RGBA reference, YUVA map",))
        same_map(m, exp_map_c, what + ("RGBA reference, YUVA map",))
        s.set_reference_yuva(rf, bg, 8, up)
        assert_bits(results(s, s.score_against_reference_yuva(df, 8, up)), exp_c, what + ("YUVA reference, YUVA probe",))
        assert_bits(results(s, s.score_against_reference_rgba(d4)), exp_c, what + ("YUVA reference, RGBA probe",))
        score, m = s.error_map_against_reference_yuva_alpha(df, 8, up)
        assert_bits(results(s, score), exp_c, what + ("YUVA reference, YUVA map",))
        same_map(m, exp_map_c, what + ("YUVA reference, YUVA map",))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [10, 12])
def test_deeper_frames_at_rgb_depth_16_are_held_to_the_checker(ctxs, oracle, table, mode, depth):
    """T[n] of the restated codes as linear planes -> the checker's route (tests/test_gpu_alpha.py's expected), with
    gpu_cases.TOL_SCORE, RTOL_AVG and ATOL_AVG, unchanged."""
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    for k, (w, h) in enumerate(SIZES):
        fmt = yuva_ref.FORMATS["420"] if (w, h) == (35, 27) else FORMATS[(k + depth // 12) % 3]
        full_range, mc = bool(k & 1), MATRIX_CODES[(k + depth) % 5]
        rp, ar, dp, ad = sub_frames(w, h, depth, full_range, mc, k, fmt, fmt)
        up, bg = UPSAMPLINGS[k % 2], BACKGROUNDS[(k + 1) % 4]
        rf, _rb = frame_of(rp, ar, depth, full_range, mc, fmt, k)
        df, _db = frame_of(dp, ad, depth, full_range, mc, fmt, k + 1)
        cr = yuva_ref.codes(rp, ar, depth, full_range, mc, 16, fmt, bg, up)
        cd = yuva_ref.codes(dp, ad, depth, full_range, mc, 16, fmt, bg, up)
        exp = expected(oracle, table, ("yuva", depth, w, h, k), cr, cd, blur)
        what = (mode, depth, w, h, fmt, up)
        pair = results(s, s.compute_ssimu2_yuva(rf, df, bg, 16, up))
        held_to_the_checker(oracle, s, mode, pair, exp, cr, cd, what + ("pair",))
        score, m = s.error_map_yuva_alpha(rf, df, bg, 16, up)                     # a pair call: before the reference is set
        assert_bits(results(s, score), pair, what + ("pair map's score",))
        s.set_reference_yuva(rf, bg, 16, up)
        cached = results(s, s.score_against_reference_yuva(df, 16, up))
        held_to_the_checker(oracle, s, mode, cached, exp, cr, cd, what + ("cached",))
        score, m_c = s.error_map_against_reference_yuva_alpha(df, 16, up)
        assert_bits(results(s, score), cached, what + ("cached map's score",))
        # the maps: those of the 16-bit calls' pipeline on the same linear values, which ssimu2_hip_map.h's tests hold
        assert m.shape == m_c.shape == (h, w) and np.isfinite(m).all() and np.isfinite(m_c).all()
        assert m.max() > 0.0 and m_c.max() > 0.0


# ---- (c) properties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_colour_under_full_transparency_does_not_move_the_result(ctxs, mode):
    s = ctxs[mode]
    w, h, bg = 129, 41, 0x1A80E6
    for k, (depth, rgb_depth, fmt) in enumerate([(8, 8, yuva_ref.FORMATS["420"]), (10, 16, yuva_ref.FORMATS["444"]),
                                                 (12, 12, yuva_ref.FORMATS["422"])]):
        rgb = synth.make_ref(w, h, seed=30 + k)
        planes_of = lambda img: (lambda p: list(p) if fmt == yuv_ref.YUV_444 else chroma_ref.subsample(p, fmt))(
            yuv_ref.forward(img, depth, True, 6))
        rp, dp = planes_of(rgb), planes_of(synth.distort(rgb, "noise", 2, seed=k))
        ar = alpha_of(w, h, depth, 2)                           # blocks of 0 and ma
        ad = ar.copy()
        rf, df = YuvFrame(rp, depth, fmt, alpha=ar), YuvFrame(dp, depth, fmt, alpha=ad)
        exp = results(s, s.compute_ssimu2_yuva(rf, df, bg, rgb_depth))
        assert exp[0] < 100.0
        # other colour where nobody sees it.  `inner`: the pixels whose whole 5 x 5 neighbourhood is hidden.  Luma changes
        # there; a chroma sample changes where the luma pixel at its top left is inner -- the bilinear blend carries it to
        # the luma pixels one before to two after that one, all of them hidden
        hidden = ad == 0
        inner = hidden.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inner &= np.roll(np.roll(hidden, dy, 0), dx, 1)
        inner[:3], inner[-3:], inner[:, :3], inner[:, -3:] = False, False, False, False     # no wrap-around
        assert inner.sum() > 50
        noise = yuva_ref.random_frame(w, h, depth, yuv_ref.YUV_444, seed=70 + k)[0]
        dq = [p.copy() for p in dp]
        dq[0][inner] = noise[0][inner]
        sy = 2 if fmt == chroma_ref.YUV_420 else 1
        sx = 2 if fmt in (chroma_ref.YUV_420, chroma_ref.YUV_422) else 1
        for p in (1, 2):
            at = inner[::sy, ::sx]
            assert at.shape == dq[p].shape and at.any()
            dq[p][at] = noise[p][::sy, ::sx][at]
            for cj, ci in np.argwhere(dq[p] != dp[p]):
                rows = slice(max(sy * cj - 1, 0), sy * cj + 3) if sy == 2 else slice(cj, cj + 1)
                cols = slice(max(sx * ci - 1, 0), sx * ci + 3) if sx == 2 else slice(ci, ci + 1)
                assert hidden[rows, cols].all(), (fmt, cj, ci)
        assert any(not np.array_equal(a, b) for a, b in zip(dq, dp))
        got = results(s, s.compute_ssimu2_yuva(rf, YuvFrame(dq, depth, fmt, alpha=ad), bg, rgb_depth))
        assert_bits(got, exp, (mode, depth, rgb_depth, fmt))


@pytest.mark.parametrize("mode", MODES)
def test_damage_to_the_alpha_plane_alone_lowers_the_score(ctxs, mode):
    s = ctxs[mode]
    w, h, bg = 129, 41, 0x1A1A1A
    for k, (depth, rgb_depth, fmt) in enumerate([(8, 8, yuva_ref.FORMATS["420"]), (10, 16, yuva_ref.FORMATS["444"])]):
        rp, ar, _dp, _ad = sub_frames(w, h, depth, True, 6, 0, fmt, fmt)     # k = 0: a gradient, none of it the background
        ar = alpha_of(w, h, depth, 0)
        rf = YuvFrame(rp, depth, fmt, alpha=ar)
        assert s.compute_ssimu2_yuva(rf, rf, bg, rgb_depth) == 100.0
        scores = []
        for shift in (1, 3):
            ad = (ar >> shift).astype(ar.dtype)
            scores.append(s.compute_ssimu2_yuva(rf, YuvFrame(rp, depth, fmt, alpha=ad), bg, rgb_depth))
        assert 100.0 > scores[0] > scores[1], (mode, depth, scores)


@pytest.mark.parametrize("mode", MODES)
def test_an_opaque_frame_at_rgb_depth_8_has_the_bits_of_the_yuv_calls(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 41
    for k, (depth, fmt) in enumerate([(8, yuva_ref.FORMATS["420"]), (10, yuva_ref.FORMATS["444"]), (12, yuva_ref.FORMATS["400"])]):
        rp, _ar, dp, _ad = sub_frames(w, h, depth, bool(k & 1), MATRIX_CODES[k], k, fmt, fmt)
        ma = (1 << depth) - 1
        full = np.full((h, w), ma, rp[0].dtype)
        rf, df = YuvFrame(rp, depth, fmt, bool(k & 1), MATRIX_CODES[k]), YuvFrame(dp, depth, fmt, bool(k & 1), MATRIX_CODES[k])
        ra = YuvFrame(rp, depth, fmt, bool(k & 1), MATRIX_CODES[k], alpha=full)
        da = YuvFrame(dp, depth, fmt, bool(k & 1), MATRIX_CODES[k], alpha=full)
        for up in UPSAMPLINGS:
            exp = results(s, s.compute_ssimu2_yuv(rf, df, 8, up))
            for bg in (0x000000, 0xC0FFEE):
                assert_bits(results(s, s.compute_ssimu2_yuva(rf, df, bg, 8, up)), exp, (mode, depth, fmt, up, bg, "no alpha plane"))
                assert_bits(results(s, s.compute_ssimu2_yuva(ra, da, bg, 8, up)), exp, (mode, depth, fmt, up, bg, "a = ma"))
            s.set_reference_yuv(rf, 8, up)
            exp_c = results(s, s.score_against_reference_yuv(df, 8, up))
            s.set_reference_yuva(rf, 0x123456, 8, up)
            assert_bits(results(s, s.score_against_reference_yuva(da, 8, up)), exp_c, (mode, depth, fmt, up, "cached"))
            assert_bits(results(s, s.score_against_reference_yuv(df, 8, up)), exp_c, (mode, depth, fmt, up, "its reference, YUV probe"))


@pytest.mark.parametrize("mode", MODES)
def test_a_composite_leaves_the_reference_and_the_averages(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 67
    ref = gpu_cases.content("text", w, h, seed=1)
    dist = synth.distort(ref, "blockq", 2)
    s.set_reference(ref)
    exp = results(s, s.score_against_reference(dist))
    for k, fmt in enumerate(FORMATS):
        planes, alpha = yuva_ref.random_frame(w + 40, h + 9, 8, fmt, seed=3 + k)    # a larger frame first: the staging
        same_codes(s.composite_yuva(YuvFrame(planes, 8, fmt, alpha=alpha), 0x808080, 16),     # buffer then holds its bytes
                   yuva_ref.codes(planes, alpha, 8, True, 6, 16, fmt, 0x808080), (mode, fmt, "larger"))
        assert np.array_equal(s.last_averages()[0], exp[1])
        planes, alpha = yuva_ref.random_frame(w, h, 10, fmt, seed=2 + k)
        for up in UPSAMPLINGS:
            same_codes(s.composite_yuva(YuvFrame(planes, 10, fmt, False, 1, alpha=alpha), 0x102030, 12, up),
                       yuva_ref.codes(planes, alpha, 10, False, 1, 12, fmt, 0x102030, up), (mode, fmt, up))
        assert np.array_equal(s.last_averages()[0], exp[1])
    assert_bits(results(s, s.score_against_reference(dist)), exp, (mode, "reference still cached"))


# ---- (d) refusals, memory, the service -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_refusals_that_need_a_context(ctxs, fmt):
    s = ctxs["fir"]
    L = s._L
    w, h = 15, 12
    cw = 8
    planes, alpha = yuva_ref.random_frame(w, h, 8, fmt, seed=1)
    planes16, alpha16 = yuva_ref.random_frame(w, h, 10, fmt, seed=1)
    out = np.empty((h, w, 3), np.uint16)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    m = np.empty((h, w), np.float32)
    mp = m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    score = ctypes.c_double()
    sc = ctypes.byref(score)
    frame = YuvFrame(planes, 8, fmt, alpha=alpha)
    with Ssimu2(0, yuva=True) as t:
        with pytest.raises(Ssimu2Error) as ei:
            t.score_against_reference_yuva(frame)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        with pytest.raises(Ssimu2Error) as ei:
            t.error_map_against_reference_yuva_alpha(frame)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
    rgb = gpu_cases.content("noise", w, h, seed=2)
    # a reference without a background: the against-reference calls are invalid, as ssimu2_score_against_reference_rgba8
    s.set_reference(rgb)
    c = frame.as_yuva_c()
    assert L.ssimu2_score_against_reference_yuva(s._ctx, ctypes.byref(c), 16, 0, sc) == _lib.ERR_INVALID_ARG
    assert "background" in L.ssimu2_last_error(s._ctx).decode()
    assert L.ssimu2_error_map_against_reference_yuva(s._ctx, ctypes.byref(c), 16, 0, mp, sc) == _lib.ERR_INVALID_ARG
    with pytest.raises(Ssimu2Error) as ei:
        s.score_against_reference_rgba(np.zeros((h, w, 4), np.uint8))
    assert ei.value.code == _lib.ERR_INVALID_ARG
    s.set_reference_yuv(YuvFrame(planes, 8, fmt), 16)
    assert L.ssimu2_score_against_reference_yuva(s._ctx, ctypes.byref(c), 16, 0, sc) == _lib.ERR_INVALID_ARG
    s.set_reference_rgba(np.concatenate([rgb, np.full((h, w, 1), 200, np.uint8)], -1), 0x336699)
    kept = results(s, s.score_against_reference_yuva(frame))

    def every_call(c, up=0, bg=0):
        """The codes of all six calls for one frame."""
        fr = ctypes.byref(c)
        return {L.ssimu2_composite_yuva(s._ctx, fr, w, h, 16, up, bg, outp),
                L.ssimu2_score_yuva(s._ctx, fr, fr, w, h, 16, up, bg, sc),            # a pair score drops the reference:
                L.ssimu2_error_map_yuva(s._ctx, fr, fr, w, h, 16, up, bg, mp, sc),    # the pair calls come first
                L.ssimu2_set_reference_yuva(s._ctx, fr, w, h, 16, up, bg),
                L.ssimu2_score_against_reference_yuva(s._ctx, fr, 16, up, sc),
                L.ssimu2_error_map_against_reference_yuva(s._ctx, fr, 16, up, mp, sc)}

    def c_frame(p=planes, a=alpha, of_depth=8, **kw):
        c = YuvFrame(p, of_depth, fmt, alpha=a).as_yuva_c()
        for name, v in kw.items():
            if name == "row_bytes":
                c.yuv.row_bytes[v[0]] = v[1]
            elif name == "null_plane":
                c.yuv.planes[v] = None
            elif name in ("alpha_row_bytes", "alpha_premultiplied", "alpha"):
                setattr(c, name, v)
            else:
                setattr(c.yuv, name, v)
        return c

    colour = fmt != yuv_ref.YUV_400
    sub = fmt in (chroma_ref.YUV_422, chroma_ref.YUV_420)
    cases = [(dict(depth=9), _lib.ERR_UNSUPPORTED), (dict(depth=16), _lib.ERR_UNSUPPORTED),
             (dict(format=0), _lib.ERR_UNSUPPORTED), (dict(format=5), _lib.ERR_UNSUPPORTED),
             (dict(matrix_coefficients=0), _lib.ERR_UNSUPPORTED), (dict(matrix_coefficients=8), _lib.ERR_UNSUPPORTED),
             (dict(full_range=2), _lib.ERR_INVALID_ARG), (dict(row_bytes=(0, w - 1)), _lib.ERR_INVALID_ARG),
             (dict(null_plane=0), _lib.ERR_INVALID_ARG),
             # the alpha plane's own
             (dict(alpha_row_bytes=w - 1), _lib.ERR_INVALID_ARG), (dict(alpha_row_bytes=0), _lib.ERR_INVALID_ARG),
             (dict(alpha_premultiplied=1), _lib.ERR_UNSUPPORTED), (dict(alpha_premultiplied=0xFFFFFFFF), _lib.ERR_UNSUPPORTED)]
    if colour:
        cases += [(dict(row_bytes=(1, (cw if sub else w) - 1)), _lib.ERR_INVALID_ARG),
                  (dict(row_bytes=(2, (cw if sub else w) - 1)), _lib.ERR_INVALID_ARG),
                  (dict(null_plane=1), _lib.ERR_INVALID_ARG), (dict(null_plane=2), _lib.ERR_INVALID_ARG)]
    for kw, code in cases:
        assert every_call(c_frame(**kw)) == {code}, kw
    # premultiplied is refused even without an alpha plane; a null plane's row_bytes is not looked at
    assert every_call(c_frame(a=None, alpha_premultiplied=1)) == {_lib.ERR_UNSUPPORTED}
    assert every_call(c_frame(a=None, alpha_row_bytes=0)) == {_lib.OK}
    s.set_reference_rgba(np.concatenate([rgb, np.full((h, w, 1), 200, np.uint8)], -1), 0x336699)     # set_reference_yuva replaced it
    c = c_frame()
    for up in (2, 3, 0xFFFFFFFF):
        assert every_call(c, up) == {_lib.ERR_INVALID_ARG}, up
    fr = ctypes.byref(c)
    for bg in (0x1000000, 0xFFFFFFFF):          # check_rgba's background rule, in the four calls that take one
        assert {L.ssimu2_composite_yuva(s._ctx, fr, w, h, 16, 0, bg, outp), L.ssimu2_set_reference_yuva(s._ctx, fr, w, h, 16, 0, bg),
                L.ssimu2_score_yuva(s._ctx, fr, fr, w, h, 16, 0, bg, sc),
                L.ssimu2_error_map_yuva(s._ctx, fr, fr, w, h, 16, 0, bg, mp, sc)} == {_lib.ERR_INVALID_ARG}, bg
    for rgb_depth in (7, 17, 0):
        assert L.ssimu2_composite_yuva(s._ctx, fr, w, h, rgb_depth, 0, 0, outp) == _lib.ERR_UNSUPPORTED
        assert L.ssimu2_score_against_reference_yuva(s._ctx, fr, rgb_depth, 0, sc) == _lib.ERR_UNSUPPORTED
    assert L.ssimu2_composite_yuva(s._ctx, fr, 0, h, 16, 0, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_composite_yuva(s._ctx, fr, w, 0, 16, 0, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_composite_yuva(s._ctx, fr, w, h, 16, 0, 0, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_composite_yuva(s._ctx, None, w, h, 16, 0, 0, outp) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_yuva(s._ctx, fr, fr, w, h, 16, 0, 0, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuva(s._ctx, fr, 16, 0, None) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_score_against_reference_yuva(s._ctx, None, 16, 0, sc) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_error_map_against_reference_yuva(s._ctx, fr, 16, 0, None, sc) == _lib.ERR_INVALID_ARG
    assert L.ssimu2_error_map_yuva(s._ctx, fr, fr, w, h, 16, 0, 0, None, sc) == _lib.ERR_INVALID_ARG
    # alpha rows of exactly w samples are enough
    c = c_frame()
    assert c.alpha_row_bytes == w
    assert L.ssimu2_composite_yuva(s._ctx, ctypes.byref(c), w, h, 16, 0, 0x336699, outp) == _lib.OK
    same_codes(out, yuva_ref.codes(planes, alpha, 8, True, 6, 16, fmt, 0x336699), "tight alpha rows")
    # 16-bit samples: odd alpha_row_bytes, an odd alpha pointer
    c16 = c_frame(planes16, alpha16, 10, alpha_row_bytes=2 * w + 1)
    assert every_call(c16) == {_lib.ERR_INVALID_ARG}
    c16 = c_frame(planes16, alpha16, 10)
    c16.alpha = c16.alpha + 1
    assert every_call(c16) == {_lib.ERR_INVALID_ARG}
    # the calls of ssimu2_hip_chroma.h in this library do not look at an alpha plane: they take the frame inside
    c = c_frame()
    assert L.ssimu2_convert_yuv_chroma(s._ctx, ctypes.byref(c.yuv), w, h, 16, 0, outp) == _lib.OK
    same_codes(out, yuva_ref.colour_codes(planes, 8, True, 6, 16, fmt), "the chroma call")
    # after all of it the reference is the one that was set, and a frame of another size is refused before any C call
    assert_bits(results(s, s.score_against_reference_yuva(frame)), kept, "reference usable after refusals")
    with pytest.raises(ValueError):
        s.score_against_reference_yuva(YuvFrame(yuva_ref.random_frame(w + 2, h, 8, fmt, seed=1)[0], 8, fmt))
    with pytest.raises(ValueError):
        s.composite_yuva(frame, 0, 16, "bicubic")
    s.set_reference_yuva(frame, 0x336699)
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(rgb)
    assert ei.value.code == _lib.ERR_UNSUPPORTED          # a reference set from these frames is a high-bit-depth reference
    assert s.score_against_reference_hbd(np.zeros((h, w, 3), np.uint16), 16) < 100.0


def test_contexts_of_the_other_libraries_refuse_the_new_calls(hip_lib, scorer):
    planes, alpha = yuva_ref.random_frame(16, 12, 8, chroma_ref.YUV_420, seed=1)
    f = YuvFrame(planes, 8, chroma_ref.YUV_420, alpha=alpha)
    with Ssimu2(0, chroma=True, extended=True) as c:
        for s in (scorer, c):
            for call in (lambda: s.composite_yuva(f, 0), lambda: s.compute_ssimu2_yuva(f, f, 0), lambda: s.set_reference_yuva(f, 0),
                         lambda: s.score_against_reference_yuva(f), lambda: s.error_map_yuva_alpha(f, f, 0),
                         lambda: s.error_map_against_reference_yuva_alpha(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED and "yuva=True" in str(ei.value)
            assert not any(hasattr(s._L, name) for name in _lib.YUVA_SYMBOLS)
        # ... and go on ignoring a frame's alpha plane
        same_codes(c.convert_yuv(f, 16), chroma_ref.codes(*planes, 8, True, 6, 16, chroma_ref.YUV_420), "the alpha plane is not looked at")


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

    for yuva in (False, True):        # each library's code object is on the device before anything is measured
        with Ssimu2(0, yuva=yuva) as s:
            s.compute_ssimu2(ref[:16, :16].copy(), dist[:16, :16].copy())
    with Ssimu2(0) as s:
        work(s)
        work(s)
        free_plain = torch.cuda.mem_get_info(0)[0]
    with Ssimu2(0, yuva=True) as s:
        work(s)
        work(s)
        assert abs(torch.cuda.mem_get_info(0)[0] - free_plain) <= (8 << 20)
        before = torch.cuda.mem_get_info(0)[0]
        planes = chroma_ref.subsample(yuv_ref.forward(dist, 8, True, 6), chroma_ref.YUV_420)
        opaque = np.full((h, w, 1), 255, np.uint8)
        s.set_reference_rgba(np.concatenate([ref, opaque], -1), 0)
        assert s.score_against_reference_rgba(np.concatenate([dist, opaque], -1)) < 100.0
        after_rgba = torch.cuda.mem_get_info(0)[0]
        assert after_rgba < before       # ... the first RGBA calls do, and the first of the new calls nothing more:
        alpha = np.full((h, w), 200, np.uint8)      # the staged planes are smaller than RGBA rows, the rest is shared
        assert s.score_against_reference_yuva(YuvFrame(planes, 8, chroma_ref.YUV_420, alpha=alpha), 8) < 100.0
        assert abs(torch.cuda.mem_get_info(0)[0] - after_rgba) <= (8 << 20)


def test_a_service_context_refuses_the_new_calls_and_scores_on(hip_lib):
    from oavif_amd import service
    w, h = 121, 41
    rgb = gpu_cases.content("text", w, h, seed=2)
    dist = synth.distort(rgb, "blockq", 2)
    planes = chroma_ref.subsample(yuv_ref.forward(rgb, 8, True, 6), chroma_ref.YUV_420)
    f = YuvFrame(planes, 8, chroma_ref.YUV_420, alpha=alpha_of(w, h, 8, 0))
    svc = service.start(max_lifetime=600)
    try:
        with Ssimu2(0, yuva=True, service=svc.socket) as remote:
            before = remote.compute_ssimu2(rgb, dist)
            for call in (lambda: remote.composite_yuva(f, 0), lambda: remote.compute_ssimu2_yuva(f, f, 0),
                         lambda: remote.set_reference_yuva(f, 0), lambda: remote.score_against_reference_yuva(f),
                         lambda: remote.error_map_yuva_alpha(f, f, 0), lambda: remote.error_map_against_reference_yuva_alpha(f)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert remote.compute_ssimu2(rgb, dist) == before
            remote.set_reference(rgb)
            assert remote.score_against_reference(rgb) == 100.0
    finally:
        assert svc.stop(timeout=30) == 0


# ---- (e) the search --------------------------------------------------------------------------------------------------
def test_search_of_an_rgba_source_scored_from_the_decoders_planes(ctxs, monkeypatch):
    """alpha.search_rgba(..., score_yuv=True) on a 4:4:4, 8-bit encode: every probe's bytes are recorded; its score is the
    RGBA score of the frame restated from its planes (yuva_ref.rgba8), bit for bit, and the chosen quantizer the one the
    search over those scores gives.  avifImageYUVToRGB is not called."""
    from oavif_amd import alpha, avif_bridge as ab, cli, tq
    if not ab.available():
        pytest.fail(f"libavif bridge unavailable: {ab.why_unavailable()}")
    s = ctxs["fir"]
    w, h, bg = 160, 96, 0xE6E6E6
    rgb = synth.make_ref(w, h, seed=21)
    a = alpha_plane("disc", w, h, 0)
    src = np.concatenate([rgb, a[..., None]], -1)
    src[a == 0, :3] = np.random.default_rng(3).integers(0, 256, (int((a == 0).sum()), 3))   # noise nobody sees
    src = np.ascontiguousarray(src)
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.quality_alpha = False, 10, 90
    probes = []
    real_encode = ab.EncoderSource.encode

    def recording(self, options, q):
        data = real_encode(self, options, q)
        probes.append((int(q), data))
        return data

    def forbidden(*args):
        raise AssertionError("avifImageYUVToRGB ran on the host")

    monkeypatch.setattr(ab.EncoderSource, "encode", recording)
    monkeypatch.setattr(ab._lib(), "avifImageYUVToRGB", forbidden)
    how = dict(score_tgt=80.0, tolerance=2.0, max_pass=6)
    r = alpha.search_rgba(src, o, bg, scorer=s, score_yuv=True, **how)
    assert 1 <= r.num_pass == len(r.history) == len(probes) <= 6 and r.last_avif_size == len(probes[-1][1])
    by_q = {}
    for (q, data), (hq, score) in zip(probes, r.history):
        assert q == hq
        with ab.decode_yuv(data) as d:
            assert (d.format, d.depth, d.has_alpha) == (yuv_ref.YUV_444, 8, True)
            restated = yuva_ref.rgba8(d.planes, d.alpha, d.full_range, d.matrix_coefficients, d.format)
        exp = s.compute_ssimu2_rgba(src, restated, bg)
        assert np.float64(score).view(np.uint64) == np.float64(exp).view(np.uint64), (q, score, exp)
        by_q[q] = exp
    replay = tq.find_target_quality(lambda q: by_q[int(q)], **how)
    assert (replay.q, replay.num_pass, replay.history) == (r.q, r.num_pass, r.history)
    assert np.float64(replay.score).view(np.uint64) == np.float64(r.score).view(np.uint64)
