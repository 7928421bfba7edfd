"""The 16-bit front end on the MI355X, plane by plane (-m gpu only).

tests/test_gpu_hbd.py holds 16-bit scores to the checker; here the instrumented build's planes are held to it bit for
bit, as tests/test_gpu_parity.py and tests/test_gpu_recursive.py hold the 8-bit path's: every code of every depth
8..16 through the sRGB tables (the scale-0 linear planes of k_pyramid_bands16, the cached XYB planes, the recursive
planes), the size grid of gpu_cases.SIZES in tight RGB and padded RGBA rows, and the fp64 stage bounds of
tests/fp64_checks.py.  Then the scores of mixed depths for value, the 64-bit offsets of the 16-bit path (the ABI's
size limit, recursive planes past 4 GiB, source rows past 4 GiB) and frames of up to 100,000 rows through both strided
hand-offs."""
import numpy as np
import pytest

import fp64_checks as fc
import gpu_cases
import hbd_ref
import ssimu2_fp64 as R
from gpu_cases import check_rg, ictx, same_bits, scrub  # noqa: F401  (ictx: a fixture)
from hbd_cases import content16, lift, rows16
from oavif_amd import Ssimu2, Ssimu2Error, _lib, synth

pytestmark = pytest.mark.gpu

LIN_REF, LIN_DIST, XYB_REF, REF_BLUR, RG_H, RG_V = 0, 1, 2, 3, 4, 5
RECURSIVE = [m for m in gpu_cases.MODES if m != "fir"]
DEPTHS = list(range(8, 17))


ictxs = gpu_cases.contexts_fixture(instrumented=True)
ctxs = gpu_cases.contexts_fixture()


# ---- the ssimu2_debug_download hook at scale 0 --------------------------------------------------------------------

def test_scale0_planes_are_downloadable_only_while_they_are_the_last_scores(ictx):
    s = ictx["fir"]
    w, h = 40, 24
    ref, dist = content16(w, h, 12, 1), content16(w, h, 12, 2, distort=True)

    def refused(what, ww=w, hh=h):
        with pytest.raises(Ssimu2Error) as ei:
            s.debug_download(what, 0, ww, hh)
        assert ei.value.code == _lib.ERR_INVALID_ARG, what

    s.compute_ssimu2_hbd(ref, dist, 12)
    same_bits(s.debug_download(LIN_REF, 0, w, h), hbd_ref.linear_planes(ref, 12), "pair ref")
    same_bits(s.debug_download(LIN_DIST, 0, w, h), hbd_ref.linear_planes(dist, 12), "pair dist")
    refused(LIN_REF, w + 2, h)                      # planes of another frame size
    refused(LIN_DIST, w, h - 1)
    u8 = synth.make_ref(w, h, 3)
    s.compute_ssimu2(u8, u8)                        # an 8-bit score is newer than them
    refused(LIN_REF)
    refused(LIN_DIST)
    s.set_reference_hbd(ref, 12)                    # a 16-bit reference: its planes, no frame's yet
    same_bits(s.debug_download(LIN_REF, 0, w, h), hbd_ref.linear_planes(ref, 12), "reference")
    refused(LIN_DIST)
    s.score_against_reference_hbd(dist, 10)
    same_bits(s.debug_download(LIN_REF, 0, w, h), hbd_ref.linear_planes(ref, 12), "cached ref")
    same_bits(s.debug_download(LIN_DIST, 0, w, h), hbd_ref.linear_planes(dist, 10), "cached dist")
    s.set_reference(u8)                             # an 8-bit reference has no scale-0 planes
    refused(LIN_REF)
    s.score_against_reference_hbd(dist, 16)
    refused(LIN_REF)
    same_bits(s.debug_download(LIN_DIST, 0, w, h), hbd_ref.linear_planes(dist, 16), "8-bit ref, 16-bit dist")
    r = ictx["recursive"]                          # the recursive modes write no linear planes
    r.compute_ssimu2_hbd(ref, dist, 12)
    with pytest.raises(Ssimu2Error) as ei:
        r.debug_download(LIN_DIST, 0, w, h)
    assert ei.value.code == _lib.ERR_INVALID_ARG


# ---- every code of every depth --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def every_code():
    ref = hbd_ref.every_code_frame()
    return ref, np.ascontiguousarray(ref[::-1, :, [1, 2, 0]])   # each channel of the frame: every code, another order


@pytest.mark.parametrize("d", DEPTHS)
def test_every_code_of_every_depth_is_bit_identical(ictx, oracle, every_code, d):
    """Each channel of both frames holds all 65,536 codes: the scale-0 planes are table(d)[min(v, 2^d - 1)] -- every
    entry of the depth's table and the clamp of every code above it -- in the pair call and in a cached pass at this
    depth and at another one; the cached XYB planes of every scale are the checker's, and so are the planes after both
    recursive passes in both recursive modes."""
    ref, dist = every_code
    w = h = 256
    other = 8 + (d - 8 + 4) % 9
    lv_r, lv_d = hbd_ref.levels(oracle, ref, d), hbd_ref.levels(oracle, dist, d)
    assert len(lv_r) == 6
    s = ictx["fir"]
    s.compute_ssimu2_hbd(ref, dist, d)
    for sc in range(6):
        same_bits(s.debug_download(LIN_REF, sc, w, h), lv_r[sc][0], (d, "pair ref", sc))
        same_bits(s.debug_download(LIN_DIST, sc, w, h), lv_d[sc][0], (d, "pair dist", sc))
    s.set_reference_hbd(ref, d)
    for sc in range(6):
        same_bits(s.debug_download(XYB_REF, sc, w, h), lv_r[sc][1], (d, "xyb", sc))
    for dd in (d, other):
        s.score_against_reference_hbd(dist, dd)
        same_bits(s.debug_download(LIN_DIST, 0, w, h), hbd_ref.linear_planes(dist, dd), (d, "cached dist", dd))
    for mode in RECURSIVE:
        r, blur = ictx[mode], gpu_cases.MODES[mode][1]
        for sc in range(6):
            r.rg_stop_after_scale(sc)
            r.compute_ssimu2_hbd(ref, dist, d)
            check_rg(r, oracle, blur, sc, w, h, lv_r[sc][1], lv_d[sc][1], (d, mode))


# ---- plane-level parity on the size grid ----------------------------------------------------------------------------

GRID = [(w, h) for w, h in gpu_cases.SIZES if w >= 8 and h >= 8]


@pytest.mark.parametrize("k", range(len(GRID)))
def test_planes_on_the_size_grid_are_bit_identical(ictx, oracle, k):
    """Genuine d-bit content, d cycling through 9..16; even cases through the tight pair call, odd ones through the
    strided hand-off (RGBA rows with padding) against a cached 16-bit reference.  FIR: linear levels 0..5 of the
    frames, the cached XYB and blur(ref * ref) planes; recursive modes: the planes after both passes, every scale."""
    w, h = GRID[k]
    d = 9 + k % 8
    strided = k % 2 == 1
    ref, dist = content16(w, h, d, 3 * k), content16(w, h, d, 3 * k + 1, distort=True)
    lv_r, lv_d = hbd_ref.levels(oracle, ref, d), hbd_ref.levels(oracle, dist, d)
    ns = len(lv_r)
    buf, view = rows16(dist, 4, 6 + k, fill=0xFFFF)

    def score(s):
        if strided:
            s.set_reference_hbd(ref, d)
            s.score_decoded_against_reference_hbd(view, bit_depth=d)
        else:
            s.compute_ssimu2_hbd(ref, dist, d)

    what = (w, h, d, "strided" if strided else "pair")
    s = ictx["fir"]
    score(s)
    assert s.last_averages()[1] == ns, what
    for sc in range(ns):
        if not strided:
            same_bits(s.debug_download(LIN_REF, sc, w, h), lv_r[sc][0], what + ("lin ref", sc))
        same_bits(s.debug_download(LIN_DIST, sc, w, h), lv_d[sc][0], what + ("lin dist", sc))
    s.set_reference_hbd(ref, d)
    for sc in range(ns):
        x = lv_r[sc][1]
        same_bits(s.debug_download(XYB_REF, sc, w, h), x, what + ("xyb", sc))
        blur = s.debug_download(REF_BLUR, sc, w, h)
        for c in range(3):
            same_bits(blur[c], oracle.blur_product(x[c], x[c], oracle.BLUR_FIR), what + ("ref blur", sc, c))
    for mode in RECURSIVE:
        r, blur = ictx[mode], gpu_cases.MODES[mode][1]
        for sc in range(ns):
            r.rg_stop_after_scale(sc)
            score(r)
            check_rg(r, oracle, blur, sc, w, h, lv_r[sc][1], lv_d[sc][1], what + (mode,))


@pytest.mark.parametrize("w,h,d", [(121, 9, 10), (333, 217, 12), (1921, 1083, 16), (129, 41, 9)])
def test_planes_against_the_fp64_reference(ictx, w, h, d):
    """test_gpu_fp64_reference.py's plane test for 16-bit frames: linear levels 0..5 of both frames, cached XYB and
    blur(ref * ref) at every scale, the recursive planes of scale 0 after each pass, within fp64_checks' stage bounds
    of hbd_ref.reference_levels."""
    ref, dist = content16(w, h, d, w + d), content16(w, h, d, h + d, distort=True)
    ns = R.nscales_of(w, h)
    lv = hbd_ref.reference_levels(ref, dist, d, list(range(ns)))
    s = ictx["fir"]
    s.compute_ssimu2_hbd(ref, dist, d)
    for sc in range(ns):
        for what in (LIN_REF, LIN_DIST):
            assert fc.lin_ulps(s.debug_download(what, sc, w, h), lv[sc][what]) <= fc.PLANE_LIN_ULPS, (what, sc)
    s.set_reference_hbd(ref, d)
    for sc in range(ns):
        assert fc.abs_dev(s.debug_download(XYB_REF, sc, w, h), lv[sc][2]) <= fc.XYB_ABS, sc
        got = s.debug_download(REF_BLUR, sc, w, h)
        for c in range(3):
            assert fc.rel_dev(got[c], R.blur(lv[sc][2][c] ** 2)) <= fc.PLANE_FIR_REL, (sc, c)
    bound = fc.RG_REL0 + fc.IIR_REL_PER_SQRT_LINE * np.sqrt(w + h)
    r = ictx["recursive"]
    r.rg_stop_after_scale(0)
    r.compute_ssimu2_hbd(ref, dist, d)
    for what, vertical in ((RG_H, False), (RG_V, True)):
        got = r.debug_download(what, 0, w, h)
        exp = fc.rg_reference(lv[0][2], lv[0][3], vertical)
        for k in range(15):
            assert fc.rel_dev(got[k], exp[k]) <= bound, (what, k)


# ---- mixed depths, for value ----------------------------------------------------------------------------------------

MIX = [8, 9, 10, 12, 14, 16]
# the recursive modes: every depth on both sides, not every pair
MIX_PAIRS = {"fir": [(a, b) for a in MIX for b in MIX],
             "recursive": list(zip(MIX, MIX[1:] + MIX[:1])) + [(16, 16)],
             "recursive_fma": list(zip(MIX, MIX[2:] + MIX[:2])) + [(8, 8)]}


@pytest.mark.parametrize("mode", list(gpu_cases.MODES))
def test_mixed_depths_score_against_the_checker(ctxs, oracle, mode):
    """A distorted frame of depth dd against a cached reference of depth dr, tight and as strided RGBA rows (and, at
    dr = 8, against the same reference set from 8-bit samples): the checker's score and averages of the two depths
    (hbd_ref.compute(d_dist=...)) within the GPU tests' bounds, and the fp64 counterpart within fp64_checks'.  Each
    pass follows a score of other content, so none finds the planes it should write already in place."""
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    w, h = 123, 77
    assert w * h <= fc.IIR_MAX_PIXELS
    for dr, dd in MIX_PAIRS[mode]:
        ref = content16(w, h, dr, 7 * dr + dd)                    # the frame: the same base, distorted
        frame = content16(w, h, dd, 7 * dr + dd, distort=True)
        exp, avg_r, ns_r = hbd_ref.compute(oracle, ref, frame, dr, blur, d_dist=dd)
        exp64 = hbd_ref.compute_fp64(ref, frame, dr, d_dist=dd)
        buf, view = rows16(frame, 4, 10, fill=0xFFFF)
        setters = [lambda: s.set_reference_hbd(ref, dr)]
        if dr == 8:
            setters.append(lambda: s.set_reference(ref.astype(np.uint8)))
        for k, set_ref in enumerate(setters):
            set_ref()
            for how, call in (("tight", lambda: s.score_against_reference_hbd(frame, dd)),
                              ("strided", lambda: s.score_decoded_against_reference_hbd(view, bit_depth=dd))):
                what = (mode, dr, dd, k, how)
                assert scrub(s, ref, dr) != exp, what
                got = call()
                avg, ns = s.last_averages()
                assert ns == ns_r, what
                assert abs(got - exp) <= gpu_cases.score_tol(exp), what + (got, exp)
                assert np.allclose(avg, avg_r, rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), what
                fc.check(got, avg, ns, exp64, mode, what, "synthetic")


# ---- 64-bit offsets of the 16-bit path ------------------------------------------------------------------------------

FLIP_TOL = 2e-3   # tests/test_gpu_parity.py


def _flip(a):
    return np.ascontiguousarray(a[::-1, ::-1])


def test_maximum_size_16bit_far_corner(hip_lib):
    """test_maximum_size_far_corner_is_addressed_correctly's 26752 x 26752 pair lifted to 257 u: a tight RGB16 frame
    is 4.29 GB, its scale-0 planes 8.6 GB, the RGBA16 rows 5.7 GB, so third-plane and far-row offsets pass 2^32 bytes.
    The pair call, the cached pass and the strided RGBA pass give the 8-bit pair score bit for bit; the mirrored pair
    agrees to FLIP_TOL.  Host arrays are freed as they go (peak about 14.3 GB)."""
    n, t, reps = 26752, 2432, 11
    base = synth.make_ref(t, t, 97)
    with Ssimu2(0) as s:
        ref = np.tile(base, (reps, reps, 1))
        dist = np.tile(synth.distort(base, "blockq", 1), (reps, reps, 1))
        assert ref.shape == (n, n, 3)
        dist[-t:, -t:] = 255 - dist[-t:, -t:]
        s8 = s.compute_ssimu2(ref, dist)
        avg8 = s.last_averages()
        assert avg8[1] == 6 and s8 < 100.0
        r16 = lift(ref)
        del ref
        d16 = lift(dist)
        del dist

        def same(got, what):
            avg, ns = s.last_averages()
            assert got == s8 and ns == 6 and np.array_equal(avg, avg8[0]), (what, got, s8)

        same(s.compute_ssimu2_hbd(r16, d16, 16), "pair")
        s.set_reference_hbd(r16, 16)
        same(s.score_against_reference_hbd(d16, 16), "cached")
        buf, view = rows16(d16, 4, 8, fill=0xFFFF)
        assert buf.nbytes > 5 << 30
        same(s.score_decoded_against_reference_hbd(view, bit_depth=16), "strided rgba")
        del buf, view
        rf = _flip(r16)
        del r16
        df = _flip(d16)
        del d16
        assert abs(s.compute_ssimu2_hbd(rf, df, 16) - s8) < FLIP_TOL


def test_recursive_16bit_planes_of_a_large_frame_cross_4_gib(hip_lib, oracle):
    """test_recursive_planes_of_a_large_frame_cross_4_gib with the frames as 12-bit codes: 8192 x 5200, every plane
    base of the recursive modes past 2^32 bytes; the first, middle and last of the 15 planes of scale 0 against the
    recursion over hbd_ref's XYB planes, bit for bit."""
    w, h = 8192, 5200
    base = synth.make_ref(1024, 1300, 31)
    u = np.tile(base, (4, 8, 1))
    ref = (u.astype(np.uint16) << 4) | (u >> 4).astype(np.uint16)    # 12-bit codes, 0..4095
    del u
    dist = np.ascontiguousarray(ref[::-1, ::-1])
    assert ref.shape == (h, w, 3) and int(ref.max()) <= 4095
    with Ssimu2(0, instrumented=True, blur=_lib.BLUR_RECURSIVE) as s:
        s.rg_stop_after_scale(0)
        s.compute_ssimu2_hbd(ref, dist, 12)
        got = s.debug_download(RG_V, 0, w, h)
    xyb_r = oracle.linear_to_xyb(hbd_ref.linear_planes(ref, 12))
    xyb_d = oracle.linear_to_xyb(hbd_ref.linear_planes(dist, 12))
    del ref, dist
    for c, k in ((0, 0), (1, 2), (2, 4)):
        xa, xb = xyb_r[c], xyb_d[c]
        src = [xa, xb, xa * xa, xb * xb, xa * xb][k]
        same_bits(got[5 * c + k], oracle.blur_plane(src, oracle.BLUR_IIR), (c, k))
        del src


def test_source_rows_past_4_gib_of_a_small_frame(hip_lib):
    """A 200 x 4400 crop of a buffer of 1 MiB + 64-byte rows: rows from 4097 on start past 2^32 bytes.  Through both
    strided calls (8-bit: the fast RGBA and the byte path of the unpack kernel; 16-bit: the front end's loader), RGB and
    RGBA, in FIR and RECURSIVE mode, with every byte outside the frame's samples at the top code: each score is the
    tight call's, bit for bit, though the pass before it left other content in every buffer the call writes."""
    w, h, row_bytes, x0 = 200, 4400, (1 << 20) + 64, 4096
    assert (h - 1) * row_bytes > 1 << 32
    u_ref = synth.make_ref(w, h, 44)
    u_dist = synth.distort(u_ref, "blockq", 2, seed=45)
    r12, d12 = content16(w, h, 12, 46), content16(w, h, 12, 47, distort=True)
    buf = np.full(h * row_bytes, 0xFF, np.uint8)
    for mode in (_lib.BLUR_FIR, _lib.BLUR_RECURSIVE):
        with Ssimu2(0, blur=mode) as s:
            for bits, ref, dist in ((8, u_ref, u_dist), (12, r12, d12)):
                if bits == 8:
                    s.set_reference(ref)
                    exp = s.score_against_reference(dist)
                else:
                    s.set_reference_hbd(ref, bits)
                    exp = s.score_against_reference_hbd(dist, bits)
                for ch in (3, 4):
                    esz = 1 if bits == 8 else 2
                    view = np.lib.stride_tricks.as_strided(buf[x0:].view(np.uint8 if bits == 8 else np.uint16),
                                                           (h, w, ch), (row_bytes, ch * esz, esz))
                    view[..., :3] = dist
                    what = (mode, bits, ch)
                    assert scrub(s, ref, None if bits == 8 else bits) != exp, what
                    if bits == 8:
                        got = s.score_decoded_against_reference(view)
                    else:
                        got = s.score_decoded_against_reference_hbd(view, bit_depth=bits)
                    assert got == exp, what + (got, exp)
                    view[...] = np.iinfo(view.dtype).max   # the whole buffer at the top code again
    del buf


@pytest.mark.parametrize("w,h", [(9, 100_000), (64, 65_536)])
def test_tall_frames_through_both_strided_hand_offs(ctxs, oracle, w, h):
    """One grid row per image row is what the 8-bit unpack launches: frames of 65,536 and 100,000 rows, 3 and 4
    channels (64-wide RGBA: the kernel's fast path, 9-wide: the byte path), 8- and 16-bit.  Each score is the tight
    call's bits and the checker's within score_tol.  Before each strided call the reference is scored against itself,
    so the frame buffer holds other rows: rows the launch did not reach would move the score."""
    s = ctxs["fir"]
    u_ref = synth.make_ref(w, h, w + 1)
    u_dist = synth.distort(u_ref, "noise", 2, seed=w)
    exp8 = oracle.compute_ssimu2(u_ref, u_dist, oracle.BLUR_FIR)
    s.set_reference(u_ref)
    tight = s.score_against_reference(u_dist)
    assert abs(tight - exp8) <= gpu_cases.score_tol(exp8)
    for ch, pad in ((3, 5), (4, 0), (4, 8)):
        buf, view = gpu_cases.decoded_like(u_dist, ch, pad, seed=ch + pad)
        assert scrub(s, u_ref) != tight
        assert s.score_decoded_against_reference(view) == tight, (w, h, ch, pad)
    r16, d16 = content16(w, h, 10, w + 2), content16(w, h, 10, w + 3, distort=True)
    exp16 = hbd_ref.compute(oracle, r16, d16, 10, oracle.BLUR_FIR)[0]
    s.set_reference_hbd(r16, 10)
    tight = s.score_against_reference_hbd(d16, 10)
    assert abs(tight - exp16) <= gpu_cases.score_tol(exp16)
    for ch, pad in ((3, 3), (4, 0), (4, 6)):
        buf, view = rows16(d16, ch, pad, fill=0xFFFF)
        assert scrub(s, r16, 10) != tight
        assert s.score_decoded_against_reference_hbd(view, bit_depth=10) == tight, (w, h, ch, pad)
