"""Frames 65,600 to 100,000 px long against the checker in every mode (-m gpu only).

The size grid (gpu_cases.SIZES) and the production frames end at 7,680 columns and 5,200 rows; the ABI takes any
w x h up to 2^31 / 3 pixels (2^28 in the recursive modes), so a 100,000 x 16 panorama strip or a 9 x 100,000 scroll
capture is a legal input with fewer pixels than a 1080p frame.  Three shapes, the smallest that reach what such frames
do to the kernels:

  W1   65,600 x 9    just past 2^16 columns, 2 scales; 4,614 jobs of the persistent vertical pass; 547 FIR strips
  W2  100,000 x 16   3 scales of 16 / 8 / 4 rows; 8,208 vertical jobs, 1,563 column groups whose partials k_finalize
                     sums; 834 FIR strips in one segment row; 1,563 staged tiles per k_rg_h wave
  T1   9 x 100,000   the transpose: 10,002 vertical batches of ten rows per job, 15,000 k_rg_h workgroups, 625 FIR
                     segments of one strip

W1 and W2 must give every k_rg_v workgroup at least 8 jobs on the device the test runs on (asserted from its CU count):
s_job, s_out and s_part are then reused many times behind the job-tail barrier, most of each job being the prefetch
queue's batches past the image.

Content is synth.make_ref with noise on top, as on the size grid; W2 also runs one block-quantised pair.  Held in all
three blur modes unless marked FIR, under the bounds of tests/gpu_cases.py alone:

1. the pair score: averages and k_finalize against the kernel-order terms (check_against_terms), in FIR the d / d^4
   sums in k_march's own order (check_fir_sums), the score within score_tol of the checker;
2. every other entry point returns the pair call's bits (score and all 108 averages), each call behind a score of other
   content at a larger size or, on the cached paths, of the reference against itself;
3. the error map against tests/errmap_ref.py (check_map), the against-reference map and a second map for bits;
4. the instrumented build's planes at scale 0 and at the last scale, bit for bit: the linear pyramid (FIR pair call; an
   8-bit frame has no stored level 0), the cached XYB and blur(ref * ref) planes, the planes after both recursive passes
   through the pair call and a cached strided pass;
5. the 16-bit front end on 10-bit content in fir and recursive (T1's FIR half is
   test_gpu_hbd_planes.py::test_tall_frames_through_both_strided_hand_offs);
6. batches (FIR) of 5 items of W1 and 3 of T1, pair form and cached-reference form: every item the bits of a single
   score at the batch rule's rows, the identical item exactly 100 with zero averages.

The CPU references (the checker's score, the kernel-order terms) are computed once per (case, mode) and kept; a map's
reference depends on the device's averages and is computed where it is used.  Every T1 map reference takes under 3 s on
the CPU, so T1's map runs in all three modes like the others."""
import numpy as np
import pytest

import errmap_ref
import gpu_cases
import hbd_ref
from gpu_cases import (MODES, MW, bits_equal, check_against_terms, check_fir_sums, check_map, decoded_like,  # noqa: F401
                       ictx, in_margins, same_bits, score_tol, scrub, stale, stale_pair)
from hbd_cases import content16, rows16
from oavif_amd import synth

pytestmark = pytest.mark.gpu

LIN_REF, LIN_DIST, XYB_REF, REF_BLUR, RG_V = 0, 1, 2, 3, 5
RG_VW, RG_VB, RG_HL, RG_N = 64, 10, 20, 5          # oavif_amd/csrc/ssimu2_recursive.h
ALL_MODES = sorted(MODES)
RECURSIVE = [m for m in ALL_MODES if m != "fir"]

SHAPES = {"W1": (65_600, 9), "W2": (100_000, 16), "T1": (9, 100_000)}
# case -> (shape, distortion); "W2q" is W2's second pair
CASES = {"W1": ("W1", ("noise", 2)), "W2": ("W2", ("noise", 2)), "W2q": ("W2", ("blockq", 2)), "T1": ("T1", ("noise", 2))}
NSCALES = {"W1": 2, "W2": 3, "T1": 2}

_FRAMES = {}      # case -> (ref, dist)
_STALE = {}       # shape -> gpu_cases.stale_pair of it
_REFERENCE = {}   # (case, mode) -> {"score", "kavg", "ns", "kord", "rows"}
_FRAMES16 = {}    # shape -> (ref, dist) of 10 bits
_REFERENCE16 = {}  # (shape, mode) -> hbd_ref.compute
_LEVELS = {}      # shape -> plane_levels


def frames(case):
    if case not in _FRAMES:
        shape, (kind, strength) = CASES[case]
        w, h = SHAPES[shape]
        ref = _FRAMES[shape][0] if shape in _FRAMES else synth.make_ref(w, h, 17 * w + h)
        _FRAMES[case] = (ref, synth.distort(ref, kind, strength, seed=w + 3 * h))
    return _FRAMES[case]


def foreign(s, shape):
    """gpu_cases.stale with the shape's larger pair made once (noise: the cheapest kind at 4 M pixels)."""
    w, h = SHAPES[shape]
    if shape not in _STALE:
        _STALE[shape] = stale_pair(w, h, 2)
    stale(s, w, h, 2, _STALE[shape])


def reference(oracle, case, mode):
    """The checker's score and the kernel-order terms' averages of a case in a mode (FIR: the d / d^4 averages in
    k_march's order at the single-score rule's rows too), computed once."""
    key = (case, mode)
    if key not in _REFERENCE:
        ref, dist = frames(case)
        h, w, _ = ref.shape
        blur = MODES[mode][1]
        rows = gpu_cases.seg_rows(w, h) if mode == "fir" else None
        out = errmap_ref.kernel_averages(oracle, ref, dist, blur, seg_rows=rows)
        _REFERENCE[key] = {"score": oracle.compute_ssimu2(ref, dist, blur), "kavg": out[0], "ns": out[1],
                           "kord": out[2] if rows else None, "rows": rows}
    return _REFERENCE[key]


def vertical_jobs(w, h, ns):
    return 3 * sum(-(-gpu_cases.scale_size(w, h, sc)[0] // RG_VW) for sc in range(ns))


def assert_regime(s, shape):
    """The regime the shape is here for, from the plan's own arithmetic and the device's CU count."""
    w, h = SHAPES[shape]
    ns = NSCALES[shape]
    cus = s.device_info()["compute_units"]
    jobs = vertical_jobs(w, h, ns)
    if shape == "T1":
        assert (h + RG_N - 1 + RG_VB - 1) // RG_VB == 10_001                # rg_v_batches before its rounding to 10,002
        assert 3 * -(-h // RG_HL) == 15_000                               # k_rg_h workgroups of scale 0
        assert -(-h // gpu_cases.march_seg_rows(w, h, 0)) == 625 and -(-w // MW) == 1
        return
    assert jobs == {"W1": 4614, "W2": 8208}[shape] and jobs >= 8 * cus, (jobs, cus)
    assert -(-w // MW) == {"W1": 547, "W2": 834}[shape]
    assert -(-h // gpu_cases.march_seg_rows(w, h, 0)) == 1                # one segment row of hundreds of strips
    assert -(-w // RG_VW) == {"W1": 1025, "W2": 1563}[shape]              # column groups = k_finalize's partials


ctxs = gpu_cases.contexts_fixture()
ictxs = gpu_cases.contexts_fixture(instrumented=True)


def pair_score(s, shape, ref, dist):
    foreign(s, shape)
    score = s.compute_ssimu2(ref, dist)
    avg, ns = s.last_averages()
    assert ns == NSCALES[shape], (shape, ns)
    return score, avg, ns


# ---- 1. score and averages ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("mode", ALL_MODES)
def test_score_and_averages_against_the_kernel_order_terms(ctxs, oracle, mode, case):
    s, shape = ctxs[mode], CASES[case][0]
    assert_regime(s, shape)
    ref, dist = frames(case)
    h, w, _ = ref.shape
    exp = reference(oracle, case, mode)
    score, avg, ns = pair_score(s, shape, ref, dist)
    what = f"{mode} {case} {w}x{h}"
    assert ns == exp["ns"], what
    check_against_terms(oracle, score, avg, ns, ref, dist, mode, what, kavg=exp["kavg"])
    if mode == "fir":
        check_fir_sums(avg, ns, w, h, exp["kord"], exp["rows"], what)
    print(f"measured: {what}: score {abs(score - exp['score']) / score_tol(exp['score']):.3e} of score_tol")
    assert abs(score - exp["score"]) <= score_tol(exp["score"]), (what, score, exp["score"])
    assert 0.0 < score < 100.0, what


# ---- 2. every entry point -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ALL_MODES)
def test_every_entry_point_returns_the_pair_call_s_bits(ctxs, mode, shape):
    s = ctxs[mode]
    w, h = SHAPES[shape]
    ref, dist = frames(shape)
    got, avg, ns = pair_score(s, shape, ref, dist)
    assert 0.0 < got < 100.0

    def same(what, score):
        a, n = s.last_averages()
        assert n == ns, (mode, shape, what)
        bits_equal(score, a, got, avg, f"{mode} {shape} {what}")

    foreign(s, shape)
    s.set_reference(ref)
    assert scrub(s, ref) != got
    same("score_against_reference", s.score_against_reference(dist))
    # RGBA rows without padding take k_unpack_rgb<true> when w % 4 == 0 (W1, W2)
    for channels, pad in ((4, 0), (4, 3), (3, 5)):
        _buf, view = decoded_like(dist, channels, pad, seed=w + pad)
        assert scrub(s, ref) != got
        same(f"strided {channels} ch + {pad}", s.score_decoded_against_reference(view))

    t_ref, p_ref = in_margins(ref, 1, w)
    t_dist, p_dist = in_margins(dist, 3, h)
    assert p_ref % 4 == 1 and p_dist % 4 == 3
    foreign(s, shape)
    same("score_device", s.score_device(p_ref, p_dist, w, h))
    foreign(s, shape)
    s.enqueue_device(p_ref, p_dist, w, h)
    same("enqueue_device", s.wait())
    foreign(s, shape)
    s.set_reference_device(p_ref, w, h)
    assert scrub(s, ref) != got
    s.enqueue_against_reference_device(p_dist)
    same("enqueue_against_reference_device", s.wait())
    del t_ref, t_dist


# ---- 3. the error map ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ALL_MODES)
def test_error_map_against_the_reference(ctxs, oracle, mode, shape):
    s = ctxs[mode]
    w, h = SHAPES[shape]
    ref, dist = frames(shape)
    got, avg, ns = pair_score(s, shape, ref, dist)
    what = f"{mode} {shape} {w}x{h}"
    foreign(s, shape)
    score, m = s.error_map(ref, dist)
    a, n = s.last_averages()
    assert n == ns and m.shape == (h, w), what
    bits_equal(score, a, got, avg, what + " error_map")
    check_map(oracle, m, avg, ns, ref, dist, MODES[mode][1], what)
    score2, m2 = s.error_map(ref, dist)
    assert score2 == score, what
    same_bits(m2, m, what + " second map")
    foreign(s, shape)
    s.set_reference(ref)
    assert scrub(s, ref) != got
    score3, m3 = s.error_map_against_reference(dist)
    bits_equal(score3, s.last_averages()[0], got, avg, what + " error_map_against_reference")
    same_bits(m3, m, what + " against-reference map")


# ---- 4. planes of the instrumented build --------------------------------------------------------------------------

def plane_levels(oracle, shape):
    """-> (linear levels, XYB levels) of both frames of the shape's pair, every scale; computed once."""
    if shape not in _LEVELS:
        ref, dist = frames(shape)
        lin = [errmap_ref.scales(oracle, errmap_ref.linear_planes(oracle, f)) for f in (ref, dist)]
        assert len(lin[0]) == NSCALES[shape]
        _LEVELS[shape] = lin, tuple([oracle.linear_to_xyb(x) for x in levels] for levels in lin)
    return _LEVELS[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fir_planes_at_the_first_and_last_scale(ictx, oracle, shape):
    """The linear pyramid's last level of both frames after the pair call (k_pyramid_bands), the cached XYB and
    blur(ref * ref) planes of scale 0 and of the last scale after set_reference (k_ref_xyb, k_ref_blur)."""
    s = ictx["fir"]
    w, h = SHAPES[shape]
    ref, dist = frames(shape)
    (lin_r, lin_d), (xyb_r, _xyb_d) = plane_levels(oracle, shape)
    last = NSCALES[shape] - 1
    foreign(s, shape)
    s.compute_ssimu2(ref, dist)
    same_bits(s.debug_download(LIN_REF, last, w, h), lin_r[last], (shape, "lin ref", last))
    same_bits(s.debug_download(LIN_DIST, last, w, h), lin_d[last], (shape, "lin dist", last))
    foreign(s, shape)
    s.set_reference(ref)
    for sc in (0, last):
        same_bits(s.debug_download(XYB_REF, sc, w, h), xyb_r[sc], (shape, "xyb", sc))
        got = s.debug_download(REF_BLUR, sc, w, h)
        for c in range(3):
            exp = oracle.blur_product(xyb_r[sc][c], xyb_r[sc][c], oracle.BLUR_FIR)
            same_bits(got[c], exp, (shape, "ref blur", sc, c))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", RECURSIVE)
def test_recursive_planes_at_the_first_and_last_scale(ictx, oracle, mode, shape):
    """The 15 planes after both recursive passes (k_pyramid_bands_xyb, k_rg_h, k_rg_v_emit) at scale 0 and at the last
    scale, through the pair call and through a cached strided pass; the score keeps its bits whichever scale is kept."""
    r, blur = ictx[mode], MODES[mode][1]
    w, h = SHAPES[shape]
    ref, dist = frames(shape)
    _lin, (xyb_r, xyb_d) = plane_levels(oracle, shape)
    _buf, view = decoded_like(dist, 4, 7, seed=h)
    rpair = None
    for sc in (0, NSCALES[shape] - 1):
        exp = gpu_cases.rg_planes(oracle, blur, xyb_r[sc], xyb_d[sc])   # what gpu_cases.check_rg holds them to

        def planes(how):
            got = r.debug_download(RG_V, sc, w, h)
            for k in range(15):
                same_bits(got[k], exp[k], (shape, mode, how, sc, k))

        r.rg_stop_after_scale(sc)
        foreign(r, shape)
        score = r.compute_ssimu2(ref, dist)
        rpair = rpair or (score, r.last_averages()[0])
        bits_equal(score, r.last_averages()[0], rpair[0], rpair[1], f"{mode} {shape} pair, scale {sc} kept")
        planes("pair")
        r.set_reference(ref)
        assert scrub(r, ref) != rpair[0]
        score = r.score_decoded_against_reference(view)
        bits_equal(score, r.last_averages()[0], rpair[0], rpair[1], f"{mode} {shape} strided, scale {sc} kept")
        planes("strided")


# ---- 5. the 16-bit front end --------------------------------------------------------------------------------------

def frames16(shape):
    if shape not in _FRAMES16:
        w, h = SHAPES[shape]
        _FRAMES16[shape] = (content16(w, h, 10, w + 2), content16(w, h, 10, w + 2, distort=True))   # one base, distorted
    return _FRAMES16[shape]


HBD_CASES = [("W1", "fir"), ("W1", "recursive"), ("W2", "fir"), ("W2", "recursive"), ("T1", "recursive")]


@pytest.mark.parametrize("shape,mode", HBD_CASES)
def test_16bit_front_end_on_10bit_content(ctxs, oracle, shape, mode):
    s = ctxs[mode]
    w, h = SHAPES[shape]
    r16, d16 = frames16(shape)
    if (shape, mode) not in _REFERENCE16:
        _REFERENCE16[shape, mode] = hbd_ref.compute(oracle, r16, d16, 10, MODES[mode][1])
    exp, kavg, ns_r = _REFERENCE16[shape, mode]
    what = f"{mode} {shape} {w}x{h} 10-bit"
    foreign(s, shape)
    pair = s.compute_ssimu2_hbd(r16, d16, 10)
    avg, ns = s.last_averages()
    assert ns == ns_r == NSCALES[shape], what
    print(f"measured: {what}: score {abs(pair - exp) / score_tol(exp):.3e} of score_tol")
    assert abs(pair - exp) <= score_tol(exp), (what, pair, exp)
    check_against_terms(oracle, pair, avg, ns, r16, d16, mode, what, kavg=kavg)
    assert 0.0 < pair < 100.0

    def same(how, score):
        a, n = s.last_averages()
        assert n == ns, (what, how)
        bits_equal(score, a, pair, avg, f"{what} {how}")

    foreign(s, shape)
    s.set_reference_hbd(r16, 10)
    assert scrub(s, r16, 10) != pair
    same("cached tight", s.score_against_reference_hbd(d16, 10))
    for ch, pad in ((3, 3), (4, 0)):
        _buf, view = rows16(d16, ch, pad, fill=0xFFFF)
        assert scrub(s, r16, 10) != pair
        same(f"strided {ch} ch + {pad}", s.score_decoded_against_reference_hbd(view, bit_depth=10))


# ---- 6. batches (FIR) ---------------------------------------------------------------------------------------------

def batch_items(shape, n, cached):
    """n distinct pairs of the shape, item n // 2 identical: the shape's reference rolled along its long side (one
    reference for all items where `cached`), damaged by noise of rising strength over block quantisation."""
    ref = frames(shape)[0]
    axis = 1 if ref.shape[1] > ref.shape[0] else 0
    refs = [ref if cached or k == 0 else np.ascontiguousarray(np.roll(ref, 977 * k, axis=axis)) for k in range(n)]
    dists = [refs[k].copy() if k == n // 2 else
             synth.distort(synth.distort(refs[k], "blockq", 2) if k % 2 else refs[k], "noise", 1 + k % 3, seed=k)
             for k in range(n)]
    assert len({d.tobytes() for d in dists}) == n
    return refs, dists


@pytest.mark.parametrize("cached", [False, True], ids=["pairs", "cached_reference"])
@pytest.mark.parametrize("shape,n", [("W1", 5), ("T1", 3)])
def test_batch_items_have_the_bits_of_single_scores_at_the_same_rows(iscorer, shape, n, cached):
    s = iscorer
    w, h = SHAPES[shape]
    refs, dists = batch_items(shape, n, cached)
    rule = [s.batch_segment_rows(w, h, 0), s.batch_segment_rows(w, h, 1)]
    assert rule == [gpu_cases.batch_seg_rows(w, h, 0), gpu_cases.batch_seg_rows(w, h, 1)]
    # a pair batch of other content and more, larger items: the batch scratch holds its values
    if shape not in _STALE:
        _STALE[shape] = stale_pair(w, h, 2)
    big, noisy = _STALE[shape]
    s.score_batch([big] * (n + 1), [noisy] * (n + 1))
    if cached:
        s.set_reference(refs[0])
        scores = s.score_batch_against_reference(dists)
    else:
        scores = s.score_batch(refs, dists)
    assert scores.shape == (n,)
    got = [(scores[k],) + s.last_batch_averages(k) for k in range(n)]
    try:
        s.set_segment_rows(rule[0], rule[1])
        if cached:
            s.set_reference(refs[0])
        for k in range(n):
            single = s.score_against_reference(dists[k]) if cached else s.compute_ssimu2(refs[k], dists[k])
            avg1, ns1 = s.last_averages()
            assert got[k][2] == ns1 == NSCALES[shape], (shape, k)
            bits_equal(got[k][0], got[k][1], single, avg1, f"{shape} n={n} cached={cached} item {k}")
    finally:
        s.set_segment_rows(0, 0)
    assert got[n // 2][0] == 100.0 and not got[n // 2][1].any()
    assert all(0.0 < g[0] < 100.0 for k, g in enumerate(got) if k != n // 2)
