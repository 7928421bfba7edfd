"""Batches of RGBA and YUV-with-alpha frames on the MI355X (include/ssimu2_hip_abatch.h).

(a) the composite codes of a batch, item by item, against the single composite calls and the numpy restatement
(tests/yuva_ref.py), bit for bit: every format, depth, RGB depth, range and upsampling, with and without an alpha plane,
at the sizes where the kernel changes path, with odd pitches and off-alignment plane starts, the middle of three items
holding the extreme samples and its neighbours other content, and past the grid's rows; (b) scores and all 108 averages
of every item of the three scoring calls against the single calls on another context, bit for bit, in both recursive
modes, behind a larger batch of other content; the equalities the header derives; the properties; five items against the
CPU checker with the bounds tests/test_gpu_yuva.py holds single scores to; (c) lifecycle, refusals in the header's order,
memory; (d) the speculative search of an RGBA source against the sequential one; (e) scorepairs --background.

Only the last test reads libavif, where it is importable: everywhere else the planes are numpy's."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import chroma_ref
import gpu_cases
import yuv_ref
import yuva_ref
from oavif_amd import Ssimu2, Ssimu2Error, _lib, alpha as alpha_mod, synth, tq
from oavif_amd.scorer import YuvFrame
from test_gpu_alpha import codes_of, expected, held_to_the_checker, laid_out, table  # noqa: F401  (table: a fixture)
from test_gpu_yuv import same_codes
from test_gpu_yuva import alpha_of, frame_of

pytestmark = pytest.mark.gpu

RECURSIVE = ["recursive", "recursive_fma"]
FORMATS = list(yuva_ref.FORMATS.values())
IDS = list(yuva_ref.FORMATS)
UPSAMPLINGS = (chroma_ref.BILINEAR, chroma_ref.NEAREST)
MATRIX_CODES = (1, 2, 5, 6, 9)
BACKGROUNDS = [0x000000, 0xFFFFFF, 0x1A80E6, 0x7B3FC2]
# tests/test_gpu_chroma.py's grid; (1027, 9) crosses the 1,024-column block, (2051, 4) has a third block that is a tail
GRID = [(1, 1), (2, 1), (3, 3), (5, 2), (9, 8), (17, 33), (129, 67), (1027, 9), (2051, 4)]
SHAPES = [(7, 9), (8, 8), (24, 17), (65, 21), (121, 40), (130, 200), (257, 33)]
NS = [1, 2, 3, 5, 17]


@pytest.fixture(scope="module")
def ctxs(hip_lib):
    """{mode: an abatch=True context} of the two recursive modes and FIR: the contexts under test."""
    out = {name: Ssimu2(0, blur=mode, abatch=True) for name, (mode, _) in gpu_cases.MODES.items()}
    yield out
    for s in out.values():
        s.close()


@pytest.fixture(scope="module")
def singles(hip_lib):
    """{mode: a yuva=True context}: the single calls an item is held to run here, on a context that never batches."""
    out = {name: Ssimu2(0, blur=gpu_cases.MODES[name][0], yuva=True) for name in RECURSIVE}
    yield out
    for s in out.values():
        s.close()


def batch_results(s, scores):
    return [(float(scores[i]),) + tuple(s.last_batch_averages(i)) for i in range(len(scores))]


def single_result(s, score):
    avg, ns = s.last_averages()
    return score, avg, ns


def same_bits(got, exp, what):
    assert got[2] == exp[2], (what, got[2], exp[2])
    gpu_cases.bits_equal(got[0], got[1], exp[0], exp[1], what)


def make_stale(s, w, h, n):
    """A larger batch of other content on the same context: more items of a larger frame, through the pair form."""
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, (2, h + 8, w + 8, 4), dtype=np.uint8)
    m = n + 3
    s.score_batch_rgba([frames[0]] * m, [frames[1]] * m, 0x445566)


# ---- (a) the composite codes -----------------------------------------------------------------------------------------
def three_items(w, h, depth, fmt, k, with_alpha):
    """Three frames of one kind: the middle one holds the extreme samples (colour at both ends; a in 0, 1, ma - 1, ma and,
    in 16-bit samples, above ma), its neighbours random content of their own."""
    out = []
    for i in range(3):
        planes, a = yuva_ref.random_frame(w, h, depth, fmt, seed=1000 * k + 7 * i + depth, extremes=(i == 1),
                                          over=(i == 1 and depth > 8))
        out.append((planes, a if with_alpha else None))
    return out


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_composite_of_a_batch_is_the_single_composite_of_each_item(ctxs, depth, fmt):
    for k, (w, h) in enumerate(GRID):
        s = ctxs[list(ctxs)[k % 3]]                              # the kernel does not depend on the blur mode
        with_alpha = k % 4 != 3
        full_range, mc, bg = bool(k & 1), MATRIX_CODES[k % 5], BACKGROUNDS[k % 4]
        items = three_items(w, h, depth, fmt, k, with_alpha)
        if k % 2:   # odd pitches and plane starts off alignment, the alpha plane included
            laid = [frame_of(p, a, depth, full_range, mc, fmt, k + i) for i, (p, a) in enumerate(items)]
            frames = [f for f, _bufs in laid]
        else:
            frames = [YuvFrame(p, depth, fmt, full_range, mc, alpha=a) for p, a in items]
        for rgb_depth in sorted({(8, depth, 16)[k % 3], (8, depth, 16)[(k + 1) % 3]}):
            for up in UPSAMPLINGS:
                got = s.composite_yuva_batch(frames, bg, rgb_depth, up)
                assert got.shape == (3, h, w, 3)
                for i, (p, a) in enumerate(items):
                    what = (w, h, depth, fmt, rgb_depth, up, with_alpha, i)
                    same_codes(got[i], yuva_ref.codes(p, a, depth, full_range, mc, rgb_depth, fmt, bg, up), what)
                    same_codes(got[i], s.composite_yuva(frames[i], bg, rgb_depth, up), what + ("the single call",))


@pytest.mark.parametrize("name,w,h,depth,rgb_depth,with_alpha", [("444", 8, 65_600, 8, 8, True), ("420", 8, 131_080, 10, 16, False)])
def test_composite_of_a_batch_past_the_grids_rows(ctxs, name, w, h, depth, rgb_depth, with_alpha):
    """gridDim.y ends at 65,535: the last rows (chroma rows for 4:2:0: 65,540 of them) are taken in the kernel's second
    round.  Two frames a batch, rows tight, so that each plane is one copy."""
    s, fmt = ctxs["recursive"], yuva_ref.FORMATS[name]
    assert (chroma_ref.chroma_shape(w, h, fmt)[0] if fmt != yuv_ref.YUV_444 else h) > 65_535
    items = [yuva_ref.random_frame(w, h, depth, fmt, seed=40 + i) for i in range(2)]
    frames = [YuvFrame(p, depth, fmt, True, 6, alpha=a if with_alpha else None) for p, a in items]
    got = s.composite_yuva_batch(frames, BACKGROUNDS[2], rgb_depth)
    for i, (p, a) in enumerate(items):
        exp = yuva_ref.codes(p, a if with_alpha else None, depth, True, 6, rgb_depth, fmt, BACKGROUNDS[2])
        same_codes(got[i], exp, (name, i))


def rgba_items(w, h, n, seed):
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    out[n // 2][..., 3] = rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w))   # the middle item: alpha at its ends
    out[n // 2][..., :3] = rng.choice(np.array([0, 255], np.uint8), (h, w, 3))
    return out


def test_composite_of_an_rgba_batch_is_the_single_composite_of_each_item(ctxs):
    k = 0
    for h in (1, 3):
        for w in (1, 3, 4, 5, 1027):
            s = ctxs[list(ctxs)[k % 3]]
            bg = BACKGROUNDS[k % 4]
            items = rgba_items(w, h, 3, k)
            views = list(items)
            if k % 2:   # padded rows, one row_bytes for all, starts off alignment
                laid = [laid_out(f, 4 * w + 12, 1 + i, seed=k + i) for i, f in enumerate(items)]
                views = [v for _buf, v in laid]
            got = s.composite_rgba_batch(views, bg)
            for i in range(3):
                same_codes(got[i], codes_of(items[i], bg), (w, h, i))
                same_codes(got[i], s.composite_rgba(views[i], bg), (w, h, i, "the single call"))
            k += 1


# ---- (b) scores ------------------------------------------------------------------------------------------------------
_pools = {}


def pool(w, h, n):
    """(the reference's RGB, n damaged RGB frames) of a shape; computed once, never changed."""
    if (w, h) not in _pools or len(_pools[(w, h)][1]) < n:
        rgb = gpu_cases.content(gpu_cases.KINDS[(w + h) % 5], w, h, seed=w)
        big = w >= 8 and h >= 8
        dists = [gpu_cases.damaged(rgb, i + 1) if big else gpu_cases.content("noise", w, h, seed=i + 50) for i in range(max(n, 17))]
        _pools[(w, h)] = (rgb, dists)
    rgb, dists = _pools[(w, h)]
    return rgb, dists[:n]


def planes_of(rgb, depth, full_range, mc, fmt):
    p = yuv_ref.forward(rgb, depth, full_range, mc)
    if fmt == yuv_ref.YUV_400:
        return [p[0]]
    return list(p) if fmt == yuv_ref.YUV_444 else chroma_ref.subsample(p, fmt)


def item_alpha(w, h, depth, i):
    a = alpha_of(w, h, depth, i).copy()
    a[h // 3:h // 3 + 2 + i % 3, w // 4:w // 4 + 3] //= 2          # a dent of the item's own
    return a


def yuva_items(w, h, n, depth, fmt, full_range, mc, with_alpha=True):
    _rgb, dists = pool(w, h, n)
    return [YuvFrame(planes_of(d, depth, full_range, mc, fmt), depth, fmt, full_range, mc,
                     alpha=item_alpha(w, h, depth, i) if with_alpha else None) for i, d in enumerate(dists)]


def set_reference(s, w, h, kind, depth, fmt, full_range, mc, bg, rgb_depth, up):
    """The shape's reference with an alpha plane, set as RGBA8 rows or as YUVA planes."""
    rgb, _ = pool(w, h, 1)
    if kind == "rgba":
        s.set_reference_rgba(np.dstack([rgb, alpha_of(w, h, 8, 0)]), bg)
    else:
        s.set_reference_yuva(YuvFrame(planes_of(rgb, depth, full_range, mc, fmt), depth, fmt, full_range, mc,
                                      alpha=alpha_of(w, h, depth, 0)), bg, rgb_depth, up)


def cases():
    """(shape, n, format, depth, how the reference is set): every shape with every n; formats, depths and reference
    kinds rotated so that each meets every n and every shape family."""
    k = 0
    for a, (w, h) in enumerate(SHAPES):
        for b, n in enumerate(NS):
            yield k, w, h, n, FORMATS[(a + b) % 4], (8, 10)[(a + 2 * b + k // 3) % 2], ("rgba", "yuva")[(a + b + k // 4) % 2]
            k += 1


@pytest.mark.parametrize("mode", RECURSIVE)
def test_yuva_batch_items_have_the_bits_of_their_single_scores(ctxs, singles, mode):
    s, one = ctxs[mode], singles[mode]
    seen = set()
    for k, w, h, n, fmt, depth, kind in cases():
        full_range, mc, bg, up = bool(k & 1), MATRIX_CODES[k % 5], BACKGROUNDS[k % 4], UPSAMPLINGS[k % 2]
        rgb_depth = (8, depth, 16)[k % 3]
        frames = yuva_items(w, h, n, depth, fmt, full_range, mc)
        make_stale(s, w, h, n)
        for ctx in (s, one):
            set_reference(ctx, w, h, kind, depth, fmt, full_range, mc, bg, rgb_depth, up)
        got = batch_results(s, s.score_batch_against_reference_yuva(frames, rgb_depth, up))
        for i, f in enumerate(frames):
            exp = single_result(one, one.score_against_reference_yuva(f, rgb_depth, up))
            same_bits(got[i], exp, (mode, w, h, n, fmt, depth, kind, i))
        assert w < 8 or h < 8 or got[0][0] < 100.0
        seen.add((fmt, depth, kind))
    assert {f for f, _, _ in seen} == set(FORMATS) and {d for _, d, _ in seen} == {8, 10} and {r for _, _, r in seen} == {"rgba", "yuva"}


@pytest.mark.parametrize("mode", RECURSIVE)
def test_rgba_batch_items_have_the_bits_of_their_single_scores(ctxs, singles, mode):
    """score_batch_against_reference_rgba against score_against_reference_rgba, score_batch_rgba against
    compute_ssimu2_rgba; padded rows on every other case."""
    s, one = ctxs[mode], singles[mode]
    for k, w, h, n, _fmt, _depth, _kind in cases():
        rgb, dists = pool(w, h, n)
        bg = BACKGROUNDS[k % 4]
        ref = np.dstack([rgb, alpha_of(w, h, 8, 0)])
        items = [np.dstack([d, item_alpha(w, h, 8, i)]) for i, d in enumerate(dists)]
        views = items
        if k % 2:
            laid = [laid_out(f, 4 * w + 20, 1 + i % 3, seed=i) for i, f in enumerate(items)]
            views = [v for _buf, v in laid]
        make_stale(s, w, h, n)
        for ctx in (s, one):
            ctx.set_reference_rgba(ref, bg)
        got = batch_results(s, s.score_batch_against_reference_rgba(views))
        exp = [single_result(one, one.score_against_reference_rgba(v)) for v in views]
        for i in range(n):
            same_bits(got[i], exp[i], (mode, w, h, n, i, "against the reference"))
        if k % 3 == 0:   # the pair form: references of their own, item i's the (i + 1)th frame
            refs = [items[(i + 1) % n] for i in range(n)] if n > 1 else [ref]
            got = batch_results(s, s.score_batch_rgba(refs, views, bg))
            for i in range(n):
                pair = single_result(one, one.compute_ssimu2_rgba(refs[i], views[i], bg))
                same_bits(got[i], pair, (mode, w, h, n, i, "pair"))
            # the pair form keeps the cached reference, as the other pair batches of the recursive modes do
            again = batch_results(s, s.score_batch_against_reference_rgba(views[:1]))
            one.set_reference_rgba(ref, bg)
            same_bits(again[0], exp[0], (mode, w, h, n, "the reference after a pair batch"))


@pytest.mark.parametrize("mode", RECURSIVE)
def test_depth_8_at_rgb_depth_8_is_the_rgba_batch_on_the_restated_frames(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate([(65, 21), (121, 40), (24, 17)]):
        fmt, full_range, mc, up, n = FORMATS[k], bool(k & 1), MATRIX_CODES[k], UPSAMPLINGS[k % 2], 3 + k
        set_reference(s, w, h, "rgba", 8, fmt, full_range, mc, BACKGROUNDS[k], 8, up)
        frames = yuva_items(w, h, n, 8, fmt, full_range, mc)
        got = batch_results(s, s.score_batch_against_reference_yuva(frames, 8, up))
        restated = [yuva_ref.rgba8(f.planes, f.alpha, full_range, mc, fmt, up) for f in frames]
        exp = batch_results(s, s.score_batch_against_reference_rgba(restated))
        for i in range(n):
            same_bits(got[i], exp[i], (mode, w, h, fmt, i))


@pytest.mark.parametrize("mode", RECURSIVE)
def test_opaque_frames_at_rgb_depth_8_are_the_yuv_batch(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h, depth) in enumerate([(65, 21, 8), (121, 40, 10), (130, 200, 8)]):
        fmt, full_range, mc, up, n = FORMATS[(k + 1) % 4], bool(k & 1), MATRIX_CODES[k + 1], UPSAMPLINGS[k % 2], 2 + k
        set_reference(s, w, h, "rgba", depth, fmt, full_range, mc, BACKGROUNDS[k + 1], 8, up)
        plain = yuva_items(w, h, n, depth, fmt, full_range, mc, with_alpha=False)
        exp = batch_results(s, s.score_batch_against_reference_yuv(plain, 8, up))
        got = batch_results(s, s.score_batch_against_reference_yuva(plain, 8, up))            # a null alpha: a = ma
        ma = (1 << depth) - 1
        full = [YuvFrame(f.planes, depth, fmt, full_range, mc, alpha=np.full((h, w), ma, f.planes[0].dtype)) for f in plain]
        got_full = batch_results(s, s.score_batch_against_reference_yuva(full, 8, up))
        for i in range(n):
            same_bits(got[i], exp[i], (mode, w, h, depth, fmt, i, "no alpha plane"))
            same_bits(got_full[i], exp[i], (mode, w, h, depth, fmt, i, "a = ma"))


@pytest.mark.parametrize("mode", RECURSIVE)
def test_hidden_colour_does_not_move_an_item_and_alpha_damage_does(ctxs, mode):
    s = ctxs[mode]
    w, h, depth, fmt = 121, 40, 10, yuva_ref.FORMATS["444"]
    set_reference(s, w, h, "yuva", depth, fmt, True, 6, 0x1A80E6, 16, chroma_ref.BILINEAR)
    frames = yuva_items(w, h, 3, depth, fmt, True, 6)
    base = batch_results(s, s.score_batch_against_reference_yuva(frames, 16))
    a = frames[1].alpha.copy()
    a[5:20, 30:70] = 0                                            # a hole in the middle item
    holed = YuvFrame(frames[1].planes, depth, fmt, True, 6, alpha=a)
    noise = yuva_ref.random_frame(w, h, depth, fmt, seed=3)[0]
    other = [p.copy() for p in frames[1].planes]
    for p, q in zip(other, noise):
        p[a == 0] = q[a == 0]                                     # 4:4:4: a sample is seen by its own pixel alone
    assert any(not np.array_equal(p, q) for p, q in zip(other, frames[1].planes))
    hidden = YuvFrame(other, depth, fmt, True, 6, alpha=a)
    one = batch_results(s, s.score_batch_against_reference_yuva([frames[0], holed, frames[2]], 16))
    two = batch_results(s, s.score_batch_against_reference_yuva([frames[0], hidden, frames[2]], 16))
    for i in range(3):
        same_bits(two[i], one[i], (mode, i, "colour under a = 0"))
    for i in (0, 2):
        same_bits(one[i], base[i], (mode, i, "a neighbour of the damaged item"))
    assert one[1][0] < base[1][0], (mode, one[1][0], base[1][0])  # the hole itself is seen


@pytest.mark.parametrize("mode", RECURSIVE)
def test_permuting_the_items_permutes_the_results(ctxs, mode):
    s = ctxs[mode]
    w, h, depth, fmt = 65, 21, 8, yuva_ref.FORMATS["420"]
    set_reference(s, w, h, "rgba", depth, fmt, False, 1, 0xFFFFFF, 8, chroma_ref.BILINEAR)
    frames = yuva_items(w, h, 5, depth, fmt, False, 1)
    base = batch_results(s, s.score_batch_against_reference_yuva(frames, 16))
    order = [3, 0, 4, 2, 1]
    got = batch_results(s, s.score_batch_against_reference_yuva([frames[j] for j in order], 16))
    for i, j in enumerate(order):
        same_bits(got[i], base[j], (mode, i, j))
    assert len({r[0] for r in base}) == 5


@pytest.mark.parametrize("mode", RECURSIVE)
def test_five_deep_items_are_held_to_the_checker(ctxs, oracle, table, mode):
    """Five 10-bit 4:2:0 items with alpha planes at 121 x 40, rgb_depth 16: T[n] of the restated composite codes as linear
    planes through the checker (tests/test_gpu_alpha.py's expected), with the bounds tests/test_gpu_yuva.py holds single
    scores to (held_to_the_checker: gpu_cases.TOL_SCORE, RTOL_AVG, ATOL_AVG and check_against_terms), unchanged."""
    s, blur = ctxs[mode], gpu_cases.MODES[mode][1]
    w, h, depth, fmt, bg, up = 121, 40, 10, yuva_ref.FORMATS["420"], 0x1A80E6, chroma_ref.BILINEAR
    set_reference(s, w, h, "yuva", depth, fmt, True, 6, bg, 16, up)
    rgb, _ = pool(w, h, 1)
    cr = yuva_ref.codes(planes_of(rgb, depth, True, 6, fmt), alpha_of(w, h, depth, 0), depth, True, 6, 16, fmt, bg, up)
    frames = yuva_items(w, h, 5, depth, fmt, True, 6)
    got = batch_results(s, s.score_batch_against_reference_yuva(frames, 16, up))
    for i, f in enumerate(frames):
        cd = yuva_ref.codes(f.planes, f.alpha, depth, True, 6, 16, fmt, bg, up)
        exp = expected(oracle, table, ("abatch", w, h, i), cr, cd, blur)
        held_to_the_checker(oracle, s, mode, got[i], exp, cr, cd, (mode, "item", i))


# ---- (c) lifecycle and refusals --------------------------------------------------------------------------------------
def _yuva_array(frames):
    return (_lib.YuvaFrameC * len(frames))(*[f.as_yuva_c() for f in frames])


def _u8pp(frames):
    P = ctypes.POINTER(ctypes.c_uint8)
    return (P * len(frames))(*[f.ctypes.data_as(P) if f is not None else P() for f in frames])


@pytest.mark.parametrize("mode", ["fir", "recursive"])
def test_refusals_in_the_headers_order(hip_lib, mode):
    import torch
    w, h, depth, fmt = 24, 17, 10, yuva_ref.FORMATS["420"]
    E, U, N = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_NO_REFERENCE
    frames = yuva_items(w, h, 3, depth, fmt, True, 6)
    rgba = [np.dstack([d, item_alpha(w, h, 8, i)]) for i, d in enumerate(pool(w, h, 3)[1])]
    codes = np.zeros((3, h, w, 3), np.uint16)
    cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], abatch=True) as s:
        L, c = s._L, s._ctx
        err = lambda: L.ssimu2_last_error(c).decode()   # noqa: E731
        out = (ctypes.c_double * 4)(*[-1.0] * 4)
        fa, pp = _yuva_array(frames), _u8pp(rgba)
        # 1. n == 0 is OK before anything else is looked at; then the missing reference; then too many items
        assert L.ssimu2_abatch_score_against_reference_yuva(c, None, 0, 16, 0, None) == _lib.OK
        assert L.ssimu2_abatch_composite_yuva(c, None, 0, w, h, 16, 0, 0, None) == _lib.OK
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, None, 0, 0, None) == _lib.OK
        assert L.ssimu2_abatch_score_rgba8(c, None, 0, None, 0, 0, w, h, 0, None) == _lib.OK
        assert L.ssimu2_abatch_composite_rgba8(c, None, 0, 0, w, h, 0, None) == _lib.OK
        assert L.ssimu2_abatch_score_against_reference_yuva(c, None, 3, 16, 0, None) == N
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, None, 0, 3, None) == N
        big = _lib.MAX_BATCH + 1
        assert L.ssimu2_abatch_score_rgba8(c, None, 0, None, 0, big, w, h, 0, None) == E and "SSIMU2_MAX_BATCH" in err()
        assert L.ssimu2_abatch_composite_yuva(c, None, big, w, h, 16, 0, 0, None) == E and "SSIMU2_MAX_BATCH" in err()
        assert L.ssimu2_abatch_composite_rgba8(c, None, 0, big, w, h, 0, None) == E and "SSIMU2_MAX_BATCH" in err()
        s.set_reference(pool(w, h, 1)[0])                           # a reference without a background
        assert L.ssimu2_abatch_score_against_reference_yuva(c, None, big, 16, 0, None) == E and "SSIMU2_MAX_BATCH" in err()
        if mode == "fir":
            # 2. FIR comes before the null pointers: the three scoring calls; the diagnostics work
            assert L.ssimu2_abatch_score_against_reference_yuva(c, None, 3, 16, 0, None) == U and "recursive modes only" in err()
            assert L.ssimu2_abatch_score_against_reference_rgba8(c, None, 0, 3, None) == U and "recursive modes only" in err()
            assert L.ssimu2_abatch_score_rgba8(c, None, 0, None, 0, 3, w, h, 0, None) == U and "recursive modes only" in err()
            assert L.ssimu2_abatch_composite_yuva(c, fa, 3, w, h, 16, 0, 0x102030, cp) == _lib.OK
            for i, f in enumerate(frames):
                same_codes(codes[i], yuva_ref.codes(f.planes, f.alpha, depth, True, 6, 16, fmt, 0x102030), (mode, i))
            assert L.ssimu2_abatch_composite_rgba8(c, pp, 4 * w, 3, w, h, 0x102030, cp) == _lib.OK
            for i, f in enumerate(rgba):
                same_codes(codes[i], codes_of(f, 0x102030), (mode, i))
            assert list(out) == [-1.0] * 4
            return
        # 3. null arrays, items and outputs
        assert L.ssimu2_abatch_score_against_reference_yuva(c, None, 3, 16, 0, out) == E
        assert L.ssimu2_abatch_score_against_reference_yuva(c, fa, 3, 16, 0, None) == E
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, None, 4 * w, 3, out) == E
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, pp, 4 * w, 3, None) == E
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, _u8pp([rgba[0], None, rgba[2]]), 4 * w, 3, out) == E
        assert "null image pointer in the batch" in err()
        assert L.ssimu2_abatch_score_rgba8(c, None, 4 * w, pp, 4 * w, 3, w, h, 0, out) == E
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * w, None, 4 * w, 3, w, h, 0, out) == E
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * w, pp, 4 * w, 3, w, h, 0, None) == E
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * w, _u8pp([rgba[0], rgba[1], None]), 4 * w, 3, w, h, 0, out) == E
        assert L.ssimu2_abatch_composite_yuva(c, None, 3, w, h, 16, 0, 0, cp) == E
        assert L.ssimu2_abatch_composite_yuva(c, fa, 3, w, h, 16, 0, 0, None) == E
        assert L.ssimu2_abatch_composite_rgba8(c, None, 4 * w, 3, w, h, 0, cp) == E
        assert L.ssimu2_abatch_composite_rgba8(c, pp, 4 * w, 3, w, h, 0, None) == E
        # 4. a zero dimension, before the frames are looked at (row_bytes 0 would be refused next)
        assert L.ssimu2_abatch_score_rgba8(c, pp, 0, pp, 0, 3, 0, h, 0, out) == E and "zero image dimension" in err()
        assert L.ssimu2_abatch_composite_yuva(c, fa, 3, w, 0, 16, 0, 0x1000000, cp) == E and "zero image dimension" in err()
        assert L.ssimu2_abatch_composite_rgba8(c, pp, 0, 3, 0, h, 0x1000000, cp) == E and "zero image dimension" in err()
        # 5. the per-frame checks come before the background rules
        pre = _yuva_array(frames)
        pre[2].alpha_premultiplied = 1
        assert L.ssimu2_abatch_score_against_reference_yuva(c, pre, 3, 16, 0, out) == U and "premultiplied" in err()
        assert L.ssimu2_abatch_composite_yuva(c, pre, 3, w, h, 16, 0, 0x1000000, cp) == U and "premultiplied" in err()
        thin = _yuva_array(frames)
        thin[1].alpha_row_bytes = 2 * w - 2
        assert L.ssimu2_abatch_score_against_reference_yuva(c, thin, 3, 16, 0, out) == E and "alpha_row_bytes" in err()
        odd = _yuva_array(frames)
        odd[1].alpha = odd[1].alpha + 1
        assert L.ssimu2_abatch_score_against_reference_yuva(c, odd, 3, 16, 0, out) == E and "2-byte aligned" in err()
        assert L.ssimu2_abatch_score_against_reference_yuva(c, fa, 3, 7, 0, out) == U       # check_chroma's: rgb_depth
        assert L.ssimu2_abatch_score_against_reference_yuva(c, fa, 3, 16, 2, out) != _lib.OK  # ... and the upsampling
        mixed = _yuva_array(frames)
        mixed[2].alpha = None                                       # mixed alpha presence
        assert L.ssimu2_abatch_score_against_reference_yuva(c, mixed, 3, 16, 0, out) == E and "score mixed frames one by one" in err()
        assert L.ssimu2_abatch_composite_yuva(c, mixed, 3, w, h, 16, 0, 0, cp) == E and "score mixed frames one by one" in err()
        other = _yuva_array(frames)
        other[1].yuv.full_range = 0
        assert L.ssimu2_abatch_score_against_reference_yuva(c, other, 3, 16, 0, out) == E and "score mixed frames one by one" in err()
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, pp, 4 * w - 1, 3, out) == E and "row_bytes" in err()
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * w, pp, 4 * w - 1, 3, w, h, 0x1000000, out) == E and "row_bytes" in err()
        assert L.ssimu2_abatch_composite_rgba8(c, pp, 4 * w - 1, 3, w, h, 0x1000000, cp) == E and "row_bytes" in err()
        # 6. the background rules: the reference has none recorded, in the single calls' wording; the upper byte
        assert L.ssimu2_abatch_score_against_reference_yuva(c, fa, 3, 16, 0, out) == E
        batch_text = err()
        one = frames[0].as_yuva_c()
        assert L.ssimu2_score_against_reference_yuva(c, ctypes.byref(one), 16, 0, out) == E and err() == batch_text
        assert "no background recorded" in batch_text
        assert L.ssimu2_abatch_score_against_reference_rgba8(c, pp, 4 * w, 3, out) == E
        batch_text = err()
        assert L.ssimu2_score_against_reference_rgba8(c, pp[0], 4 * w, out) == E and err() == batch_text
        assert "no background recorded" in batch_text
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * w, pp, 4 * w, 3, w, h, 0x1000000, out) == E and "background_rgb" in err()
        assert L.ssimu2_abatch_composite_yuva(c, fa, 3, w, h, 16, 0, 0x1000000, cp) == E and "background_rgb" in err()
        assert L.ssimu2_abatch_composite_rgba8(c, pp, 4 * w, 3, w, h, 0x1000000, cp) == E and "background_rgb" in err()
        # 7., 8. an item above 2^28 pixels, and "fewer items per call": before anything is allocated or read (the
        # items are 24 x 17 frames: a call that went on would read beyond them)
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info(0)
        assert L.ssimu2_abatch_score_rgba8(c, pp, 4 * 16385, pp, 4 * 16385, 2, 16385, 16384, 0, out) == E and "2^28" in err()
        many = _u8pp([rgba[0]] * _lib.MAX_BATCH)
        rc = L.ssimu2_abatch_score_rgba8(c, many, 32, many, 32, _lib.MAX_BATCH, 8, 1 << 25, 0, out)
        assert rc == E and "fewer items per call" in err()
        assert torch.cuda.mem_get_info(0)[0] == free0 and list(out) == [-1.0] * 4
        # the context scores on
        s.set_reference_rgba(rgba[0], 0x808080)
        assert s.score_batch_against_reference_rgba(rgba)[0] == 100.0


@pytest.mark.parametrize("mode", RECURSIVE)
def test_out_of_memory_leaves_the_context_scoring_with_the_bits_it_had(hip_lib, mode):
    """SSIMU2_ERR_OOM by the route tests/test_gpu_hbatch.py takes: 4,096 device-resident items of 2048 x 1536 need more
    planes than the device has, and the device form refuses without touching a frame.  The buffers are the ones these
    batches share; afterwards a YUVA batch and an RGBA batch have the bits they had before."""
    w, h, depth, fmt = 65, 21, 10, yuva_ref.FORMATS["422"]
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], abatch=True) as s:
        L, c = s._L, s._ctx
        set_reference(s, w, h, "rgba", depth, fmt, True, 6, 0x1A80E6, 16, chroma_ref.BILINEAR)
        frames = yuva_items(w, h, 3, depth, fmt, True, 6)
        rgba = [np.dstack([d, item_alpha(w, h, 8, i)]) for i, d in enumerate(pool(w, h, 3)[1])]
        before = batch_results(s, s.score_batch_against_reference_yuva(frames, 16)), batch_results(s, s.score_batch_against_reference_rgba(rgba))
        out = (ctypes.c_double * 1)(-1.0)
        rc = L.ssimu2_hbatch_score_rgb16_device(c, 4096, 8192, 2048 * 1536 * 6, _lib.MAX_BATCH, 2048, 1536, 12, out)
        assert rc == _lib.ERR_OOM and "hipMalloc(recursive batch planes" in L.ssimu2_last_error(c).decode()
        assert out[0] == -1.0
        after = batch_results(s, s.score_batch_against_reference_yuva(frames, 16)), batch_results(s, s.score_batch_against_reference_rgba(rgba))
        for a, b in zip(before, after):
            for i in range(3):
                same_bits(b[i], a[i], (mode, i, "after the refused planes"))


def test_set_blur_in_between_and_the_composite_leaves_the_averages(hip_lib):
    w, h, depth, fmt = 65, 21, 8, yuva_ref.FORMATS["420"]
    frames = yuva_items(w, h, 3, depth, fmt, True, 6)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) as s:
        set_reference(s, w, h, "rgba", depth, fmt, True, 6, 0x102030, 8, chroma_ref.BILINEAR)
        a = batch_results(s, s.score_batch_against_reference_yuva(frames, 8))
        s.composite_yuva_batch(frames[:2], 0xFFFFFF, 16)             # a diagnostic: the reference and the averages stay
        s.composite_rgba_batch([np.zeros((h, w, 4), np.uint8)], 0)
        for i in range(3):
            same_bits((a[i][0],) + tuple(s.last_batch_averages(i)), a[i], (i, "after the diagnostics"))
        same_bits(batch_results(s, s.score_batch_against_reference_yuva(frames, 8))[1], a[1], "the reference after the diagnostics")
        s.set_blur(_lib.BLUR_RECURSIVE_FMA)                          # drops the reference
        with pytest.raises(Ssimu2Error) as ei:
            s.score_batch_against_reference_yuva(frames, 8)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
        set_reference(s, w, h, "rgba", depth, fmt, True, 6, 0x102030, 8, chroma_ref.BILINEAR)
        b = batch_results(s, s.score_batch_against_reference_yuva(frames, 8))
        with Ssimu2(0, blur=_lib.BLUR_RECURSIVE_FMA, yuva=True) as one:
            set_reference(one, w, h, "rgba", depth, fmt, True, 6, 0x102030, 8, chroma_ref.BILINEAR)
            for i, f in enumerate(frames):
                same_bits(b[i], single_result(one, one.score_against_reference_yuva(f, 8)), (i, "after set_blur"))
        s.set_blur(_lib.BLUR_FIR)
        s.set_reference_rgba(np.zeros((h, w, 4), np.uint8), 0)
        with pytest.raises(Ssimu2Error) as ei:
            s.score_batch_against_reference_yuva(frames, 8)
        assert ei.value.code == _lib.ERR_UNSUPPORTED


def test_a_context_that_never_makes_these_calls_has_the_memory_of_an_hbatch_context(hip_lib):
    import torch
    w, h = 257, 130
    rgb, dists = pool(w, h, 4)
    yuv = [YuvFrame(planes_of(d, 8, True, 6, yuva_ref.FORMATS["420"]), 8, yuva_ref.FORMATS["420"]) for d in dists]

    def work(s):
        s.set_reference(rgb)
        s.score_batch_against_reference_yuv(yuv)
        s.score_batch(dists, dists)
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    def used(**flag):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, **flag) as s:
            return free0 - work(s)

    for flag in ("hbatch", "abatch"):                                # a library's code objects are loaded by its first launches
        used(**{flag: True})
    used_h, used_a = used(hbatch=True), used(abatch=True)
    assert used_a == used_h, (used_a, used_h)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) as s:
        free1 = work(s)
        assert work(s) == free1                                      # steady
        s.set_reference_rgba(np.dstack([rgb, alpha_of(w, h, 8, 0)]), 0)
        rgba = [np.dstack([d, alpha_of(w, h, 8, 1)]) for d in dists]
        s.score_batch_rgba(rgba * 8, rgba * 8, 0)                   # 32 pairs: rows and codes beyond what the YUV batch staged
        assert torch.cuda.mem_get_info(0)[0] < free1


def test_the_other_libraries_contexts_are_unaffected(hip_lib):
    f = YuvFrame([np.zeros((8, 8), np.uint8)], 8, _lib.YUV_400)
    rgba = np.zeros((8, 8, 4), np.uint8)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, hbatch=True) as s:
        for name in _lib.ABATCH_SYMBOLS:
            assert not hasattr(s._L, name), name
        for call in (lambda: s.score_batch_against_reference_yuva([f]), lambda: s.composite_yuva_batch([f], 0),
                     lambda: s.score_batch_against_reference_rgba([rgba]), lambda: s.score_batch_rgba([rgba], [rgba], 0),
                     lambda: s.composite_rgba_batch([rgba], 0)):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "abatch=True" in str(ei.value)
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) as s:
        assert s.abatch and s.hbatch and s.rbatch and s.yuva and s.chroma and s.maps and s.yuv and s.extended


def test_a_service_context_refuses_every_call_and_goes_on_scoring(hip_lib):
    from oavif_amd import service
    w, h = 24, 17
    rgb, dists = pool(w, h, 2)
    frames = yuva_items(w, h, 2, 8, yuva_ref.FORMATS["444"], True, 6)
    rgba = [np.zeros((h, w, 4), np.uint8)] * 2
    svc = service.start(max_lifetime=120)
    try:
        with Ssimu2(0, service=svc.socket, abatch=True) as s:
            exp = s.compute_ssimu2(rgb, dists[0])
            for call in (lambda: s.score_batch_against_reference_yuva(frames), lambda: s.composite_yuva_batch(frames, 0),
                         lambda: s.score_batch_against_reference_rgba(rgba), lambda: s.score_batch_rgba(rgba, rgba, 0),
                         lambda: s.composite_rgba_batch(rgba, 0)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert s.compute_ssimu2(rgb, dists[0]) == exp
    finally:
        assert svc.stop(timeout=30) == 0


# ---- (d) the search ----------------------------------------------------------------------------------------------------
class FakeDecoded(SimpleNamespace):
    closed = False

    def close(self):
        self.closed = True

    def pixels(self):
        return self.rows


def synthetic_codecs(src):
    """codec_frame(q) of a stand-in codec over an RGBA source: coarser colour and a coarser alpha plane for lower q, handed
    over as 8-bit 4:2:0 planes with an alpha plane (what avif_bridge.decode_yuv leaves) or as RGBA rows (decode_common)."""
    h, w, _ = src.shape
    codec = gpu_cases.pseudo_codec(np.ascontiguousarray(src[..., :3]))
    handed = []

    def alpha_at(q):
        step = 1 + (100 - q) // 8
        return ((src[..., 3].astype(np.uint32) // step) * step).astype(np.uint8)

    def yuv(q):
        dec, size = codec(q)
        f = FakeDecoded(planes=planes_of(dec, 8, True, 6, yuva_ref.FORMATS["420"]), depth=8, format=yuva_ref.FORMATS["420"],
                        full_range=True, matrix_coefficients=6, alpha=alpha_at(q), alpha_premultiplied=False, height=h, width=w)
        handed.append(f)
        return f, size

    def rgba(q):
        dec, size = codec(q)
        f = FakeDecoded(rows=np.dstack([dec, alpha_at(q)]), channels=4, height=h, width=w)
        handed.append(f)
        return f, size

    return yuv, rgba, handed


@pytest.mark.parametrize("mode", RECURSIVE)
@pytest.mark.parametrize("score_yuv", [True, False], ids=["yuva", "rgba"])
def test_the_speculative_search_is_the_sequential_one(ctxs, singles, mode, score_yuv):
    s, one = ctxs[mode], singles[mode]
    w, h, bg = 64, 48, 0x1A1A1A
    src = np.dstack([synth.make_ref(w, h, seed=21), alpha_of(w, h, 8, 0)])
    yuv, rgba, handed = synthetic_codecs(src)
    codec_frame = yuv if score_yuv else rgba
    how = dict(score_tgt=80.0, tolerance=0.5, max_pass=6)
    one.set_reference_rgba(src, bg)

    def probe(q):
        f, _size = codec_frame(q)
        try:
            if score_yuv:
                return one.score_against_reference_yuva(alpha_mod.yuva_frame(f), 8, "bilinear")
            return one.score_against_reference_rgba(f.rows)
        finally:
            f.close()

    a = tq.find_target_quality(probe, how["score_tgt"], how["tolerance"], how["max_pass"])
    assert a.num_pass >= 2, a
    bits = lambda r: np.array([sc for _q, sc in r.history] + [r.score]).view(np.uint64)   # noqa: E731
    name = "score_batch_against_reference_yuva" if score_yuv else "score_batch_against_reference_rgba"
    calls, real = [], getattr(s, name)
    setattr(s, name, lambda frames, *args: (calls.append(len(frames)), real(frames, *args))[1])
    try:
        for fan in (1, 2, 4):
            for first in (1, 4):
                del handed[:], calls[:]
                b, stats, sizes = alpha_mod.search_rgba_speculative_frames(s, src, bg, codec_frame, max_fanout=fan,
                                                                           first_wave_fanout=first, score_yuv=score_yuv, **how)
                what = (mode, score_yuv, fan, first, a, b, stats)
                assert (b.q, b.num_pass) == (a.q, a.num_pass), what
                assert [q for q, _ in b.history] == [q for q, _ in a.history], what
                assert np.array_equal(bits(a), bits(b)), what
                assert len(handed) == stats.probes_issued >= b.num_pass and all(f.closed for f in handed), what
                assert all(n >= tq.MIN_BATCHED_WAVE for n in calls) and (fan > 1 or not calls), what
                if fan > 1:
                    assert calls, what                               # a wave of two or more, scored by one call
    finally:
        delattr(s, name)


@pytest.mark.parametrize("score_yuv", [True, False], ids=["yuva", "rgba"])
def test_a_real_search_through_libavif_is_search_rgba(hip_lib, score_yuv):
    ab = pytest.importorskip("oavif_amd.avif_bridge")
    if not ab.available():
        pytest.skip("libavif is not importable here")
    from oavif_amd import cli
    w, h, bg = 96, 64, 0x1A1A1A
    src = np.dstack([synth.make_ref(w, h, seed=5), alpha_of(w, h, 8, 0)])
    options = cli.AvifEncOptions()
    options.tenbit, options.speed, options.quality_alpha = False, 10, 90
    with Ssimu2(0, blur=_lib.BLUR_RECURSIVE, yuva=True) as one, Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) as s:
        a = alpha_mod.search_rgba(src, options, bg, scorer=one, score_yuv=score_yuv)
        b, stats, sizes = alpha_mod.search_rgba_speculative(src, options, bg, scorer=s, score_yuv=score_yuv, max_fanout=2)
    assert (b.q, b.num_pass) == (a.q, a.num_pass) and [q for q, _ in b.history] == [q for q, _ in a.history]
    assert np.array_equal(np.array([sc for _q, sc in a.history]).view(np.uint64), np.array([sc for _q, sc in b.history]).view(np.uint64))
    assert stats.probes_issued >= b.num_pass and b.buf_q in sizes


# ---- (e) scorepairs --background ---------------------------------------------------------------------------------------
def test_scorepairs_with_a_background_scores_rgba_pairs_as_the_single_calls_do(ctxs, singles, tmp_path):
    from oavif_amd import pam, scorepairs
    s, one = ctxs["recursive"], singles["recursive"]
    lines, frames = [], {}
    for k, (w, h) in enumerate([(24, 17), (65, 21), (24, 17)]):          # two sizes: two groups, the first of two pairs
        rgb, dists = pool(w, h, 3)
        ref = np.dstack([rgb, alpha_of(w, h, 8, 0)])
        dist = np.dstack([dists[k], item_alpha(w, h, 8, k)]) if k else dists[0]      # the first distorted file has no alpha
        for name, a in ((f"r{k}.pam", ref), (f"d{k}.pam", dist)):
            (tmp_path / name).write_bytes(pam.write_pam(a))
        frames[k] = (ref, dist if dist.shape[2] == 4 else np.dstack([dist, np.full((h, w), 255, np.uint8)]))
        lines.append(f"r{k}.pam\td{k}.pam")
    tsv, out = tmp_path / "pairs.tsv", tmp_path / "out.csv"
    tsv.write_text("\n".join(lines) + "\n")
    assert scorepairs.main([str(tsv), str(out), "--blur", "recursive", "--background", "1A80E6"], scorer=s) == 0
    rows = out.read_text().splitlines()[1:]
    assert len(rows) == 3
    for k, row in enumerate(rows):
        exp = one.compute_ssimu2_rgba(frames[k][0], frames[k][1], 0x1A80E6)
        assert float(row.split(",")[-1]) == exp and exp < 100.0, (k, row, exp)
