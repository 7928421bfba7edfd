"""RGBA input on the MI355X (include/ssimu2_hip_ext.h), in all three blur modes: the composite codes
of k_composite_rgba8 against numpy's integer arithmetic, bit identity with the 8-bit path on opaque frames, colour
hidden under a = 0, alpha damage, genuine content against the checker, the context's hygiene among 8-bit, 16-bit and
RGBA calls, the scoring service's refusal, and the search.

The expected values of genuine content come from numpy alone: codes n = a*c + (255 - a)*b -> T[n] as fp32 planes ->
errmap_ref.score_lin (the checker route over linear planes), held with the bounds tests/test_gpu_hbd.py holds
16-bit content to (gpu_cases.score_tol, RTOL_AVG / ATOL_AVG, gpu_cases.check_against_terms), unchanged."""
import numpy as np
import pytest

import errmap_ref
import gpu_cases
from oavif_amd import Ssimu2, Ssimu2Error, _lib, scorer as scorer_mod, synth

pytestmark = pytest.mark.gpu

MODES = list(gpu_cases.MODES)
BACKGROUNDS = [0x000000, 0xFFFFFF, 0x1A80E6, int(np.random.default_rng(77).integers(0, 1 << 24))]


ctxs = gpu_cases.contexts_fixture(extended=True)


@pytest.fixture(scope="module")
def table(hip_lib):
    return scorer_mod.alpha_table()


def codes_of(rgba, bg):
    """(h, w, 3) uint16: n = a*c + (255 - a)*b in numpy's integer arithmetic."""
    a = rgba[..., 3:4].astype(np.int64)
    b = np.array([(bg >> 16) & 255, (bg >> 8) & 255, bg & 255], np.int64)
    n = a * rgba[..., :3].astype(np.int64) + (255 - a) * b
    assert n.min() >= 0 and n.max() <= 65025
    return np.ascontiguousarray(n.astype(np.uint16))


def laid_out(rgba, row_bytes, offset, seed):
    """`rgba` in rows `row_bytes` apart starting `offset` bytes into a noise-filled buffer -> (buffer, (h, w, 4) view)."""
    h, w, _ = rgba.shape
    assert row_bytes >= 4 * w
    buf = np.random.default_rng(seed).integers(0, 256, offset + row_bytes * h + 8, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], (h, w, 4), (row_bytes, 4, 1))
    view[...] = rgba
    return buf, view


def rgba_of(rgb, alpha):
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = rgb
    out[..., 3] = alpha
    return out


def alpha_plane(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "disc":       # opaque inside, a soft edge a sixth of the radius wide, transparent outside
        r = np.hypot(xx - w / 2.0, yy - h / 2.0)
        rad = 0.4 * min(w, h)
        return np.clip((rad - r) / (rad / 6.0) * 255.0 + 128.0, 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    return (((xx // 13 + yy // 11) % 3 != 0) * 255).astype(np.uint8)   # "binary": blocks of 0 and 255


def results(s, score):
    avg, ns = s.last_averages()
    return score, avg, ns


def assert_bits(got, exp, what):
    assert got[2] == exp[2], (what, got[2], exp[2])
    gpu_cases.bits_equal(got[0], got[1], exp[0], exp[1], what)


# ---- (a) the codes ----------------------------------------------------------------------------------------------
def every_pair_frame():
    """256 x 256: a = y, R = x, G and B two fixed permutations of x: every (a, c) pair occurs in each channel."""
    yy, xx = np.mgrid[0:256, 0:256]
    g = (xx * 167 + 13) & 255                                   # odd multiplier: a bijection of 0..255
    b = np.random.default_rng(256).permutation(256)[xx]
    return np.ascontiguousarray(np.stack([xx, g, b, yy], -1).astype(np.uint8))


@pytest.mark.parametrize("bg", BACKGROUNDS, ids=[f"{b:06X}" for b in BACKGROUNDS])
def test_every_alpha_colour_pair_composites_to_numpys_integer(ctxs, bg):
    frame = every_pair_frame()
    exp = codes_of(frame, bg)
    for mode in MODES:       # the kernel does not depend on the blur mode; every context has its own buffers
        got = ctxs[mode].composite_rgba(frame, bg)
        assert got.dtype == np.uint16 and got.shape == exp.shape
        assert np.array_equal(got, exp), (mode, np.argwhere(got != exp)[:4].tolist())
    r, g, b = (bg >> 16) & 255, (bg >> 8) & 255, bg & 255
    assert np.array_equal(ctxs["fir"].composite_rgba(frame, (r, g, b)), exp)


@pytest.mark.parametrize("h", [1, 2, 9])
def test_noise_frames_at_every_width_pitch_and_alignment(ctxs, h):
    s = ctxs["fir"]
    k = 0
    for w in (1, 2, 3, 4, 5, 7, 9, 63, 65, 130):
        frame = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 4), dtype=np.uint8)
        for pad in (0, 1, 3, 64):
            bg = BACKGROUNDS[k % 4]
            exp = codes_of(frame, bg)
            buf, view = laid_out(frame, 4 * w + pad, k % 4, seed=k)
            assert view.ctypes.data % 4 == (buf.ctypes.data + k % 4) % 4
            got = s.composite_rgba(view, bg)
            assert np.array_equal(got, exp), (w, h, pad, k % 4, np.argwhere(got != exp)[:4].tolist())
            k += 1


@pytest.mark.parametrize("w,h", [(1027, 5), (4100, 3), (8, 65_600)])
def test_codes_past_one_block_in_x_and_past_the_grid_s_rows(ctxs, w, h):
    """A block of k_composite_rgba8 takes 1,024 pixels of a row: 1027 = 1,024 + 3 has a second block that is a tail
    alone, 4100 = 4 * 1,024 + 4 a fifth block of one whole group.  gridDim.y ends at 65,535: 8 x 65,600 is the smallest
    frame whose last 65 rows are taken in the kernel's second round (y += gridDim.y)."""
    s = ctxs["fir"]
    assert w > 1024 or h > 65_535
    frame = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for k, pad in enumerate((0, 1, 3, 64)):
        bg = BACKGROUNDS[k % 4]
        exp = codes_of(frame, bg)
        buf, view = laid_out(frame, 4 * w + pad, k % 4, seed=k)
        assert view.ctypes.data % 4 == (buf.ctypes.data + k % 4) % 4
        got = s.composite_rgba(view, bg)
        assert got.dtype == np.uint16 and got.shape == exp.shape
        assert np.array_equal(got, exp), (w, h, pad, k % 4, np.argwhere(got != exp)[:4].tolist())


# ---- (b) opaque frames are the 8-bit path ------------------------------------------------------------------------
def test_opaque_frame_of_65600_rows_scores_as_its_rgb_bit_for_bit(ctxs):
    """9 x 65,600 (FIR): the composite's second row round in front of the pair score and the cached score."""
    s = ctxs["fir"]
    w, h = 9, 65_600
    ref = synth.make_ref(w, h, seed=17 * w + h)
    dist = synth.distort(ref, "noise", 2, seed=w + 3 * h)
    exp = results(s, s.compute_ssimu2(ref, dist))
    assert 0.0 < exp[0] < 100.0 and exp[2] == 2
    s.set_reference(ref)
    exp_c = results(s, s.score_against_reference(dist))
    _br, r4 = laid_out(rgba_of(ref, 255), 4 * w + 5, 1, seed=1)
    _bd, d4 = laid_out(rgba_of(dist, 255), 4 * w + 12, 2, seed=2)
    gpu_cases.stale(s, w, h, 1)
    assert_bits(results(s, s.compute_ssimu2_rgba(r4, d4, 0xE680FF)), exp, "9x65600 pair")
    s.set_reference_rgba(r4, 0xE680FF)
    assert s.score_against_reference_rgba(r4) == 100.0
    assert_bits(results(s, s.score_against_reference_rgba(d4)), exp_c, "9x65600 cached")



@pytest.mark.parametrize("mode", MODES)
def test_opaque_frames_score_as_their_rgb_bit_for_bit(ctxs, mode):
    s = ctxs[mode]
    for k, (w, h) in enumerate(gpu_cases.SIZES):
        kind = gpu_cases.KINDS[k % len(gpu_cases.KINDS)]
        ref = gpu_cases.content(kind, w, h, seed=k)
        dist = synth.distort(ref, "blockq", 2) if w >= 8 and h >= 8 else gpu_cases.content("noise", w, h, seed=k + 50)
        exp = results(s, s.compute_ssimu2(ref, dist))
        s.set_reference(ref)
        exp_c = results(s, s.score_against_reference(dist))
        _br, r4 = laid_out(rgba_of(ref, 255), 4 * w + 5, 1, seed=k)
        _bd, d4 = laid_out(rgba_of(dist, 255), 4 * w + 12, 2, seed=k + 1)
        for bg in (0x1A1A1A, 0xE680FF):
            what = (mode, w, h, kind, f"{bg:06X}")
            assert_bits(results(s, s.compute_ssimu2_rgba(r4, d4, bg)), exp, what + ("pair",))
            s.set_reference_rgba(r4, bg)
            assert_bits(results(s, s.score_against_reference_rgba(d4)), exp_c, what + ("cached",))
            assert_bits(results(s, s.score_against_reference_rgba(_bd[2:2 + (4 * w + 12) * h], row_bytes=4 * w + 12)), exp_c,
                        what + ("cached, flat",))


# ---- (c) colour under a = 0 does not exist -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_colour_under_full_transparency_does_not_enter_the_result(ctxs, mode):
    s = ctxs[mode]
    w, h, bg = 333, 217, 0x1A80E6
    rgb = gpu_cases.content("gradient", w, h, seed=3)
    alpha = alpha_plane("disc", w, h, 0)
    hidden = alpha == 0
    assert hidden.sum() > 1000 and (alpha == 255).sum() > 1000
    ref0, dist0 = rgba_of(rgb, alpha), rgba_of(synth.distort(rgb, "blockq", 2), alpha)
    ref0[hidden, :3] = 0
    dist0[hidden, :3] = 0
    ref1, dist1 = ref0.copy(), dist0.copy()
    ref1[hidden, :3] = np.random.default_rng(1).integers(0, 256, (int(hidden.sum()), 3))
    dist1[hidden, :3] = np.random.default_rng(2).integers(0, 256, (int(hidden.sum()), 3))
    assert np.array_equal(s.composite_rgba(ref1, bg), s.composite_rgba(ref0, bg))
    exp = results(s, s.compute_ssimu2_rgba(ref0, dist0, bg))
    assert exp[0] < 100.0
    assert_bits(results(s, s.compute_ssimu2_rgba(ref1, dist1, bg)), exp, (mode, "pair"))
    s.set_reference_rgba(ref0, bg)
    exp_c = results(s, s.score_against_reference_rgba(dist0))
    s.set_reference_rgba(ref1, bg)
    assert_bits(results(s, s.score_against_reference_rgba(dist1)), exp_c, (mode, "cached"))
    # two frames that differ only where nobody can see
    assert s.score_against_reference_rgba(ref0) == 100.0
    assert s.compute_ssimu2_rgba(ref0, ref1, bg) == 100.0     # (a pair score drops the cached reference)
    # ... which the alpha-dropping 8-bit hand-off does see
    s.set_reference(np.ascontiguousarray(ref0[..., :3]))
    assert s.score_decoded_against_reference(ref1) < 100.0


# ---- (d) a frame of the background's colour is the background ------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_background_coloured_frame_with_any_alpha_is_the_flat_frame(ctxs, mode):
    s = ctxs[mode]
    w, h = 129, 41
    for k, bg in enumerate(BACKGROUNDS):
        colour = np.array([(bg >> 16) & 255, (bg >> 8) & 255, bg & 255], np.uint8)
        flat = np.broadcast_to(colour, (h, w, 3))
        veiled = rgba_of(flat, alpha_plane(("noise", "disc", "binary", "noise")[k], w, h, k))
        opaque = rgba_of(flat, 255)
        assert s.compute_ssimu2_rgba(opaque, veiled, bg) == 100.0, (mode, f"{bg:06X}")
        assert s.compute_ssimu2_rgba(veiled, opaque, bg) == 100.0, (mode, f"{bg:06X}")
        s.set_reference_rgba(opaque, bg)
        assert s.score_against_reference_rgba(veiled) == 100.0, (mode, f"{bg:06X}")


# ---- (e), (f) against the checker ----------------------------------------------------------------------------------
_expected = {}


def expected(oracle, table, key, cr, cd, blur):
    """(score, (6, 18) averages, nscales) of two code frames in the checker's mode `blur`; computed once per key."""
    if (key, blur) not in _expected:
        lin_r = table[cr].transpose(2, 0, 1).copy()
        lin_d = table[cd].transpose(2, 0, 1).copy()
        _expected[(key, blur)] = errmap_ref.score_lin(oracle, lin_r, lin_d, blur)
    return _expected[(key, blur)]


def held_to_the_checker(oracle, s, mode, got, exp, cr, cd, what):
    score, avg, ns = got
    assert ns == exp[2], what
    print(f"measured: {what}: score {score!r}, checker {exp[0]!r}, |d| {abs(score - exp[0]):.2e}")
    assert abs(score - exp[0]) <= gpu_cases.score_tol(exp[0]), (what, score, exp[0])
    assert np.allclose(avg, exp[1], rtol=gpu_cases.RTOL_AVG, atol=gpu_cases.ATOL_AVG), what
    return gpu_cases.check_against_terms(oracle, score, avg, ns, cr, cd, mode, what, kavg=exp[1])


@pytest.mark.parametrize("mode", MODES)
def test_alpha_damage_is_seen(ctxs, oracle, table, mode):
    s = ctxs[mode]
    w, h, bg = 256, 192, 0x1A1A1A
    rgb = gpu_cases.content("gradient", w, h, seed=5)          # over a dark grey that is none of its colours
    ref = rgba_of(rgb, alpha_plane("disc", w, h, 0))
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.hypot(xx - w / 2.0 - 2, yy - h / 2.0 + 1)           # the same disc two pixels aside, with a wider edge
    dist = rgba_of(rgb, np.clip((0.4 * h - r) / (0.4 * h / 4.0) * 255.0 + 128.0, 0, 255).astype(np.uint8))
    assert np.array_equal(ref[..., :3], dist[..., :3]) and (ref[..., 3] != dist[..., 3]).any()
    cr, cd = codes_of(ref, bg), codes_of(dist, bg)
    exp = expected(oracle, table, ("damage", w, h), cr, cd, gpu_cases.MODES[mode][1])
    got = results(s, s.compute_ssimu2_rgba(ref, dist, bg))
    assert got[0] < 100.0 - 1.0, got[0]
    held_to_the_checker(oracle, s, mode, got, exp, cr, cd, f"{mode} alpha damage {w}x{h}")
    s.set_reference(np.ascontiguousarray(rgb))                 # the alpha-dropping hand-off sees no damage at all
    assert s.score_decoded_against_reference(dist) == 100.0


@pytest.mark.parametrize("mode", MODES)
def test_genuine_content_against_the_checker(ctxs, oracle, table, mode):
    s = ctxs[mode]
    blur = gpu_cases.MODES[mode][1]
    k, worst = 0, 0.0
    for w, h in [(256, 192), (333, 217), (129, 41)]:
        for akind in ("disc", "noise", "binary"):
            bg = BACKGROUNDS[k % 4]
            rgb = gpu_cases.content(gpu_cases.KINDS[k % 5], w, h, seed=k)
            alpha = alpha_plane(akind, w, h, k)
            ref = rgba_of(rgb, alpha)
            dalpha = np.clip(alpha.astype(np.int64) + np.random.default_rng(k + 9).integers(-3, 4, (h, w)), 0, 255)
            dist = rgba_of(synth.distort(rgb, "blockq", 2), dalpha.astype(np.uint8))
            cr, cd = codes_of(ref, bg), codes_of(dist, bg)
            exp = expected(oracle, table, (w, h, akind), cr, cd, blur)
            _br, rv = laid_out(ref, 4 * w + 3, 3, seed=k)
            _bd, dv = laid_out(dist, 4 * w + 64, 1, seed=k + 1)
            what = f"{mode} {akind} alpha {w}x{h} over {bg:06X}"
            worst = max(worst, held_to_the_checker(oracle, s, mode, results(s, s.compute_ssimu2_rgba(rv, dv, bg)), exp,
                                                   cr, cd, what + ", pair"))
            s.set_reference_rgba(rv, bg)
            worst = max(worst, held_to_the_checker(oracle, s, mode, results(s, s.score_against_reference_rgba(dv)), exp,
                                                   cr, cd, what + ", cached"))
            k += 1
    print(f"measured: genuine RGBA content, {mode}: worst average {worst:.3e} of its bound")


# ---- (g) the context among its other callers -----------------------------------------------------------------------
def _walk_ops(w, h):
    rgb = gpu_cases.content("text", w, h, seed=11)
    dist = synth.distort(rgb, "blockq", 3)
    r16 = rgb.astype(np.uint16) * np.uint16(257) + np.uint16(3)
    d16 = dist.astype(np.uint16) * np.uint16(257) + np.uint16(1)
    ref4 = rgba_of(rgb, alpha_plane("disc", w, h, 0))
    dist4 = rgba_of(dist, alpha_plane("noise", w, h, 1))
    bg, bg2 = 0x1A1A1A, 0xE6E6E6

    def cached(setter, scorer_call):
        def run(s):
            setter(s)
            return results(s, scorer_call(s))
        return run

    return {
        "pair 8": lambda s: results(s, s.compute_ssimu2(rgb, dist)),
        "pair 16": lambda s: results(s, s.compute_ssimu2_hbd(r16, d16, 16)),
        "pair rgba": lambda s: results(s, s.compute_ssimu2_rgba(ref4, dist4, bg)),
        "pair rgba, other background": lambda s: results(s, s.compute_ssimu2_rgba(ref4, dist4, bg2)),
        "cached 8": cached(lambda s: s.set_reference(rgb), lambda s: s.score_against_reference(dist)),
        "cached 16": cached(lambda s: s.set_reference_hbd(r16, 16), lambda s: s.score_against_reference_hbd(d16, 16)),
        "cached rgba": cached(lambda s: s.set_reference_rgba(ref4, bg), lambda s: s.score_against_reference_rgba(dist4)),
        "rgba reference, 8-bit frame": cached(lambda s: s.set_reference_rgba(ref4, bg2), lambda s: s.score_against_reference(dist)),
        "rgba reference, 16-bit frame": cached(lambda s: s.set_reference_rgba(ref4, bg2),
                                               lambda s: s.score_against_reference_hbd(d16, 16)),
        "codes": lambda s: (0.0, s.composite_rgba(dist4, bg2).astype(np.float64), 0),
    }


@pytest.mark.parametrize("mode", MODES)
def test_interleaved_calls_equal_fresh_contexts(ctxs, mode):
    w, h = 333, 217
    ops = _walk_ops(w, h)
    fresh = {}
    for name, op in ops.items():
        with Ssimu2(0, blur=gpu_cases.MODES[mode][0], extended=True) as s:
            fresh[name] = op(s)
    names = list(ops)
    order = names + names[::-1] + [names[i] for i in np.random.default_rng(5).permutation(len(names))]
    with Ssimu2(0, blur=gpu_cases.MODES[mode][0], extended=True) as s:
        gpu_cases.stale(s, w, h, 1)                    # a larger frame's bytes in every buffer first
        for i, name in enumerate(order):
            got = ops[name](s)
            assert got[2] == fresh[name][2], (mode, i, name)
            assert np.array_equal(np.asarray(got[1]), np.asarray(fresh[name][1])) and got[0] == fresh[name][0], (mode, i, name)
    # the mixed forms are the pair scores of the same frames: an 8-bit frame u is the code 255 u
    rgb_dist = synth.distort(gpu_cases.content("text", w, h, seed=11), "blockq", 3)
    ref4 = rgba_of(gpu_cases.content("text", w, h, seed=11), alpha_plane("disc", w, h, 0))
    s = ctxs[mode]
    exp = results(s, s.compute_ssimu2_rgba(ref4, rgba_of(rgb_dist, 255), 0xE6E6E6))
    assert_bits(fresh["rgba reference, 8-bit frame"], exp, (mode, "8-bit frame against an RGBA reference"))


def test_what_an_rgba_reference_refuses_and_what_refuses_rgba(ctxs, scorer):
    s = ctxs["fir"]
    w, h = 64, 20
    rgb = gpu_cases.content("noise", w, h, seed=1)
    ref4 = rgba_of(rgb, alpha_plane("noise", w, h, 2))
    with Ssimu2(0, extended=True) as t:
        with pytest.raises(Ssimu2Error) as ei:
            t.score_against_reference_rgba(ref4)
        assert ei.value.code == _lib.ERR_NO_REFERENCE
    s.set_reference_rgba(ref4, 0x808080)
    with pytest.raises(Ssimu2Error) as ei:
        s.error_map_against_reference(rgb)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    assert s.score_against_reference(rgb) <= 100.0           # an 8-bit frame against it works
    kept = s.last_averages()
    assert np.array_equal(s.composite_rgba(rgba_of(rgb, 7), 0x123456), codes_of(rgba_of(rgb, 7), 0x123456))
    assert np.array_equal(s.last_averages()[0], kept[0])     # a composite alone leaves the last score's averages
    assert s.score_against_reference_rgba(ref4) == 100.0     # and the reference is still cached
    s.set_reference(rgb)                                     # a reference that recorded no background
    with pytest.raises(Ssimu2Error) as ei:
        s.score_against_reference_rgba(ref4)
    assert ei.value.code == _lib.ERR_INVALID_ARG and "background" in str(ei.value)
    assert s.score_against_reference(rgb) == 100.0
    with pytest.raises(ValueError):
        s.compute_ssimu2_rgba(ref4, ref4, 0x1000000)
    bad = np.lib.stride_tricks.as_strided(ref4, (h, w, 4), (4 * w - 4, 4, 1))     # rows that overlap: copied, still scored
    assert s.compute_ssimu2_rgba(bad, bad, 0) == 100.0
    with pytest.raises(Ssimu2Error) as ei:                   # the C check itself
        s._call(s._L.ssimu2_set_reference_rgba8, scorer_mod._u8p(ref4), 4 * w - 1, w, h, 0)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(Ssimu2Error) as ei:
        s._call(s._L.ssimu2_set_reference_rgba8, scorer_mod._u8p(ref4), 4 * w, w, h, 0x01000000)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(Ssimu2Error) as ei:
        s._call(s._L.ssimu2_set_reference_rgba8, scorer_mod._u8p(ref4), 4 * w, 0, h, 0)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    # a context of the product library has none of it
    for call in (lambda: scorer.composite_rgba(ref4, 0), lambda: scorer.compute_ssimu2_rgba(ref4, ref4, 0),
                 lambda: scorer.set_reference_rgba(ref4, 0), lambda: scorer.score_against_reference_rgba(ref4)):
        with pytest.raises(Ssimu2Error) as ei:
            call()
        assert ei.value.code == _lib.ERR_UNSUPPORTED and "extended=True" in str(ei.value)


def test_a_context_without_rgba_calls_allocates_nothing_new(hip_lib):
    import torch
    w, h = 1920, 1080
    ref = synth.make_ref(w, h, seed=4)
    dist = synth.distort(ref, "blockq", 2)
    torch.cuda.synchronize()

    def work(s):
        s.set_reference(ref)
        s.score_against_reference(dist)
        s.compute_ssimu2(ref, dist)

    for extended in (False, True):      # each library's code object is on the device before anything is measured
        with Ssimu2(0, extended=extended) as s:
            s.compute_ssimu2(ref[:16, :16].copy(), dist[:16, :16].copy())
    with Ssimu2(0) as s:
        work(s)
        work(s)
        free_plain = torch.cuda.mem_get_info(0)[0]
    with Ssimu2(0, extended=True) as s:
        work(s)
        work(s)
        assert abs(torch.cuda.mem_get_info(0)[0] - free_plain) <= (8 << 20)
        before = torch.cuda.mem_get_info(0)[0]
        s.compute_ssimu2_rgba(rgba_of(ref, 255), rgba_of(dist, 255), 0)
        assert torch.cuda.mem_get_info(0)[0] < before       # ... the first RGBA call does


# ---- (h) the scoring service does not serve these calls ------------------------------------------------------------
def test_a_service_context_refuses_rgba_and_scores_on(hip_lib):
    from oavif_amd import service
    w, h = 121, 41
    rgb = gpu_cases.content("text", w, h, seed=2)
    dist = synth.distort(rgb, "blockq", 2)
    ref4 = rgba_of(rgb, alpha_plane("disc", w, h, 0))
    svc = service.start(max_lifetime=600)
    try:
        with Ssimu2(0, extended=True, service=svc.socket) as remote:
            before = remote.compute_ssimu2(rgb, dist)
            for call in (lambda: remote.composite_rgba(ref4, 0), lambda: remote.compute_ssimu2_rgba(ref4, ref4, 0),
                         lambda: remote.set_reference_rgba(ref4, 0), lambda: remote.score_against_reference_rgba(ref4)):
                with pytest.raises(Ssimu2Error) as ei:
                    call()
                assert ei.value.code == _lib.ERR_UNSUPPORTED
            assert remote.compute_ssimu2(rgb, dist) == before
            remote.set_reference(rgb)
            assert remote.score_against_reference(rgb) == 100.0
        with Ssimu2(0) as local:
            assert local.compute_ssimu2(rgb, dist) == before
    finally:
        assert svc.stop(timeout=30) == 0


# ---- (i) the search ------------------------------------------------------------------------------------------------
def test_search_of_an_rgba_source(ctxs, oracle, table):
    from oavif_amd import alpha, avif_bridge as ab, cli
    if not ab.available():
        pytest.skip(f"libavif bridge unavailable: {ab.why_unavailable()}")
    s = ctxs["fir"]
    w, h, bg = 256, 192, 0xE6E6E6
    rgb = synth.make_ref(w, h, seed=21)
    a = alpha_plane("disc", w, h, 0)
    src = rgba_of(rgb, a)
    src[a == 0, :3] = np.random.default_rng(3).integers(0, 256, (int((a == 0).sum()), 3))   # noise nobody sees
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.quality_alpha = False, 10, 90
    r = alpha.search_rgba(src, o, bg, scorer=s, score_tgt=80.0, tolerance=2.0, max_pass=6)
    assert 1 <= r.num_pass == len(r.history) <= 6 and 0 <= r.q <= 100
    assert (r.q, r.score) in r.history and r.last_avif_size > 0
    assert all(np.isfinite(sc) and sc <= 100.0 for _q, sc in r.history)
    by_q = {}
    for q, sc in r.history:
        assert by_q.setdefault(q, sc) == sc              # one quantizer, one score
    # the chosen quantizer once more, scored by hand: numpy codes -> checker
    with ab.EncoderSource(src, 8, o) as enc, ab.decode_common(enc.encode(o, r.q)) as frame:
        assert frame.channels == 4
        dec = np.array(frame.pixels(), copy=True)
    cr, cd = codes_of(src, bg), codes_of(dec, bg)
    exp = expected(oracle, table, ("search", r.q), cr, cd, gpu_cases.MODES["fir"][1])
    print(f"measured: search q {r.q}: score {r.score!r}, checker {exp[0]!r}")
    assert abs(r.score - exp[0]) <= gpu_cases.score_tol(exp[0]), (r.score, exp[0])
