"""The checker against an independent fp64 SSIMULACRA2 (tests/ssimu2_fp64.py), CPU only.

Every device test compares the kernels with the checker, and the kernels equal the checker stage by stage, so a
mistake in the checker's statement of the operation (a constant, an edge rule, the scale loop, a formula) would pass
everything else.  Here the checker is held to a restatement that shares no code with it: first the reference
itself is pinned (its taps, its blur, identical frames, the scale count), then the checker stage by stage, then
scores and averages on the fixtures, the kernels' size grid, content kinds, extreme frames and one frame 65,600 px
long, and finally the bounds are shown to be tight enough: every structural variant of a stage misses them, every
last-bit variant meets them.  Bounds and measures: tests/fp64_checks.py, measured by tests/tools/cpu_fp64_campaign.py.
"""
import os
import sys

import numpy as np
import pytest

from oavif_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import fp64_checks as fc  # noqa: E402
import ssimu2_fp64 as R  # noqa: E402
from gpu_cases import SIZES, content  # noqa: E402

_REF = {}   # case name -> R.evaluate result


def _reference(name, ref, dist):
    if name not in _REF:
        _REF[name] = R.evaluate(ref, dist)
    return _REF[name]


# ---- the reference itself ------------------------------------------------------------------------------------------

def test_taps_equal_the_checkers_fp64_taps(oracle):
    t = R.taps()
    t64, _t32, _n2, _d1 = oracle.gauss_taps()
    assert np.abs(t[4:] - t64).max() <= 1e-12
    assert np.abs(t[::-1] - t).max() <= 1e-15 and abs(t.sum() - 1.0) <= 1e-12
    # the recursion's impulse response is exactly 9 taps long: nothing beyond offset 4
    imp = np.zeros(61)
    imp[30] = 1.0
    resp = R.recursive_blur_line(imp)
    assert np.abs(np.delete(resp, range(26, 35))).max() <= 1e-14


@pytest.mark.parametrize("h,w", [(1, 1), (2, 9), (9, 2), (13, 11)])
def test_blur_is_the_direct_zero_padded_convolution(h, w):
    p = np.random.default_rng(h * 31 + w).random((h, w))
    t = R.taps()
    k = np.outer(t, t)
    exp = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            for dy in range(-4, 5):
                for dx in range(-4, 5):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        exp[y, x] += k[dy + 4, dx + 4] * p[y + dy, x + dx]
    assert np.abs(R.blur(p) - exp).max() <= 1e-15


def test_identical_frames_score_exactly_100():
    for w, h, seed in ((64, 48, 1), (131, 173, 2), (8, 8, 3)):
        img = synth.make_ref(w, h, seed)
        e = R.evaluate(img, img.copy())
        assert e["score"] == 100.0 and not e["averages"].any() and e["nscales"] >= 1


def test_scale_count_table():
    """The table of tests/test_oracle.py::test_scale_count_and_small_images."""
    for (w, h, expect) in [(7, 50, 0), (8, 8, 2), (15, 9, 2), (16, 16, 3), (64, 64, 5),
                           (112, 112, 5), (113, 113, 6), (128, 128, 6), (127, 300, 6), (300, 100, 5)]:
        assert R.nscales_of(w, h) == expect, (w, h)
        ref = synth.make_ref(w, h, 3)
        e = R.evaluate(ref, synth.distort(ref, "noise", 3))
        assert e["nscales"] == expect and not e["averages"][expect:].any(), (w, h)
        assert (e["score"] == 100.0) == (expect == 0)


# ---- the checker against the reference, stage by stage --------------------------------------------------------------

def test_srgb_table_is_the_fp32_of_the_fp64_curve(oracle):
    assert np.array_equal(oracle.srgb_lut(), R.srgb_to_linear(np.arange(256)).astype(np.float32))


def test_xyb_of_every_rgb8_colour(oracle):
    lut = oracle.srgb_lut()
    v = np.arange(1 << 24, dtype=np.uint32)
    worst = 0.0
    for lo in range(0, 1 << 24, 1 << 21):
        c = v[lo:lo + (1 << 21)]
        rgb = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255]).reshape(3, 1, -1)
        got = oracle.linear_to_xyb(lut[rgb])
        worst = max(worst, float(np.abs(got - R.to_xyb(R.srgb_to_linear(rgb))).max()))
    assert worst <= fc.XYB_ABS, worst


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (2, 2), (8, 8), (9, 13), (131, 173)])
def test_downsample2(oracle, h, w):
    p = np.random.default_rng(h + 100 * w).random((3, h, w)).astype(np.float32)
    got = oracle.downsample2(p)
    exp = R.downsample2(p.astype(np.float64))
    assert got.shape == exp.shape == (3, (h + 1) // 2, (w + 1) // 2)
    ulp = np.spacing(np.abs(exp).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - exp) / ulp).max() <= fc.DOWNSAMPLE_ULP


def _blur_planes(oracle):
    rng = np.random.default_rng(7)
    out = []
    for h, w in [(1, 1), (2, 9), (9, 2), (13, 11), (64, 64), (217, 333)]:
        out.append(rng.random((h, w)).astype(np.float32))
        xyb = oracle.linear_to_xyb(oracle.srgb_lut()[synth.make_ref(w, h, h + w)].transpose(2, 0, 1))
        out += [xyb[0], xyb[1], xyb[2]]
    return out


def test_blur_fir_and_exact(oracle):
    for p in _blur_planes(oracle):
        got = oracle.blur_plane(p, oracle.BLUR_FIR)
        assert np.abs(got - R.blur(p)).max() <= fc.BLUR_REL["fir"] * np.abs(p).max(), p.shape
        # products as the score forms them; OR_BLUR_EXACT exists for products only
        sq = R.blur(p.astype(np.float64) ** 2)
        for mode, key in ((oracle.BLUR_FIR, "fir"), (oracle.BLUR_EXACT, "exact")):
            got = oracle.blur_product(p, p, mode)
            assert np.abs(got - sq).max() <= fc.BLUR_REL[key] * np.square(p).max(), (p.shape, key)


@pytest.mark.parametrize("n", [16, 256, 4096])
def test_blur_recursive_error_grows_with_the_line_only(oracle, n):
    """The fp32 recursion's error random-walks along a line: bounded by a constant times sqrt(line length)."""
    rng = np.random.default_rng(n)
    for shape in ((24, n), (n, 24)):
        p = (0.3 + 0.1 * rng.random(shape)).astype(np.float32)
        exp = R.blur(p)
        for mode in (oracle.BLUR_IIR, oracle.BLUR_IIR_FMA):
            err = np.abs(oracle.blur_plane(p, mode) - exp).max() / np.abs(p).max()
            assert err <= fc.IIR_REL_PER_SQRT_LINE * np.sqrt(max(shape)), (shape, mode, err)


# ---- scores and averages --------------------------------------------------------------------------------------------

def _extreme_pairs():
    h, w = 70, 90
    black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    prim = content("primaries", w, h, 0)
    one = synth.make_ref(w, h, 9)
    one_px = one.copy()
    one_px[h // 2, w // 3] ^= np.uint8(0x40)
    corner = one.copy()
    corner[0, 0] = 255 - corner[0, 0]
    return {"black-white": (black, white), "white-black": (white, black), "primaries-black": (prim, black),
            "primaries-rolled": (prim, np.roll(prim, 5, axis=1)), "one-pixel": (one, one_px),
            "one-corner-pixel": (one, corner)}


def _cases(golden):
    arrays, meta = golden
    out = {f"golden-{p['name']}": (arrays["ref"], arrays[p["name"]]) for p in meta["pairs"]}
    out["golden-odd"] = (arrays["odd_ref"], arrays["odd_dist"])
    for w, h in SIZES:
        ref = synth.make_ref(w, h, 17 * w + h)     # the pairs of tests/test_gpu_mode_matrix.py
        out[f"size-{w}x{h}"] = (ref, synth.distort(ref, "noise", 2, seed=w + 3 * h))
    for kind in ("gradient", "primaries", "checker", "text", "noise"):
        ref = content(kind, 250, 190, 5)
        out[f"content-{kind}"] = (ref, synth.distort(ref, "band", 2, seed=3))
    out.update({f"extreme-{k}": v for k, v in _extreme_pairs().items()})
    ref = synth.make_ref(1920, 1080, 3000)
    out["1080p"] = (ref, synth.distort(ref, "blockq", 1, seed=3))
    w, h = 65_600, 9                               # W1 of tests/test_gpu_long_frames.py: the checker is the reference there
    ref = synth.make_ref(w, h, 17 * w + h)
    out[f"long-{w}x{h}"] = (ref, synth.distort(ref, "noise", 2, seed=w + 3 * h))
    return out


def _kind(name):
    """gpu_cases.content kinds and the flat extreme frames are "synthetic" (fc: fp32 noise as large as the signal)"""
    return "synthetic" if name.startswith("content") or (name.startswith("extreme") and "pixel" not in name) \
        else "natural"


CASE_GROUPS = ["golden", "size", "content", "extreme", "1080p", "long"]


@pytest.mark.parametrize("group", CASE_GROUPS)
def test_checker_scores_and_averages_against_the_reference(oracle, golden, group):
    """FIR and EXACT everywhere; the recursive orders where the frame is small enough for their bounds to mean
    something (fc.IIR_MAX_PIXELS)."""
    for name, (ref, dist) in _cases(golden).items():
        if not name.startswith(group):
            continue
        exp = _reference(name, ref, dist)
        h, w, _ = ref.shape
        modes = {"fir": oracle.BLUR_FIR, "exact": oracle.BLUR_EXACT}
        if w * h <= fc.IIR_MAX_PIXELS:
            modes.update(recursive=oracle.BLUR_IIR, recursive_fma=oracle.BLUR_IIR_FMA)
        for mode, blur in modes.items():
            s, avg, ns = oracle.compute_ssimu2(ref, dist, blur, omp=w * h > 10 ** 6, return_averages=True)
            fc.check(s, avg, ns, exp, mode, f"{name} {mode}", _kind(name))
            if exp["nscales"] == 0 or np.array_equal(ref, dist):
                assert s == exp["score"] == 100.0, name


def test_reference_error_map_against_the_fp32_map(oracle, golden):
    """errmap_ref's fp32 map (the device map's own reference) against the fp64 map of section 9: per pixel relative to
    the peak, and the mean is sum w_i |a_i| when the frame divides into whole pixels at every scale."""
    arrays, meta = golden
    for ref, dist in ((arrays["ref"], arrays["avif_q49"]), (arrays["odd_ref"], arrays["odd_dist"])):
        m64, e = R.error_map(ref, dist)
        m32, _own, ns = errmap_ref.reference_map(oracle, ref, dist, oracle.BLUR_FIR)
        assert ns == e["nscales"]
        assert np.abs(m32 - m64).max() <= fc.MAP_PIXEL_REL["fir"] * m64.max()
        h, w, _ = ref.shape
        if w % (1 << (ns - 1)) == 0 and h % (1 << (ns - 1)) == 0:
            assert abs(m64.mean() - e["weighted_sum"]) <= 1e-12 * e["weighted_sum"]
            assert abs(m32.mean(dtype=np.float64) - e["weighted_sum"]) <= fc.MAP_MEAN_REL["fir"] * e["weighted_sum"]


def _scale_parts(oracle, tm, coef, w, h):
    """errmap_ref.compose scale by scale: -> each scale's density at full resolution (their sum in order is compose's
    map: 0 + x is x exactly)."""
    parts = []
    for s in range(len(tm)):
        only = np.zeros_like(coef)
        only[s] = coef[s]
        parts.append(errmap_ref.compose(tm, only, w, h))
    return parts


def _wrong_maps(oracle, tm, avg, e, w, h):
    """Two structurally wrong fp32 FIR maps: -> {name: map}.  "shifted": the density of scale 1 taken at (x >> 1) + 1,
    clamped to the scale's last column (an off-by-one in k_map_compose's gather).  "dropped": the artifact L4
    coefficient of one channel at one scale left 0 -- the one whose term w_i a_i weighs most in the reference's sum, so
    that the variant is a wrong map and not the drop of a zero weight."""
    ns = len(tm)
    coef = errmap_ref.coefficients(oracle, avg, ns)
    parts = _scale_parts(oracle, tm, coef, w, h)
    xs = np.arange(w)
    w1 = (w + 1) // 2
    src = np.minimum((xs >> 1) + 1, w1 - 1) << 1
    shifted = np.zeros((h, w), np.float32)
    for s, p in enumerate(parts):
        shifted = shifted + (p[:, src] if s == 1 else p)
    art_l4 = [(wt * abs(e["averages"][s, st]), s, st) for wt, s, st in R.weight_walk(ns) if st >= 6 and (st - 6) % 4 == 1]
    _top, s_drop, st_drop = max(art_l4)
    less = coef.copy()
    less[s_drop, st_drop] = 0
    return {"shifted": shifted, "dropped": errmap_ref.compose(tm, less, w, h)}


def test_reference_error_map_of_16_bit_frames_against_the_fp32_map(oracle):
    """hbd_ref.error_map_fp32 (the 16-bit device map's own reference: bit for bit in the recursive modes, within 48 *
    2^-24 in FIR) against hbd_ref.error_map_fp64 on fc.MAP_HBD_CASES, inside fc.MAP_PIXEL_REL_HBD / MAP_MEAN_REL_HBD;
    and those bounds still tell a wrong map from rounding: each structural variant of the FIR map misses the pixel
    bound by fc.DISCRIMINATION_FACTOR on every case.  Measured: FIR pixel 1.1e-3 .. 2.8e-3 of the peak, recursive
    2.1e-2 .. 2.8e-2; the shifted scale misses the FIR pixel bound 9 to 51 times over, the dropped coefficient 28 to
    82 times."""
    import hbd_ref
    for w, h, d in fc.MAP_HBD_CASES:
        ref, dist = fc.map_hbd_pair(w, h, d)
        m64, e = hbd_ref.error_map_fp64(ref, dist, d)
        assert m64.shape == (h, w) and e["nscales"] == R.nscales_of(w, h)
        if fc.map_tiles(w, h, e["nscales"]):
            assert abs(m64.mean() - e["weighted_sum"]) <= 1e-12 * e["weighted_sum"]
        for mode, blur in (("fir", oracle.BLUR_FIR), ("recursive", oracle.BLUR_IIR)):
            m32, tm, avg = hbd_ref.error_map_fp32(oracle, ref, dist, d, blur)
            assert len(tm) == e["nscales"]
            dev = fc.map_deviation(m32, m64, e)
            print(f"measured: {w}x{h} {d}-bit {mode}: " + fc.map_deviation_text(dev, fc.MAP_PIXEL_REL_HBD[mode],
                                                                                 fc.MAP_MEAN_REL_HBD[mode]))
            assert dev["pixel"] <= fc.MAP_PIXEL_REL_HBD[mode], (w, h, d, mode, dev)
            assert dev["mean"] is None or dev["mean"] <= fc.MAP_MEAN_REL_HBD[mode], (w, h, d, mode, dev)
            if mode == "fir":
                for name, wrong in _wrong_maps(oracle, tm, avg, e, w, h).items():
                    miss = fc.map_deviation(wrong, m64, e)["pixel"] / fc.MAP_PIXEL_REL_HBD["fir"]
                    print(f"measured: {w}x{h} {d}-bit variant {name}: {miss:.1f} x the pixel bound")
                    assert miss >= fc.DISCRIMINATION_FACTOR, (w, h, d, name, miss)


# ---- discrimination: the bounds tell a wrong operation from fp32 rounding --------------------------------------------

STRUCTURAL = {"edge_clamp": 0x1, "edge_mirror": 0x2, "gauss9": 0x4, "gauss11": 0x8, "downsample_xyb": 0x10,
              "downsample_floor": 0x20, "size_test_after": 0x40}
LAST_BIT = {"srgb_powf": 0x80, "cbrt_libm": 0x100, "sums_f32": 0x200, "prodfirst": 0}


def test_structural_variants_miss_the_bounds_and_last_bit_variants_meet_them(oracle, golden):
    """Every single-stage variant of the checker (tests/golden/pin_kit's catalogue) on every golden fixture where it
    changes the computation: a structural one (another edge rule, another Gaussian, another pyramid) misses at least
    one FIR check by fc.DISCRIMINATION_FACTOR; a last-bit one (another fp32 rounding) meets all of them.  If the FIR
    bounds are loosened far enough to let a wrong operation through, this fails."""
    arrays, meta = golden
    fixtures = {p["name"]: (arrays["ref"], arrays[p["name"]]) for p in meta["pairs"] if p["name"] != "identical"}
    fixtures["odd"] = (arrays["odd_ref"], arrays["odd_dist"])
    for name, (ref, dist) in fixtures.items():
        exp = _reference(f"golden-{name}", ref, dist)
        odd = any(n % 2 for n in ref.shape[:2])
        for var, bit in STRUCTURAL.items():
            if var == "downsample_floor" and not odd:
                continue                                     # floor and ceil halving agree on even sizes
            s, avg, ns = oracle.compute_ssimu2_variant(ref, dist, oracle.BLUR_FIR, bit, return_averages=True)
            r = fc.ratios(fc.deviation(s, avg, ns, exp), exp, "fir")
            assert max(r.values()) >= fc.DISCRIMINATION_FACTOR, (name, var, r)
        for var, bit in LAST_BIT.items():
            blur = oracle.BLUR_FIR_PRODFIRST if var == "prodfirst" else oracle.BLUR_FIR
            s, avg, ns = oracle.compute_ssimu2_variant(ref, dist, blur, bit, return_averages=True)
            r = fc.ratios(fc.deviation(s, avg, ns, exp), exp, "fir")
            assert max(r.values()) <= 1.0, (name, var, r)
