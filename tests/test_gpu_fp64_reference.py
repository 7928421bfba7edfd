"""The HIP kernels against the independent fp64 SSIMULACRA2 of tests/ssimu2_fp64.py (-m gpu only).

Every other device test compares the kernels with the checker, which they equal stage by stage; these hold them to
a statement of the operation that shares no code with either.  Scores and all 108 averages in the three blur modes
over the kernels' size grid, content kinds and extreme frames (plus one cached-reference call per case); the
instrumented build's intermediate planes; FIR scores at 1080p and 4K; and the error map.  Bounds: tests/fp64_checks.py
(measured on CPU through the checker, whose planes are the device's bits; tests/tools/cpu_fp64_campaign.py).  The
recursive modes are held to their bounds only up to fc.IIR_MAX_PIXELS, beyond which fp32 recursion noise is as large
as a wrong stage.
"""
import os
import sys

import numpy as np
import pytest

from oavif_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_checks as fc  # noqa: E402
import ssimu2_fp64 as R  # noqa: E402
from gpu_cases import MODES, SIZES, content, contexts_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _reference(key, ref, dist):
    if key not in _REF:
        _REF[key] = R.evaluate(ref, dist)
    return _REF[key]


ctxs = contexts_fixture()


def _cases(group):
    if group == "size":
        for w, h in SIZES:
            ref = synth.make_ref(w, h, 17 * w + h)
            yield f"{w}x{h}", "natural", ref, synth.distort(ref, "noise", 2, seed=w + 3 * h)
    elif group == "content":
        for kind in ("gradient", "primaries", "checker", "text", "noise"):
            ref = content(kind, 250, 190, 5)
            yield kind, "synthetic", ref, synth.distort(ref, "band", 2, seed=3)
    else:
        h, w = 70, 90
        black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
        prim = content("primaries", w, h, 0)
        one = synth.make_ref(w, h, 9)
        one_px = one.copy()
        one_px[h // 2, w // 3] ^= np.uint8(0x40)
        for name, (a, b) in {"black-white": (black, white), "white-black": (white, black),
                             "primaries-black": (prim, black), "primaries-rolled": (prim, np.roll(prim, 5, axis=1)),
                             "one-pixel": (one, one_px)}.items():
            yield name, "natural" if name == "one-pixel" else "synthetic", a, b


@pytest.mark.parametrize("group", ["size", "content", "extreme"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_scores_and_averages_against_the_fp64_reference(ctxs, mode, group):
    s = ctxs[mode]
    for name, kind, ref, dist in _cases(group):
        h, w, _ = ref.shape
        if mode != "fir" and w * h > fc.IIR_MAX_PIXELS:
            continue
        exp = _reference((group, name), ref, dist)
        got = s.compute_ssimu2(ref, dist)
        avg, ns = s.last_averages()
        fc.check(got, avg, ns, exp, mode, f"{mode} {group} {name}", kind)
        s.set_reference(ref)
        cached = s.score_against_reference(dist)
        avg_c, ns_c = s.last_averages()
        fc.check(cached, avg_c, ns_c, exp, mode, f"{mode} {group} {name} cached", kind)


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_large_fir_scores_against_the_fp64_reference(ctxs, w, h):
    ref = synth.make_ref(w, h, w + h)
    dist = synth.distort(ref, "noise", 1, seed=3)
    exp = R.evaluate(ref, dist)
    got = ctxs["fir"].compute_ssimu2(ref, dist)
    avg, ns = ctxs["fir"].last_averages()
    fc.check(got, avg, ns, exp, "fir", f"{w}x{h}", "natural")


@pytest.mark.parametrize("w,h", [(121, 9), (333, 217), (1921, 1083), (3840, 2160)])
def test_instrumented_planes_against_the_fp64_reference(iscorer, hip_lib, w, h):
    """Linear pyramid levels of both frames (what 0 / 1), the cached XYB planes (2) and the FIR blur of ref * ref (3)
    at every scale; the recursive planes after the horizontal pass and after both (4 / 5) at scale 0."""
    from oavif_amd import Ssimu2
    ref = synth.make_ref(w, h, 5 * w + h)
    dist = synth.distort(ref, "blockq", 2, seed=4)
    ns = R.nscales_of(w, h)
    lv = fc.reference_levels(ref, dist, list(range(ns)))
    iscorer.compute_ssimu2(ref, dist)
    for s in range(1, ns):
        for what in (0, 1):
            got = iscorer.debug_download(what, s, w, h)
            assert fc.lin_ulps(got, lv[s][what]) <= fc.PLANE_LIN_ULPS, (what, s)
    iscorer.set_reference(ref)
    for s in range(ns):
        got = iscorer.debug_download(2, s, w, h)
        assert fc.abs_dev(got, lv[s][2]) <= fc.XYB_ABS, (2, s)
        got = iscorer.debug_download(3, s, w, h)
        for c in range(3):
            assert fc.rel_dev(got[c], R.blur(lv[s][2][c] ** 2)) <= fc.PLANE_FIR_REL, (3, s, c)
    bound = fc.RG_REL0 + fc.IIR_REL_PER_SQRT_LINE * np.sqrt(w + h)
    with Ssimu2(0, instrumented=True, blur=_lib.BLUR_RECURSIVE) as rs:
        rs.rg_stop_after_scale(0)
        rs.compute_ssimu2(ref, dist)
        for what, vertical in ((4, False), (5, True)):
            got = rs.debug_download(what, 0, w, h)
            exp = fc.rg_reference(lv[0][2], lv[0][3], vertical)
            for k in range(15):
                assert fc.rel_dev(got[k], exp[k]) <= bound, (what, k)
        rs.rg_stop_after_scale(-1)


@pytest.mark.parametrize("w,h", [(128, 96), (131, 173), (640, 352)])
@pytest.mark.parametrize("mode", ["fir", "recursive"])
def test_error_map_against_the_fp64_map(ctxs, mode, w, h):
    """Device map against the section-9 map in fp64: per pixel relative to its peak; its mean against
    sum w_i |a_i| of the reference when every scale tiles the frame (w, h multiples of 2^(nscales - 1))."""
    ref = synth.make_ref(w, h, w * h)
    dist = synth.distort(ref, "blockq", 2, seed=7)
    m64, e = R.error_map(ref, dist)
    _score, m = ctxs[mode].error_map(ref, dist)
    assert m.shape == m64.shape
    assert np.abs(m - m64).max() <= fc.MAP_PIXEL_REL[mode] * m64.max()
    ns = e["nscales"]
    if w % (1 << (ns - 1)) == 0 and h % (1 << (ns - 1)) == 0:
        assert abs(m.mean(dtype=np.float64) - e["weighted_sum"]) <= fc.MAP_MEAN_REL[mode] * e["weighted_sum"]


mctxs = contexts_fixture(maps=True, extended=True, yuv=True)
_REF_MAP16 = {}


@pytest.mark.parametrize("w,h,d", fc.MAP_HBD_CASES, ids=[f"{w}x{h}-{d}bit" for w, h, d in fc.MAP_HBD_CASES])
@pytest.mark.parametrize("mode", ["fir", "recursive"])
def test_error_map_of_16_bit_frames_against_the_fp64_map(mctxs, mode, w, h, d):
    """error_map_hbd against hbd_ref.error_map_fp64, which shares no code with the kernels or with tests/errmap_ref.py:
    per pixel relative to the fp64 map's peak, and the mean against sum w_i |a_i| where every scale tiles the frame, in
    the 16-bit bounds of tests/fp64_checks.py (tests/test_fp64_reference.py shows that they tell a wrong map from
    rounding).  The fp64 map is computed once per case."""
    import hbd_ref
    ref, dist = fc.map_hbd_pair(w, h, d)
    if (w, h, d) not in _REF_MAP16:
        _REF_MAP16[w, h, d] = hbd_ref.error_map_fp64(ref, dist, d)
    m64, e = _REF_MAP16[w, h, d]
    _score, m = mctxs[mode].error_map_hbd(ref, dist, d)
    assert mctxs[mode].last_averages()[1] == e["nscales"]
    dev = fc.map_deviation(m, m64, e)
    print(f"measured: {mode} {w}x{h} {d}-bit: " + fc.map_deviation_text(dev, fc.MAP_PIXEL_REL_HBD[mode],
                                                                         fc.MAP_MEAN_REL_HBD[mode]))
    assert dev["pixel"] <= fc.MAP_PIXEL_REL_HBD[mode], (mode, w, h, d, dev)
    assert dev["mean"] is None or dev["mean"] <= fc.MAP_MEAN_REL_HBD[mode], (mode, w, h, d, dev)
