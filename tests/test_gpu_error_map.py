"""The per-pixel error map on the MI355X (ssimu2_error_map_*), in the FIR mode and in both evaluation orders of the
published recursion, against the numpy reference of tests/errmap_ref.py."""
import os
import sys
import time

import numpy as np
import pytest

from oavif_amd import _lib, synth
from oracle import ssimu2_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import errmap_ref  # noqa: E402
import gpu_cases  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"fir": (_lib.BLUR_FIR, orc.BLUR_FIR), "recursive": (_lib.BLUR_RECURSIVE, orc.BLUR_IIR),
         "recursive_fma": (_lib.BLUR_RECURSIVE_FMA, orc.BLUR_IIR_FMA)}   # (scorer mode, oracle BLUR_*)


@pytest.fixture(scope="module", params=sorted(MODES))
def mode(request, hip_lib):
    from oavif_amd import Ssimu2
    s = Ssimu2(0, blur=MODES[request.param][0])
    yield request.param, s, MODES[request.param][1]
    s.close()


def _check_against_reference(oracle, s, blur, ref, dist, what):
    """The map pixel by pixel (gpu_cases.check_map: bit for bit in the recursive modes, within MAP_K * 2^-24 in FIR),
    its mean, and the score's averages and k_finalize against the same terms (gpu_cases.check_against_terms)."""
    score, m = s.error_map(ref, dist)
    avg, ns = s.last_averages()
    mode = next(k for k, v in MODES.items() if v[1] == blur)
    _worst, own = gpu_cases.check_map(oracle, m, avg, ns, ref, dist, blur, what)
    gpu_cases.check_against_terms(oracle, score, avg, ns, ref, dist, mode, what, kavg=own)
    return score, m


def test_map_matches_the_reference_on_the_golden_pairs(mode, oracle, golden):
    name, s, blur = mode
    arrays, _meta = golden
    ref = arrays["ref"]
    for k in ("avif_q20", "avif_q65", "blockq2", "noise1", "blur1"):
        _check_against_reference(oracle, s, blur, ref, arrays[k], f"{name} {k}")
    _check_against_reference(oracle, s, blur, arrays["odd_ref"], arrays["odd_dist"], f"{name} odd")


# 4160 x 75: five scales, 3 * (65 + 33 + 17 + 9 + 5) = 387 jobs of the recursive vertical pass -- more than the device has
# CUs, so its persistent workgroups each take a second job behind the job-tail barrier (1920 x 1080 is 180 jobs) -- and
# scale 0 runs two rounds of the prefetch queue, batches past the image included.
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (33, 17), (129, 67), (4160, 75)])
def test_map_matches_the_reference_on_ragged_and_tiny_sizes(mode, oracle, w, h):
    name, s, blur = mode
    if (w, h) == (4160, 75):
        jobs = 3 * sum(-(-w // (64 << k)) for k in range(5))
        assert jobs == 387 and jobs > s.device_info()["compute_units"]
    ref = synth.make_ref(w, h, seed=w * 7 + h) if min(w, h) >= 2 else np.full((h, w, 3), 77, np.uint8)
    dist = synth.distort(ref, "blockq", 2, seed=5) if min(w, h) >= 2 else np.full((h, w, 3), 200, np.uint8)
    score, m = _check_against_reference(oracle, s, blur, ref, dist, f"{name} {w}x{h}")
    if min(w, h) < 8:  # no scale to score
        assert score == 100.0 and not m.any()
    if (w, h) == (4160, 75):
        assert s.last_averages()[1] == 5


def test_map_matches_the_reference_at_1080p(mode, oracle):
    name, s, blur = mode
    ref = synth.make_ref(1920, 1080, seed=11)
    dist = synth.distort(ref, "blockq", 2, seed=3)
    _check_against_reference(oracle, s, blur, ref, dist, f"{name} 1920x1080")


@pytest.mark.parametrize("group", gpu_cases.HARD_GROUPS)
def test_map_matches_the_reference_on_extreme_content(mode, oracle, group):
    """Black against white, flat against noise, saturated primaries, a 1-px checkerboard, thin text and frames that
    differ in one sample: 60 to 90 of the 108 averages are exactly 0 (coefficient 0), L4 coefficients w / a^3 reach
    3e27, densities span 1e-15 .. 1e3 within one map and fourth powers come close to the subnormal range.  Bit for bit
    in the recursive modes, per pixel within MAP_K * 2^-24 in FIR and 0 exactly where the reference is 0; a second map
    of the same pair has the first one's bits."""
    name, s, blur = mode
    for i, (ref, dist) in enumerate(gpu_cases.group_pairs(group)):
        score, m = _check_against_reference(oracle, s, blur, ref, dist, f"{name} {group} {i}")
        assert np.isfinite(m).all()
        if np.array_equal(ref, dist):
            assert score == 100.0 and not m.any()
        score2, m2 = s.error_map(ref, dist)
        assert score2 == score and np.array_equal(m2.view(np.uint32), m.view(np.uint32)), (name, group, i)


def test_identical_frames_give_a_zero_map(mode):
    _name, s, _blur = mode
    ref = synth.make_ref(256, 160, seed=2)
    score, m = s.error_map(ref, ref)
    assert score == 100.0 and not m.any()


def test_mean_identity_score_bits_and_determinism(mode, oracle):
    _name, s, _blur = mode
    ref = synth.make_ref(384, 256, seed=4)
    dist = synth.distort(ref, "blockq", 3, seed=8)
    plain = s.compute_ssimu2(ref, dist)
    avg_plain, ns = s.last_averages()
    score, m = s.error_map(ref, dist)
    avg, ns2 = s.last_averages()
    assert score == plain and ns2 == ns == 6 and np.array_equal(avg, avg_plain)
    _walk, total = errmap_ref.weighted_terms(oracle, avg, ns)
    assert np.mean(m, dtype=np.float64) == pytest.approx(total, rel=1e-5)
    score2, m2 = s.error_map(ref, dist)
    assert score2 == score and np.array_equal(m2.view(np.uint32), m.view(np.uint32))


def test_against_reference_map_equals_the_pair_map(mode):
    _name, s, _blur = mode
    ref = synth.make_ref(320, 200, seed=6)
    d1 = synth.distort(ref, "blockq", 2, seed=1)
    d2 = synth.distort(ref, "noise", 1, seed=2)
    pair_score, pair_map = s.error_map(ref, d1)
    s.set_reference(ref)
    before = s.score_against_reference(d2)
    avg_before, _ = s.last_averages()
    score, m = s.error_map_against_reference(d1)
    assert score == pair_score and np.array_equal(m.view(np.uint32), pair_map.view(np.uint32))
    assert s.score_against_reference(d2) == before
    assert np.array_equal(s.last_averages()[0], avg_before)


def test_map_is_local(mode):
    _name, s, _blur = mode
    ref = synth.make_ref(512, 512, seed=9)
    far = synth.distort(ref, "blockq", 4, seed=1)
    y0, y1, x0, x1 = 300, 380, 120, 230
    dist = ref.copy()
    dist[y0:y1, x0:x1] = far[y0:y1, x0:x1]
    _score, m = s.error_map(ref, dist)
    _avg, ns = s.last_averages()
    yy, xx = np.unravel_index(int(np.argmax(m)), m.shape)
    assert y0 <= yy < y1 and x0 <= xx < x1, (yy, xx)
    g = (1 << (ns - 1)) * 5
    inside = m[max(y0 - g, 0):y1 + g, max(x0 - g, 0):x1 + g].sum(dtype=np.float64)
    assert inside >= 0.9 * m.sum(dtype=np.float64)


def test_4k_map_time(mode):
    name, s, _blur = mode
    ref = synth.make_ref(3840, 2160, seed=5)
    dist = synth.distort(ref, "blockq", 2)
    s.compute_ssimu2(ref, dist)
    s.error_map(ref, dist)   # first map call allocates
    t0 = time.perf_counter()
    plain = s.compute_ssimu2(ref, dist)
    t1 = time.perf_counter()
    score, m = s.error_map(ref, dist)
    t2 = time.perf_counter()
    assert score == plain and m.shape == (2160, 3840) and np.isfinite(m).all()
    print(f"{name} 4K host call: score {1e3 * (t1 - t0):.2f} ms, score + map {1e3 * (t2 - t1):.2f} ms")


def test_map_memory_is_allocated_on_use_and_returned(hip_lib):
    import torch
    from oavif_amd import Ssimu2
    w, h = 3840, 2160
    ref = synth.make_ref(w, h, seed=1)
    dist = synth.distort(ref, "blockq", 2)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    with Ssimu2(0) as s:
        s.compute_ssimu2(ref, dist)
        free_plain, _ = torch.cuda.mem_get_info(0)
        s.compute_ssimu2(ref, dist)
        assert torch.cuda.mem_get_info(0)[0] == free_plain   # scoring alone allocates nothing more
        s.error_map(ref, dist)
        free_map, _ = torch.cuda.mem_get_info(0)
    free1, _ = torch.cuda.mem_get_info(0)
    extra = free_plain - free_map
    print(f"4K: plain context {(free0 - free_plain) / 2**20:.1f} MiB, map buffers {extra / 2**20:.1f} MiB "
          f"({extra / (w * h):.1f} bytes per pixel)")
    assert 0.9 * 20 * w * h <= extra <= 1.2 * 20 * w * h
    assert free1 >= free0 - (8 << 20)
