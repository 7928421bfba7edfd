"""The timing hooks of the instrumented build on the MI355X (include/ssimu2_hip_internal.h: ssimu2_time_device,
ssimu2_time_stage, ssimu2_time_march_rotating, ssimu2_time_blur_stage_rotating, ssimu2_time_kernels,
ssimu2_measure_read_stream), on an instrumented context of this module's own.

136 x 24 is the smallest frame with a pyramid, more than one scale in a plan and a ragged strip: three scales
(136 x 24, 68 x 12, 34 x 6), two strips of which the second is partial.  Every hook succeeds there with a finite
duration >= 0, and the context scores afterwards -- a pair, and a pass against a reference set anew -- with the bits of
a fresh product context: the hooks overwrite the reference's linear pyramid and drop the reference, and leave nothing
else behind.  7 x 7 has no scale: the hooks that launch per workgroup launch nothing, report 0 bytes, and a score
afterwards is exactly 100."""
import math
import os
import sys

import numpy as np
import pytest

from oavif_amd import Ssimu2, _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_cases import bits_equal, on_device  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 136, 24
BLUR_BYTES = 2 * 4 * 3 * (136 * 24 + 68 * 12 + 34 * 6)  # every plane element of the three scales read once, written once
STAGES = (_lib.STAGE_PYRAMID, _lib.STAGE_MARCH, _lib.STAGE_FINALIZE)


def packed(frames):
    """Same-size frames back to back on the device -> (the tensor that owns them, the device address of each frame)."""
    size = frames[0].size
    buf = on_device(frames, size)
    return buf, [buf.data_ptr() + k * size for k in range(len(frames))]


def duration(ms):
    assert math.isfinite(ms) and ms >= 0.0, ms


@pytest.fixture(scope="module")
def hooks(hip_lib):
    """An instrumented context of this module's own, two 136 x 24 pairs on the device, and what a fresh product context
    returns for the first pair: (score, averages) of the pair score and of a pass against the reference."""
    ref = synth.make_ref(W, H, 11)
    ref2 = synth.make_ref(W, H, 12)
    frames = [ref, synth.distort(ref, "blockq", 2, seed=11), ref2, synth.distort(ref2, "noise", 2, seed=12)]
    fresh = Ssimu2(0)
    try:
        pair = (fresh.compute_ssimu2(frames[0], frames[1]), fresh.last_averages()[0])
        fresh.set_reference(frames[0])
        cached = (fresh.score_against_reference(frames[1]), fresh.last_averages()[0])
    finally:
        fresh.close()
    assert 0.0 < pair[0] < 100.0
    buf, addrs = packed(frames)
    s = Ssimu2(0, instrumented=True)
    yield s, frames, addrs, pair, cached
    s.close()
    del buf


def scores_as_fresh(s, frames, pair, cached, what):
    score = s.compute_ssimu2(frames[0], frames[1])
    bits_equal(score, s.last_averages()[0], pair[0], pair[1], f"pair score after {what}")
    s.set_reference(frames[0])
    score = s.score_against_reference(frames[1])
    bits_equal(score, s.last_averages()[0], cached[0], cached[1], f"pass against the reference after {what}")


def hook_time_device(s, a, pair):
    ms, score = s.time_device(a[0], a[1], W, H, 2)
    duration(ms)
    assert np.float64(score).tobytes() == np.float64(pair[0]).tobytes()


def hook_time_stage(s, a, pair):
    for stage in STAGES:
        duration(s.time_stage(a[0], a[1], W, H, stage, 2))


def hook_time_march_rotating(s, a, pair):
    duration(s.time_march_rotating([a[0], a[2]], [a[1], a[3]], W, H, 3))


def hook_time_blur_stage_rotating(s, a, pair):
    ms, nbytes = s.time_blur_stage_rotating([a[0], a[2]], W, H, 3)
    duration(ms)
    assert nbytes == BLUR_BYTES == 102816


def hook_time_kernels_pair(s, a, pair):
    times, wall_timed, wall_plain = s.time_kernels(W, H, [a[1], a[3]], 2, d_refs=[a[0], a[2]])
    assert tuple(times) == ("pyramid", "march", "finalize") and s.last_march() == "k_march"
    for ms in list(times.values()) + [wall_timed, wall_plain]:
        duration(ms)


def hook_time_kernels_cached(s, a, pair):
    times, wall_timed, wall_plain = s.time_kernels(W, H, [a[1], a[3]], 2, d_ref=a[0])
    assert tuple(times) == ("pyramid", "march_refblur", "finalize") and s.last_march() == "k_march_refblur"
    for ms in list(times.values()) + [wall_timed, wall_plain]:
        duration(ms)


def hook_measure_read_stream(s, a, pair):
    gbs = s.measure_read_stream(1 << 20, 2)
    assert math.isfinite(gbs) and gbs > 0.0, gbs   # bytes over a duration: finite exactly when that is positive


HOOKS = [hook_time_device, hook_time_stage, hook_time_march_rotating, hook_time_blur_stage_rotating,
         hook_time_kernels_pair, hook_time_kernels_cached, hook_measure_read_stream]


@pytest.mark.parametrize("hook", HOOKS, ids=lambda f: f.__name__[5:])
def test_hook_runs_and_leaves_the_context_scoring_as_a_fresh_one(hooks, hook):
    s, frames, addrs, pair, cached = hooks
    hook(s, addrs, pair)
    scores_as_fresh(s, frames, pair, cached, hook.__name__[5:])


def test_hooks_on_a_frame_without_a_scale(hooks):
    """7 x 7: no scale, no workgroup of the marching body.  The hooks answer with a duration and 0 bytes per launch."""
    s = hooks[0]
    ref = synth.make_ref(7, 7, 3)
    dist = synth.distort(ref, "noise", 3, seed=3)
    buf, a = packed([ref, dist])
    for stage in STAGES:
        duration(s.time_stage(a[0], a[1], 7, 7, stage, 2))
    duration(s.time_march_rotating([a[0], a[1]], [a[1], a[0]], 7, 7, 3))
    ms, nbytes = s.time_blur_stage_rotating([a[0], a[1]], 7, 7, 3)
    duration(ms)
    assert nbytes == 0.0
    assert s.compute_ssimu2(ref, dist) == 100.0
    del buf
