"""A plain `bench.py --gpus 1 --steps N --warmup W` does what its headline figure needs and nothing else: set-up, warm-up,
the N timed steps, the line.  Everything else the line can carry is measured only with --full."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("cache_resident", "roofline", "valu_roofline", "stages_ms", "score_roofline", "two_context_ratio",
             "cached_reference", "recursive_blur_mode", "default_search_mode", "by_resolution",
             "ms_per_search_pass_4k_gpu_side", "decoded_frame_handoff_4k", "search_pass_end_to_end_4k",
             "search_end_to_end_4k", "quantizer_match_vs_cpu", "published_quality_ladder", "collective", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_is_the_headline_figure_alone(hip_lib, oracle):
    from oavif_amd import synth
    steps, warmup = 40, 10
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "ssimulacra2_megapixels_per_sec" and d["unit"] == "MP/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    mp = d["config"]["width"] * d["config"]["height"] / 1e6
    assert (d["config"]["width"], d["config"]["height"]) == (3840, 2160)
    assert abs(d["value"] - mp / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert not [k for k in FULL_ONLY if k in d]
    # `scores` is the score of pair 0 (the seeded frames as they are), as on a --full line
    ref = synth.make_ref(3840, 2160, seed=0)
    dst = synth.distort(ref, "blockq", 2)
    assert abs(d["scores"][0] - oracle.compute_ssimu2(ref, dst, oracle.BLUR_FIR)) <= 1e-3
    # what the run spends outside its warm-up and timed steps: start-up, set-up, the line, exit
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    assert outside < 30.0, outside
