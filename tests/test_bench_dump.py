"""bench.py --dump-outputs: the last timed step's score and plane averages, written as .npy, are what the CPU checker
computes on the same seeded pair; --steps is the number of steps timed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dump_outputs_are_the_last_timed_steps_score(hip_lib, oracle, tmp_path):
    from oavif_amd import synth
    w, h, steps, nctx, npairs = 512, 384, 7, 2, 8
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "2",
                        "--streams", str(nctx), "--pairs", str(npairs), "--width", str(w), "--height", str(h),
                        "--no-cpu-baseline", "--no-by-resolution", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == steps and d["repeats"] == 1
    assert sorted(os.listdir(out)) == ["plane_averages.npy", "score.npy"]
    score = np.load(out / "score.npy")
    avg = np.load(out / "plane_averages.npy")
    assert score.dtype == np.float64 and score.shape == (1,)
    assert avg.dtype == np.float64 and avg.shape == (6, 18)

    # the pair of the last timed step, built as bench.py builds it (rank 0's seeded frames, rolled and flipped)
    c_last = (steps - 1) % nctx
    k = c_last + nctx * (((steps - 1) // nctx) % npairs)
    ref = synth.make_ref(w, h, seed=0)
    dst = synth.distort(ref, "blockq", 2)
    shift = (k * w) // (nctx * npairs)
    ref, dst = np.roll(ref, shift, 1), np.roll(dst, shift, 1)
    if k & 1:
        ref, dst = ref[::-1], dst[::-1]
    exp, avg_o, ns_o = oracle.compute_ssimu2(ref, dst, oracle.BLUR_FIR, return_averages=True)
    assert ns_o == 6
    assert abs(score[0] - exp) <= 1e-3, (score[0], exp)
    assert np.allclose(avg, avg_o, rtol=1e-4, atol=1e-9)
