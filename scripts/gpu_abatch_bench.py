"""Batches of YUV frames with an alpha plane in the recursive blur mode against single passes, on the GPU box (DESIGN.md
section 20) -> profiles/abatch_score.json.

    python scripts/gpu_abatch_bench.py [--out profiles/abatch_score.json] [--quick]

The protocol of scripts/gpu_hbatch_bench.py, unchanged (window and summary: scripts/gpu_batch_bench.py).  Per frame size
(256x256, 512x512, 1280x720, 1920x1080), per kind of frame (8-bit and 10-bit 4:2:0 with an alpha plane, rgb_depth 16)
and batch size N (1, 2, 4, 16) in SSIMU2_BLUR_RECURSIVE, alternating in one process A B C A B C ... (ROUNDS rounds; the
spread of each is reported):
    A  N single score_against_reference_yuva calls on one context, one after the other
    B  the same over two contexts on two threads, each with the reference cached
    C  one score_batch_against_reference_yuva call of N frames
The reference is an RGBA8 frame over a grey background (set_reference_rgba).  The probes of one wave of a speculative
search are such N frames: decodes of one image in HOST memory (pageable, as a decoder leaves them), so every side uploads
its planes inside the timed call.  A and B are the code paths a caller had
before; C is never compared with itself.  Every mode rotates over the same set of distinct frames; every shape is warmed
up; a timed window is at least WINDOW_S of work; the clock is the host's around whole blocking calls.  All figures are
frames per second over whole calls, not kernel times.

Every GPU step is a child process of its own under `timeout`; the parent stops at the first child that fails.
"""
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_batch_bench import ROUNDS, WINDOW_S, summarise, timed  # noqa: E402

SIZES = [(256, 256), (512, 512), (1280, 720), (1920, 1080)]
DEPTHS = [8, 10]
BATCHES = [1, 2, 4, 16]
CHUNK = 16            # frames per pass of every mode: a multiple of every N
DISTINCT = 32         # distinct frames the modes rotate over
CHILD_TIMEOUT_S = 200
BACKGROUND = 0x1A1A1A


def make_frames(w, h, depth, count):
    """`count` distinct 4:2:0 frames of `depth` bits (full range, BT.601) with an alpha plane (a disc with a soft edge)
    in host memory, and the RGBA8 reference they are damaged copies of."""
    import numpy as np
    from oavif_amd import _lib, synth
    from oavif_amd.scorer import YuvFrame
    ref = synth.make_ref(w, h, 0)
    dist = synth.distort(ref, "blockq", 2)
    c = dist.astype(np.float64) / 255.0
    y = 0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]
    cb = (c[..., 2] - y) / 1.772
    cr = (c[..., 0] - y) / 1.402
    m = (1 << depth) - 1
    dtype = np.uint8 if depth == 8 else np.uint16
    q = lambda a, bias: np.clip(np.floor(a * m + bias + 0.5), 0, m).astype(dtype)   # noqa: E731
    planes = [q(y, 0.0), q(cb, float(1 << (depth - 1)))[::2, ::2], q(cr, float(1 << (depth - 1)))[::2, ::2]]
    yy, xx = np.mgrid[0:h, 0:w]
    rad = 0.4 * min(w, h)
    disc = np.clip((rad - np.hypot(xx - w / 2.0, yy - h / 2.0)) / (rad / 6.0) + 0.5, 0.0, 1.0)
    alpha = np.floor(disc * m + 0.5).astype(dtype)
    frames = []
    for k in range(count):
        rolled = [np.ascontiguousarray(np.roll(p, (k * 6 % p.shape[0], k * 10 % p.shape[1]), (0, 1))) for p in planes]
        a = np.ascontiguousarray(np.roll(alpha, k % 3, 1))
        frames.append(YuvFrame(rolled, depth, _lib.YUV_420, True, 6, alpha=a))
    return np.dstack([ref, np.floor(disc * 255 + 0.5).astype(np.uint8)]), frames


def child_cells(w, h, depth, quick):
    import oavif_amd
    from oavif_amd import _lib
    ref, frames = make_frames(w, h, depth, CHUNK if quick else DISTINCT)
    P = len(frames)
    ctx = [oavif_amd.Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) for _ in range(2)]
    for c in ctx:
        c.set_reference_rgba(ref, BACKGROUND)
    pool = ThreadPoolExecutor(max_workers=2)

    def run_a(base, n):
        s = ctx[0]
        for i in range(base, base + CHUNK):
            s.score_against_reference_yuva(frames[i], 16)

    def half(args):
        s, idx = args
        for i in idx:
            s.score_against_reference_yuva(frames[i], 16)

    def run_b(base, n):
        # the pass's frames split over the two contexts, both busy for the whole pass whatever n is: the stronger yardstick
        idx = list(range(base, base + CHUNK))
        list(pool.map(half, [(ctx[0], idx[0::2]), (ctx[1], idx[1::2])]))

    def run_c(base, n):
        for g in range(base, base + CHUNK, n):
            ctx[0].score_batch_against_reference_yuva(frames[g:g + n], 16)

    state = {"at": 0}

    def rotating(fn, n):
        def call():
            fn(state["at"], n)
            state["at"] = (state["at"] + CHUNK) % P
        return call

    def measure(modes):
        est = {}
        for k, fn in modes.items():   # warm-up of every shape, and the estimate that sizes the window
            fn()
            t0 = time.perf_counter()
            fn()
            fn()
            est[k] = (time.perf_counter() - t0) / 2
        runs = {k: [] for k in modes}
        for _ in range(ROUNDS):
            for k, fn in modes.items():
                runs[k].append(timed(fn, CHUNK, est[k]))
        return {k: summarise(v) for k, v in runs.items()}

    cells = []
    for n in BATCHES:
        res = measure({"A": rotating(run_a, n), "B": rotating(run_b, n), "C": rotating(run_c, n)})
        cell = {"w": w, "h": h, "n": n, "depth": depth, "format": "4:2:0 with alpha", "rgb_depth": 16, "mode": "recursive",
                "distinct_frames": P, "A_single_one_context": res["A"], "B_single_two_contexts": res["B"], "C_batch": res["C"],
                "C_over_A": res["C"]["pairs_per_s"] / res["A"]["pairs_per_s"],
                "C_over_B": res["C"]["pairs_per_s"] / res["B"]["pairs_per_s"],
                "spread_max": max(r["spread"] for r in res.values())}
        cells.append(cell)
        print(f"# {depth}-bit 4:2:0 with alpha {w}x{h} N={n}: A {res['A']['us_per_pair']:.1f} B {res['B']['us_per_pair']:.1f} "
              f"C {res['C']['us_per_pair']:.1f} us/frame  C/A {cell['C_over_A']:.2f}  C/B {cell['C_over_B']:.2f}  "
              f"spread {cell['spread_max']:.3f}", file=sys.stderr)
    pool.shutdown()
    for c in ctx:
        c.close()
    return {"cells": cells}


def run_child(args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(f"child {' '.join(args)} ended with status {p.returncode}: stopping", file=sys.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main(argv):
    if "--child" in argv:
        w, h = (int(x) for x in argv[argv.index("--size") + 1].split("x"))
        print(json.dumps(child_cells(w, h, int(argv[argv.index("--depth") + 1]), "--quick" in argv)))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "abatch_score.json")
    extra = ["--quick"] if "--quick" in argv else []
    import oavif_amd
    record = {"what": "score_batch_against_reference_yuva (C: one call of N host frames) against N single "
                      "score_against_reference_yuva calls on one context (A) and over two contexts on two threads (B), "
                      "SSIMU2_BLUR_RECURSIVE, 4:2:0 planes and an alpha plane in pageable host memory, rgb_depth 16, an RGBA8 "
                      "reference over 0x1A1A1A; rates in frames per "
                      "second over whole blocking calls (the field names are gpu_batch_bench's: a pair is a frame here), "
                      "host clock; median of the rounds, spread = (max - min) / median",
              "version": oavif_amd.version(), "rounds": ROUNDS, "window_s": WINDOW_S, "cells": []}
    status = 0
    for w, h in SIZES:
        for depth in DEPTHS if status == 0 else []:
            r = run_child(["--child", "cells", "--size", f"{w}x{h}", "--depth", str(depth)] + extra)
            if r is None:
                status = 1
                break
            record["cells"] += r["cells"]
    record["complete"] = status == 0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(f"wrote {out} ({len(record['cells'])} cells, complete={record['complete']})")
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
