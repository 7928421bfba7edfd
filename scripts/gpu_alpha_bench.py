#!/usr/bin/env python3
"""What the RGBA composite pass costs: the pair score of two RGBA frames
(ssimu2_score_rgba8) beside the 16-bit pair score (ssimu2_score_rgb16) and the 8-bit one (ssimu2_score_rgb8) of the
same content on the same context, at 1920x1080 and 3840x2160, in FIR and RECURSIVE.

All frames lie in page-locked host memory (ssimu2_host_alloc).  Each call is host frames in, score out, so its time
holds the uploads: 3, 6 and 4 bytes per pixel and frame for the three forms.  The forms are timed in interleaved
blocks after a warm-up, median of the blocks' medians.  The composite kernel alone is read off a kernel trace of the
same script, in a run of its own:

    python scripts/gpu_alpha_bench.py [--reps 40] [--out out/alpha_score.json]
    rocprofv3 --kernel-trace --stats -d out/alpha_trace -- python scripts/gpu_alpha_bench.py --reps 8
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import oavif_amd
    from oavif_amd import _lib, synth
    out = {"reps": args.reps, "device": oavif_amd.query_device(0), "library": oavif_amd.version(), "background": "1A80E6",
           "bytes_uploaded_per_pixel_and_frame": {"rgb8": 3, "rgb16": 6, "rgba8": 4}, "sizes": {}}

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ms)), float(min(ms))

    for w, h in ((1920, 1080), (3840, 2160)):
        ref = synth.make_ref(w, h, 0)
        dist = synth.distort(ref, "blockq", 2)
        yy, xx = np.mgrid[0:h, 0:w]
        alpha = np.clip((0.45 * h - np.hypot(xx - w / 2.0, yy - h / 2.0)) / 24.0 * 255.0, 0, 255).astype(np.uint8)
        rec = {}
        for name, blur in (("fir", _lib.BLUR_FIR), ("recursive", _lib.BLUR_RECURSIVE)):
            with oavif_amd.Ssimu2(0, blur=blur, extended=True) as s:
                def pinned(a):
                    p = s.host_alloc(a.shape if a.dtype == np.uint8 else (a.nbytes,))
                    p.reshape(-1)[...] = a.reshape(-1).view(np.uint8)
                    return p if a.dtype == np.uint8 else p.view(np.uint16).reshape(a.shape)

                r8, d8 = pinned(ref), pinned(dist)
                r16, d16 = pinned(ref.astype(np.uint16) * np.uint16(257)), pinned(dist.astype(np.uint16) * np.uint16(257))
                r4, d4 = pinned(np.dstack([ref, alpha])), pinned(np.dstack([dist, alpha]))
                forms = {"rgb8": lambda: s.compute_ssimu2(r8, d8), "rgb16": lambda: s.compute_ssimu2_hbd(r16, d16, 16),
                         "rgba8": lambda: s.compute_ssimu2_rgba(r4, d4, 0x1A80E6)}
                scores = {k: f() for k, f in forms.items()}
                for _ in range(3):
                    for f in forms.values():
                        f()
                blocks = {k: [] for k in forms}
                for _ in range(4):
                    for k, f in forms.items():
                        blocks[k].append(timed(f, max(1, args.reps // 4)))
                m = {k: {"median_ms": round(float(np.median([b[0] for b in v])), 4), "min_ms": round(min(b[1] for b in v), 4)}
                     for k, v in blocks.items()}
                m["scores"] = scores
                m["rgba8_minus_rgb16_ms"] = round(m["rgba8"]["median_ms"] - m["rgb16"]["median_ms"], 4)
                m["rgba8_minus_rgb8_ms"] = round(m["rgba8"]["median_ms"] - m["rgb8"]["median_ms"], 4)
                rec[name] = m
                del r8, d8, r16, d16, r4, d4
        out["sizes"][f"{w}x{h}"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
