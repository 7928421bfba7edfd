#!/usr/bin/env python3
"""What the error map of a 16-bit or YUV frame costs beside the score it follows, at 1920x1080
and 3840x2160, in FIR and RECURSIVE: one map context per blur mode, host frames in, result out, the median of 15 blocking
calls after 3 warm-ups.

* compute_ssimu2_hbd against error_map_hbd at depth 10 (a pair of frames);
* score_against_reference_yuv against error_map_against_reference_yuv of a 10-bit 4:4:4 frame at rgb_depth 16,
  against an 8-bit reference (what --score-yuv 1 scores);
* as the yardstick, compute_ssimu2 against error_map of the same content at 8 bits on the same build.

A map call is its score call plus the map pass and the download of w * h floats, so `map_pass_ms` is the difference of the
two medians.

    python scripts/gpu_map_hbd_bench.py [--out profiles/map_hbd.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1920, 1080), (3840, 2160))
CALLS, WARM = 15, 3


def median_ms(fn, calls=CALLS, warm=WARM):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import hbd_cases
    import yuv_ref
    import oavif_amd
    from oavif_amd import _lib, synth
    from oavif_amd.scorer import YuvFrame
    out = {"device": oavif_amd.query_device(0), "library": oavif_amd.version(), "calls": CALLS, "warm_ups": WARM,
           "scale0_input_bytes_per_pixel_of_the_map_pass": {"8-bit": 6, "16-bit": 24}, "sizes": {}}
    for w, h in SIZES:
        ref = synth.make_ref(w, h, 0)
        dist = synth.distort(ref, "blockq", 2)
        r10, d10 = hbd_cases.to_depth(ref, 10, 1), hbd_cases.to_depth(dist, 10, 2)
        y10 = [np.ascontiguousarray(p) for p in yuv_ref.forward(dist, 10, True, 6)]
        rec = {}
        for name, blur in (("fir", _lib.BLUR_FIR), ("recursive", _lib.BLUR_RECURSIVE)):
            with oavif_amd.Ssimu2(0, blur=blur, maps=True, yuv=True) as s:
                f10 = YuvFrame(y10, 10)
                pairs = {"rgb8": (lambda: s.compute_ssimu2(ref, dist), lambda: s.error_map(ref, dist)),
                         "rgb16 depth 10": (lambda: s.compute_ssimu2_hbd(r10, d10, 10), lambda: s.error_map_hbd(r10, d10, 10))}
                m = {}
                for form, (score, emap) in pairs.items():
                    m[form] = measure(score, emap)
                s.set_reference(ref)
                m["yuv10 against an 8-bit reference"] = measure(lambda: s.score_against_reference_yuv(f10, 16),
                                                                lambda: s.error_map_against_reference_yuv(f10, 16))
                m["rgb8 against an 8-bit reference"] = measure(lambda: s.score_against_reference(dist),
                                                               lambda: s.error_map_against_reference(dist))
                rec[name] = m
        out["sizes"][f"{w}x{h}"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 0


def measure(score, emap):
    """-> the medians of the score call and of its map form, and their difference: the map pass and its download."""
    value = score()
    got, _m = emap()
    assert got == value, (got, value)
    sm, smin = median_ms(score)
    mm, mmin = median_ms(emap)
    return {"score": value, "score_ms": {"median": sm, "min": smin}, "map_ms": {"median": mm, "min": mmin},
            "map_pass_ms": round(mm - sm, 4)}


if __name__ == "__main__":
    sys.exit(main())
