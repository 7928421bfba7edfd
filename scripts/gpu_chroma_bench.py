#!/usr/bin/env python3
"""What scoring a decoder's 4:2:0 planes costs and saves, at 1920x1080 and 3840x2160:

* CPU (one thread): avifImageYUVToRGB as the reference calls it -- 8-bit RGB out, libavif's default path -- on 8-bit and
  10-bit 4:2:0 images, and beside it the built-in converter (avoidLibYUV = 1), which is what the device computes.
* GPU, one chroma context per blur mode (FIR, RECURSIVE), pageable host frames in, score out: the pass against a cached
  reference of a 4:2:0 frame, of the 4:4:4 frame it was subsampled from, and of the RGB8 rows of that frame; the forms
  take turns within one process, median of 15 blocking calls each after 3 warm-up rounds.  Beside them 4:2:2, nearest
  upsampling and depth 10.

The conversion kernels alone are read off a kernel trace of the same script, in a run of its own:

    python scripts/gpu_chroma_bench.py [--out out/chroma_input.json] [--cpu-only] [--gpu-only]
    rocprofv3 --kernel-trace --stats -f csv -d out/chroma_trace -- python scripts/gpu_chroma_bench.py --gpu-only
    python scripts/gpu_chroma_bench.py --trace out/chroma_trace --out out/chroma_kernels.json
"""
import argparse
import collections
import csv
import ctypes
import json
import os
import re
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gpu_yuv_bench import CALLS, SIZES, content, median_ms  # noqa: E402

WARM = 3
YUV_420 = 3


class AvifImage420:
    """An avifImage of given 4:2:0 planes, and avifImageYUVToRGB on it."""

    def __init__(self, planes, depth):
        from oavif_amd import avif_bridge as ab
        self.ab, self.L = ab, ab._lib()
        self.h, self.w = planes[0].shape
        self.im = self.L.avifImageCreate(self.w, self.h, depth, YUV_420)
        ctypes.c_uint32.from_address(self.im + ab._IMG_YUVRANGE).value = 1
        ctypes.c_uint16.from_address(self.im + ab._IMG_MC).value = 6
        assert self.L.avifImageAllocatePlanes(self.im, ab._PLANES_YUV) == 0
        size = planes[0].itemsize
        for k in range(3):
            ph, pw = planes[k].shape
            ptr, row = ab._ptr(self.im, ab._IMG_YUVPLANES + 8 * k), ab._u32(self.im, ab._IMG_YUVROWBYTES + 4 * k)
            dst = np.ctypeslib.as_array((ctypes.c_uint8 * (row * ph)).from_address(ptr)).reshape(ph, row)
            dst[:, :pw * size] = np.ascontiguousarray(planes[k]).view(np.uint8).reshape(ph, pw * size)

    def to_rgb8(self, avoid_libyuv):
        ab, L = self.ab, self.L
        rgb = ctypes.create_string_buffer(ab._RGB_SIZE)
        L.avifRGBImageSetDefaults(rgb, self.im)
        struct.pack_into("<I", rgb, ab._RGB_DEPTH, 8)
        struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGB)
        struct.pack_into("<i", rgb, 24, 1 if avoid_libyuv else 0)
        assert L.avifRGBImageAllocatePixels(rgb) == 0

        def call():
            assert L.avifImageYUVToRGB(self.im, rgb) == 0
        return call, (lambda: L.avifRGBImageFreePixels(rgb))

    def close(self):
        self.L.avifImageDestroy(self.im)


def cpu_part():
    import chroma_ref
    import yuv_ref
    from oavif_amd import avif_bridge as ab
    out = {"libavif": ab.versions(), "threads": 1, "calls": CALLS, "yuv420_to_rgb8_ms": {}}
    for w, h in SIZES:
        _ref, dist = content(w, h)
        for depth in (8, 10):
            img = AvifImage420(chroma_ref.subsample(yuv_ref.forward(dist, depth, True, 6), YUV_420), depth)
            rec = {}
            for name, avoid in (("default", False), ("built_in", True)):
                call, free = img.to_rgb8(avoid)
                rec[name] = dict(zip(("median", "min"), median_ms(call)))
                free()
            img.close()
            out["yuv420_to_rgb8_ms"][f"{w}x{h} depth {depth}"] = rec
    return out


def gpu_part():
    import time
    import chroma_ref
    import yuv_ref
    import oavif_amd
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    out = {"device": oavif_amd.query_device(0), "library": oavif_amd.version(), "calls": CALLS, "warm_up_rounds": WARM,
           "bytes_uploaded_per_pixel": {"rgb8": 3, "yuv444_8": 3, "yuv420_8": 1.5, "yuv420_8_nearest": 1.5, "yuv422_8": 2,
                                        "yuv444_10": 6, "yuv420_10": 3}, "sizes": {}}
    for w, h in SIZES:
        ref, dist = content(w, h)
        y8 = [np.ascontiguousarray(p) for p in yuv_ref.forward(dist, 8, True, 6)]
        y10 = [np.ascontiguousarray(p) for p in yuv_ref.forward(dist, 10, True, 6)]
        rec = {}
        for name, blur in (("fir", _lib.BLUR_FIR), ("recursive", _lib.BLUR_RECURSIVE)):
            with oavif_amd.Ssimu2(0, blur=blur, chroma=True) as s:
                s.set_reference(ref)
                f444_8, f444_10 = YuvFrame(y8, 8), YuvFrame(y10, 10)
                f420_8 = YuvFrame(chroma_ref.subsample(y8, 3), 8, 3)
                f422_8 = YuvFrame(chroma_ref.subsample(y8, 2), 8, 2)
                f420_10 = YuvFrame(chroma_ref.subsample(y10, 3), 10, 3)
                forms = {"yuv420_8": lambda: s.score_against_reference_yuv(f420_8, 16),
                         "yuv444_8": lambda: s.score_against_reference_yuv(f444_8, 16),
                         "rgb8": lambda: s.score_decoded_against_reference(dist),
                         "yuv420_8_nearest": lambda: s.score_against_reference_yuv(f420_8, 16, "nearest"),
                         "yuv422_8": lambda: s.score_against_reference_yuv(f422_8, 16),
                         "yuv420_10": lambda: s.score_against_reference_yuv(f420_10, 16),
                         "yuv444_10": lambda: s.score_against_reference_yuv(f444_10, 16)}
                m = {"scores": {k: f() for k, f in forms.items()}}
                ms = collections.defaultdict(list)
                for r in range(WARM + CALLS):          # the forms take turns
                    for k, f in forms.items():
                        t = time.perf_counter()
                        f()
                        if r >= WARM:
                            ms[k].append((time.perf_counter() - t) * 1e3)
                for k, v in ms.items():
                    m[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4),
                            "max_ms": round(float(max(v)), 4)}
                rec[name] = m
        out["sizes"][f"{w}x{h}"] = rec
    return out


def trace_part(directory):
    """Median dispatch duration of every conversion kernel in a rocprofv3 kernel trace, by kernel and grid."""
    paths = [os.path.join(d, f) for d, _ds, fs in os.walk(directory) for f in fs if f.endswith("kernel_trace.csv")]
    assert paths, f"no *kernel_trace.csv under {directory}"
    found = collections.defaultdict(list)
    for path in paths:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if "yuv" not in name:
                    continue
                name = re.sub(r"\(.*", "", re.sub(r"^void\s+", "", name)).replace("ssimu2::", "")
                grid = f'{row["Grid_Size_X"]}x{row["Grid_Size_Y"]}'
                found[f"{name} grid {grid}"].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2),
                "max_us": round(float(max(v)), 2)} for k, v in sorted(found.items())}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--trace", default="", help="summarise the kernel trace rocprofv3 wrote under this directory")
    args = ap.parse_args()
    out = {}
    if args.trace:
        out["kernels"] = trace_part(args.trace)
    else:
        if not args.gpu_only:
            out["cpu"] = cpu_part()
        if not args.cpu_only:
            out["gpu"] = gpu_part()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
