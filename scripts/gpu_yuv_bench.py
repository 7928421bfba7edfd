#!/usr/bin/env python3
"""What scoring a decoder's YUV planes costs and saves, at 1920x1080 and 3840x2160:

* CPU (one thread): avifImageYUVToRGB as the reference calls it -- 8-bit RGB out, libyuv's fixed-point conversion -- on
  8-bit and 10-bit 4:4:4 images: what a probe stops paying.  Beside it, how far that RGB is from libavif's exact
  (built-in) conversion: share of differing samples and the largest difference, per matrix, on 97x53 random planes.
* GPU, one yuv context per blur mode (FIR, RECURSIVE), host frames in, score out, median of 15 blocking calls:
  score_against_reference_yuv of an 8-bit and of a 10-bit frame at rgb_depth 16, beside
  score_decoded_against_reference on the frame's RGB8 rows and score_decoded_against_reference_hbd on its RGB16 rows.

The conversion kernel alone is read off a kernel trace of the same script, in a run of its own:

    python scripts/gpu_yuv_bench.py [--out out/yuv_input.json] [--cpu-only] [--gpu-only]
    rocprofv3 --kernel-trace --stats -d out/yuv_trace -- python scripts/gpu_yuv_bench.py --gpu-only
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1920, 1080), (3840, 2160))
CALLS = 15


def median_ms(fn, calls=CALLS, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


class AvifImage:
    """An avifImage of given planes, and avifImageYUVToRGB on it."""

    def __init__(self, planes, depth, full_range=True, mc=6):
        from oavif_amd import avif_bridge as ab
        self.ab, self.L = ab, ab._lib()
        h, w = planes[0].shape
        self.w, self.h = w, h
        self.im = self.L.avifImageCreate(w, h, depth, 1)
        ctypes.c_uint32.from_address(self.im + ab._IMG_YUVRANGE).value = 1 if full_range else 0
        ctypes.c_uint16.from_address(self.im + ab._IMG_MC).value = mc
        assert self.L.avifImageAllocatePlanes(self.im, ab._PLANES_YUV) == 0
        size = planes[0].itemsize
        for k in range(3):
            ptr, row = ab._ptr(self.im, ab._IMG_YUVPLANES + 8 * k), ab._u32(self.im, ab._IMG_YUVROWBYTES + 4 * k)
            dst = np.ctypeslib.as_array((ctypes.c_uint8 * (row * h)).from_address(ptr)).reshape(h, row)
            dst[:, :w * size] = np.ascontiguousarray(planes[k]).view(np.uint8).reshape(h, w * size)

    def to_rgb(self, rgb_depth=8, avoid_libyuv=False):
        """-> (call, pixels): call() converts once into pixels(), an (h, w, 3) view; free() afterwards."""
        ab, L = self.ab, self.L
        rgb = ctypes.create_string_buffer(ab._RGB_SIZE)
        L.avifRGBImageSetDefaults(rgb, self.im)
        struct.pack_into("<I", rgb, ab._RGB_DEPTH, rgb_depth)
        struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGB)
        struct.pack_into("<i", rgb, 24, 1 if avoid_libyuv else 0)
        assert L.avifRGBImageAllocatePixels(rgb) == 0
        pix, row = struct.unpack_from("<QI", rgb.raw, ab._RGB_PIXELS)
        sample = ctypes.c_uint8 if rgb_depth == 8 else ctypes.c_uint16
        n = row // ctypes.sizeof(sample)
        rows = np.ctypeslib.as_array((sample * (n * self.h)).from_address(pix)).reshape(self.h, n)

        def call():
            assert L.avifImageYUVToRGB(self.im, rgb) == 0
        return call, rows, (lambda: L.avifRGBImageFreePixels(rgb))

    def close(self):
        self.L.avifImageDestroy(self.im)


def content(w, h):
    from oavif_amd import synth
    ref = synth.make_ref(w, h, 0)
    return ref, synth.distort(ref, "blockq", 2)


def cpu_part():
    import yuv_ref
    from oavif_amd import avif_bridge as ab
    out = {"libavif": ab.versions(), "threads": 1, "calls": CALLS, "yuv_to_rgb8_ms": {}, "libyuv_against_built_in": {}}
    for w, h in SIZES:
        _ref, dist = content(w, h)
        for depth in (8, 10):
            img = AvifImage(yuv_ref.forward(dist, depth, True, 6), depth)
            rec = {}
            for name, avoid in (("libyuv", False), ("built_in", True)):
                call, _rows, free = img.to_rgb(8, avoid)
                rec[name] = dict(zip(("median", "min"), median_ms(call)))
                free()
            img.close()
            out["yuv_to_rgb8_ms"][f"{w}x{h} depth {depth}"] = rec
    for depth in (8, 10, 12):
        for mc in (1, 6, 9):
            img = AvifImage(yuv_ref.random_planes(97, 53, depth, seed=depth + mc), depth, True, mc)
            got = []
            for avoid in (False, True):
                call, rows, free = img.to_rgb(8, avoid)
                call()
                got.append(rows[:, :97 * 3].astype(np.int32))
                free()
            img.close()
            d = np.abs(got[0] - got[1])
            out["libyuv_against_built_in"][f"depth {depth} matrix {mc}"] = {"differing_share": round(float((d != 0).mean()), 4),
                                                                            "largest": int(d.max())}
    return out


def gpu_part():
    import yuv_ref
    import oavif_amd
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    out = {"device": oavif_amd.query_device(0), "library": oavif_amd.version(), "calls": CALLS,
           "bytes_uploaded_per_pixel": {"rgb8": 3, "rgb16": 6, "yuv8": 3, "yuv10": 6}, "sizes": {}}
    for w, h in SIZES:
        ref, dist = content(w, h)
        y8 = [np.ascontiguousarray(p) for p in yuv_ref.forward(dist, 8, True, 6)]
        y10 = [np.ascontiguousarray(p) for p in yuv_ref.forward(dist, 10, True, 6)]
        rgb16 = yuv_ref.codes(*y8, 8, True, 6, 16)
        rec = {}
        for name, blur in (("fir", _lib.BLUR_FIR), ("recursive", _lib.BLUR_RECURSIVE)):
            with oavif_amd.Ssimu2(0, blur=blur, yuv=True) as s:
                s.set_reference(ref)
                f8, f10 = YuvFrame(y8, 8), YuvFrame(y10, 10)
                forms = {"rgb8": lambda: s.score_decoded_against_reference(dist),
                         "rgb16": lambda: s.score_decoded_against_reference_hbd(rgb16, bit_depth=16),
                         "yuv8": lambda: s.score_against_reference_yuv(f8, 16),
                         "yuv10": lambda: s.score_against_reference_yuv(f10, 16)}
                m = {"scores": {k: f() for k, f in forms.items()}}
                for k, f in forms.items():
                    m[k] = dict(zip(("median_ms", "min_ms"), median_ms(f)))
                rec[name] = m
        out["sizes"][f"{w}x{h}"] = rec
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    args = ap.parse_args()
    out = {}
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
