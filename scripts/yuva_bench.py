#!/usr/bin/env python3
"""What scoring a transparent AVIF from the decoder's own planes costs and saves: an 8-bit 4:2:0
frame with an alpha plane at 1920x1080 and 3840x2160, from pageable host memory, one yuva context per blur mode
(RECURSIVE, the search's default, and FIR), the reference set once from the RGBA source.

* baseline: score_against_reference_rgba on libavif's RGBA rows of the same decode -- the parent commit's way;
* new call: score_against_reference_yuva on the planes (rgb_depth 8: no division; 2.5 bytes per pixel uploaded, not 4);
* host time saved: the avifImageYUVToRGB call that made those RGBA rows, timed on the CPU (one thread);
* the division: the same call with the two forms of the exact division forced (OAVIF_YUVA_DIVISION = mulhi | plain),
  at rgb_depth 8 and at rgb_depth 16, where the rule takes mulhi.

The forms take turns within one process and rotate over three decoded frames (three quantizers of one source); median,
minimum and maximum of CALLS blocking calls per frame each, after WARM warm-up rounds.

    python scripts/yuva_bench.py [--out profiles/yuva_score.json] [--cpu-only] [--sizes 1920x1080,3840x2160]
"""
import argparse
import collections
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1920, 1080), (3840, 2160))
QUANTIZERS = (45, 60, 75)
CALLS, WARM = 15, 3
BACKGROUND = 0xE6E6E6
YUV_420 = 3
DIVISION_ENV = "OAVIF_YUVA_DIVISION"


def source(w, h):
    """An RGBA source: the project's synthetic photo under a disc with a soft edge, noise where nobody sees it."""
    from oavif_amd import synth
    rgb = synth.make_ref(w, h, 0)
    yy, xx = np.mgrid[0:h, 0:w]
    rad = 0.4 * min(w, h)
    a = np.clip((rad - np.hypot(xx - w / 2.0, yy - h / 2.0)) / (rad / 6.0) * 255.0 + 128.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a[..., None]], -1))


def decoded_frames(src):
    """Three encodes of `src` (4:2:0, 8-bit) -> [(planes, alpha, RGBA rows, ms of avifImageYUVToRGB)]: copies in pageable
    host memory of what decode_yuv hands out and of what libavif's default conversion makes of the same image."""
    from oavif_amd import avif_bridge as ab, cli
    L = ab._lib()
    o = cli.AvifEncOptions()
    o.tenbit, o.speed, o.quality_alpha = False, 10, 90
    out = []
    with ab.EncoderSource(src, 8, o, yuv_format=YUV_420) as enc:
        for q in QUANTIZERS:
            data = enc.encode(o, q)
            with ab.decode_yuv(data) as d:
                assert (d.format, d.depth, d.has_alpha) == (YUV_420, 8, True)
                planes = [np.array(p, copy=True) for p in d.planes]      # copies: the views die with the decoder
                alpha = np.array(d.alpha, copy=True)
                how = (d.full_range, d.matrix_coefficients)
                img = ab._ptr(d._dec, ab._DEC_IMAGE)
                rgb = ctypes.create_string_buffer(ab._RGB_SIZE)      # decode_common's conversion: RGBA, 8-bit, defaults
                L.avifRGBImageSetDefaults(rgb, img)
                struct.pack_into("<I", rgb, ab._RGB_DEPTH, 8)
                struct.pack_into("<I", rgb, ab._RGB_FORMAT, ab._RGB_FORMAT_RGBA)
                assert L.avifRGBImageAllocatePixels(rgb) == 0
                try:
                    ms = []
                    for _ in range(WARM + CALLS):
                        t = time.perf_counter()
                        assert L.avifImageYUVToRGB(img, rgb) == 0
                        ms.append((time.perf_counter() - t) * 1e3)
                    pix, row = struct.unpack_from("<QI", rgb.raw, ab._RGB_PIXELS)
                    rows = np.ctypeslib.as_array((ctypes.c_uint8 * (row * d.height)).from_address(pix)).reshape(d.height, row)
                    rgba = np.array(rows[:, :d.width * 4].reshape(d.height, d.width, 4), copy=True)
                finally:
                    L.avifRGBImageFreePixels(rgb)
            out.append({"q": q, "bytes": len(data), "planes": planes, "alpha": alpha, "how": how, "rgba": rgba,
                        "yuv_to_rgb_ms": ms[WARM:]})
    return out


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4),
            "calls": len(ms)}


def forced(how, fn):
    """fn() with the division form `how` forced (None: the library's rule)."""
    def call():
        if how is None:
            return fn()
        os.environ[DIVISION_ENV] = how
        try:
            return fn()
        finally:
            del os.environ[DIVISION_ENV]
    return call


def gpu_part(src, frames):
    import oavif_amd
    from oavif_amd import _lib
    from oavif_amd.scorer import YuvFrame
    out = {}
    for name, blur in (("recursive", _lib.BLUR_RECURSIVE), ("fir", _lib.BLUR_FIR)):
        with oavif_amd.Ssimu2(0, blur=blur, yuva=True) as s:
            s.set_reference_rgba(src, BACKGROUND)
            yf = [YuvFrame(f["planes"], 8, YUV_420, *f["how"], alpha=f["alpha"]) for f in frames]
            forms = {"rgba_baseline": lambda i: s.score_against_reference_rgba(frames[i]["rgba"]),
                     "yuva": lambda i: s.score_against_reference_yuva(yf[i], 8)}
            for rgb_depth in (8, 16):
                for how in ("mulhi", "plain"):
                    forms[f"yuva_rgb{rgb_depth}_{how}"] = (lambda i, d=rgb_depth, how=how:
                                                           forced(how, lambda: s.score_against_reference_yuva(yf[i], d))())
            rec = {"scores": {k: [f(i) for i in range(len(frames))] for k, f in forms.items()}}
            # the three forms of the division are one result: the same codes, hence the same scores
            sc = rec["scores"]
            rec["division_forms_agree"] = {
                "scores_rgb8": sc["yuva"] == sc["yuva_rgb8_mulhi"] == sc["yuva_rgb8_plain"],
                "scores_rgb16": sc["yuva_rgb16_mulhi"] == sc["yuva_rgb16_plain"],
                "scores_repeat": sc["yuva"] == [forms["yuva"](i) for i in range(len(frames))]}
            for d in (8, 16):
                codes = {how: forced(how, lambda: s.composite_yuva(yf[0], BACKGROUND, d))() for how in (None, "mulhi", "plain")}
                rec["division_forms_agree"][f"differing_codes_rgb{d}"] = {
                    how: int((codes[how] != codes[None]).sum()) for how in ("mulhi", "plain")}
            agree = rec["division_forms_agree"]
            assert all(v is True or v == {"mulhi": 0, "plain": 0} for v in agree.values()), agree
            ms = collections.defaultdict(list)
            for r in range(WARM + CALLS):                  # the forms take turns, each over the frames in rotation
                for i in range(len(frames)):
                    for k, f in forms.items():
                        t = time.perf_counter()
                        f(i)                                # blocking: returns with the score
                        if r >= WARM:
                            ms[k].append((time.perf_counter() - t) * 1e3)
            for k, v in ms.items():
                rec[k] = stats(v)
            rec["yuva_over_baseline"] = round(rec["yuva"]["median_ms"] / rec["rgba_baseline"]["median_ms"], 4)
            out[name] = rec
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--cpu-only", action="store_true", help="the host part alone: encodes, decodes, avifImageYUVToRGB")
    ap.add_argument("--sizes", default=",".join(f"{w}x{h}" for w, h in SIZES))
    args = ap.parse_args()
    from oavif_amd import avif_bridge as ab
    out = {"libavif": ab.versions(), "calls_per_frame": CALLS, "warm_up_rounds": WARM, "frames_in_rotation": len(QUANTIZERS),
           "background": f"{BACKGROUND:06X}", "bytes_uploaded_per_pixel": {"rgba_baseline": 4, "yuva": 2.5}, "sizes": {}}
    if not args.cpu_only:
        import oavif_amd
        out["device"], out["library"] = oavif_amd.query_device(0), oavif_amd.version()
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        src = source(w, h)
        frames = decoded_frames(src)
        rec = {"frames": [{"q": f["q"], "avif_bytes": f["bytes"]} for f in frames],
               "host_avifImageYUVToRGB_rgba8": stats([m for f in frames for m in f["yuv_to_rgb_ms"]])}
        if not args.cpu_only:
            rec.update(gpu_part(src, frames))
        out["sizes"][f"{w}x{h}"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
