"""SSIMULACRA2 of an AVIF from the decoder's own Y, U and V planes, converted to RGB on the device with the exact colour
matrix at full precision (include/ssimu2_hip_yuv.h); a 4:2:0 or 4:2:2 file's chroma is upsampled
there too, as libavif's built-in converter does it (include/ssimu2_hip_chroma.h, section 16).

    python -m oavif_amd.yuvscore REF.png|REF.avif DIST.avif [--rgb-depth N] [--blur fir|recursive|recursive_fma] [--compare]
                                 [--map OUT.png|.pam|.pfm] [--chroma-upsampling bilinear|nearest]

prints the score of DIST against REF through the YUV path; `--map` also writes where DIST is damaged, the error map of
that very score (ssimu2_error_map_against_reference_yuv, include/ssimu2_hip_map.h), in errmap's formats.  A PNG reference is taken as 8-bit RGB (alpha dropped, 16
bits truncated, as the search takes its source); an AVIF reference goes through the YUV path too.  `--compare` adds
the score of libavif's 8-bit RGB output of DIST (avifImageYUVToRGB at depth 8: libyuv's fixed-point conversion), which
is what the reference program scores.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import _lib
from .scorer import MATRIX_COEFFICIENTS, Ssimu2, YuvFrame

BLUR_MODES = {"fir": _lib.BLUR_FIR, "recursive": _lib.BLUR_RECURSIVE, "recursive_fma": _lib.BLUR_RECURSIVE_FMA}
MAP_FORMATS = (".pfm", ".pam", ".png")   # errmap.FORMATS


def rgb_depth_arg(text: str) -> int:
    try:
        v = int(text, 10)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--rgb-depth must be an integer 8..16, got {text!r}")
    if not 8 <= v <= 16:
        raise argparse.ArgumentTypeError(f"--rgb-depth must be 8..16, got {v}")
    return v


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m oavif_amd.yuvscore",
                                 description="SSIMULACRA2 of an AVIF scored from its decoded YUV planes")
    ap.add_argument("ref", help="reference: a PNG, or an AVIF (scored from its YUV planes too)")
    ap.add_argument("dist", help="distorted image: an AVIF")
    ap.add_argument("--rgb-depth", type=rgb_depth_arg, default=16, metavar="N",
                    help="depth of the RGB codes the planes are converted to, 8..16 (default 16: full precision)")
    ap.add_argument("--blur", choices=sorted(BLUR_MODES), default="fir")
    ap.add_argument("--compare", action="store_true", help="also print the score of libavif's 8-bit RGB output")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--map", default=None, metavar="OUT",
                    help="also write the error map of the YUV-path score: OUT.pfm (float), .pam or .png (8-bit, "
                         "normalised to the maximum), as python -m oavif_amd.errmap writes it")
    ap.add_argument("--chroma-upsampling", choices=("bilinear", "nearest"), default="bilinear",
                    help="how the chroma of a 4:2:0 or 4:2:2 file is upsampled (default bilinear: libavif's automatic choice)")
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    ap = parser()
    a = ap.parse_args(argv)
    if not a.dist.lower().endswith(".avif"):
        ap.error(f"DIST must be an AVIF, got {a.dist!r}")
    if not a.ref.lower().endswith((".png", ".avif")):
        ap.error(f"REF must be a PNG or an AVIF, got {a.ref!r}")
    if a.map is not None and not a.map.lower().endswith(MAP_FORMATS):
        ap.error(f"--map must end in one of {', '.join(MAP_FORMATS)}, got {a.map!r}")
    return a


def frame_of(decoded) -> YuvFrame:
    """avif_bridge.DecodedYuv -> YuvFrame (views: valid while `decoded` is open); ValueError for what the scorer does
    not convert."""
    if decoded.has_alpha:
        raise ValueError("the image has an alpha plane: score it with python -m oavif_amd.alpha")
    if decoded.format not in (_lib.YUV_444, _lib.YUV_422, _lib.YUV_420, _lib.YUV_400):
        raise ValueError(f"pixel format {decoded.format} is not converted on the device")
    if decoded.matrix_coefficients not in MATRIX_COEFFICIENTS:
        raise ValueError(f"matrix coefficients {decoded.matrix_coefficients} are not converted on the device")
    return YuvFrame(decoded.planes, decoded.depth, decoded.format, decoded.full_range, decoded.matrix_coefficients)


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import avif_bridge as ab, cli
    try:
        dist_data = open(a.dist, "rb").read()
        with Ssimu2(a.device, blur=BLUR_MODES[a.blur], chroma=True) as s, \
                ab.decode_yuv(dist_data) as dist:
            if a.ref.lower().endswith(".avif"):
                with ab.decode_yuv(open(a.ref, "rb").read()) as ref:
                    if (ref.width, ref.height) != (dist.width, dist.height):
                        raise ValueError(f"{a.ref} is {ref.width}x{ref.height}, {a.dist} is {dist.width}x{dist.height}")
                    s.set_reference_yuv(frame_of(ref), a.rgb_depth, a.chroma_upsampling)
            else:
                rgb = cli.load_source(a.ref).rgb
                if rgb.shape[:2] != (dist.height, dist.width):
                    raise ValueError(f"{a.ref} is {rgb.shape[1]}x{rgb.shape[0]}, {a.dist} is {dist.width}x{dist.height}")
                s.set_reference(rgb)
            if a.map is None:
                print(f"yuv {s.score_against_reference_yuv(frame_of(dist), a.rgb_depth, a.chroma_upsampling):.6f}")
            else:
                from . import errmap
                score, m = s.error_map_against_reference_yuv(frame_of(dist), a.rgb_depth, a.chroma_upsampling)
                data, peak = errmap.encode(m, os.path.splitext(a.map)[1].lower())
                with open(a.map, "wb") as f:
                    f.write(data)
                if peak is not None:
                    print(f"yuvscore: map maximum {peak!r} (= 255)", file=sys.stderr)
                print(f"yuv {score:.6f}")
            if a.compare:
                with ab.decode_common(dist_data) as rgb8:
                    print(f"rgb8 {s.score_decoded_against_reference(rgb8.rows.reshape(-1), rgb8.row_bytes, rgb8.channels):.6f}")
    except (ValueError, OSError, ab.AvifBridgeError, cli.CliError) as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
