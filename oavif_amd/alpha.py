"""Alpha-aware SSIMULACRA2: RGBA frames composited over an opaque background on the device and then scored
(include/ssimu2_hip_ext.h).

    python -m oavif_amd.alpha REF DIST [--background RRGGBB]... [--blur fir|recursive|recursive_fma]
                              [--rgb-depth N] [--chroma-upsampling bilinear|nearest]

prints one score per background and their minimum.  REF and DIST are PNGs, or AVIFs, which are scored from the decoder's
own Y, U, V and alpha planes (include/ssimu2_hip_yuva.h, DESIGN.md section 17: no conversion on the host, any of the
four formats, depth 8 to 12; --rgb-depth and --chroma-upsampling say how their colour is converted).  One background hides exactly the halos of its own colour, so the
default is two, a dark and a light grey.  `search_rgba` is the target-quality search of an RGBA source whose passes are
scored that way: colour hidden under transparent pixels does not move the score, damage to the alpha plane does.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import _lib
from .scorer import Ssimu2, YuvFrame, background_rgb

DEFAULT_BACKGROUNDS = (0x1A1A1A, 0xE6E6E6)
BLUR_MODES = {"fir": _lib.BLUR_FIR, "recursive": _lib.BLUR_RECURSIVE, "recursive_fma": _lib.BLUR_RECURSIVE_FMA}


def parse_background(text: str) -> int:
    """'RRGGBB' (six hex digits) -> 0xRRGGBB."""
    if len(text) != 6 or any(ch not in "0123456789abcdefABCDEF" for ch in text):
        raise argparse.ArgumentTypeError(f"background must be six hex digits RRGGBB, got {text!r}")
    return int(text, 16)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m oavif_amd.alpha",
                                 description="SSIMULACRA2 of two PNGs or AVIFs with transparency, composited over each background")
    ap.add_argument("ref")
    ap.add_argument("dist")
    ap.add_argument("--background", action="append", type=parse_background, metavar="RRGGBB",
                    help="opaque background colour; may be given several times (default: 1A1A1A and E6E6E6)")
    ap.add_argument("--blur", choices=sorted(BLUR_MODES), default="fir")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rgb-depth", type=int, default=8, metavar="N",
                    help="AVIF input: depth of the colour codes the planes are converted to, 8..16 (default 8)")
    ap.add_argument("--chroma-upsampling", choices=("bilinear", "nearest"), default="bilinear",
                    help="AVIF input: how 4:2:2 and 4:2:0 chroma is upsampled (default bilinear)")
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    a = parser().parse_args(argv)
    if not a.background:
        a.background = list(DEFAULT_BACKGROUNDS)
    return a


def as_rgba(pixels: np.ndarray) -> np.ndarray:
    """(h, w, 3|4) uint8 -> (h, w, 4) uint8; an RGB source counts as opaque."""
    a = np.asarray(pixels)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"need an 8-bit RGB or RGBA image, got {a.dtype} {a.shape}")
    if a.shape[2] == 4:
        return np.ascontiguousarray(a)
    return np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=2)


def load_rgba(path: str) -> np.ndarray:
    from . import png
    with open(path, "rb") as f:
        pixels, _channels, hbd, _icc = png.load_png(f.read())
    if hbd:
        raise ValueError(f"{path}: 16-bit PNG; the RGBA scorer takes 8-bit samples")
    return as_rgba(pixels)


def is_avif(path: str) -> bool:
    return path.lower().endswith(".avif")


def yuva_frame(decoded) -> YuvFrame:
    """avif_bridge.DecodedYuv -> the YuvFrame of its planes and alpha plane (views: valid while `decoded` is open)."""
    return YuvFrame(decoded.planes, decoded.depth, decoded.format, decoded.full_range, decoded.matrix_coefficients,
                    alpha=decoded.alpha, alpha_premultiplied=decoded.alpha_premultiplied)


def score_over(scorer: Ssimu2, ref: np.ndarray, dist: np.ndarray, backgrounds) -> list:
    """[(0xRRGGBB, score)] of the RGBA pair over each background."""
    return [(bg, scorer.compute_ssimu2_rgba(ref, dist, bg)) for bg in (background_rgb(b) for b in backgrounds)]


def score_files(scorer: Ssimu2, ref_path: str, dist_path: str, backgrounds, rgb_depth: int = 8,
                chroma_upsampling: str = "bilinear") -> list:
    """[(0xRRGGBB, score)] of two files of which at least one is an AVIF, on a yuva=True context: an AVIF is scored from
    the decoder's planes (no avifImageYUVToRGB on the host), a PNG from its RGBA rows; both are composited over each
    background on the device.  Raises ValueError when the two sizes differ."""
    from . import avif_bridge as ab

    def opened(path):
        if is_avif(path):
            with open(path, "rb") as f:
                return ab.decode_yuv(f.read())
        return load_rgba(path)

    ref = opened(ref_path)
    try:
        dist = opened(dist_path)
        try:
            size = lambda x: (x.height, x.width) if isinstance(x, ab.DecodedYuv) else x.shape[:2]
            if size(ref) != size(dist):
                raise ValueError(f"{ref_path} is {size(ref)[1]}x{size(ref)[0]}, {dist_path} is {size(dist)[1]}x{size(dist)[0]}")
            how = (int(rgb_depth), chroma_upsampling)
            rf = yuva_frame(ref) if isinstance(ref, ab.DecodedYuv) else None
            df = yuva_frame(dist) if isinstance(dist, ab.DecodedYuv) else None
            out = []
            for bg in (background_rgb(b) for b in backgrounds):
                if rf is not None and df is not None:
                    score = scorer.compute_ssimu2_yuva(rf, df, bg, *how)
                elif rf is not None:
                    scorer.set_reference_yuva(rf, bg, *how)
                    score = scorer.score_against_reference_rgba(dist)
                else:
                    scorer.set_reference_rgba(ref, bg)
                    score = scorer.score_against_reference_yuva(df, *how)
                out.append((bg, score))
            return out
        finally:
            if isinstance(dist, ab.DecodedYuv):
                dist.close()
    finally:
        if isinstance(ref, ab.DecodedYuv):
            ref.close()


def search_rgba(source_rgba, options, background, scorer: Ssimu2 | None = None, score_tgt: float | None = None,
                tolerance: float | None = None, max_pass: int | None = None, score_yuv: bool = False, rgb_depth: int = 8,
                chroma_upsampling: str = "bilinear"):
    """The target-quality search (oavif_tq_find_target_quality) of an (h, w, 4) uint8 source with straight alpha,
    every pass scored composited over `background`.  `options`: cli.AvifEncOptions (speed, tune, quality_alpha, ...);
    score_tgt / tolerance / max_pass default to its fields.  Each pass encodes from one avif_bridge.EncoderSource
    (four channels), decodes with decode_common and hands libavif's RGBA rows to score_against_reference_rgba as they
    are.  `scorer`: an Ssimu2(..., extended=True); None = one on device 0 for the duration of the call.
    `score_yuv=True` (a yuva=True scorer): the reference is set as before, from the RGBA source, and each pass is
    decode_yuv -> score_against_reference_yuva on the decoder's own Y, U, V and alpha planes, converted to colour codes of
    `rgb_depth` bits with `chroma_upsampling` and composited on the device: avifImageYUVToRGB never runs on the host.
    -> tq.TQResult (last_avif_size: bytes of the last pass)."""
    from . import avif_bridge as ab, tq
    if np.asarray(source_rgba).ndim != 3 or np.asarray(source_rgba).shape[2] != 4:
        raise ValueError("search_rgba needs an (h, w, 4) RGBA source")
    src = as_rgba(source_rgba)
    depth = ab.output_depth(options.tenbit, False)
    own = scorer is None
    s = (Ssimu2(0, yuva=True) if score_yuv else Ssimu2(0, extended=True)) if own else scorer
    last = {"size": 0}
    try:
        s.set_reference_rgba(src, background)
        with ab.EncoderSource(ab.prescale_source(src, depth), depth, options) as enc:
            def probe(q: int) -> float:
                data = enc.encode(options, int(q))
                if score_yuv:
                    with ab.decode_yuv(data) as planes:
                        if (planes.height, planes.width) != src.shape[:2]:
                            raise ValueError(f"codec returned {planes.width}x{planes.height}, expected {src.shape[1]}x{src.shape[0]}")
                        score = s.score_against_reference_yuva(yuva_frame(planes), int(rgb_depth), chroma_upsampling)
                    last["size"] = len(data)
                    return score
                with ab.decode_common(data) as frame:
                    if (frame.height, frame.width) != src.shape[:2]:
                        raise ValueError(f"codec returned {frame.width}x{frame.height}, expected {src.shape[1]}x{src.shape[0]}")
                    rows = frame.rows if frame.channels == 4 else as_rgba(frame.pixels())   # no alpha plane left: opaque
                    score = s.score_against_reference_rgba(rows)
                last["size"] = len(data)
                return score

            out = tq.find_target_quality(probe, options.score_tgt if score_tgt is None else score_tgt,
                                         options.tolerance if tolerance is None else tolerance,
                                         options.max_pass if max_pass is None else max_pass)
    finally:
        if own:
            s.close()
    out.last_avif_size = last["size"]
    return out


def search_rgba_speculative_frames(scorer: Ssimu2, source_rgba, background, codec_frame, score_tgt: float = 80.0,
                                   tolerance: float = 2.0, max_pass: int = 6, max_fanout: int = 4, first_wave_fanout: int = 1,
                                   score_yuv: bool = True, rgb_depth: int = 8, chroma_upsampling: str = "bilinear"):
    """The core of search_rgba_speculative, over any codec: codec_frame(q) -> (frame, avif size), where `frame` is what
    avif_bridge.decode_yuv (`score_yuv`: `planes`, `depth`, `format`, `full_range`, `matrix_coefficients`, `alpha`,
    `alpha_premultiplied`) or avif_bridge.decode_common (else: `channels`, `rows`, `pixels()`) leaves behind, with
    `height`, `width` and `close()`.  The reference is set once, from `source_rgba` over `background`; the waves are
    tq.speculative_frame_waves'; a wave of tq.MIN_BATCHED_WAVE or more frames of one kind is one
    score_batch_against_reference_yuva (`score_yuv`) or score_batch_against_reference_rgba call on `scorer`, an
    Ssimu2(..., abatch=True) in a recursive blur mode; a smaller or mixed wave goes through the single calls search_rgba
    makes.  -> (TQResult, SpecStats, {q: avif size})."""
    from . import tq
    if not getattr(scorer, "abatch", False):
        raise ValueError("search_rgba_speculative needs an Ssimu2(..., abatch=True) context: without the batch library "
                         "every wave would be scored frame by frame (use search_rgba for that)")
    if np.asarray(source_rgba).ndim != 3 or np.asarray(source_rgba).shape[2] != 4:
        raise ValueError("search_rgba_speculative needs an (h, w, 4) RGBA source")
    src = as_rgba(source_rgba)
    scorer.set_reference_rgba(src, background)
    how = (int(rgb_depth), chroma_upsampling)
    least = tq.MIN_BATCHED_WAVE   # the measurement gave no reason to raise it for frames with alpha

    def kind(frame):
        return (frame.depth, frame.format, int(frame.full_range), frame.matrix_coefficients, frame.alpha is None)

    def rgba_of(frame):
        return frame.pixels() if frame.channels == 4 else as_rgba(frame.pixels())   # no alpha plane left: opaque

    def score_frames(frames):
        if score_yuv:
            if len(frames) >= least and all(kind(f) == kind(frames[0]) for f in frames):
                return list(scorer.score_batch_against_reference_yuva([yuva_frame(f) for f in frames], *how))
            return [scorer.score_against_reference_yuva(yuva_frame(f), *how) for f in frames]
        if len(frames) >= least:
            return list(scorer.score_batch_against_reference_rgba([rgba_of(f) for f in frames]))
        return [scorer.score_against_reference_rgba(f.rows if f.channels == 4 else as_rgba(f.pixels())) for f in frames]

    return tq.speculative_frame_waves(codec_frame, score_frames, src.shape[:2], score_tgt, tolerance, max_pass, max_fanout,
                                      first_wave_fanout)


def search_rgba_speculative(source_rgba, options, background, scorer: Ssimu2 | None = None, score_tgt: float | None = None,
                            tolerance: float | None = None, max_pass: int | None = None, max_fanout: int = 4,
                            first_wave_fanout: int = 1, score_yuv: bool = True, rgb_depth: int = 8,
                            chroma_upsampling: str = "bilinear"):
    """search_rgba with several probes in flight on ONE context: the encodes and decodes of a wave run on `max_fanout`
    threads (one avif_bridge.EncoderSource, whose encode calls are independent), and a wave of tq.MIN_BATCHED_WAVE or
    more frames is scored by one batch call of include/ssimu2_hip_abatch.h (search_rgba_speculative_frames).  `scorer`: an
    Ssimu2(..., abatch=True) in a recursive blur mode; None = one in _lib.BLUR_RECURSIVE on device 0 for the duration of
    the call.  An item of a batch has the bits of its single score and the speculative search equals the sequential one,
    so with the same codec and blur mode q, num_pass, history and scores are search_rgba's.
    -> (tq.TQResult, tq.SpecStats, {q: avif size})."""
    from . import avif_bridge as ab
    src = as_rgba(source_rgba) if np.asarray(source_rgba).ndim == 3 and np.asarray(source_rgba).shape[2] == 4 else None
    if src is None:
        raise ValueError("search_rgba_speculative needs an (h, w, 4) RGBA source")
    depth = ab.output_depth(options.tenbit, False)
    own = scorer is None
    s = Ssimu2(0, blur=_lib.BLUR_RECURSIVE, abatch=True) if own else scorer
    try:
        with ab.EncoderSource(ab.prescale_source(src, depth), depth, options) as enc:
            def codec_frame(q: int):
                data = enc.encode(options, int(q))
                return (ab.decode_yuv(data) if score_yuv else ab.decode_common(data)), len(data)

            return search_rgba_speculative_frames(
                s, src, background, codec_frame, options.score_tgt if score_tgt is None else score_tgt,
                options.tolerance if tolerance is None else tolerance, options.max_pass if max_pass is None else max_pass,
                max_fanout, first_wave_fanout, score_yuv, rgb_depth, chroma_upsampling)
    finally:
        if own:
            s.close()


def main(argv=None) -> int:
    a = parse_args(argv)
    if is_avif(a.ref) or is_avif(a.dist):
        try:
            with Ssimu2(a.device, blur=BLUR_MODES[a.blur], yuva=True) as s:
                scores = score_files(s, a.ref, a.dist, a.background, a.rgb_depth, a.chroma_upsampling)
        except ValueError as e:
            print(f"Error: {e}", file=sys.stderr)
            return 1
        return report(scores)
    ref, dist = load_rgba(a.ref), load_rgba(a.dist)
    if ref.shape != dist.shape:
        print(f"Error: {a.ref} is {ref.shape[1]}x{ref.shape[0]}, {a.dist} is {dist.shape[1]}x{dist.shape[0]}", file=sys.stderr)
        return 1
    with Ssimu2(a.device, blur=BLUR_MODES[a.blur], extended=True) as s:
        scores = score_over(s, ref, dist, a.background)
    return report(scores)


def report(scores) -> int:
    for bg, score in scores:
        print(f"{bg:06X} {score:.6f}")
    print(f"min {min(score for _, score in scores):.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
