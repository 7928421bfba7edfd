"""Per-pixel SSIMULACRA2 error map of a pair of images on the MI355X.

    python -m oavif_amd.errmap REF DIST OUT [--blur fir|recursive|recursive_fma] [--full-depth]

Loads both images the way the CLI loads its source (cli.load_source), scores DIST against REF
and writes where it is damaged (ssimu2_error_map_rgb8; the map's definition is in
include/ssimu2_hip.h and DESIGN.md section 9).  With --full-depth a 16-bit PNG keeps its 16-bit
samples (ssimu2_error_map_rgb16 at depth 16, include/ssimu2_hip_map.h; an 8-bit image counts as
the samples 257 u); without it every input is reduced to 8 bits.  The score is the one line on
stdout.  OUT by its extension:
  .pfm  the map itself, 32-bit float (greyscale "Pf", little-endian, rows bottom to top)
  .pam  8-bit greyscale, normalised to the map's maximum
  .png  the same as PNG
For the 8-bit forms the maximum goes to stderr.  Exit status 1 on any error (a missing file, no
usable GPU: the library's message on stderr).
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
import zlib

import numpy as np

BLURS = {"fir": 0, "recursive": 1, "recursive_fma": 2}   # _lib.BLUR_*
FORMATS = (".pfm", ".pam", ".png")


def to_grey8(m: np.ndarray):
    """-> ((h, w) uint8 map normalised to its maximum, that maximum)."""
    peak = float(m.max()) if m.size else 0.0
    if not peak > 0.0:
        return np.zeros(m.shape, np.uint8), peak
    return np.clip(np.rint(m.astype(np.float64) * (255.0 / peak)), 0, 255).astype(np.uint8), peak


def pfm_bytes(m: np.ndarray) -> bytes:
    h, w = m.shape
    return f"Pf\n{w} {h}\n-1.0\n".encode() + np.ascontiguousarray(m[::-1], dtype="<f4").tobytes()


def png_bytes(g: np.ndarray) -> bytes:
    """8-bit greyscale PNG of a (h, w) uint8 array (filter 0 on every row, zlib from the standard library)."""
    h, w = g.shape

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = g
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def encode(m: np.ndarray, ext: str):
    """-> (file bytes, maximum used for normalising or None)."""
    if ext == ".pfm":
        return pfm_bytes(m), None
    g, peak = to_grey8(m)
    if ext == ".pam":
        from .pam import write_pam
        return write_pam(g[..., None]), peak
    return png_bytes(g), peak


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m oavif_amd.errmap",
                                 description="Per-pixel SSIMULACRA2 error map of DIST against REF (MI355X).")
    ap.add_argument("ref")
    ap.add_argument("dist")
    ap.add_argument("out", help="output map: .pfm (float), .pam or .png (8-bit, normalised to the maximum)")
    ap.add_argument("--blur", choices=sorted(BLURS), default="fir", help="blur mode of the scorer (default fir)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--full-depth", action="store_true",
                    help="score a 16-bit PNG's 16-bit samples (ssimu2_error_map_rgb16 at depth 16; an 8-bit image "
                         "counts as the samples 257 u) instead of reducing every input to 8 bits")
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    return parser().parse_args(argv)


def load_rgb16(path: str) -> np.ndarray:
    """(h, w, 3) uint16 samples of depth 16 of an image: a 16-bit PNG's own (grey replicated, alpha dropped), any other
    image's 8-bit samples u as 257 u (the same normalised values)."""
    from .cli import CliError, load_source
    if os.path.splitext(path)[1].lower() == ".png":
        from .png import PngError, load_png
        try:
            arr = load_png(open(path, "rb").read())[0]
        except PngError as e:
            raise CliError(e.name)
        if arr.dtype == np.uint16:
            rgb = np.repeat(arr[..., :1], 3, axis=2) if arr.shape[2] < 3 else arr[..., :3]
            return np.ascontiguousarray(rgb)
    return np.multiply(load_source(path).rgb, np.uint16(257), dtype=np.uint16)


def main(argv=None) -> int:
    a = parse_args(argv)
    ext = os.path.splitext(a.out)[1].lower()
    if ext not in FORMATS:
        print(f"errmap: output must end in one of {', '.join(FORMATS)}", file=sys.stderr)
        return 1
    for path in (a.ref, a.dist):
        if not os.path.isfile(path):
            print(f"errmap: {path}: no such file", file=sys.stderr)
            return 1
    from .cli import CliError, load_source
    try:
        if a.full_depth:
            ref, dist = load_rgb16(a.ref), load_rgb16(a.dist)
        else:
            ref, dist = load_source(a.ref).rgb, load_source(a.dist).rgb
    except CliError as e:
        print(f"errmap: {e.name}", file=sys.stderr)
        return 1
    if ref.shape != dist.shape:
        print(f"errmap: sizes differ: {ref.shape[1]}x{ref.shape[0]} and {dist.shape[1]}x{dist.shape[0]}", file=sys.stderr)
        return 1
    try:
        from .scorer import Ssimu2
        with Ssimu2(a.device, blur=BLURS[a.blur], maps=a.full_depth) as s:
            score, m = s.error_map_hbd(ref, dist, 16) if a.full_depth else s.error_map(ref, dist)
    except Exception as e:   # no library, no usable device, a HIP error: the library's message
        print(f"errmap: {e}", file=sys.stderr)
        return 1
    data, peak = encode(m, ext)
    with open(a.out, "wb") as f:
        f.write(data)
    if peak is not None:
        print(f"errmap: map maximum {peak!r} (= 255)", file=sys.stderr)
    print(f"{score:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
