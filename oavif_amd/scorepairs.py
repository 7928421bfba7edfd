"""Score a list of image pairs with the batch scorer.

    python -m oavif_amd.scorepairs PAIRS.tsv OUT.csv [--batch B] [--device D] [--blur fir|recursive|recursive_fma]
                                   [--background RRGGBB]

PAIRS.tsv holds one `ref<TAB>dist` path pair per line (PNG or PAM, through the project's own loaders; relative paths are
taken from the list's directory; blank lines and lines starting with '#' are skipped).  Pairs are grouped by frame
size, every group is scored with Ssimu2.score_batch in batches of at most B pairs (one launch set each), and OUT.csv
gets one row per pair in input order: line, ref, dist, width, height, score.  8-bit RGB; 16-bit PNGs are truncated to
8 bits and alpha is dropped, as the search's reference is.  --blur: the blur mode the pairs are scored in.  The default
is fir, SSIMU2_BLUR_FIR on the product library, as the command always scored.  recursive and recursive_fma -- the
published recursion -- bind the library of include/ssimu2_hip_rbatch.h, whose batches score in those modes with the
bits of single scores.  --background RRGGBB (six hex digits; a recursive --blur only): alpha is
not dropped -- every frame is taken as RGBA (one without an alpha channel counts as opaque), both sides of a pair are
composited over that colour on the device and the batches go through Ssimu2.score_batch_rgba, the library of
include/ssimu2_hip_abatch.h.  Without it nothing changes.
"""
from __future__ import annotations

import csv
import os
import sys
from typing import Callable, List, Sequence, Tuple

import numpy as np

DEFAULT_BATCH = 64
BLUR_MODES = ("fir", "recursive", "recursive_fma")   # --blur; the index is the SSIMU2_BLUR_* value


class PairListError(Exception):
    """A line of the pair list that cannot be scored; carries the 1-based line number."""

    def __init__(self, line: int, msg: str):
        super().__init__(f"line {line}: {msg}")
        self.line = line


def load_rgb8(path: str) -> np.ndarray:
    """A PNG or PAM file as the scorer's (h, w, 3) uint8 frame: gray replicated, alpha dropped, 16 bits >> 8."""
    ext = os.path.splitext(path)[1].lower()
    data = open(path, "rb").read()
    if ext == ".pam":
        from .pam import load_pam
        raster, w, h, ch = load_pam(data)
        arr = np.frombuffer(raster, np.uint8).reshape(h, w, ch)
    elif ext == ".png":
        from .png import load_png
        arr, _ch, _hbd, _icc = load_png(data)
    else:
        raise ValueError(f"unsupported image format {ext or path!r} (PNG or PAM)")
    from .cli import to_rgb8
    return to_rgb8(arr)


def load_rgba8(path: str) -> np.ndarray:
    """A PNG or PAM file as an (h, w, 4) uint8 frame with straight alpha: gray replicated, 16 bits >> 8, a file without
    an alpha channel opaque."""
    ext = os.path.splitext(path)[1].lower()
    data = open(path, "rb").read()
    if ext == ".pam":
        from .pam import load_pam
        raster, w, h, ch = load_pam(data)
        arr = np.frombuffer(raster, np.uint8).reshape(h, w, ch)
    elif ext == ".png":
        from .png import load_png
        arr, _ch, _hbd, _icc = load_png(data)
    else:
        raise ValueError(f"unsupported image format {ext or path!r} (PNG or PAM)")
    from .cli import to_rgb8
    arr = np.asarray(arr)
    if arr.dtype == np.uint16:
        arr = (arr >> 8).astype(np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    has_alpha = arr.shape[2] in (2, 4)
    alpha = arr[:, :, -1] if has_alpha else np.full(arr.shape[:2], 255, np.uint8)
    return np.ascontiguousarray(np.dstack([to_rgb8(arr), alpha]))


def parse_pairs(text: str, base_dir: str = "") -> List[Tuple[int, str, str]]:
    """-> [(line number, ref path, dist path)] of a pair list."""
    out = []
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.strip("\r\n")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        parts = line.split("\t")
        if len(parts) != 2 or not parts[0].strip() or not parts[1].strip():
            raise PairListError(no, "expected `ref<TAB>dist`")
        out.append((no, os.path.join(base_dir, parts[0].strip()), os.path.join(base_dir, parts[1].strip())))
    return out


def score_pairs(scorer, pairs: Sequence[Tuple[int, str, str]], batch: int = DEFAULT_BATCH,
                load: Callable[[str], np.ndarray] = load_rgb8, background: int | None = None):
    """Score `pairs` ([(line, ref path, dist path)]) with `scorer.score_batch(refs, dists)` -- with a `background`
    (0xRRGGBB; `load` then yields RGBA frames) `scorer.score_batch_rgba(refs, dists, background)` --: pairs grouped by frame
    size in order of first appearance, each group in batches of at most `batch`, frames loaded one batch at a time.
    -> [(line, ref, dist, w, h, score)] in input order.  A file that is missing or unreadable, or a pair whose frames
    differ in size, raises PairListError with the pair's line before anything is scored."""
    if batch < 1:
        raise ValueError("batch must be at least 1")
    sizes = []
    for line, rp, dp in pairs:   # sizes first: a bad line is reported before any GPU work
        shapes = []
        for path in (rp, dp):
            if not os.path.isfile(path):
                raise PairListError(line, f"no such file: {path}")
            try:
                shapes.append(load(path).shape)
            except Exception as e:   # a decoder's own error, with the line that names the file
                raise PairListError(line, f"cannot read {path}: {e}") from e
        if shapes[0] != shapes[1]:
            raise PairListError(line, f"ref is {shapes[0][1]}x{shapes[0][0]}, dist is {shapes[1][1]}x{shapes[1][0]}")
        sizes.append(shapes[0])
    groups = {}
    for i, shape in enumerate(sizes):
        groups.setdefault(shape, []).append(i)
    scores = [None] * len(pairs)
    for shape, members in groups.items():
        for at in range(0, len(members), batch):
            chunk = members[at:at + batch]
            refs = [load(pairs[i][1]) for i in chunk]
            dists = [load(pairs[i][2]) for i in chunk]
            got = scorer.score_batch(refs, dists) if background is None else scorer.score_batch_rgba(refs, dists, background)
            if len(got) != len(chunk):
                raise RuntimeError("score_batch returned the wrong number of scores")
            for i, s in zip(chunk, got):
                scores[i] = float(s)
    return [(line, rp, dp, sizes[i][1], sizes[i][0], scores[i]) for i, (line, rp, dp) in enumerate(pairs)]


def write_csv(rows, f) -> None:
    wr = csv.writer(f, lineterminator="\n")
    wr.writerow(["line", "ref", "dist", "width", "height", "score"])
    for line, rp, dp, w, h, score in rows:
        wr.writerow([line, rp, dp, w, h, repr(score)])


def make_scorer(device: int, blur: str, background: int | None = None):
    """The scorer of a run that brings none: the product library in fir, as ever; in a recursive mode the library whose
    batch calls score in it; with a background the one whose batches composite RGBA frames."""
    from .scorer import Ssimu2
    if background is not None:
        return Ssimu2(device, blur=BLUR_MODES.index(blur), abatch=True)
    if blur == "fir":
        return Ssimu2(device)
    return Ssimu2(device, blur=BLUR_MODES.index(blur), rbatch=True)


USAGE = ("usage: python -m oavif_amd.scorepairs PAIRS.tsv OUT.csv [--batch B] [--device D] [--blur fir|recursive|recursive_fma] "
         "[--background RRGGBB]")


def main(argv=None, scorer=None) -> int:
    args = list(sys.argv[1:] if argv is None else argv)
    batch, device, blur, background, pos = DEFAULT_BATCH, 0, "fir", None, []
    i = 0
    while i < len(args):
        if args[i] == "--blur":
            if i + 1 >= len(args) or args[i + 1] not in BLUR_MODES:
                print(f"--blur needs one of {', '.join(BLUR_MODES)}", file=sys.stderr)
                return 2
            blur = args[i + 1]
            i += 2
        elif args[i] == "--background":
            text = args[i + 1] if i + 1 < len(args) else ""
            if len(text) != 6 or any(ch not in "0123456789abcdefABCDEF" for ch in text):
                print("--background needs six hex digits RRGGBB", file=sys.stderr)
                return 2
            background = int(text, 16)
            i += 2
        elif args[i] in ("--batch", "--device"):
            if i + 1 >= len(args) or not args[i + 1].lstrip("-").isdigit():
                print(f"{args[i]} needs an integer", file=sys.stderr)
                return 2
            if args[i] == "--batch":
                batch = int(args[i + 1])
            else:
                device = int(args[i + 1])
            i += 2
        else:
            pos.append(args[i])
            i += 1
    if len(pos) != 2 or batch < 1:
        print(USAGE, file=sys.stderr)
        return 2
    if background is not None and blur == "fir":
        print("--background needs --blur recursive or recursive_fma: batches of RGBA frames run in those modes", file=sys.stderr)
        return 2
    from . import _lib
    batch = min(batch, _lib.MAX_BATCH)
    try:
        pairs = parse_pairs(open(pos[0]).read(), os.path.dirname(os.path.abspath(pos[0])))
    except (OSError, PairListError) as e:
        print(f"{pos[0]}: {e}", file=sys.stderr)
        return 1
    own = scorer is None
    if own:
        scorer = make_scorer(device, blur) if background is None else make_scorer(device, blur, background)
    try:
        rows = (score_pairs(scorer, pairs, batch) if background is None
                else score_pairs(scorer, pairs, batch, load_rgba8, background))
    except PairListError as e:
        print(f"{pos[0]}: {e}", file=sys.stderr)
        return 1
    finally:
        if own:
            scorer.close()
    with open(pos[1], "w", newline="") as f:
        write_csv(rows, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
