"""Host-side mirror of /root/reference/src/tq.zig over the C ABI (include/oavif_tq.h).

`find_target_quality` is `tq.findTargetQuality` (tq.zig:124-210) with the pass
(`computeScoreAtQuality`, tq.zig:21-38) injected as `probe(q) -> score`;
`search_hip` binds the scorer half of each pass to the MI355X scorer and takes the CPU
codec (encode at q -> decode -> RGB8) as a callback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Callable, List, Tuple

import numpy as np

from . import _lib
from .scorer import Ssimu2, Ssimu2Error


@dataclass
class TQResult:
    q: int = 0
    score: float = 0.0
    num_pass: int = 0
    buf_q: int = -1
    history: List[Tuple[int, float]] = field(default_factory=list)
    last_avif_size: int = 0


def _options(score_tgt: float, tolerance: float, max_pass: int) -> _lib.TQOptions:
    return _lib.TQOptions(float(score_tgt), float(tolerance), int(max_pass))


def _result(r: _lib.TQResult) -> TQResult:
    return TQResult(q=int(r.q), score=float(r.score), num_pass=int(r.num_pass), buf_q=int(r.buf_q),
                    history=[(int(r.history[i].q), float(r.history[i].score))
                             for i in range(r.history_len)])


def _trampoline(cfunctype, body):
    """`body(*args)` as a C callback of type `cfunctype` (the `user` pointer is dropped).  An exception in it is
    collected and the callback returns -100, which ends the C search like the Zig `try` at tq.zig:150; `_finish`
    raises it again once the C call has returned.  -> (callback, collected exceptions)"""
    err: list = []

    def cb(_user, *args):
        try:
            body(*args)
            return 0
        except Exception as e:
            err.append(e)
            return -100

    return cfunctype(cb), err


def _finish(rc: int, err: list, what: Callable[[], str]) -> None:
    """After the C search: the callback's own exception first, else the search's code with the text `what()` fetches."""
    if err:
        raise err[0]
    if rc != 0:
        raise Ssimu2Error(rc, what())


def predict_q_from_score(tgt: float) -> int:
    return int(_lib.lib().oavif_tq_predict_q_from_score(float(tgt)))


def interpolate_quantizer(lo: int, hi: int, history, target: float) -> int:
    n = len(history)
    arr = (_lib.TQPass * max(n, 1))()
    for i, (q, s) in enumerate(history):
        arr[i].q, arr[i].score = int(q), float(s)
    return int(_lib.lib().oavif_tq_interpolate_quantizer(lo, hi, arr, n, float(target)))


def find_target_quality(probe: Callable[[int], float], score_tgt: float = 80.0,
                        tolerance: float = 2.0, max_pass: int = 6) -> TQResult:
    def body(q, out):
        out[0] = float(probe(int(q)))

    cb, err = _trampoline(_lib.PROBE_FN, body)
    res = _lib.TQResult()
    opts = _options(score_tgt, tolerance, max_pass)
    rc = _lib.lib().oavif_tq_find_target_quality(ctypes.byref(opts), cb, None, ctypes.byref(res))
    _finish(rc, err, lambda: "oavif_tq_find_target_quality failed")
    return _result(res)


@dataclass
class SpecStats:
    waves: int = 0           # batches of concurrent probes = the latency of the search in passes
    probes_issued: int = 0   # quantizers encoded + scored in total
    cache_hits: int = 0      # passes answered by an earlier wave


def find_target_quality_speculative(batch_probe: Callable[[List[int]], List[float]],
                                    score_tgt: float = 80.0, tolerance: float = 2.0,
                                    max_pass: int = 6, max_fanout: int = 4, first_wave_fanout: int = 0):
    """`findTargetQuality` with several probes in flight (include/oavif_tq.h, "speculative probe
    fan-out").  batch_probe(qs) -> scores probes the quantizers of one wave, qs[0] being the one
    the search waits for.  `first_wave_fanout`: probes of the first wave (0 = max_fanout; 1 = the
    model's guess alone, so a one-pass search costs what the sequential search costs).
    -> (TQResult, SpecStats); the TQResult equals the sequential one."""
    def body(qs, n, out):
        want = [int(qs[i]) for i in range(n)]
        got = list(batch_probe(want))
        if len(got) != n:
            raise ValueError(f"batch_probe returned {len(got)} scores for {n} quantizers")
        for i in range(n):
            out[i] = float(got[i])

    cb, err = _trampoline(_lib.BATCH_PROBE_FN, body)
    res = _lib.TQResult()
    stats = _lib.TQSpecStats()
    opts = _options(score_tgt, tolerance, max_pass)
    so = _lib.TQSpecOptions(int(max_fanout), int(first_wave_fanout))
    rc = _lib.lib().oavif_tq_find_target_quality_speculative(ctypes.byref(opts), ctypes.byref(so), cb, None,
                                                             ctypes.byref(res), ctypes.byref(stats))
    _finish(rc, err, lambda: "oavif_tq_find_target_quality_speculative failed")
    return _result(res), SpecStats(int(stats.waves), int(stats.probes_issued), int(stats.cache_hits))


def search_speculative_hip(scorers, ref_rgb: np.ndarray,
                           codec: Callable[[int], Tuple[np.ndarray, int]], score_tgt: float = 80.0,
                           tolerance: float = 2.0, max_pass: int = 6, max_fanout: int | None = None,
                           first_wave_fanout: int = 1):
    """One search with its probes fanned over `scorers` (one context = one HIP stream each, same
    device) and as many host threads: every probe of a wave runs codec(q) -- the CPU encode +
    decode -- and scores its frame on its own context, so the GPU work of one probe overlaps the
    CPU work of the others (BASELINE configs[2]).  The first wave is the model's guess alone by
    default (`first_wave_fanout=1`): searches that end on their first pass -- most, on typical
    content -- then cost exactly a sequential search, and speculation starts with the second wave.
    -> (TQResult, SpecStats, {q: avif size})."""
    from concurrent.futures import ThreadPoolExecutor
    scorers = list(scorers)
    if not scorers:
        raise ValueError("need at least one scorer context")
    fan = min(len(scorers), _lib.TQ_MAX_FANOUT) if max_fanout is None else int(max_fanout)
    if fan > len(scorers):
        raise ValueError("max_fanout exceeds the number of scorer contexts")
    ref = np.ascontiguousarray(ref_rgb, dtype=np.uint8)
    have_ref = [False] * fan   # a context gets the reference when a wave first uses it: a search that
    sizes: dict = {}           # ends on its first (one-probe) wave uploads it once, like the sequential one

    def one(args):
        slot, q = args
        if not have_ref[slot]:          # a slot is used by one thread at a time
            scorers[slot].set_reference(ref)
            have_ref[slot] = True
        dec, size = codec(q)
        dec = np.ascontiguousarray(dec, dtype=np.uint8)
        if dec.shape != ref.shape:
            raise ValueError(f"codec returned {dec.shape}, expected {ref.shape}")
        sizes[q] = int(size)
        return scorers[slot].score_against_reference(dec)

    with ThreadPoolExecutor(max_workers=fan) as pool:
        def batch(qs):
            return list(pool.map(one, list(enumerate(qs))))

        res, stats = find_target_quality_speculative(batch, score_tgt, tolerance, max_pass, fan,
                                                     min(int(first_wave_fanout), fan))
    res.last_avif_size = sizes.get(res.buf_q, 0)
    return res, stats, sizes


def search_hip(scorer: Ssimu2, ref_rgb: np.ndarray,
               codec: Callable[[int], Tuple[np.ndarray, int]], score_tgt: float = 80.0,
               tolerance: float = 2.0, max_pass: int = 6) -> TQResult:
    """codec(q) -> (decoded (h, w, 3) uint8, avif size in bytes): the CPU encode+decode."""
    L = _lib.lib()
    ref = np.ascontiguousarray(ref_rgb, dtype=np.uint8)
    h, w, _ = ref.shape
    nbytes = w * h * 3

    def body(q, out_rgb, out_size):
        dec, size = codec(int(q))
        dec = np.ascontiguousarray(dec, dtype=np.uint8)
        if dec.shape != ref.shape:
            raise ValueError(f"codec returned {dec.shape}, expected {ref.shape}")
        ctypes.memmove(out_rgb, dec.ctypes.data, nbytes)
        out_size[0] = int(size)

    cb, err = _trampoline(_lib.CODEC_FN, body)
    res = _lib.TQResult()
    last = ctypes.c_size_t()
    opts = _options(score_tgt, tolerance, max_pass)
    rc = L.oavif_tq_search_hip(ctypes.byref(opts), scorer._ctx,
                               ref.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w, h, cb, None,
                               ctypes.byref(res), ctypes.byref(last))
    _finish(rc, err, lambda: L.ssimu2_last_error(scorer._ctx).decode())
    out = _result(res)
    out.last_avif_size = int(last.value)
    return out


def search_hip_frames(scorer: Ssimu2, ref_rgb: np.ndarray, codec_frame, score_tgt: float = 80.0,
                      tolerance: float = 2.0, max_pass: int = 6, ref_bit_depth: int | None = None) -> TQResult:
    """The search with the decoded-frame hand-off: codec_frame(q) -> (frame, avif size)
    where `frame` is what decodeAvifCommon leaves behind (oavif_amd.avif_bridge.DecodedFrame: libavif's own
    8-bit RGB or RGBA rows, `rows` / `row_bytes` / `channels`, closed here after the score).  The rows go to
    the device as they are (`ssimu2_score_against_reference_strided`); the alpha-dropping copy loop of
    io.decodeAvifToRgb (io.zig:654-663) never runs on the host.  Same control flow, q and scores as
    search_hip (the device unpacks to the same tight RGB8).
    A frame decoded at rgb_depth > 8 (avif_bridge.decode_common(data, rgb_depth)) is scored at that depth
    (`ssimu2_score_against_reference_strided16`).  A uint16 `ref_rgb` is a high-bit-depth source and needs its
    `ref_bit_depth` (8..16); the default, a uint8 source, is the reference's search exactly.
    A frame of the decoder's own planes (avif_bridge.decode_yuv: `planes`, `depth`, `format`, `full_range`,
    `matrix_coefficients`) is converted on the device at full precision and scored
    (`ssimu2_score_against_reference_yuv`, rgb_depth 16); the scorer must be an Ssimu2(..., yuv=True)."""
    if ref_bit_depth is None:
        if np.asarray(ref_rgb).dtype == np.uint16:
            raise ValueError("a uint16 ref_rgb needs ref_bit_depth")
        ref = np.ascontiguousarray(ref_rgb, dtype=np.uint8)
        scorer.set_reference(ref)
    else:
        ref = np.asarray(ref_rgb)
        scorer.set_reference_hbd(ref, int(ref_bit_depth))
    last = {"size": 0}

    def probe(q: int) -> float:
        frame, size = codec_frame(int(q))
        try:
            if (frame.height, frame.width) != ref.shape[:2]:
                raise ValueError(f"codec returned {frame.width}x{frame.height}, expected {ref.shape[1]}x{ref.shape[0]}")
            depth = getattr(frame, "rgb_depth", 8)
            if hasattr(frame, "matrix_coefficients"):
                from .scorer import YuvFrame
                score = scorer.score_against_reference_yuv(
                    YuvFrame(frame.planes, frame.depth, frame.format, frame.full_range, frame.matrix_coefficients), 16)
            elif depth > 8:
                score = scorer.score_decoded_against_reference_hbd(frame.rows.reshape(-1), frame.row_bytes,
                                                                   frame.channels, depth)
            else:
                score = scorer.score_decoded_against_reference(frame.rows.reshape(-1), frame.row_bytes, frame.channels)
        finally:
            frame.close()
        last["size"] = int(size)
        return score

    out = find_target_quality(probe, score_tgt, tolerance, max_pass)
    out.last_avif_size = last["size"]
    return out


# The smallest wave of YUV frames search_speculative_hip_frames scores with one batch call.  DESIGN.md section 19: a
# batch of one is a loss against the single call (section 18 measured the same), smaller waves go frame by frame.
MIN_BATCHED_WAVE = 2


def speculative_frame_waves(codec_frame, score_frames, size_hw, score_tgt: float, tolerance: float, max_pass: int,
                            max_fanout: int, first_wave_fanout: int):
    """The wave logic of the speculative searches that score decoded frames on ONE context: the codec_frame(q) ->
    (frame, avif size) calls of a wave -- the CPU encode and decode -- run on `max_fanout` threads, every job is waited
    for, the frames (each `height` x `width` = size_hw, else ValueError) go to score_frames(frames) -> their scores in
    order, and every frame handed over is closed, also when a job or the scoring raises (the first job's exception is
    raised then).  What a wave of how many frames of which kind costs -- one batch call or single calls -- is
    score_frames' own.  -> (TQResult, SpecStats, {q: avif size})."""
    from concurrent.futures import ThreadPoolExecutor
    fan = max(1, min(int(max_fanout), _lib.TQ_MAX_FANOUT))
    sizes: dict = {}
    with ThreadPoolExecutor(max_workers=fan) as pool:
        def wave(qs):
            jobs = [pool.submit(codec_frame, int(q)) for q in qs]
            frames, failed = [], None
            for q, job in zip(qs, jobs):    # every job is waited for, so that every frame handed over is closed
                try:
                    frame, size = job.result()
                except Exception as e:
                    failed = failed or e
                    continue
                frames.append(frame)
                sizes[q] = int(size)
            try:
                if failed is not None:
                    raise failed
                for frame in frames:
                    if (frame.height, frame.width) != tuple(size_hw):
                        raise ValueError(f"codec returned {frame.width}x{frame.height}, expected {size_hw[1]}x{size_hw[0]}")
                return [float(x) for x in score_frames(frames)]
            finally:
                for frame in frames:
                    frame.close()

        res, stats = find_target_quality_speculative(wave, score_tgt, tolerance, max_pass, fan,
                                                     min(max(int(first_wave_fanout), 0), fan))
    res.last_avif_size = sizes.get(res.buf_q, 0)
    return res, stats, sizes


def search_speculative_hip_frames(scorer: Ssimu2, ref_rgb: np.ndarray, codec_frame, score_tgt: float = 80.0,
                                  tolerance: float = 2.0, max_pass: int = 6, max_fanout: int = 4,
                                  first_wave_fanout: int = 1, ref_bit_depth: int | None = None):
    """search_hip_frames with several probes in flight on ONE context (an Ssimu2(..., hbatch=True) in a recursive blur
    mode): the codec_frame(q) calls of a wave -- the CPU encode and decode -- run on `max_fanout` threads, and a wave
    of MIN_BATCHED_WAVE or more YUV frames (the decoder's own planes, all of one kind) is scored by one
    score_batch_against_reference_yuv call, rgb_depth 16.  A smaller wave, and frames that are not YUV planes, go through
    the single calls search_hip_frames uses.  Every frame is closed here (speculative_frame_waves).  An item of a batch
    has the bits of its single score and the speculative search equals the sequential one, so q, num_pass, history and
    scores are search_hip_frames' with the same codec.  A scorer made without hbatch=True is refused here (ValueError):
    it would score every wave frame by frame and lose what the function is for.
    -> (TQResult, SpecStats, {q: avif size})."""
    from .scorer import YuvFrame
    if not getattr(scorer, "hbatch", False):
        raise ValueError("search_speculative_hip_frames needs an Ssimu2(..., hbatch=True) context: without the batch "
                         "library every wave would be scored frame by frame (use search_hip_frames for that)")
    if ref_bit_depth is None:
        if np.asarray(ref_rgb).dtype == np.uint16:
            raise ValueError("a uint16 ref_rgb needs ref_bit_depth")
        ref = np.ascontiguousarray(ref_rgb, dtype=np.uint8)
        scorer.set_reference(ref)
    else:
        ref = np.asarray(ref_rgb)
        scorer.set_reference_hbd(ref, int(ref_bit_depth))

    def yuv_of(frame):
        return YuvFrame(frame.planes, frame.depth, frame.format, frame.full_range, frame.matrix_coefficients)

    def single(frame) -> float:
        depth = getattr(frame, "rgb_depth", 8)
        if hasattr(frame, "matrix_coefficients"):
            return scorer.score_against_reference_yuv(yuv_of(frame), 16)
        if depth > 8:
            return scorer.score_decoded_against_reference_hbd(frame.rows.reshape(-1), frame.row_bytes, frame.channels, depth)
        return scorer.score_decoded_against_reference(frame.rows.reshape(-1), frame.row_bytes, frame.channels)

    def kind(frame):
        return (frame.depth, frame.format, int(frame.full_range), frame.matrix_coefficients)

    def score_frames(frames):
        yuv = [f for f in frames if hasattr(f, "matrix_coefficients")]
        if len(yuv) == len(frames) >= MIN_BATCHED_WAVE and all(kind(f) == kind(yuv[0]) for f in yuv):
            return list(scorer.score_batch_against_reference_yuv([yuv_of(f) for f in frames], 16))
        return [single(f) for f in frames]

    return speculative_frame_waves(codec_frame, score_frames, ref.shape[:2], score_tgt, tolerance, max_pass, max_fanout,
                                   first_wave_fanout)


def prescale(src: np.ndarray, out_depth: int) -> np.ndarray:
    """The source rescaled to the encoder's depth as io.encodeAvifToBuffer does on every pass
    (io.zig:566-617), to be computed once per search (include/oavif_tq.h).  src uint8 or uint16
    (full 16-bit range); out_depth 8 or 10."""
    L = _lib.lib()
    a = np.ascontiguousarray(src)
    u8p, u16p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint16)
    if a.dtype == np.uint8 and out_depth == 10:
        out = np.empty(a.shape, np.uint16)
        L.oavif_prescale_8_to_10(a.ctypes.data_as(u8p), a.size, out.ctypes.data_as(u16p))
    elif a.dtype == np.uint16 and out_depth == 10:
        out = np.empty(a.shape, np.uint16)
        L.oavif_prescale_16_to_10(a.ctypes.data_as(u16p), a.size, out.ctypes.data_as(u16p))
    elif a.dtype == np.uint16 and out_depth == 8:
        out = np.empty(a.shape, np.uint8)
        L.oavif_prescale_16_to_8(a.ctypes.data_as(u16p), a.size, out.ctypes.data_as(u8p))
    elif a.dtype == np.uint8 and out_depth == 8:
        out = a  # io.zig:609-612: the source is handed over as it is
    else:
        raise ValueError("src must be uint8 or uint16, out_depth 8 or 10")
    return out
