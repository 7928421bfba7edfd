"""One image through the target-quality search (main.zig:102-113): what `python -m oavif_amd.cli` and the batch
driver both run between loading an image and writing its AVIF."""
from __future__ import annotations


def search_image(src, o, scorers, prepared, found=None, note=None):
    """Find the quantizer of `src` (cli.Source) under the options `o` (cli.AvifEncOptions) and return
    (tq.TQResult, the AVIF bytes at its q).

    `scorers`: the scorer contexts of the search; more than one fans the probes of a wave over them and as many host
    threads (include/oavif_tq.h, "speculative probe fan-out": same q, score and pass count).  `prepared`: the source as
    the encoder takes it (cli.encoder_input), made once per image; None when the libavif bridge is off.  With the bridge
    a probe's decoded frame goes to the device in libavif's own RGB(A) rows (the alpha-dropping
    copy loop of io.decodeAvifToRgb, io.zig:654-663, never runs on the host); without it, and with fan-out, the codec
    hands over tight RGB8.

    The bytes of the last probe are reused only when its quantizer is the chosen one (EncBuffer, tq.zig:31-35;
    main.zig:109-113), otherwise the image is encoded once more at the chosen q.  With fan-out every probe is kept:
    any of a wave may be the answer.  `found(result)`, when given, runs once the search has ended and before that
    encode: the CLI reports the quantizer there, as main.zig:106 does, so the line is out when the encode fails.

    `o.score_yuv` (--score-yuv 1; needs the bridge, one scorer, and that scorer an Ssimu2(..., yuv=True)): a probe hands
    over the decoder's own Y, U and V planes (avif_bridge.decode_yuv) and avifImageYUVToRGB never runs on the host.  An
    image with an alpha plane, subsampled chroma or a matrix the scorer does not convert goes through the RGB path as
    before, with one line to `note` saying so."""
    from . import cli, tq
    fanout = len(scorers) > 1
    cache = {}

    def encode(q: int) -> bytes:
        data = cli._encode(src.pixels, o, q, icc=src.icc, prepared=prepared)
        if not fanout:
            cache.clear()
        cache[q] = data
        return data

    def codec(q: int):
        data = encode(q)
        return cli._decode_rgb(data), len(data)

    how = dict(score_tgt=o.score_tgt, tolerance=o.tolerance, max_pass=o.max_pass)
    if fanout:
        r, _stats, _sizes = tq.search_speculative_hip(scorers, src.rgb, codec, **how)
        r.buf_q = r.q if r.q in cache else r.buf_q
    elif prepared is not None:
        from . import avif_bridge

        yuv = {"on": bool(getattr(o, "score_yuv", False))}

        def fall_back(why: str):
            yuv["on"] = False
            if note is not None:
                note(f"note: --score-yuv: {why}; scoring libavif's 8-bit RGB instead")

        if yuv["on"] and not getattr(scorers[0], "yuv", False):
            fall_back("the scorer context was not created with yuv=True")

        def codec_frame(q: int):
            data = encode(q)
            if yuv["on"]:
                from .scorer import MATRIX_COEFFICIENTS
                f = avif_bridge.decode_yuv(data)
                if not f.has_alpha and f.format in (1, 4) and f.matrix_coefficients in MATRIX_COEFFICIENTS:
                    return f, len(data)
                f.close()
                fall_back("the decoded image has an alpha plane" if f.has_alpha else
                          f"pixel format {f.format} / matrix {f.matrix_coefficients} is not converted on the device")
            return avif_bridge.decode_common(data), len(data)
        r = tq.search_hip_frames(scorers[0], src.rgb, codec_frame, **how)
    else:
        r = tq.search_hip(scorers[0], src.rgb, codec, **how)
    if found is not None:
        found(r)
    data = cache.get(r.q) if r.buf_q == r.q else None
    if data is None:
        data = cli._encode(src.pixels, o, r.q, icc=src.icc, prepared=prepared)
    return r, data
