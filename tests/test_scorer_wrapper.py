"""oavif_amd.scorer.Ssimu2 over a stub library: what each method refuses before any C call, how a non-zero return code
surfaces, and where w / h / row_bytes / channels / bit_depth / n land in the C call -- the positions read off the
prototypes of include/*.h.  No library, no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oavif_amd.scorer import Ssimu2, Ssimu2Error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST_ERROR = "the stub refused"
H, W = 6, 10          # every frame of this file
REF_ADDR, DIST_ADDR = 0x1000, 0x2000   # "device addresses": never dereferenced


def _prototypes():
    """{function: [parameter names]} of the two headers the scorer binds."""
    out = {}
    for header in ("ssimu2_hip.h", "ssimu2_hip_internal.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for name, args in re.findall(r"\b(ssimu2_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            out[name] = [re.sub(r"\[.*\]", "", a).split()[-1].lstrip("*") for a in args.split(",") if a.strip() != "void"]
    return out


PROTOTYPES = _prototypes()


class _StubFunction:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def __call__(self, *args):
        if self.name == "ssimu2_last_error":
            return LAST_ERROR.encode()
        self.lib.calls.append((self.name, args))
        if self.lib.rc == 0 and self.name in self.lib.effects:
            self.lib.effects[self.name](*args)
        return self.lib.rc


class StubLibrary:
    """Every attribute is a C function that records its arguments and returns `rc`."""

    def __init__(self):
        self.calls, self.rc, self.effects = [], 0, {}

    def __getattr__(self, name):
        fn = _StubFunction(self, name)
        self.__dict__[name] = fn      # one bound object per function, as ctypes.CDLL keeps
        return fn


def make_scorer(instrumented=False):
    s = Ssimu2.__new__(Ssimu2)
    s._L, s._ctx, s.instrumented, s.device = StubLibrary(), ctypes.c_void_p(0xC0FFEE), instrumented, 0
    return s


def _addr(arg):
    if isinstance(arg, int):
        return arg
    return ctypes.cast(arg, ctypes.c_void_p).value


def frame(dtype=np.uint8, h=H, w=W, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 255, (h, w, c)).astype(dtype)


def padded(dtype, c=4, pad=3):
    """(H, W, c) view of rows `pad` samples longer than the pixels: an avifRGBImage with row padding."""
    buf = np.zeros((H, W * c + pad), dtype)
    return np.lib.stride_tricks.as_strided(buf, (H, W, c), (buf.strides[0], c * buf.itemsize, buf.itemsize))


A8, B8, A16, B16 = frame(seed=1), frame(seed=2), frame(np.uint16, seed=3), frame(np.uint16, seed=4)
P8, P16 = padded(np.uint8), padded(np.uint16)

# method, arguments, C function, {C parameter: value it must carry}, {C parameter: address it must carry}
SUCCESS = [
    ("compute_ssimu2", (A8, B8), "ssimu2_score_rgb8", dict(w=W, h=H, channels=3), dict(ref=A8, dist=B8)),
    ("error_map", (A8, B8), "ssimu2_error_map_rgb8", dict(w=W, h=H, channels=3), dict(ref=A8, dist=B8)),
    ("error_map_against_reference", (B8,), "ssimu2_error_map_against_reference", {}, dict(dist=B8)),
    ("set_reference", (A8,), "ssimu2_set_reference", dict(w=W, h=H), dict(ref=A8)),
    ("score_against_reference", (B8,), "ssimu2_score_against_reference", {}, dict(dist=B8)),
    ("score_decoded_against_reference", (P8,), "ssimu2_score_against_reference_strided",
     dict(row_bytes=W * 4 + 3, channels=4), dict(pixels=P8)),
    ("score_decoded_against_reference", (B8.reshape(-1), W * 3, 3), "ssimu2_score_against_reference_strided",
     dict(row_bytes=W * 3, channels=3), dict(pixels=B8)),
    ("compute_ssimu2_hbd", (A16, B16, 10), "ssimu2_score_rgb16", dict(w=W, h=H, channels=3, bit_depth=10),
     dict(ref=A16, dist=B16)),
    ("set_reference_hbd", (A16, 12), "ssimu2_set_reference_rgb16", dict(w=W, h=H, bit_depth=12), dict(ref=A16)),
    ("score_against_reference_hbd", (B16, 16), "ssimu2_score_against_reference_rgb16", dict(bit_depth=16), dict(dist=B16)),
    ("score_decoded_against_reference_hbd", (P16,), "ssimu2_score_against_reference_strided16",
     dict(row_bytes=(W * 4 + 3) * 2, channels=4, bit_depth=16), dict(pixels=P16)),
    ("score_decoded_against_reference_hbd", (B16.reshape(-1), W * 6, 3, 10), "ssimu2_score_against_reference_strided16",
     dict(row_bytes=W * 6, channels=3, bit_depth=10), dict(pixels=B16)),
    ("score_device", (REF_ADDR, DIST_ADDR, W, H), "ssimu2_score_rgb8_device", dict(w=W, h=H),
     dict(d_ref=REF_ADDR, d_dist=DIST_ADDR)),
    ("enqueue_device", (REF_ADDR, DIST_ADDR, W, H), "ssimu2_enqueue_rgb8_device", dict(w=W, h=H),
     dict(d_ref=REF_ADDR, d_dist=DIST_ADDR)),
    ("set_reference_device", (REF_ADDR, W, H), "ssimu2_set_reference_device", dict(w=W, h=H), dict(d_ref=REF_ADDR)),
    ("enqueue_against_reference_device", (DIST_ADDR,), "ssimu2_enqueue_against_reference_device", {}, dict(d_dist=DIST_ADDR)),
    ("wait", (), "ssimu2_wait", {}, {}),
    ("score_batch", ([A8, A8], [B8, A8]), "ssimu2_score_batch_rgb8", dict(n=2, w=W, h=H), {}),
    ("score_batch_against_reference", ([B8, A8, B8],), "ssimu2_score_batch_against_reference", dict(n=3), {}),
    ("score_batch_device", (REF_ADDR, DIST_ADDR, 512, 5, W, H), "ssimu2_score_batch_rgb8_device",
     dict(item_stride_bytes=512, n=5, w=W, h=H), dict(d_refs=REF_ADDR, d_dists=DIST_ADDR)),
    ("score_batch_against_reference_device", (DIST_ADDR, 512, 5), "ssimu2_score_batch_against_reference_device",
     dict(item_stride_bytes=512, n=5), dict(d_dists=DIST_ADDR)),
    ("last_averages", (), "ssimu2_last_averages", {}, {}),
    ("last_batch_averages", (4,), "ssimu2_last_batch_averages", dict(item=4), {}),
    ("set_blur", (1,), "ssimu2_ctx_set_blur", dict(mode=1), {}),
]
IDS = [f"{c[0]}-{i}" for i, c in enumerate(SUCCESS)]


def _value(arg):
    return arg.value if hasattr(arg, "value") else arg


@pytest.mark.parametrize("method,args,cfn,values,addresses", SUCCESS, ids=IDS)
def test_one_c_call_with_every_size_where_the_header_puts_it(method, args, cfn, values, addresses):
    s = make_scorer()
    getattr(s, method)(*args)
    assert [name for name, _ in s._L.calls] == [cfn]
    got = s._L.calls[0][1]
    params = PROTOTYPES[cfn]
    assert len(got) == len(params), (cfn, params)
    assert _addr(got[0]) == 0xC0FFEE                                   # the context comes first
    for name, want in values.items():
        assert _value(got[params.index(name)]) == want, (cfn, name)
    for name, want in addresses.items():
        assert _addr(got[params.index(name)]) == (want if isinstance(want, int) else want.ctypes.data), (cfn, name)


@pytest.mark.parametrize("method,args,cfn,values,addresses", SUCCESS, ids=IDS)
def test_nonzero_code_raises_with_the_code_and_the_librarys_text(method, args, cfn, values, addresses):
    s = make_scorer()
    s._L.rc = -4
    with pytest.raises(Ssimu2Error) as ei:
        getattr(s, method)(*args)
    assert ei.value.code == -4
    assert str(ei.value) == f"ssimu2 error -4: {LAST_ERROR}"
    assert [name for name, _ in s._L.calls] == [cfn]                 # nothing is called after the failure


def test_batch_calls_pass_one_pointer_per_frame():
    s = make_scorer()
    refs, dists = [A8, A8.copy(), A8], [B8, A8, B8.copy()]
    s.score_batch(refs, dists)
    s.score_batch_against_reference(dists)
    (_, pair), (_, cached) = s._L.calls
    assert [_addr(pair[1][i]) for i in range(3)] == [f.ctypes.data for f in refs]
    assert [_addr(pair[2][i]) for i in range(3)] == [f.ctypes.data for f in dists]
    assert [_addr(cached[1][i]) for i in range(3)] == [f.ctypes.data for f in dists]


def test_results_come_from_what_the_library_wrote():
    s = make_scorer()

    def score(*a):
        a[-1]._obj.value = 71.25

    def scores(*a):
        for i in range(3):
            a[-1][i] = 10.0 + i

    def averages(*a):
        for i in range(108):
            a[-2][i] = float(i)
        a[-1]._obj.value = 5

    def emap(*a):
        a[-1]._obj.value = 71.25
        a[-2][H * W - 1] = 0.5

    s._L.effects.update(ssimu2_score_rgb8=score, ssimu2_score_against_reference=score, ssimu2_wait=score,
                        ssimu2_score_against_reference_strided=score, ssimu2_score_rgb16=score,
                        ssimu2_score_against_reference_rgb16=score, ssimu2_score_against_reference_strided16=score,
                        ssimu2_score_rgb8_device=score, ssimu2_score_batch_rgb8=scores,
                        ssimu2_score_batch_against_reference=scores, ssimu2_score_batch_rgb8_device=scores,
                        ssimu2_score_batch_against_reference_device=scores, ssimu2_last_averages=averages,
                        ssimu2_last_batch_averages=averages, ssimu2_error_map_rgb8=emap,
                        ssimu2_error_map_against_reference=emap)
    assert s.compute_ssimu2(A8, B8) == 71.25
    assert s.score_against_reference(B8) == 71.25
    assert s.score_decoded_against_reference(P8) == 71.25
    assert s.compute_ssimu2_hbd(A16, B16, 16) == 71.25
    assert s.score_against_reference_hbd(B16, 16) == 71.25
    assert s.score_decoded_against_reference_hbd(P16) == 71.25
    assert s.score_device(REF_ADDR, DIST_ADDR, W, H) == 71.25
    assert s.wait() == 71.25
    for got in (s.score_batch([A8] * 3, [B8] * 3), s.score_batch_against_reference([B8] * 3),
                s.score_batch_device(REF_ADDR, DIST_ADDR, 512, 3, W, H),
                s.score_batch_against_reference_device(DIST_ADDR, 512, 3)):
        assert got.dtype == np.float64 and got.tolist() == [10.0, 11.0, 12.0]
    for avg, ns in (s.last_averages(), s.last_batch_averages(2)):
        assert ns == 5 and avg.shape == (6, 18) and avg.dtype == np.float64
        assert np.array_equal(avg.reshape(-1), np.arange(108.0))
    for sc, m in (s.error_map(A8, B8), s.error_map_against_reference(B8)):
        assert sc == 71.25 and m.shape == (H, W) and m.dtype == np.float32 and m[H - 1, W - 1] == 0.5


def test_an_empty_batch_returns_without_a_c_call():
    s = make_scorer()
    for got in (s.score_batch([], []), s.score_batch_against_reference([])):
        assert got.shape == (0,) and got.dtype == np.float64
    assert s._L.calls == []


WIDE8, WIDE16, GRAY = frame(w=W + 1), frame(np.uint16, w=W + 1), np.zeros((H, W), np.uint8)
LOOSE8 = np.zeros((H, W, 8), np.uint8)[..., ::2]          # pixels of a row not tightly packed
LOOSE16 = np.zeros((H, W, 8), np.uint16)[..., ::2]

# method, arguments, exception, its text (None = any): refused whatever the context holds
REFUSED = [
    ("compute_ssimu2", (GRAY, B8), ValueError, "ref must be (h, w, 3) uint8, got (6, 10)"),
    ("compute_ssimu2", (A8, frame(c=4)), ValueError, "dist must be (h, w, 3) uint8, got (6, 10, 4)"),
    ("compute_ssimu2", (A8, WIDE8), ValueError, "ref and dist must have the same shape"),
    ("error_map", (A8, GRAY), ValueError, "dist must be (h, w, 3) uint8, got (6, 10)"),
    ("error_map", (WIDE8, B8), ValueError, "ref and dist must have the same shape"),
    ("error_map_against_reference", (GRAY,), ValueError, "dist must be (h, w, 3) uint8, got (6, 10)"),
    ("set_reference", (GRAY,), ValueError, "ref must be (h, w, 3) uint8, got (6, 10)"),
    ("score_against_reference", (GRAY,), ValueError, "dist must be (h, w, 3) uint8, got (6, 10)"),
    ("score_decoded_against_reference", (A16,), TypeError, "pixels must be uint8"),
    ("score_decoded_against_reference", (LOOSE8,), ValueError, "pixels of a row must be tightly packed"),
    ("score_decoded_against_reference", (B8.reshape(-1),), ValueError, "flat buffers need row_bytes and channels"),
    ("score_decoded_against_reference", (B8.reshape(-1), W * 3), ValueError, "flat buffers need row_bytes and channels"),
    ("compute_ssimu2_hbd", (A8, B16, 16), TypeError, "ref must be uint16 (16-bit samples), got uint8"),
    ("compute_ssimu2_hbd", (A16, B8, 16), TypeError, "dist must be uint16 (16-bit samples), got uint8"),
    ("compute_ssimu2_hbd", (A16, GRAY.astype(np.uint16), 16), ValueError, "dist must be (h, w, 3) uint16, got (6, 10)"),
    ("compute_ssimu2_hbd", (A16, WIDE16, 16), ValueError, "ref and dist must have the same shape"),
    ("set_reference_hbd", (A8, 16), TypeError, "ref must be uint16 (16-bit samples), got uint8"),
    ("set_reference_hbd", (GRAY.astype(np.uint16), 16), ValueError, "ref must be (h, w, 3) uint16, got (6, 10)"),
    ("score_against_reference_hbd", (B8, 16), TypeError, "dist must be uint16 (16-bit samples), got uint8"),
    ("score_decoded_against_reference_hbd", (P8,), TypeError, "rows must be uint16, got uint8"),
    ("score_decoded_against_reference_hbd", (LOOSE16,), ValueError, "pixels of a row must be tightly packed"),
    ("score_decoded_against_reference_hbd", (B16.reshape(-1),), ValueError, "flat buffers need row_bytes and channels"),
    ("score_batch", ([A8, WIDE8], [B8, B8]), ValueError, "refs: the frames of a batch must have one size"),
    ("score_batch", ([A8, A8], [B8, GRAY]), ValueError, "dists[1] must be (h, w, 3) uint8, got (6, 10)"),
    ("score_batch", ([A8, A8], [B8]), ValueError, "refs and dists must hold the same number of frames"),
    ("score_batch", ([A8], [WIDE8]), ValueError, "refs and dists must have the same shape"),
    ("score_batch_against_reference", ([B8, WIDE8],), ValueError, "dists: the frames of a batch must have one size"),
]
# the same against a cached reference of another size
REFUSED_AGAINST_REFERENCE = [
    ("error_map_against_reference", (WIDE8,), "dist shape differs from the reference's"),
    ("score_against_reference", (WIDE8,), "dist shape differs from the reference's"),
    ("score_against_reference_hbd", (WIDE16, 16), "dist shape differs from the reference's"),
    ("score_decoded_against_reference", (WIDE8,), "frame size differs from the reference's"),
    ("score_decoded_against_reference_hbd", (WIDE16,), "frame size differs from the reference's"),
    ("score_batch_against_reference", ([WIDE8, WIDE8],), "dist shape differs from the reference's"),
]


@pytest.mark.parametrize("method,args,exc,text", REFUSED, ids=[f"{c[0]}-{i}" for i, c in enumerate(REFUSED)])
def test_bad_input_is_refused_before_any_c_call(method, args, exc, text):
    s = make_scorer()
    with pytest.raises(exc) as ei:
        getattr(s, method)(*args)
    assert type(ei.value) is exc and str(ei.value) == text
    assert s._L.calls == []


@pytest.mark.parametrize("setter", ["set_reference", "set_reference_hbd", "set_reference_device", "time_kernels"])
@pytest.mark.parametrize("method,args,text", REFUSED_AGAINST_REFERENCE,
                         ids=[f"{c[0]}" for c in REFUSED_AGAINST_REFERENCE])
def test_a_frame_of_another_size_than_the_reference_is_refused_before_any_c_call(setter, method, args, text):
    """Every call that caches a reference records its shape; a frame of another shape never reaches the library."""
    s = make_scorer(instrumented=(setter == "time_kernels"))
    if setter == "set_reference":
        s.set_reference(A8)
    elif setter == "set_reference_hbd":
        s.set_reference_hbd(A16, 16)
    elif setter == "set_reference_device":
        s.set_reference_device(REF_ADDR, W, H)
    else:
        s.time_kernels(W, H, [DIST_ADDR], 1, d_ref=REF_ADDR)     # the cached-reference form sets the reference itself
    del s._L.calls[:]
    with pytest.raises(ValueError) as ei:
        getattr(s, method)(*args)
    assert str(ei.value) == text
    assert s._L.calls == []
    # a frame of the reference's size goes through
    same = tuple(A16 if a is WIDE16 else A8 if a is WIDE8 else [A8, A8] if isinstance(a, list) else a for a in args)
    getattr(s, method)(*same)
    assert len(s._L.calls) == 1


def test_the_recorded_reference_shape_follows_successful_calls_only():
    s = make_scorer()
    s.score_against_reference(WIDE8)            # nothing recorded yet: the library decides (SSIMU2_ERR_NO_REFERENCE)
    s.score_decoded_against_reference(WIDE8)
    assert len(s._L.calls) == 2
    s._L.rc = -3
    for call in (lambda: s.set_reference(A8), lambda: s.set_reference_hbd(A16, 16), lambda: s.set_reference_device(REF_ADDR, W, H)):
        with pytest.raises(Ssimu2Error):
            call()
    s._L.rc = 0
    s.score_against_reference(WIDE8)            # a failed set_reference records nothing
    s.set_reference(WIDE8)
    s.score_against_reference(WIDE8)
    with pytest.raises(ValueError):
        s.score_against_reference(A8)
    s.compute_ssimu2(A8, B8)                    # pair calls and batches leave the record alone
    s.score_batch([A8], [B8])
    s.score_against_reference(WIDE8)
    i = make_scorer(instrumented=True)
    i.set_reference(WIDE8)
    i.time_kernels(W, H, [DIST_ADDR], 1, d_refs=[REF_ADDR])      # the pair form does not set a reference
    i.score_against_reference(WIDE8)
    with pytest.raises(ValueError):
        i.score_against_reference(A8)


HOOKS = [
    ("set_batch_segment_rows", (96,), "ssimu2_instr_set_batch_segment_rows", dict(rows_scale0=96)),
    ("batch_segment_rows", (W, H, 1), "ssimu2_instr_batch_segment_rows", dict(w=W, h=H, scale=1)),
    ("time_device", (REF_ADDR, DIST_ADDR, W, H, 7), "ssimu2_time_device", dict(w=W, h=H, iters=7)),
    ("time_stage", (REF_ADDR, DIST_ADDR, W, H, 1, 7), "ssimu2_time_stage", dict(w=W, h=H, stage=1, iters=7)),
    ("measure_read_stream", (1 << 20, 3), "ssimu2_measure_read_stream", dict(bytes=1 << 20, iters=3)),
    ("placed_streams", (), "ssimu2_instr_placed_streams", {}),
    ("rg_stop_after_scale", (2,), "ssimu2_instr_rg_stop_after_scale", dict(scale=2)),
    ("time_march_rotating", ([REF_ADDR], [DIST_ADDR], W, H, 7), "ssimu2_time_march_rotating",
     dict(npairs=1, w=W, h=H, iters=7)),
    ("time_blur_stage_rotating", ([REF_ADDR, DIST_ADDR], W, H, 7), "ssimu2_time_blur_stage_rotating",
     dict(nframes=2, w=W, h=H, iters=7)),
    ("time_kernels", (W, H, [DIST_ADDR, DIST_ADDR], 7, REF_ADDR), "ssimu2_time_kernels", dict(n=2, w=W, h=H, iters=7)),
    ("set_segment_rows", (96, 48), "ssimu2_instr_set_segment_rows", dict(rows_scale0=96, rows_other_scales=48)),
    ("cache_reference_blur", (False,), "ssimu2_instr_cache_reference_blur", dict(enabled=0)),
    ("last_march", (), "ssimu2_instr_last_march", {}),
]


@pytest.mark.parametrize("method,args,cfn,values", HOOKS, ids=[c[0] for c in HOOKS])
def test_hooks_need_the_instrumented_build_and_marshal_like_the_rest(method, args, cfn, values):
    s = make_scorer()
    with pytest.raises(RuntimeError) as ei:
        getattr(s, method)(*args)
    assert not isinstance(ei.value, Ssimu2Error) and "instrumented=True" in str(ei.value)
    assert s._L.calls == []
    s = make_scorer(instrumented=True)
    getattr(s, method)(*args)
    assert [name for name, _ in s._L.calls] == [cfn]
    got, params = s._L.calls[0][1], PROTOTYPES[cfn]
    assert len(got) == len(params) and _addr(got[0]) == 0xC0FFEE
    for name, want in values.items():
        assert _value(got[params.index(name)]) == want, (cfn, name)
    s._L.rc = -1
    with pytest.raises(Ssimu2Error) as ei:
        getattr(s, method)(*args)
    assert ei.value.code == -1 and LAST_ERROR in str(ei.value)


def test_debug_download_sizes_its_planes_by_scale():
    s = make_scorer(instrumented=True)

    def dims(*a):
        a[-2]._obj.value, a[-1]._obj.value = 3, 2      # (10, 6) halved twice, rounding up
    s._L.effects["ssimu2_debug_download"] = dims
    assert s.debug_download(2, 2, W, H).shape == (3, 2, 3)
    assert s.debug_download(4, 2, W, H).shape == (15, 2, 3)
    name, got = s._L.calls[0]
    params = PROTOTYPES[name]
    assert [got[params.index(p)] for p in ("what", "scale", "w", "h")] == [2, 2, W, H]
