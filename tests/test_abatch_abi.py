"""The library of RGBA and YUV-with-alpha batches without a GPU (include/ssimu2_hip_abatch.h): the
header against the binding table, the library's exports (the hbatch library's and the five new calls, nothing else) and
the other nine libraries' (what their tables say, none of the new calls), the header as C, build.py's tables (the six
earlier ones as they were, the tenth library in a seventh), the budgets of the new kernels from the compiler's metadata,
what every new call answers to a null context, the Python flag, and the wave logic of the speculative RGBA search with a
stand-in scorer."""
import ctypes
import os
import subprocess
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import isa_text
from test_abi import _declared_functions, _exported
from test_binding_signatures import check, prototypes
from test_build_units import _includes
from test_hbatch_abi import _kernels, _plain

HEADER = "ssimu2_hip_abatch.h"
UNIT = "ssimu2_abatch.hip"
NAMES = ["ssimu2_abatch_score_against_reference_yuva", "ssimu2_abatch_composite_yuva",
         "ssimu2_abatch_score_against_reference_rgba8", "ssimu2_abatch_score_rgba8", "ssimu2_abatch_composite_rgba8"]


@pytest.fixture(scope="module")
def abatch_lib(hip_lib):
    from oavif_amd import _lib
    return _lib.abatch_lib()


def test_header_and_binding_agree():
    from oavif_amd import _lib
    assert list(_lib.ABATCH_FUNCTIONS) == NAMES                          # header order
    assert _lib.ABATCH_SYMBOLS == tuple(_lib.ABATCH_FUNCTIONS)
    assert set(_declared_functions(HEADER)) == set(NAMES)
    assert list(prototypes(HEADER)) == NAMES
    others = (set(_lib.PUBLIC_FUNCTIONS) | set(_lib.HOOK_FUNCTIONS) | set(_lib.EXT_FUNCTIONS) | set(_lib.YUV_FUNCTIONS) |
              set(_lib.MAP_FUNCTIONS) | set(_lib.CHROMA_FUNCTIONS) | set(_lib.YUVA_FUNCTIONS) | set(_lib.RBATCH_FUNCTIONS) |
              set(_lib.HBATCH_FUNCTIONS))
    assert not set(NAMES) & others
    assert os.path.basename(_lib.ABATCH_LIB_PATH) == "liboavif_hip_abatch.so"
    with open(os.path.join(isa_text.ROOT, "include", HEADER)) as f:
        assert '#include "ssimu2_hip_hbatch.h"' in f.read()


@pytest.mark.parametrize("name", NAMES)
def test_signature_matches_the_header(name):
    from oavif_amd import _lib
    restype, argtypes = _lib.ABATCH_FUNCTIONS[name]
    check(name, prototypes(HEADER)[name], restype, argtypes)


def test_the_library_exports_the_hbatch_library_plus_the_five_calls(abatch_lib):
    from oavif_amd import _lib
    plain, below = _plain(_lib.ABATCH_LIB_PATH), _plain(_lib.HBATCH_LIB_PATH)
    assert plain - below == set(NAMES) and below <= plain
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    want = (public | set(_lib.EXT_SYMBOLS) | set(_lib.YUV_SYMBOLS) | set(_lib.MAP_SYMBOLS) | set(_lib.CHROMA_SYMBOLS) |
            set(_lib.YUVA_SYMBOLS) | set(_lib.RBATCH_SYMBOLS) | set(_lib.HBATCH_SYMBOLS) | set(NAMES))
    assert plain == want, plain ^ want
    for name in want:
        assert hasattr(abatch_lib, name), name


def test_the_other_nine_libraries_export_what_they_did(hip_lib):
    from oavif_amd import _lib
    public = set(_declared_functions("ssimu2_hip.h")) | set(_declared_functions("oavif_tq.h"))
    ext, yuv, maps = set(_lib.EXT_SYMBOLS), set(_lib.YUV_SYMBOLS), set(_lib.MAP_SYMBOLS)
    chroma, yuva, rbatch, hbatch = set(_lib.CHROMA_SYMBOLS), set(_lib.YUVA_SYMBOLS), set(_lib.RBATCH_SYMBOLS), set(_lib.HBATCH_SYMBOLS)
    want = {_lib.LIB_PATH: public, _lib.INSTR_LIB_PATH: public | set(_lib.INSTR_SYMBOLS), _lib.EXT_LIB_PATH: public | ext,
            _lib.YUV_LIB_PATH: public | ext | yuv, _lib.MAP_LIB_PATH: public | ext | yuv | maps,
            _lib.CHROMA_LIB_PATH: public | ext | yuv | maps | chroma,
            _lib.YUVA_LIB_PATH: public | ext | yuv | maps | chroma | yuva,
            _lib.RBATCH_LIB_PATH: public | ext | yuv | maps | chroma | yuva | rbatch,
            _lib.HBATCH_LIB_PATH: public | ext | yuv | maps | chroma | yuva | rbatch | hbatch}
    assert len(want) == 9
    for path, names in want.items():
        got = {s for s in _exported(path) if s.startswith(("ssimu2_", "oavif_"))}
        assert got == names, (path, got ^ names)
        assert not got & set(NAMES), path


def test_the_two_public_headers_the_shim_the_service_and_the_host_know_nothing_of_it():
    for header in ("ssimu2_hip.h", "oavif_tq.h"):
        assert not set(_declared_functions(header)) & set(NAMES)
    for path in (("oavif_amd", "zig", "fssimu2.zig"), ("oavif_amd", "csrc", "oavif_host.c"), ("oavif_amd", "csrc", "oavif_scored.cpp"),
                 ("oavif_amd", "csrc", "remote_client.h"), ("oavif_amd", "csrc", "remote_client.cpp")):
        with open(os.path.join(isa_text.ROOT, *path)) as f:
            assert "abatch" not in f.read(), path


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "ssimu2_hip_abatch.h"\n'
                   "int main(void) {\n"
                   "    double out[1];\n"
                   "    uint16_t codes[3];\n"
                   "    const uint8_t* rows[1] = {0};\n"
                   "    ssimu2_yuva_frame f = {{{0, 0, 0}, {0, 0, 0}, 8, SSIMU2_YUV_420, 1, 6}, 0, 0, 0};\n"
                   "    int rc = ssimu2_abatch_score_against_reference_yuva(0, &f, 1, 16, SSIMU2_CHROMA_BILINEAR, out);\n"
                   "    rc |= ssimu2_abatch_composite_yuva(0, &f, 1, 1, 1, 16, SSIMU2_CHROMA_NEAREST, 0x102030, codes);\n"
                   "    rc |= ssimu2_abatch_score_against_reference_rgba8(0, rows, 4, 1, out);\n"
                   "    rc |= ssimu2_abatch_score_rgba8(0, rows, 4, rows, 4, 1, 1, 1, 0x102030, out);\n"
                   "    rc |= ssimu2_abatch_composite_rgba8(0, rows, 4, 1, 1, 1, 0x102030, codes);\n"
                   "    rc |= ssimu2_hbatch_score_against_reference_rgb16(0, 0, 0, 10, out);\n"   # the header below comes with it
                   "    return rc == 0 ? SSIMU2_MAX_BATCH : 0;\n"
                   "}\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(isa_text.ROOT, "include"), str(src)], check=True)


def test_build_keeps_its_six_tables_and_knows_the_tenth_library_in_a_seventh(hip_lib):
    from oavif_amd import _lib, build
    assert list(build.LIBRARIES) == [build.LIB_PATH, build.INSTR_LIB_PATH, build.EXT_LIB_PATH, build.YUV_LIB_PATH]
    assert build.MAP_LIBRARIES == {build.MAP_LIB_PATH: [*build.YUV_SOURCES, "ssimu2_map.hip"]}
    assert build.CHROMA_LIBRARIES == {build.CHROMA_LIB_PATH: [*build.MAP_SOURCES, "ssimu2_chroma.hip"]}
    assert build.YUVA_LIBRARIES == {build.YUVA_LIB_PATH: [*build.CHROMA_SOURCES, "ssimu2_yuva.hip"]}
    assert build.RBATCH_LIBRARIES == {build.RBATCH_LIB_PATH: [*build.YUVA_SOURCES, "ssimu2_rbatch.hip"]}
    assert build.HBATCH_LIBRARIES == {build.HBATCH_LIB_PATH: [*build.RBATCH_SOURCES, "ssimu2_hbatch.hip"]}
    assert build.ABATCH_LIBRARIES == {build.ABATCH_LIB_PATH: build.ABATCH_SOURCES}
    assert build.ABATCH_SOURCES == [*build.HBATCH_SOURCES, UNIT]
    for table in (build.LIBRARIES, build.MAP_LIBRARIES, build.CHROMA_LIBRARIES, build.YUVA_LIBRARIES, build.RBATCH_LIBRARIES,
                  build.HBATCH_LIBRARIES):
        assert build.ABATCH_LIB_PATH not in table
    assert build.abatch_units() == [UNIT]
    assert build.hbatch_units() == ["ssimu2_hbatch.hip"]
    assert UNIT not in (*build.compile_units(), *build.map_units(), *build.chroma_units(), *build.yuva_units(),
                        *build.rbatch_units(), *build.hbatch_units())
    assert os.path.samefile(os.path.dirname(build.ABATCH_LIB_PATH), os.path.dirname(_lib.ABATCH_LIB_PATH))
    assert os.path.basename(build.ABATCH_LIB_PATH) == "liboavif_hip_abatch.so"
    assert os.path.exists(os.path.join(build.CSRC, UNIT)) and os.path.exists(build.ABATCH_LIB_PATH)   # built by build.build()


def test_build_rebuilds_when_the_tenth_library_is_missing(hip_lib, monkeypatch, tmp_path):
    from oavif_amd import build
    assert not build.libs_need_build()
    monkeypatch.setattr(build, "ABATCH_LIBRARIES", {str(tmp_path / "liboavif_hip_abatch.so"): build.ABATCH_SOURCES})
    assert build.libs_need_build()


def test_the_unit_is_a_front_end_over_the_host_header():
    from oavif_amd import build
    inc = _includes(os.path.join(build.CSRC, UNIT))
    assert {"ssimu2_host.h", HEADER, "ssimu2_yuv_pixel.h", "ssimu2_alpha_pixel.h"} <= inc
    assert not inc & {"ssimu2_hip.hip", "ssimu2_kernels.h", "ssimu2_recursive.h"}
    assert "c_k" not in isa_text.unit_asm(UNIT)
    # one definition of the composite's arithmetic and of the frame checks: the shared header's and ssimu2_yuva.hip's
    for unit in ("ssimu2_yuva.hip", "ssimu2_ext.hip"):
        assert "ssimu2_alpha_pixel.h" in _includes(os.path.join(build.CSRC, unit))
    text = {u: open(os.path.join(build.CSRC, u)).read() for u in (UNIT, "ssimu2_yuva.hip", "ssimu2_ext.hip", "ssimu2_alpha_pixel.h")}
    for what in ("struct YuvaK", "uint32_t yuva_code(", "YuvaK yuva_constants(", "uint32_t composite_code("):
        assert [u for u, t in text.items() if what in t] == ["ssimu2_alpha_pixel.h"], what
    assert "premultiplied" not in text[UNIT] and "alpha_row_bytes smaller" not in text[UNIT]   # check_yuva's, not restated
    assert "OAVIF_YUVA_DIVISION" not in text[UNIT] and "DIV_PLAIN" not in text[UNIT]


# ---- budgets of the new kernels, from the compiler's metadata -------------------------------------------------------
def test_every_new_kernel_has_no_lds_no_scratch_and_no_spill():
    meta = _kernels(isa_text.unit_asm(UNIT))
    yuva = {n: k for n, k in meta.items() if "k_yuva_batch_to_codes" in n}
    rgba = {n: k for n, k in meta.items() if "k_composite_rgba8_batch" in n}
    # <S, SUB, V, BILINEAR, DIV>: six shapes at S = 1 without a division, six at S = 1 and six at S = 2 with umul64hi
    assert len(yuva) == 18, sorted(yuva)
    assert len(rgba) == 1 and len(meta) == 19                       # the unit's only kernels
    for name, k in {**yuva, **rgba}.items():
        assert k["group_segment_fixed_size"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
    single = {n: k["vgpr_count"] for n, k in _kernels(isa_text.unit_asm("ssimu2_yuva.hip")).items() if "k_yuva_to_codes" in n}
    single.update({n: k["vgpr_count"] for n, k in _kernels(isa_text.unit_asm("ssimu2_ext.hip")).items() if "k_composite_rgba8" in n})
    print("measured VGPRs, batch:", {n: k["vgpr_count"] for n, k in {**yuva, **rgba}.items()})
    print("measured VGPRs, single:", single)


# ---- the calls and the Python side ---------------------------------------------------------------------------------
def test_null_context_is_an_invalid_argument(abatch_lib):
    from oavif_amd import _lib
    L, E, out = abatch_lib, _lib.ERR_INVALID_ARG, (ctypes.c_double * 2)()
    y = np.zeros((8, 8), np.uint8)
    frames = (_lib.YuvaFrameC * 2)()
    for fr in frames:
        fr.yuv.planes[0], fr.yuv.row_bytes[0], fr.yuv.depth, fr.yuv.format = y.ctypes.data, 8, 8, _lib.YUV_400
        fr.yuv.full_range, fr.yuv.matrix_coefficients = 1, 6
    rgba = np.zeros((8, 8, 4), np.uint8)
    P = ctypes.POINTER(ctypes.c_uint8)
    pp = (P * 2)(*[rgba.ctypes.data_as(P)] * 2)
    codes = np.zeros((2, 8, 8, 3), np.uint16)
    cp = codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    assert L.ssimu2_abatch_score_against_reference_yuva(None, frames, 2, 16, 0, out) == E
    assert L.ssimu2_abatch_composite_yuva(None, frames, 2, 8, 8, 16, 0, 0, cp) == E
    assert L.ssimu2_abatch_score_against_reference_rgba8(None, pp, 32, 2, out) == E
    assert L.ssimu2_abatch_score_rgba8(None, pp, 32, pp, 32, 2, 8, 8, 0, out) == E
    assert L.ssimu2_abatch_composite_rgba8(None, pp, 32, 2, 8, 8, 0, cp) == E
    # the null context comes before n == 0
    assert L.ssimu2_abatch_score_against_reference_yuva(None, None, 0, 16, 0, None) == E
    assert L.ssimu2_abatch_composite_yuva(None, None, 0, 8, 8, 16, 0, 0, None) == E
    assert L.ssimu2_abatch_score_against_reference_rgba8(None, None, 0, 0, None) == E
    assert L.ssimu2_abatch_score_rgba8(None, None, 0, None, 0, 0, 8, 8, 0, None) == E
    assert L.ssimu2_abatch_composite_rgba8(None, None, 0, 0, 8, 8, 0, None) == E


def test_same_version_as_the_product_library(hip_lib, abatch_lib):
    assert abatch_lib.ssimu2_version() == hip_lib.ssimu2_version()


def test_the_flag():
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    from oavif_amd.scorer import YuvFrame
    assert Ssimu2.abatch is False
    with pytest.raises(ValueError) as ei:
        Ssimu2(0, instrumented=True, abatch=True)
    assert "instrumented=True and abatch=True are different libraries" in str(ei.value)
    s = Ssimu2.__new__(Ssimu2)        # no library, no device: a context without the flag makes none of the calls
    s._L = None
    f = YuvFrame([np.zeros((8, 8), np.uint8)], 8, _lib.YUV_400)
    rgba = np.zeros((1, 8, 8, 4), np.uint8)
    for hbatch in (False, True):      # the 16-bit batch library's flag does not bring these calls
        s.hbatch = hbatch
        for call in (lambda: s.score_batch_against_reference_yuva([f]), lambda: s.composite_yuva_batch([f], 0),
                     lambda: s.score_batch_against_reference_rgba(rgba), lambda: s.score_batch_rgba(rgba, rgba, 0),
                     lambda: s.composite_rgba_batch(rgba, 0), lambda: s.score_batch_against_reference_yuva([])):
            with pytest.raises(Ssimu2Error) as ei:
                call()
            assert ei.value.code == _lib.ERR_UNSUPPORTED and "abatch=True" in str(ei.value)


def test_no_cpu_fallback_without_device(abatch_lib):
    """Without a GPU the library refuses as the product library does; with one the flag implies every earlier one."""
    import torch
    from oavif_amd import Ssimu2, Ssimu2Error, _lib
    if torch.cuda.is_available():
        with Ssimu2(0, abatch=True) as s:
            assert s.abatch and s.hbatch and s.rbatch and s.yuva and s.chroma and s.maps and s.yuv and s.extended
        return
    with pytest.raises(Ssimu2Error) as ei:
        Ssimu2(0, abatch=True)
    assert ei.value.code == _lib.ERR_NO_DEVICE


def test_the_python_side_refuses_what_it_would_otherwise_do_quietly():
    """The speculative search does not fall back to single calls on a context without the flag, and a batch of frames
    of two sizes or of something else than frames is refused before any C call (no library, no device here)."""
    from oavif_amd import Ssimu2, _lib, alpha
    from oavif_amd.scorer import YuvFrame
    s = Ssimu2.__new__(Ssimu2)
    s._L, s.abatch, s.hbatch, s.yuva = None, True, True, True
    small, large = YuvFrame([np.zeros((8, 8), np.uint8)], 8, _lib.YUV_400), YuvFrame([np.zeros((8, 9), np.uint8)], 8, _lib.YUV_400)
    for call in (s.score_batch_against_reference_yuva, lambda fr: s.composite_yuva_batch(fr, 0)):
        with pytest.raises(ValueError) as ei:
            call([small, large])
        assert "one size" in str(ei.value)
        with pytest.raises(TypeError):
            call([small, np.zeros((8, 8), np.uint8)])
    with pytest.raises(ValueError) as ei:
        s.score_batch_against_reference_rgba([np.zeros((8, 8, 4), np.uint8), np.zeros((8, 9, 4), np.uint8)])
    assert "one size" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        s.score_batch_rgba([np.zeros((8, 8, 4), np.uint8)], [np.zeros((8, 8, 4), np.uint8)] * 2, 0)
    assert "same number" in str(ei.value)
    s.abatch = False
    src = np.zeros((8, 8, 4), np.uint8)
    with pytest.raises(ValueError) as ei:
        alpha.search_rgba_speculative_frames(s, src, 0, lambda q: None)
    assert "abatch=True" in str(ei.value)


def test_rows_of_one_pitch_go_through_as_they_are_and_mixed_pitches_are_made_tight():
    from oavif_amd import Ssimu2
    wide = np.zeros((4, 40), np.uint8)
    a = np.lib.stride_tricks.as_strided(wide, (4, 8, 4), (40, 4, 1))
    b = np.lib.stride_tricks.as_strided(wide.copy(), (4, 8, 4), (40, 4, 1))
    frames, arr, row_bytes = Ssimu2._rgba_batch([a, b], "frames")
    assert row_bytes == 40 and frames[0].ctypes.data == a.ctypes.data and len(arr) == 2
    frames, arr, row_bytes = Ssimu2._rgba_batch([a, np.zeros((4, 8, 4), np.uint8)], "frames")
    assert row_bytes == 32 and all(f.flags.c_contiguous for f in frames)


# ---- the wave logic of the speculative RGBA search, with a stand-in scorer -------------------------------------------
class FakeFrame(SimpleNamespace):
    closed = False

    def close(self):
        self.closed = True

    def pixels(self):
        return self.rows


class FakeScorer:
    """What search_rgba_speculative_frames asks of a scorer: a monotone score of the frame's q, and a record of the calls."""
    abatch = True

    def __init__(self):
        self.calls = []
        self.reference = None

    def set_reference_rgba(self, src, bg):
        self.reference = (src.shape, bg)
        self.calls.append(("set", 1))

    @staticmethod
    def _score(q):
        return 40.0 + 0.55 * q

    def score_against_reference_yuva(self, frame, rgb_depth, up):
        self.calls.append(("single", 1))
        return self._score(int(frame.planes[0][0, 0]))

    def score_batch_against_reference_yuva(self, frames, rgb_depth, up):
        self.calls.append(("batch", len(frames)))
        return np.array([self._score(int(f.planes[0][0, 0])) for f in frames])

    def score_against_reference_rgba(self, rows):
        self.calls.append(("single", 1))
        return self._score(int(rows[0, 0, 0]))

    def score_batch_against_reference_rgba(self, frames):
        self.calls.append(("batch", len(frames)))
        return np.array([self._score(int(f[0, 0, 0])) for f in frames])


def fake_codec(handed, score_yuv, fail_at=None, w=8, h=8):
    from oavif_amd import _lib
    lock = threading.Lock()

    def codec_frame(q):
        if q == fail_at:
            raise RuntimeError(f"the encoder failed at q {q}")
        if score_yuv:
            f = FakeFrame(planes=[np.full((h, w), q, np.uint8)], depth=8, format=_lib.YUV_400, full_range=True,
                          matrix_coefficients=6, alpha=np.full((h, w), 255, np.uint8), alpha_premultiplied=False, height=h, width=w)
        else:
            f = FakeFrame(rows=np.full((h, w, 4), q, np.uint8), channels=4, height=h, width=w)
        with lock:
            handed.append(f)
        return f, 1000 + q

    return codec_frame


@pytest.mark.parametrize("score_yuv", [True, False], ids=["yuva", "rgba"])
def test_waves_of_two_or_more_make_one_batch_call_and_every_frame_is_closed(hip_lib, score_yuv):
    from oavif_amd import alpha, tq
    src = np.zeros((8, 8, 4), np.uint8)
    how = dict(score_tgt=80.0, tolerance=0.5, max_pass=6)
    seq = tq.find_target_quality(lambda q: FakeScorer._score(int(q)), **how)
    assert seq.num_pass >= 2
    for fan in (1, 2, 4):
        for first in (1, 4):
            handed, s = [], FakeScorer()
            res, stats, sizes = alpha.search_rgba_speculative_frames(s, src, 0x102030, fake_codec(handed, score_yuv), max_fanout=fan,
                                                                     first_wave_fanout=first, score_yuv=score_yuv, **how)
            what = (score_yuv, fan, first, s.calls, stats)
            assert s.calls[0] == ("set", 1) and s.reference == ((8, 8, 4), 0x102030), what     # the reference: once
            assert [c for c in s.calls if c[0] == "set"] == [("set", 1)], what
            assert (res.q, res.num_pass, res.history) == (seq.q, seq.num_pass, seq.history), what
            assert res.last_avif_size == 1000 + res.buf_q and all(sizes[q] == 1000 + q for q in sizes), what
            assert len(handed) == stats.probes_issued and all(f.closed for f in handed), what
            batches = [n for kind, n in s.calls if kind == "batch"]
            singles = [n for kind, n in s.calls if kind == "single"]
            # a wave is one batch call or, below the threshold, single calls: one call per wave of two or more
            assert all(n >= tq.MIN_BATCHED_WAVE for n in batches), what
            assert sum(batches) + len(singles) == stats.probes_issued, what
            assert len(batches) + len(singles) == stats.waves, what
            if fan == 1:
                assert not batches, what
            else:
                assert batches, what


@pytest.mark.parametrize("score_yuv", [True, False], ids=["yuva", "rgba"])
def test_every_frame_is_closed_when_one_job_raises(hip_lib, score_yuv):
    from oavif_amd import alpha, tq
    src = np.zeros((8, 8, 4), np.uint8)
    first = []
    tq.find_target_quality_speculative(lambda qs: (first.append(list(qs)), [50.0] * len(qs))[1], 80.0, 0.5, 6, 4, 4)
    assert len(first[0]) >= 2                                       # the first wave of this search has several probes
    handed, s = [], FakeScorer()
    with pytest.raises(RuntimeError) as ei:
        alpha.search_rgba_speculative_frames(s, src, 0, fake_codec(handed, score_yuv, fail_at=first[0][1]), score_tgt=80.0,
                                             tolerance=0.5, max_pass=6, max_fanout=4, first_wave_fanout=4, score_yuv=score_yuv)
    assert "the encoder failed" in str(ei.value)
    assert len(handed) == len(first[0]) - 1 and all(f.closed for f in handed)
    assert [c for c in s.calls if c[0] != "set"] == []              # nothing of the failed wave was scored
    # a frame of another size is refused, and closed
    handed, s = [], FakeScorer()
    with pytest.raises(ValueError) as ei:
        alpha.search_rgba_speculative_frames(s, src, 0, fake_codec(handed, score_yuv, w=9), score_tgt=80.0, tolerance=0.5,
                                             max_pass=6, max_fanout=2, first_wave_fanout=2, score_yuv=score_yuv)
    assert "codec returned 9x8, expected 8x8" in str(ei.value) and handed and all(f.closed for f in handed)


# ---- scorepairs --background -------------------------------------------------------------------------------------------
class PairScorer:
    closed = False

    def __init__(self):
        self.calls = []

    def score_batch(self, refs, dists):
        self.calls.append(("rgb", [r.shape for r in refs], None))
        return np.full(len(refs), 1.0)

    def score_batch_rgba(self, refs, dists, background):
        self.calls.append(("rgba", [(r.shape, int(r[0, 0, 3]), int(d[0, 0, 3])) for r, d in zip(refs, dists)], background))
        return np.full(len(refs), 2.0)

    def close(self):
        self.closed = True


def test_scorepairs_background_option(tmp_path, monkeypatch, capsys):
    from oavif_amd import pam, scorepairs, scorer
    rgba = np.zeros((8, 16, 4), np.uint8)
    rgba[..., 3] = 7
    (tmp_path / "r.pam").write_bytes(pam.write_pam(rgba))
    (tmp_path / "d.pam").write_bytes(pam.write_pam(np.zeros((8, 16, 3), np.uint8)))       # no alpha channel: opaque
    tsv, out = tmp_path / "pairs.tsv", tmp_path / "out.csv"
    tsv.write_text("r.pam\td.pam\n")
    made = []

    def stand_in(device, blur, background=None):
        made.append((device, blur, background, PairScorer()))
        return made[-1][3]
    monkeypatch.setattr(scorepairs, "make_scorer", stand_in)
    assert scorepairs.main([str(tsv), str(out), "--blur", "recursive", "--background", "1A80e6"]) == 0
    assert out.read_text().splitlines()[1].endswith(",16,8,2.0")
    assert scorepairs.main([str(tsv), str(out), "--blur", "recursive"]) == 0          # without it nothing changes
    assert out.read_text().splitlines()[1].endswith(",16,8,1.0")
    assert [(d, b, bg) for d, b, bg, _ in made] == [(0, "recursive", 0x1A80E6), (0, "recursive", None)]
    assert made[0][3].calls == [("rgba", [((8, 16, 4), 7, 255)], 0x1A80E6)] and made[0][3].closed
    assert made[1][3].calls == [("rgb", [(8, 16, 3)], None)]
    for bad in (["--background"], ["--background", "12345"], ["--background", "GGGGGG"], ["--background", "0x1A80E6"]):
        assert scorepairs.main([str(tsv), str(out), "--blur", "recursive", *bad]) == 2, bad
    assert "--background needs six hex digits" in capsys.readouterr().err
    assert scorepairs.main([str(tsv), str(out), "--background", "000000"]) == 2         # FIR: the batches do not run there
    assert "--background needs --blur recursive" in capsys.readouterr().err
    assert len(made) == 2                                                              # a bad option makes no scorer
    bound = []
    monkeypatch.undo()
    monkeypatch.setattr(scorer, "Ssimu2", lambda *a, **kw: bound.append((a, kw)))
    scorepairs.make_scorer(2, "recursive_fma", 0x102030)
    assert bound == [((2,), {"blur": 2, "abatch": True})]
